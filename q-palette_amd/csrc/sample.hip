// qpal_sample: the next token of up to 128 sequences from their fp32 logits — temperature, top-k, top-p and a seeded draw, one
// launch, per-row parameters on the device (DESIGN.md §14 has the contract word for word).  The reference's decode loop draws
// every token with sample(logits, temperature=0.6, top_k=5) (eval/measure_latency.py:102-135: logits / T, keep >= the k-th
// largest, softmax, argmax(probs / Exp(1))); this is that race with a counter-based generator, plus top-p.
//
// Workgroup = one row, 16 waves.  A 128 k row (513 KB) does not fit LDS and is read from L2 once per pass:
//   greedy rows, rows without a filter            1 pass  (argmax / the race)
//   top-k   the k-th largest value                3 passes: radix select (11 + 11 + 10 bits, most significant first) over the
//           order-preserving unsigned image of the fp32 bits, LDS histogram of COUNTS
//   top-p   the mass threshold                    1 pass for the row maximum + 3 passes of the same select with a histogram of
//           MASS exp((l - lmax) / T) over the top-k set, as 2^-40 fixed point in 64-bit integers
//   the race over the kept set                    1 pass (Philox only for groups of four tokens with a kept one)
// qpal_sample_trunc adds min-p, top-a and typical-p, all judged on the one distribution q over the nucleus N:
//   any of the three on, top-p off                1 pass for the row maximum (top-p rows have it already)
//   min-p, top-a                                  predicates w >= wmin of the race pass: no pass of their own
//   top-a, typical-p                              1 pass over N: S = sum w and M = sum w (zmax - z), 2^-40 fixed point
//   typical-p                                     3 passes: the same select over the image of d = |(zmax - z) - M / S|, ascending
// It is the second instantiation of the one kernel body; rows with none of the three on take qpal_sample's branches in it.
// Integer LDS atomics only: sums do not depend on the order of arrival, so two launches are bitwise equal, and the mass of a set
// is exact in the summands (each exp truncated to 2^-40: at most 2^17 * 2^-40 = 2^-23 of the total, which is >= 1).
#include <hip/hip_runtime.h>

#include "qpal_common.h"

namespace qpal {

struct SampleParams {
    const float *logits;
    long ld;
    int rows, vocab;
    const float *temperature;
    const int *top_k;
    const float *top_p;
    const long *seed, *ctr;
    long *token;
    const float *min_p, *top_a, *typical_p;  // qpal_sample_trunc only; each may be null
};

constexpr int kSampleBins = 2048;

// order-preserving unsigned image of an fp32 value: a < b <=> key(a) < key(b); -0 and +0 share a key; NaN: 0 (below -inf)
__device__ __forceinline__ uint32_t sample_key(float l) {
    if (l != l) return 0u;
    if (l == 0.f) return 0x80000000u;
    const uint32_t u = __builtin_bit_cast(uint32_t, l);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

__device__ __forceinline__ unsigned long long shfl_down_u64(unsigned long long v, int off) {
    const uint32_t lo = __shfl_down((uint32_t)v, off, 64), hi = __shfl_down((uint32_t)(v >> 32), off, 64);
    return ((unsigned long long)hi << 32) | lo;
}

struct SampleShared {
    unsigned long long hist[kSampleBins];
    unsigned long long rem;   // what is left of the target inside the selected bin
    unsigned long long acc[2];  // S and M of a truncating row
    int bin;                  // the selected bin; -1: nothing to select (no mass)
    float redv[16];
    int redi[16];
    int redf[16];             // a truncating row: the lowest index of the row maximum per wave
};

// (zmax - z[i]) of a token and its weight exp(-(zmax - z[i])), as every pass computes them.  gap is NaN only for inf - inf (or a
// NaN logit, which no set holds): a logit equal to the maximum has gap 0, anything else is infinitely far.
__device__ __forceinline__ float sample_weight(float v, float lmax, float T) {
    const float d = v - lmax;  // NaN only for inf - inf (or a NaN logit: below every floor >= 1)
    return d == d ? expf(d / T) : (v == lmax ? 1.0f : 0.f);
}
__device__ __forceinline__ float sample_gap(float v, float lmax, float T) {
    const float g = (lmax - v) / T;
    return g == g ? g : (v == lmax ? 0.f : __builtin_inff());
}
__device__ __forceinline__ unsigned long long sample_fixed(float w) { return (unsigned long long)(w * 1099511627776.0f); }  // 2^40, truncated; w in [0, 1]

// What a select ranks: key(v, k) says whether the token is in the set and gives its 32-bit key, mass(v) its weight (MASS only).
struct LogitCountKey {  // top-k: every token, by its logit
    __device__ __forceinline__ bool key(float v, uint32_t &k) const { k = sample_key(v); return true; }
    __device__ __forceinline__ unsigned long long mass(float) const { return 1ull; }
};
struct LogitMassKey {  // top-p: the tokens at or above floor, by their logit, with the mass exp((l - lmax) / T)
    uint32_t floor;
    float lmax, T;
    __device__ __forceinline__ bool key(float v, uint32_t &k) const { k = sample_key(v); return k >= floor; }
    __device__ __forceinline__ unsigned long long mass(float v) const { return sample_fixed(sample_weight(v, lmax, T)); }
};
struct TypicalMassKey {  // typical-p: the tokens at or above floor, by d = |gap - cen| ASCENDING (the complement of d's image), same mass
    uint32_t floor;
    float lmax, T, cen;
    __device__ __forceinline__ bool key(float v, uint32_t &k) const {
        if (sample_key(v) < floor) return false;
        k = ~sample_key(fabsf(sample_gap(v, lmax, T) - cen));
        return true;
    }
    __device__ __forceinline__ unsigned long long mass(float v) const { return sample_fixed(sample_weight(v, lmax, T)); }
};

// Radix select, most significant digit first, over the keys kf gives.  MASS = false: the largest key K with #{key >= K} >= target
// (the target-th largest key).  MASS = true: the largest key K with mass{key >= K} >= frac * mass{all of kf's set}.  Returns
// max(K, none), the same in every thread; with no mass at all (MASS): none.
template <bool MASS, class KeyF>
__device__ uint32_t sample_select(SampleShared &sh, const float *row, int vocab, bool vec, unsigned long long target, uint32_t none, float frac,
                                  const KeyF kf) {
    const int tid = threadIdx.x, lane = tid & 63;
    uint32_t prefix = 0u;
    int done_bits = 0;
#pragma unroll 1
    for (int pass = 0; pass < 3; pass++) {
        const int nbits = pass < 2 ? 11 : 10, shift = 32 - done_bits - nbits;
        for (int i = tid; i < kSampleBins; i += 1024) sh.hist[i] = 0ull;
        __syncthreads();
        row_pass4(row, vocab, vec, [&](int, int n, const float (&v)[4]) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (e >= n) continue;
                uint32_t key;
                if (!kf.key(v[e], key)) continue;
                if (done_bits && (key >> (32 - done_bits)) != prefix) continue;
                unsigned long long wgt = 1ull;
                if constexpr (MASS) {
                    wgt = kf.mass(v[e]);
                    if (wgt == 0ull) continue;
                }
                atomicAdd(&sh.hist[(key >> shift) & ((1u << nbits) - 1u)], wgt);
            }
        });
        __syncthreads();
        if (tid < 64) {  // wave 0: lane L owns bins 32 L .. 32 L + 31; suffix sums over the lanes, then a walk inside one lane
            unsigned long long own = 0ull;
            for (int b = 0; b < 32; b++) own += sh.hist[32 * lane + b];
            unsigned long long incl = own;  // sum over lanes >= this one
#pragma unroll
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long t = shfl_down_u64(incl, off);
                if (lane + off < 64) incl += t;
            }
            unsigned long long tgt = target;
            if (MASS && pass == 0) {
                const uint32_t tlo = __shfl((uint32_t)incl, 0, 64), thi = __shfl((uint32_t)(incl >> 32), 0, 64);
                const unsigned long long total = ((unsigned long long)thi << 32) | tlo;
                tgt = (unsigned long long)((double)frac * (double)total);
                if (tgt > total) tgt = total;
                if (tgt < 1ull) tgt = 1ull;
                if (total == 0ull) tgt = 0ull;
            }
            const unsigned long long above = incl - own;
            const bool mine = tgt != 0ull && incl >= tgt && above < tgt;
            if (mine) {
                unsigned long long cum = above;
                int b = 31;
                for (; b > 0; b--) {
                    const unsigned long long hb = sh.hist[32 * lane + b];
                    if (cum + hb >= tgt) break;
                    cum += hb;
                }
                sh.bin = 32 * lane + b;
                sh.rem = tgt - cum;
            }
            if (__ballot(mine) == 0ull && lane == 0) {  // no mass (or fewer keys than the target): nothing to select
                sh.bin = -1;
                sh.rem = 0ull;
            }
        }
        __syncthreads();
        const int bin = sh.bin;
        target = sh.rem;
        __syncthreads();  // (sh.bin / sh.hist are rewritten by the next pass)
        if (bin < 0) return none;
        prefix = (prefix << nbits) | (uint32_t)bin;
        done_bits += nbits;
    }
    return prefix > none ? prefix : none;
}

// TRUNC = false: qpal_sample.  TRUNC = true: qpal_sample_trunc; a row with none of the three filters on takes the same branches.
template <bool TRUNC>
__global__ __launch_bounds__(1024) void sample_kernel(const SampleParams p) {
    __shared__ SampleShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long ctr = p.ctr[b];
    if (ctr < 0) return;  // inactive row: token[b] keeps what it held
    const float T = p.temperature[b], top_p = p.top_p[b];
    const int top_k = p.top_k[b], vocab = p.vocab;
    const unsigned long long seed = (unsigned long long)p.seed[b];
    const float *row = p.logits + (long)b * p.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const bool greedy = !(T > 0.f) || top_k == 1;

    uint32_t thr = 1u;  // kept set: key >= thr (1: everything but NaN)
    // a truncating row keeps, of that set, {w >= wmin and image(d) >= dthr}, d = |gap - cen|; fb: where the row maximum stands
    bool trunc = false;
    float mx = kNegInf, wmin = 0.f, cen = 0.f;
    uint32_t dthr = 0u;
    if (!greedy) {
        if (top_k > 1 && top_k < vocab) thr = sample_select<false>(sh, row, vocab, vec, (unsigned long long)top_k, 0u, 1.f, LogitCountKey{});
        if (thr < 1u) thr = 1u;
        float min_p = 0.f, top_a = 0.f, typical_p = 1.f;
        if constexpr (TRUNC) {
            if (p.min_p) min_p = p.min_p[b];
            if (p.top_a) top_a = p.top_a[b];
            if (p.typical_p) typical_p = p.typical_p[b];
            trunc = min_p > 0.f || top_a > 0.f || (typical_p > 0.f && typical_p < 1.f);
        }
        const bool nucleus = top_p > 0.f && top_p < 1.f;
        if (nucleus || trunc) {
            row_pass4(row, vocab, vec, [&](int, int n, const float (&v)[4]) {
#pragma unroll
                for (int e = 0; e < 4; e++)
                    if (e < n && v[e] > mx) mx = v[e];
            });
            mx = wave_max(mx);
            if (lane == 0) sh.redv[wave] = mx;
            __syncthreads();
            mx = sh.redv[0];
#pragma unroll
            for (int w = 1; w < 16; w++) mx = sh.redv[w] > mx ? sh.redv[w] : mx;
            __syncthreads();
            if (nucleus && mx > kNegInf) thr = sample_select<true>(sh, row, vocab, vec, 0ull, thr, top_p, LogitMassKey{thr, mx, T});
        }
        if constexpr (TRUNC) {
            trunc = trunc && mx > kNegInf;  // no logit above -inf: nothing to judge, token 0
            if (trunc) {
                const bool typical = typical_p > 0.f && typical_p < 1.f;
                if (min_p > 0.f) wmin = min_p < 1.f ? min_p : 1.f;
                if (top_a > 0.f || typical) {  // S and M over N, exact in their summands
                    if (tid < 2) sh.acc[tid] = 0ull;
                    __syncthreads();
                    unsigned long long s_fix = 0ull, m_fix = 0ull;
                    row_pass4(row, vocab, vec, [&](int, int n, const float (&v)[4]) {
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            if (e >= n || sample_key(v[e]) < thr) continue;
                            const float w = sample_weight(v[e], mx, T);
                            const unsigned long long wf = sample_fixed(w);
                            if (wf == 0ull) continue;
                            s_fix += wf;
                            m_fix += sample_fixed(w * sample_gap(v[e], mx, T));  // w > 0: the gap is finite, the product in [0, 1 / e]
                        }
                    });
#pragma unroll
                    for (int off = 32; off >= 1; off >>= 1) {
                        s_fix += shfl_down_u64(s_fix, off);
                        m_fix += shfl_down_u64(m_fix, off);
                    }
                    if (lane == 0) {
                        atomicAdd(&sh.acc[0], s_fix);
                        atomicAdd(&sh.acc[1], m_fix);
                    }
                    __syncthreads();
                    const double S = (double)sh.acc[0], M = (double)sh.acc[1];  // S >= 2^40: the maximum is in N
                    if (top_a > 0.f) {
                        const float wa = top_a / (float)(S * 9.094947017729282e-13);  // 2^-40
                        wmin = wa > wmin ? wa : wmin;
                    }
                    if (typical) {
                        cen = (float)(M / S);
                        dthr = sample_select<true>(sh, row, vocab, vec, 0ull, 0u, typical_p, TypicalMassKey{thr, mx, T, cen});
                    }
                }
            }
        }
    }

    // ---- the race (greedy: the plain argmax) over the kept set; lowest index on ties; nothing selected: 0
    float best = kNegInf;
    int besti = 0x7fffffff, fb = 0x7fffffff;
    const uint32_t ctr_lo = (uint32_t)(unsigned long long)ctr, ctr_hi = (uint32_t)((unsigned long long)ctr >> 32);
    row_pass4(row, vocab, vec, [&](int j, int n, const float (&v)[4]) {
        bool keep[4], any = false;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            keep[e] = e < n && sample_key(v[e]) >= thr;
            if constexpr (TRUNC) {
                if (trunc && keep[e]) {
                    if (v[e] == mx && fb == 0x7fffffff) fb = 4 * j + e;
                    const float g = sample_gap(v[e], mx, T);
                    keep[e] = sample_weight(v[e], mx, T) >= wmin && ~sample_key(fabsf(g - cen)) >= dthr;
                }
            }
            any |= keep[e];
        }
        if (!any) return;
        uint32_t x[4] = {0u, 0u, 0u, 0u};
        if (!greedy) philox4x32_10((uint32_t)j, 0u, ctr_lo, ctr_hi, (uint32_t)seed, (uint32_t)(seed >> 32), x);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (!keep[e]) continue;
            float s = v[e];
            if (!greedy) {
                const float u = ((float)(x[e] >> 9) + 0.5f) * 1.1920928955078125e-07f;  // 2^-23: exact, in (0, 1)
                const float ex = -logf(u);
                s = v[e] / T - logf(ex);
            }
            if (s > best) best = s, besti = 4 * j + e;  // tokens ascend within a thread: strict > keeps the lowest index
        }
    });
    if constexpr (TRUNC) {  // an empty intersection falls back to the row maximum's lowest index
        if (trunc) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                const int of = __shfl_xor(fb, m, 64);
                fb = of < fb ? of : fb;
            }
            if (lane == 0) sh.redf[wave] = fb;
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const float ob = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(besti, m, 64);
        if (ob > best || (ob == best && oi < besti)) best = ob, besti = oi;
    }
    if (lane == 0) {
        sh.redv[wave] = best;
        sh.redi[wave] = besti;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; w++) {
            const float v = sh.redv[w];
            const int vi = sh.redi[w];
            if (v > best || (v == best && vi < besti)) best = v, besti = vi;
        }
        if constexpr (TRUNC) {
            if (trunc && (unsigned)besti >= (unsigned)vocab)
                for (int w = 0; w < 16; w++) besti = sh.redf[w] < besti ? sh.redf[w] : besti;
        }
        if ((unsigned)besti >= (unsigned)vocab) besti = 0;  // NaN / all -inf: still a valid row of the embedding
        p.token[b] = besti;
    }
}

}  // namespace qpal

using namespace qpal;

static int sample_launch(const float *logits_f32, long ld_logits, int rows, int vocab, const float *temperature, const int *top_k,
                         const float *top_p, const float *min_p, const float *top_a, const float *typical_p, const long *seed,
                         const long *ctr, long *token, void *stream) {
    if (!logits_f32 || !temperature || !top_k || !top_p || !seed || !ctr || !token) return QPAL_E_NULL;
    if (rows < 1 || rows > 128 || vocab < 1 || vocab > (1 << 30) || ld_logits < vocab) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(logits_f32) & 3) || (reinterpret_cast<uintptr_t>(temperature) & 3) ||
        (reinterpret_cast<uintptr_t>(top_k) & 3) || (reinterpret_cast<uintptr_t>(top_p) & 3) || (reinterpret_cast<uintptr_t>(seed) & 7) ||
        (reinterpret_cast<uintptr_t>(ctr) & 7) || (reinterpret_cast<uintptr_t>(token) & 7) || (reinterpret_cast<uintptr_t>(min_p) & 3) ||
        (reinterpret_cast<uintptr_t>(top_a) & 3) || (reinterpret_cast<uintptr_t>(typical_p) & 3))
        return QPAL_E_ALIGN;
    SampleParams p{logits_f32, ld_logits, rows, vocab, temperature, top_k, top_p, seed, ctr, token, min_p, top_a, typical_p};
    if (min_p || top_a || typical_p)
        hipLaunchKernelGGL(sample_kernel<true>, dim3(rows), dim3(1024), 0, static_cast<hipStream_t>(stream), p);
    else
        hipLaunchKernelGGL(sample_kernel<false>, dim3(rows), dim3(1024), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_sample(const float *logits_f32, long ld_logits, int rows, int vocab, const float *temperature, const int *top_k,
                           const float *top_p, const long *seed, const long *ctr, long *token, void *stream) {
    return sample_launch(logits_f32, ld_logits, rows, vocab, temperature, top_k, top_p, nullptr, nullptr, nullptr, seed, ctr, token, stream);
}

extern "C" int qpal_sample_trunc(const float *logits_f32, long ld_logits, int rows, int vocab, const float *temperature, const int *top_k,
                                 const float *top_p, const float *min_p, const float *top_a, const float *typical_p, const long *seed,
                                 const long *ctr, long *token, void *stream) {
    return sample_launch(logits_f32, ld_logits, rows, vocab, temperature, top_k, top_p, min_p, top_a, typical_p, seed, ctr, token, stream);
}
