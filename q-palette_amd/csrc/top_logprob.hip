// qpal_top_logprob: the n <= 64 likeliest tokens of up to 128 rows of fp32 logits and their log-probabilities under the plain
// softmax of the row — the "top_logprobs" of a completion API and the per-position alternatives of decoder.Score (include/qpal.h
// and DESIGN.md §27 have the contract word for word).  Order: value descending (fp32 values, NaN read as -inf, -0 == +0), equal
// values by ascending token id.  Every log-probability and the lse are bitwise those of qpal_token_logprob for that token on the
// same row: the maximum and the exp-sum are formed exactly as csrc/logprob.hip forms them.
//
// Workgroup = one row, 16 waves, as in sample.hip and logprob.hip: a 128 k row (513 KB) is read from L2 once per pass.
//   pass 1   the row maximum                      + histogram of key bits 31 .. 21
//   pass 2   sum of expf(l - max)                 + histogram of key bits 20 .. 10 inside the selected bin
//   pass 3                                          histogram of key bits  9 ..  0 -> K, the key of the n-th largest value
//   pass 4   tokens above K (and those at K where all of them fit) into an LDS list of at most 64 entries
//   ties     more holders of K than slots left: groups of 4096 tokens in ascending order, an ordered compaction over the
//            workgroup (ballots inside a wave, a count per wave), until the slots are full — the lowest ids win
//   finish   wave 0 ranks the list by (key descending, id ascending) by counting, so the arrival order in LDS does not show,
//            and forms each entry's log-probability in fp64 as token_logprob_kernel does
// key: the order-preserving unsigned image of the fp32 bits (sample.hip's, with NaN at the key of -inf).  LDS integer atomics
// only (counts: independent of arrival order); no global atomics, no workspace, no scratch, vector stores only.
#include <hip/hip_runtime.h>

#include "qpal_common.h"

namespace qpal {

struct TopLogprobParams {
    const float *logits;
    long ld;
    int rows, vocab, n;
    int *top_id;
    float *top_logprob, *lse;
    const long long *active;
};

constexpr int kTopBins = 2048, kTopMax = 64;

// a < b <=> key(a) < key(b) on fp32 values; -0 and +0 share a key; NaN shares the key of -inf
__device__ __forceinline__ uint32_t top_key(float l) {
    if (l != l) l = kNegInf;
    if (l == 0.f) return 0x80000000u;
    const uint32_t u = __builtin_bit_cast(uint32_t, l);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

struct TopShared {
    uint32_t hist[kTopBins];
    uint32_t bin, rem, cnt;  // the selected bin, what is left of the target inside it, the bin's own count
    int nlist;
    float redm[16], reds[16];
    int wcnt[16];
    float val[kTopMax];
    int id[kTopMax];
};

__device__ __forceinline__ void top_clear(TopShared &sh) {
    for (int i = threadIdx.x; i < kTopBins; i += 1024) sh.hist[i] = 0u;
    __syncthreads();
}

// The bin that holds the target-th largest entry of sh.hist (1 <= target <= the total): wave 0, lane L owns bins 32 L .. 32 L + 31;
// suffix sums over the lanes, then a walk inside one lane.  Ends with a barrier: sh.bin / sh.rem / sh.cnt are set for everyone.
__device__ __forceinline__ void top_pick(TopShared &sh, uint32_t target) {
    __syncthreads();
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 64) {
        uint32_t own = 0u;
        for (int b = 0; b < 32; b++) own += sh.hist[32 * lane + ((b + lane) & 31)];  // (rotated: the lanes hit different banks)
        uint32_t incl = own;  // sum over lanes >= this one
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t t = __shfl_down(incl, off, 64);
            if (lane + off < 64) incl += t;
        }
        const uint32_t above = incl - own;
        if (incl >= target && above < target) {  // exactly one lane
            uint32_t cum = above;
            int b = 31;
            for (; b > 0; b--) {
                const uint32_t hb = sh.hist[32 * lane + b];
                if (cum + hb >= target) break;
                cum += hb;
            }
            sh.bin = 32 * lane + b;
            sh.rem = target - cum;
            sh.cnt = sh.hist[32 * lane + b];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(1024) void top_logprob_kernel(const TopLogprobParams p) {
    __shared__ TopShared sh;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (p.active && p.active[b] < 0) return;  // inactive row: no output is written
    const int vocab = p.vocab, n = p.n, ne = n < vocab ? n : vocab;
    const float *row = p.logits + (long)b * p.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    if (tid == 0) sh.nlist = 0;

    // ---- pass 1: the maximum, as logprob.hip forms it; digit 0 of every key
    top_clear(sh);
    float mx = kNegInf;
    row_pass4(row, vocab, vec, [&](int, int m, const float (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e >= m) continue;
            if (v[e] > mx) mx = v[e];  // (a NaN is never above)
            atomicAdd(&sh.hist[top_key(v[e]) >> 21], 1u);
        }
    });
    mx = wave_max(mx);
    if (lane == 0) sh.redm[wave] = mx;
    top_pick(sh, (uint32_t)ne);
    mx = sh.redm[0];
#pragma unroll
    for (int w = 1; w < 16; w++) mx = fmaxf(mx, sh.redm[w]);
    uint32_t prefix = sh.bin, rem = sh.rem;
    __syncthreads();  // (sh.bin / sh.hist are rewritten below)

    // ---- pass 2: the exp-sum, in logprob.hip's order; digit 1 of the keys inside the selected bin
    top_clear(sh);
    float s = 0.f;
    row_pass4(row, vocab, vec, [&](int, int m, const float (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e >= m) continue;
            const float d = v[e] - mx;  // NaN: a NaN logit (weight 0), or inf - inf (+inf rows: the +inf entries share the mass)
            s += d == d ? expf(d) : (v[e] == mx ? 1.0f : 0.f);
            const uint32_t key = top_key(v[e]);
            if ((key >> 21) == prefix) atomicAdd(&sh.hist[(key >> 10) & 2047u], 1u);
        }
    });
    s = wave_sum(s);
    if (lane == 0) sh.reds[wave] = s;
    top_pick(sh, rem);
    prefix = (prefix << 11) | sh.bin, rem = sh.rem;
    __syncthreads();

    // ---- pass 3: digit 2 -> K, the key of the ne-th largest value; rem of its cnt holders are listed
    top_clear(sh);
    row_pass4(row, vocab, vec, [&](int, int m, const float (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e >= m) continue;
            const uint32_t key = top_key(v[e]);
            if ((key >> 10) == prefix) atomicAdd(&sh.hist[key & 1023u], 1u);
        }
    });
    top_pick(sh, rem);
    const uint32_t K = (prefix << 10) | sh.bin;
    rem = sh.rem;
    const bool excess = sh.cnt > rem;  // more holders of K than slots left for them

    // ---- pass 4: the tokens above K, and those at K where they all fit, in the order they arrive (ranked below)
    row_pass4(row, vocab, vec, [&](int j, int m, const float (&v)[4]) {
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (e >= m) continue;
            const uint32_t key = top_key(v[e]);
            if (excess ? key > K : key >= K) {
                const int slot = atomicAdd(&sh.nlist, 1);
                if (slot < kTopMax) {
                    sh.val[slot] = v[e] != v[e] ? kNegInf : v[e];
                    sh.id[slot] = 4 * j + e;
                }
            }
        }
    });

    // ---- ties: the rem lowest ids among the holders of K into slots ne - rem .. ne - 1
    if (excess) {
        const int ngrp = (vocab + 3) >> 2, first = ne - (int)rem;
        const unsigned long long below = (1ull << lane) - 1ull;
        int base = 0;  // holders in the groups behind us (the same in every thread)
#pragma unroll 1
        for (int j0 = 0; j0 < ngrp && base < (int)rem; j0 += 1024) {
            const int j = j0 + tid, i0 = 4 * j;
            const int m = j < ngrp ? (vocab - i0 < 4 ? vocab - i0 : 4) : 0;
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            bool tie[4];
            int before = 0, wtot = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (e < m) v[e] = row[i0 + e];
                tie[e] = e < m && top_key(v[e]) == K;
                const unsigned long long bal = __ballot(tie[e]);
                before += __popcll(bal & below);
                wtot += __popcll(bal);
            }
            if (lane == 0) sh.wcnt[wave] = wtot;
            __syncthreads();
            int pos = base + before;
#pragma unroll
            for (int w = 0; w < 16; w++) {
                const int c = sh.wcnt[w];
                pos += w < wave ? c : 0;
                base += c;
            }
#pragma unroll
            for (int e = 0; e < 4; e++) {
                if (!tie[e]) continue;
                if (pos < (int)rem) {
                    sh.val[first + pos] = v[e] != v[e] ? kNegInf : v[e];
                    sh.id[first + pos] = i0 + e;
                }
                pos++;
            }
            __syncthreads();  // (sh.wcnt is rewritten by the next group)
        }
    }
    __syncthreads();
    if (tid >= 64) return;

    // ---- finish: wave 0, lane j = list entry j; its rank by counting; the log-probability as token_logprob_kernel combines it
    float part[16];
#pragma unroll
    for (int w = 0; w < 16; w++) part[w] = sh.reds[w];
#pragma unroll
    for (int st = 1; st < 16; st <<= 1)
#pragma unroll
        for (int w = 0; w < 16; w += 2 * st) part[w] += part[w + st];
    const bool held = lane < ne;
    const float lt = held ? sh.val[lane] : kNegInf;
    const int my_id = held ? sh.id[lane] : -1;
    const uint32_t my_key = top_key(lt);
    int rank = 0;
    for (int i = 0; i < ne; i++) {
        const uint32_t ki = top_key(sh.val[i]);
        const int ii = sh.id[i];
        rank += ki > my_key || (ki == my_key && ii < my_id);
    }
    float lp, ls;
    if (mx == kNegInf) {  // no logit above -inf: nothing has a probability
        lp = ls = kNegInf;
    } else if (mx == -kNegInf) {
        ls = mx;
        lp = lt == mx ? -logf(part[0]) : kNegInf;
    } else {
        const double lg = (double)logf(part[0]);  // part[0] >= 1: the maximum's own term
        ls = (float)((double)mx + lg);
        lp = (float)(((double)lt - (double)mx) - lg);
    }
    const long out = (long)b * n;
    if (held) {
        p.top_id[out + rank] = my_id;
        p.top_logprob[out + rank] = lp;
    } else if (lane < n) {  // fewer tokens than entries
        p.top_id[out + lane] = -1;
        p.top_logprob[out + lane] = kNegInf;
    }
    if (p.lse && lane == 0) p.lse[b] = ls;
}

}  // namespace qpal

using namespace qpal;

extern "C" int qpal_top_logprob(const float *logits_f32, long ld_logits, int rows, int vocab, int n, int *top_id, float *top_logprob,
                                float *lse, const long long *active, void *stream) {
    if (!logits_f32 || !top_id || !top_logprob) return QPAL_E_NULL;
    if (rows < 1 || rows > 128 || vocab < 1 || vocab > (1 << 30) || ld_logits < vocab || n < 1 || n > kTopMax) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(logits_f32) & 3) || (reinterpret_cast<uintptr_t>(top_id) & 3) || (reinterpret_cast<uintptr_t>(top_logprob) & 3) ||
        (reinterpret_cast<uintptr_t>(lse) & 3) || (reinterpret_cast<uintptr_t>(active) & 7))
        return QPAL_E_ALIGN;
    TopLogprobParams p{logits_f32, ld_logits, rows, vocab, n, top_id, top_logprob, lse, active};
    hipLaunchKernelGGL(top_logprob_kernel, dim3(rows), dim3(1024), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
