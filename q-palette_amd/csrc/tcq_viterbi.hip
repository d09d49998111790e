// TCQ encoder: the tail-biting Viterbi search of the bitshift trellis (L = 16, V = 2, T = 256 values, 128 steps), bit for bit
// bitshift_codebook(L=16, KV, V=2, tlut_bits=S, decode_mode="quantlut_sym", tlut=tlut16.float()).quantize(X)
// (reference: lib/codebook/bitshift.py:202-294).  qpal_tcq_viterbi in include/qpal.h states the contract.
//
// Layout.  One workgroup runs one sequence at a time and loops over sequences (fixed grid: the workspace does not
// grow with B).  Step i keeps only best_i[g] = min_d cost_{i-1}[g + d 2^(16-KV)] for the G = 2^(16-KV) groups in LDS (double
// buffered); cost_{i-1}[p] = err_{i-1}(p) + best_{i-1}[p >> KV] is recomputed for every candidate p instead of being stored —
// the same fp32 value the reference stores, so nothing changes bit-wise, and no 256 KiB cost array.  Lane l of a wave owns
// group 64 c + l of chunk c and walks its 2^KV candidates in order of d (strict <: ties go to the lowest d, as CPU torch.min).
// The chosen d's leave as KV ballots per 64 groups (KV bits per group per step) in the workspace; one lane backtracks.
#include "qpal_common.h"

// The reference materialises d*d before the sum: no fused multiply-add anywhere in this file.
#pragma clang fp contract(off)

namespace {

constexpr int kSteps = 128;  // T / V
constexpr int kL = 16;

template <int KV>
struct VitGeom {
    static constexpr int G = 1 << (kL - KV);              // groups (states >> KV) = successors' shared predecessor sets
    static constexpr int F = 1 << KV;                     // candidates per group
    static constexpr int NT = G < 1024 ? G : 1024;        // threads per workgroup: one lane per group of a 64-group chunk
    static constexpr int NW = NT / 64;                    // waves
    static constexpr int C = G / 64;                      // 64-group chunks
    static constexpr int CPW = C / NW;                    // chunks per wave
    static constexpr long BP_WORDS = (long)(kSteps - 1) * C * KV;  // uint64 ballots per workgroup
    static constexpr int GRID = qpal::kNumCU * 16 / NW;   // 16 waves per CU when the LDS allows
};

__device__ __forceinline__ float h2f(uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16); }

// squared error of state p's reconstruction pair against (x0, x1): the quantlut_sym hash into the sign-folded codebook image
__device__ __forceinline__ float vit_err(uint32_t p, float x0, float x1, const uint32_t *tab, int esh, uint32_t emask) {
    const uint32_t h = __umul24(p, p + 1u);  // (p + 1) p: only the low 16 bits are used
    const uint32_t e = tab[(h >> esh) & emask];
    const float d0 = h2f(e) - x0;
    const float d1 = h2f(e >> 16) - x1;
    const float s0 = d0 * d0;
    const float s1 = d1 * d1;
    return s0 + s1;
}

__device__ __forceinline__ void argmin_merge(float &bv, uint32_t &bs, float v, uint32_t s) {
    if (v < bv || (v == bv && s < bs)) {
        bv = v;
        bs = s;
    }
}

template <int KV>
__global__ __launch_bounds__(VitGeom<KV>::NT) void tcq_viterbi_kernel(int32_t *__restrict__ states, uint32_t *__restrict__ hat,
                                                                      const uint16_t *__restrict__ x, const uint32_t *__restrict__ tlut,
                                                                      int B, int S, uint64_t *__restrict__ ws) {
    using Gm = VitGeom<KV>;
    constexpr int G = Gm::G, F = Gm::F, NT = Gm::NT, NW = Gm::NW, C = Gm::C, CPW = Gm::CPW;
    extern __shared__ uint32_t tab[];  // 2^(S+1) entries (8 << S bytes of dynamic LDS): fp16 pair of hash bits (sign | index), sign folded into element 0
    __shared__ float best[2][G];
    __shared__ float xs[2 * kSteps];
    __shared__ float red_v[NW];
    __shared__ uint32_t red_s[NW];
    __shared__ int st[kSteps];
    __shared__ int ov_s;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ne = 2 << S;
    for (int e = tid; e < ne; e += NT) tab[e] = tlut[e & ((1 << S) - 1)] ^ ((uint32_t)(e >> S) << 15);
    const int esh = 15 - S;
    const uint32_t emask = (uint32_t)ne - 1u;
    uint64_t *bp = ws + (long)blockIdx.x * Gm::BP_WORDS;

    for (int b = blockIdx.x; b < B; b += gridDim.x) {
        for (int pass = 0; pass < 2; ++pass) {
            __syncthreads();  // the previous pass is done with xs / best / st
            // pass 0: X rolled by 128 values (torch.roll(X, 128, 0) on 256 values), no masks; pass 1: X, both masks
            for (int t = tid; t < 2 * kSteps; t += NT) xs[t] = h2f(x[(long)b * 2 * kSteps + (pass == 0 ? (t + kSteps) & 255 : t)]);
            const int ov = pass == 0 ? -1 : ov_s;
            // best_0: 0, or the start mask (+inf outside the overlap group): cost_0[p] = err_0(p) + best_0[p >> KV]
            for (int g = tid; g < G; g += NT) best[0][g] = (ov < 0 || g == ov) ? 0.f : __builtin_inff();
            __syncthreads();
            for (int i = 1; i < kSteps; ++i) {
                const float x0 = xs[2 * i - 2], x1 = xs[2 * i - 1];
                const float *prev = best[(i - 1) & 1];
                float *cur = best[i & 1];
#pragma unroll 1
                for (int cc = 0; cc < CPW; ++cc) {
                    const int c = wave + cc * NW;
                    const uint32_t g = (uint32_t)(c * 64 + lane);
                    float bv = 0.f;
                    int bd = 0;
#pragma unroll 8
                    for (int d = 0; d < F; ++d) {
                        const uint32_t p = g + ((uint32_t)d << (kL - KV));
                        const float v = vit_err(p, x0, x1, tab, esh, emask) + prev[p >> KV];
                        if (d == 0 || v < bv) {
                            bv = v;
                            bd = d;
                        }
                    }
                    cur[g] = bv;
                    uint64_t w = 0;
#pragma unroll
                    for (int bit = 0; bit < KV; ++bit) {
                        const uint64_t m = __ballot((bd >> bit) & 1);
                        if (lane == bit) w = m;
                    }
                    if (lane < KV) bp[((long)(i - 1) * C + c) * KV + lane] = w;
                }
                __syncthreads();
            }
            // final argmin of cost_127 (lowest state on ties); pass 1 only over the end mask: s & (G - 1) == overlap
            {
                const float x0 = xs[2 * kSteps - 2], x1 = xs[2 * kSteps - 1];
                const float *prev = best[(kSteps - 1) & 1];
                float bv = __builtin_inff();
                uint32_t bs = 0xffffffffu;
#pragma unroll 1
                for (int cc = 0; cc < CPW; ++cc) {
                    const uint32_t g = (uint32_t)((wave + cc * NW) * 64 + lane);
                    if (ov >= 0 && g != (uint32_t)ov) continue;
                    for (int d = 0; d < F; ++d) {
                        const uint32_t s = g + ((uint32_t)d << (kL - KV));
                        argmin_merge(bv, bs, vit_err(s, x0, x1, tab, esh, emask) + prev[s >> KV], s);
                    }
                }
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) {
                    const float ov_ = __shfl_xor(bv, o);
                    const uint32_t os_ = __shfl_xor(bs, o);
                    argmin_merge(bv, bs, ov_, os_);
                }
                if (lane == 0) {
                    red_v[wave] = bv;
                    red_s[wave] = bs;
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave's ballots have left before the backtracking lane reads them
            __syncthreads();
            if (tid == 0) {
                float bv = red_v[0];
                uint32_t s = red_s[0];
                for (int w = 1; w < NW; ++w) argmin_merge(bv, s, red_v[w], red_s[w]);
                st[kSteps - 1] = (int)s;
                const int lo = pass == 0 ? kSteps / 2 + 1 : 1;  // pass 0 needs the walk down to state 64 only
                for (int i = kSteps - 1; i >= lo; --i) {
                    const uint32_t g = s >> KV;
                    const uint64_t *wp = bp + ((long)(i - 1) * C + (g >> 6)) * KV;
                    uint32_t d = 0;
#pragma unroll
                    for (int bit = 0; bit < KV; ++bit)  // L1-bypassing loads: lines of an earlier sequence may sit in this CU's L1
                        d |= (uint32_t)((__hip_atomic_load(wp + bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (g & 63)) & 1u) << bit;
                    s = g + (d << (kL - KV));
                    st[i - 1] = (int)s;
                }
                if (pass == 0) ov_s = st[kSteps / 2] >> KV;
            }
        }
        __syncthreads();
        for (int t = tid; t < kSteps; t += NT) {
            const uint32_t s = (uint32_t)st[t];
            states[(long)b * kSteps + t] = (int32_t)s;
            if (hat) hat[(long)b * kSteps + t] = tab[(__umul24(s, s + 1u) >> esh) & emask];
        }
    }
}

template <int KV>
int launch_viterbi(int32_t *states, void *hat, const void *x, const void *tlut, int B, int S, void *ws, hipStream_t stream) {
    using Gm = VitGeom<KV>;
    const int grid = B < Gm::GRID ? B : Gm::GRID;
    hipLaunchKernelGGL(tcq_viterbi_kernel<KV>, dim3(grid), dim3(Gm::NT), (size_t)(8u << S), stream, states,
                       static_cast<uint32_t *>(hat), static_cast<const uint16_t *>(x), static_cast<const uint32_t *>(tlut), B, S,
                       static_cast<uint64_t *>(ws));
    return (int)hipGetLastError();
}

template <int KV>
long ws_bytes() {
    return (long)VitGeom<KV>::GRID * VitGeom<KV>::BP_WORDS * 8;
}

}  // namespace

extern "C" {

long qpal_tcq_viterbi_ws_bytes(int KV) {
    switch (KV) {
        case 2: return ws_bytes<2>();
        case 3: return ws_bytes<3>();
        case 4: return ws_bytes<4>();
        case 5: return ws_bytes<5>();
        case 6: return ws_bytes<6>();
        case 7: return ws_bytes<7>();
        case 8: return ws_bytes<8>();
        case 9: return ws_bytes<9>();
        case 10: return ws_bytes<10>();
        default: return 0;
    }
}

int qpal_tcq_viterbi(int32_t *states, void *hat_or_null, const void *x_f16, const void *tlut_f16, int B, int S, int KV, void *ws,
                     void *stream) {
    if (!states || !x_f16 || !tlut_f16 || !ws) return QPAL_E_NULL;
    if (S < 9 || S > 11 || KV < 2 || KV > 10) return QPAL_E_PARAM;
    if (B < 1) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(states) & 3) || (reinterpret_cast<uintptr_t>(hat_or_null) & 3) ||
        (reinterpret_cast<uintptr_t>(x_f16) & 1) || (reinterpret_cast<uintptr_t>(tlut_f16) & 3) || (reinterpret_cast<uintptr_t>(ws) & 7))
        return QPAL_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (KV) {
        case 2: return launch_viterbi<2>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
        case 3: return launch_viterbi<3>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
        case 4: return launch_viterbi<4>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
        case 5: return launch_viterbi<5>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
        case 6: return launch_viterbi<6>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
        case 7: return launch_viterbi<7>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
        case 8: return launch_viterbi<8>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
        case 9: return launch_viterbi<9>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
        default: return launch_viterbi<10>(states, hat_or_null, x_f16, tlut_f16, B, S, ws, s);
    }
}

}  // extern "C"
