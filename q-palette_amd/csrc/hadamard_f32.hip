// fp32-in, fp32-out Hadamard rotation for the quantiser's incoherence preprocessing: W * SU and the proxy Hessian are
// rotated at full fp32 precision (qpal_hadamard rounds to fp16, which is right for activations but not for what LDLQ
// consumes).  Replaces matmul_hadUt_head on the quantiser's path (reference: lib/utils/matmul_had.py:95-120, the
// third-party fast_hadamard_transform + a hadK matmul in fp32).
//
// One workgroup per block of hd = K * P consecutive elements of a row (P = 2^logP >= 16), viewed as [K][P]:
//   A. the whole block is read with coalesced 16-byte loads, multiplied by su and stored in LDS (the row stays there);
//      the +-1 signs of hadK are packed into bit masks beside it;
//   B. WHT_P over the P axis: fp32 butterflies in registers, one pass per group of index bits, LDS between passes;
//   C. K > 1: u[j][c] = sum_i hadK[j][i] t[i][c] in fp32 (sign flips and adds: 4 rows x 4 columns per thread);
//      K = 1: u = t.  out = u * post_scale / sqrt(hd), 16-byte stores.
// Every block is read completely (A) before a barrier, and written only in C: out == in is allowed.
//
// LDS layout: element i lives at swz(i) = i ^ (((i >> 5) & 15) << 2), a permutation inside every aligned run of 64 words
// that keeps float4 slots whole.  With it every LDS access of the kernel is bank-conflict-free:
//   * 16-byte accesses by consecutive float4 slots (A, C): within each lane group of ds_read_b128 / ds_write_b128 the slots
//     are permuted inside aligned runs of 8 and 16;
//   * the first pass (bits 0..R-1, R = 4 or 5): thread g reads its own 2^R consecutive elements as float4s; slot 8g + s goes to
//     (8g + s) ^ (g & 15), distinct modulo 16 over any 16 lanes with distinct g & 15;
//   * the later passes (b0 >= 5): the 32 lanes of a ds_read_b32 / ds_write_b32 group read 32 consecutive elements of one
//     aligned run of 32, which swz only permutes.
#include "launch.h"
#include "qpal_common.h"

namespace qpal {
namespace hf32 {

typedef float float4_t __attribute__((ext_vector_type(4)));

constexpr int kLdsBytes = 160 * 1024;

struct Params {
    float *out;             // fp32 [rows][n]
    const float *in;        // fp32 [rows][n] (may be out)
    const float *su;        // fp32 [n] or null
    const uint16_t *hadk;   // fp16 [K][K], +-1 (null when K == 1)
    int rows, n, hd, K, logP;
    int W;                  // 32-bit mask words per hadK row
    int hd_lds;             // hd rounded up to 64 (swz stays inside)
    float scale;            // post_scale / sqrt(hd)
    int npass;              // butterfly passes after the first
    int r[3];               // index bits of each of them (the first pass takes min(5, logP))
};

__device__ __forceinline__ int swz(int i) { return i ^ (((i >> 5) & 15) << 2); }

// 2^R-point Walsh-Hadamard butterflies in registers (Sylvester order: bit s of j <-> index bit b0 + s)
template <int R>
__device__ __forceinline__ void butterfly(float (&v)[1 << R]) {
    static_for<0, R>([&](auto sc) {
        constexpr int s = decltype(sc)::value;
#pragma unroll
        for (int j = 0; j < (1 << R); j++) {
            if (!(j & (1 << s))) {
                const float a = v[j], b = v[j | (1 << s)];
                v[j] = a + b;
                v[j | (1 << s)] = a - b;
            }
        }
    });
}

// first pass: index bits [0, R), thread g owns the 2^R consecutive elements from g << R
template <int R, int NT>
__device__ __forceinline__ void pass_first(float *buf, int hd, int tid) {
    constexpr int E = 1 << R;
    for (int g = tid; g < (hd >> R); g += NT) {
        float v[E];
#pragma unroll
        for (int s = 0; s < E; s += 4) {
            const float4_t t = *reinterpret_cast<const float4_t *>(buf + swz((g << R) + s));
            v[s] = t[0], v[s + 1] = t[1], v[s + 2] = t[2], v[s + 3] = t[3];
        }
        butterfly<R>(v);
#pragma unroll
        for (int s = 0; s < E; s += 4)
            *reinterpret_cast<float4_t *>(buf + swz((g << R) + s)) = float4_t{v[s], v[s + 1], v[s + 2], v[s + 3]};
    }
}

// a later pass: index bits [b0, b0 + R), b0 >= 5
template <int R, int NT>
__device__ __forceinline__ void pass_lds(float *buf, int hd, int b0, int tid) {
    constexpr int E = 1 << R;
    for (int g = tid; g < (hd >> R); g += NT) {
        const int i0 = ((g >> b0) << (b0 + R)) | (g & ((1 << b0) - 1));
        float v[E];
#pragma unroll
        for (int j = 0; j < E; j++) v[j] = buf[swz(i0 + (j << b0))];
        butterfly<R>(v);
#pragma unroll
        for (int j = 0; j < E; j++) buf[swz(i0 + (j << b0))] = v[j];
    }
}

template <int NT>
__device__ __forceinline__ void pass_lds_r(int r, float *buf, int hd, int b0, int tid) {
    switch (r) {
        case 1: pass_lds<1, NT>(buf, hd, b0, tid); break;
        case 2: pass_lds<2, NT>(buf, hd, b0, tid); break;
        case 3: pass_lds<3, NT>(buf, hd, b0, tid); break;
        case 4: pass_lds<4, NT>(buf, hd, b0, tid); break;
        default: pass_lds<5, NT>(buf, hd, b0, tid); break;
    }
}

template <int NT>
__global__ __launch_bounds__(NT) void had_f32_kernel(Params p) {
    extern __shared__ float buf[];  // [hd_lds] block (swizzled) + [K][W] sign masks of hadK
    uint32_t *mask = reinterpret_cast<uint32_t *>(buf + p.hd_lds);
    const int tid = threadIdx.x;
    const int bpr = p.n / p.hd;
    const int row = blockIdx.x / bpr, blk = blockIdx.x - row * bpr;
    const long off = (long)row * p.n + (long)blk * p.hd;
    const int nq = p.hd >> 2;

    // ---- A: block * su -> LDS; hadK signs -> bit masks
    {
        const float4_t *src = reinterpret_cast<const float4_t *>(p.in + off);
        const float4_t *su = p.su ? reinterpret_cast<const float4_t *>(p.su + (long)blk * p.hd) : nullptr;
        for (int f = tid; f < nq; f += NT) {
            float4_t v = src[f];
            if (su) v *= su[f];
            *reinterpret_cast<float4_t *>(buf + swz(f << 2)) = v;
        }
    }
    for (int t = tid; t < p.K * p.W && p.K > 1; t += NT) {
        const int j = t / p.W, w = t - j * p.W;
        uint32_t bits = 0;
        for (int b = 0; b < 32; b++) {
            const int i = (w << 5) + b;
            if (i < p.K && (p.hadk[j * p.K + i] & 0x8000u)) bits |= 1u << b;
        }
        mask[t] = bits;
    }
    __syncthreads();

    // ---- B: WHT over the low logP index bits
    if (p.logP >= 5) pass_first<5, NT>(buf, p.hd, tid);
    else pass_first<4, NT>(buf, p.hd, tid);
    __syncthreads();
    int b0 = p.logP >= 5 ? 5 : 4;
    for (int ps = 0; ps < p.npass; ps++) {
        pass_lds_r<NT>(p.r[ps], buf, p.hd, b0, tid);
        b0 += p.r[ps];
        __syncthreads();
    }

    // ---- C: hadK over the K axis, scale, store
    float4_t *dst = reinterpret_cast<float4_t *>(p.out + off);
    if (p.K == 1) {
        for (int f = tid; f < nq; f += NT) dst[f] = *reinterpret_cast<const float4_t *>(buf + swz(f << 2)) * p.scale;
        return;
    }
    const int lq = p.logP - 2;  // column quads per row of the [K][P] view: 2^lq
    const int nitems = (p.K >> 2) << lq;
    for (int it = tid; it < nitems; it += NT) {
        const int jq = it >> lq, cq = it & ((1 << lq) - 1);
        float4_t acc[4] = {};
        for (int i0 = 0; i0 < p.K; i0 += 32) {
            uint32_t m[4];
#pragma unroll
            for (int r = 0; r < 4; r++) m[r] = mask[((jq << 2) + r) * p.W + (i0 >> 5)];
            const int ie = p.K - i0 < 32 ? p.K - i0 : 32;
            for (int ii = 0; ii < ie; ii++) {
                const float4_t t = *reinterpret_cast<const float4_t *>(buf + swz((((i0 + ii) << lq) + cq) << 2));
#pragma unroll
                for (int r = 0; r < 4; r++) acc[r] += ((m[r] >> ii) & 1u) ? -t : t;
            }
        }
#pragma unroll
        for (int r = 0; r < 4; r++) dst[((((jq << 2) + r) << lq) + cq)] = acc[r] * p.scale;
    }
}

template <int NT>
static int launch(const Params &p, size_t lds, hipStream_t stream) {
    return launch_lds<had_f32_kernel<NT>>(dim3(p.rows * (p.n / p.hd)), dim3(NT), lds, kLdsBytes, stream, p);
}

}  // namespace hf32
}  // namespace qpal

using namespace qpal::hf32;

extern "C" int qpal_hadamard_f32(float *out, const float *in, const float *su, const void *hadk, int rows, int n, int hd, int K,
                                 float post_scale, void *stream) {
    if (!out || !in) return QPAL_E_NULL;
    if (K < 1 || K > 256) return QPAL_E_PARAM;
    if (K > 1 && !hadk) return QPAL_E_NULL;
    if (K > 1 && K % 4) return QPAL_E_PARAM;  // every factor of get_hadK: 12, 20, ..., 172
    if (rows < 1 || n < 1 || hd < 1 || n % hd || hd % K) return QPAL_E_SHAPE;
    if ((long)rows * (n / hd) > 0x7fffffffL) return QPAL_E_SHAPE;  // 1-D grid: one workgroup per block
    const int P = hd / K;
    if (P < 16 || (P & (P - 1))) return QPAL_E_SHAPE;
    int logP = 0;
    while ((1 << logP) < P) logP++;
    const int W = K > 1 ? (K + 31) / 32 : 0;
    const int hd_lds = (hd + 63) & ~63;
    const size_t lds = sizeof(float) * (size_t)hd_lds + sizeof(uint32_t) * (size_t)(K * W);
    if (lds > (size_t)kLdsBytes) return QPAL_E_SHAPE;
    // 16-byte loads and stores of every row: n * 4 bytes is a multiple of 16 (hd % 16 == 0 above)
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(su)) & 15)
        return QPAL_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(hadk) & 1) return QPAL_E_ALIGN;
    Params p{out, in, su, static_cast<const uint16_t *>(hadk), rows, n, hd, K, logP, W, hd_lds,
             (float)((double)post_scale / sqrt((double)hd)), 0, {0, 0, 0}};
    // passes after the first (which takes min(5, logP) bits): as few as possible, at most 5 bits each, balanced
    const int rest = logP - (logP >= 5 ? 5 : 4);
    p.npass = (rest + 4) / 5;
    for (int i = 0; i < p.npass; i++) p.r[i] = rest / p.npass + (i < rest % p.npass ? 1 : 0);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (hd <= 4096) return launch<256>(p, lds, s);
    if (hd <= 16384) return launch<512>(p, lds, s);
    return launch<1024>(p, lds, s);
}
