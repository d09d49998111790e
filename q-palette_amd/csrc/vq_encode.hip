// VQ / SQ encoder: nearest codeword of every vec-group, with the in-block LDLQ error feedback of LDLQ_VQ
// (reference: lib/codebook/vq_codebook.py quantize, lib/algo/ldlq.py LDLQ_VQ).  qpal_vq_encode in include/qpal.h states the
// contract.
//
// Layout.  The fp32 codebook sits in LDS (at most 4096 x 4 x 4 B = 64 KiB) and is widened to fp64 on read.
//  * no L: every group on its own.  A lane owns R groups and walks all codewords in index order; every lane of a wave reads the
//    same codeword, so the LDS read is a broadcast.
//  * L: one wave per row (rows are independent inside a column block), groups from the last to the first.  The row's block
//    errors w - hat live in registers (lane l holds elements l and l + 64: blocks are at most 128 columns); the feedback dot
//    product reads one column of the L block per element, stored column-major so a wave's read is one contiguous 1 KiB line
//    pair that every row of the block shares through L2.  Lanes split the codewords (lane l: l, l + 64, ...) and the wave
//    reduces (d, index) lexicographically.
// Distance: sum over v in order of fl((t_v - c_v)^2), fp64, no fused multiply-add; strict < in index order, so ties go to the
// lowest index (CPU torch.argmin).
#include "qpal_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxBlockCols = 128;  // two error registers per lane
constexpr int kNearestThreads = 256;
constexpr int kNearestR = 4;        // groups per lane (the codeword read is shared by R distances)
constexpr int kLdlqWaves = 8;       // rows per workgroup on the L path

template <int VEC>
struct CW;
template <>
struct CW<1> {
    static __device__ __forceinline__ void get(const float *cb, int n, double *c) { c[0] = (double)cb[n]; }
};
template <>
struct CW<2> {
    static __device__ __forceinline__ void get(const float *cb, int n, double *c) {
        const float2 v = reinterpret_cast<const float2 *>(cb)[n];
        c[0] = (double)v.x;
        c[1] = (double)v.y;
    }
};
template <>
struct CW<4> {
    static __device__ __forceinline__ void get(const float *cb, int n, double *c) {
        const float4 v = reinterpret_cast<const float4 *>(cb)[n];
        c[0] = (double)v.x;
        c[1] = (double)v.y;
        c[2] = (double)v.z;
        c[3] = (double)v.w;
    }
};

template <int VEC>
__device__ __forceinline__ double dist(const double *t, const double *c) {
    double d = 0.0;
#pragma unroll
    for (int v = 0; v < VEC; ++v) {
        const double e = t[v] - c[v];
        const double s = e * e;
        d = v == 0 ? s : d + s;
    }
    return d;
}

__device__ __forceinline__ void load_codebook(float *cb, const float *__restrict__ lut, int n) {
    for (int e = threadIdx.x; e < n; e += blockDim.x) cb[e] = lut[e];
    __syncthreads();
}

template <int VEC>
__global__ __launch_bounds__(kNearestThreads) void vq_nearest_kernel(int32_t *__restrict__ idx, double *__restrict__ hat,
                                                                     const double *__restrict__ w, int ld,
                                                                     const float *__restrict__ lut, int m, int cols, int bits) {
    extern __shared__ __attribute__((aligned(16))) float cb[];
    const int N = 1 << bits;
    load_codebook(cb, lut, N * VEC);
    const int G = cols / VEC, ldi = ld / VEC;
    const long total = (long)m * G;
    const long stride = (long)gridDim.x * kNearestThreads * kNearestR;
    for (long base = (long)blockIdx.x * kNearestThreads * kNearestR + threadIdx.x; base < total; base += stride) {
        double t[kNearestR][VEC], best[kNearestR];
        int bi[kNearestR];
        long off[kNearestR];
#pragma unroll
        for (int r = 0; r < kNearestR; ++r) {
            const long q = base + (long)r * kNearestThreads;
            const long row = q / G, g = q - row * G;
            off[r] = q < total ? row * ld + g * VEC : -1;
#pragma unroll
            for (int v = 0; v < VEC; ++v) t[r][v] = off[r] >= 0 ? w[off[r] + v] : 0.0;
            best[r] = __builtin_inf();
            bi[r] = 0;
        }
#pragma unroll 4
        for (int n = 0; n < N; ++n) {
            double c[VEC];
            CW<VEC>::get(cb, n, c);
#pragma unroll
            for (int r = 0; r < kNearestR; ++r) {
                const double d = dist<VEC>(t[r], c);
                if (d < best[r]) {
                    best[r] = d;
                    bi[r] = n;
                }
            }
        }
#pragma unroll
        for (int r = 0; r < kNearestR; ++r) {
            if (off[r] < 0) continue;
            const long row = off[r] / ld, col = off[r] - row * ld;
            idx[row * ldi + col / VEC] = bi[r];
            if (hat) {
#pragma unroll
                for (int v = 0; v < VEC; ++v) hat[off[r] + v] = (double)cb[bi[r] * VEC + v];
            }
        }
    }
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

template <int VEC>
__global__ __launch_bounds__(64 * kLdlqWaves) void vq_ldlq_kernel(int32_t *__restrict__ idx, double *__restrict__ hat,
                                                                  const double *__restrict__ w, const double *__restrict__ prod,
                                                                  const double *__restrict__ lt, int ld, int ld_l,
                                                                  const float *__restrict__ lut, int m, int cols, int bits) {
    extern __shared__ __attribute__((aligned(16))) float cb[];
    const int N = 1 << bits;
    load_codebook(cb, lut, N * VEC);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int G = cols / VEC, ldi = ld / VEC;
    for (int row = blockIdx.x * kLdlqWaves + wave; row < m; row += gridDim.x * kLdlqWaves) {
        const double *wr = w + (long)row * ld;
        const double *pr = prod ? prod + (long)row * ld : nullptr;
        double e0 = 0.0, e1 = 0.0;  // w - hat of elements lane, lane + 64 (set once their group is done)
        for (int g = G - 1; g >= 0; --g) {
            const int c0 = g * VEC, lo = c0 + VEC;  // feedback from the elements of later groups in the block
            double t[VEC];
#pragma unroll
            for (int b = 0; b < VEC; ++b) {
                const double *col = lt + (long)(c0 + b) * ld_l;
                double acc = 0.0;
                if (lane >= lo && lane < cols) acc = col[lane] * e0;
                if (lane + 64 >= lo && lane + 64 < cols) acc = acc + col[lane + 64] * e1;
                acc = wave_sum(acc);
                double x = wr[c0 + b] + acc;  // (w + L^T (w - hat)) + prod, LDLQ_VQ's association
                if (pr) x = x + pr[c0 + b];
                t[b] = x;
            }
            double best = __builtin_inf();
            int bi = 0;
            for (int n = lane; n < N; n += 64) {
                double c[VEC];
                CW<VEC>::get(cb, n, c);
                const double d = dist<VEC>(t, c);
                if (d < best) {
                    best = d;
                    bi = n;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const double od = __shfl_xor(best, o);
                const int oi = __shfl_xor(bi, o);
                if (od < best || (od == best && oi < bi)) {
                    best = od;
                    bi = oi;
                }
            }
            // NaN distances never win a comparison: every lane keeps its own index.  Take lane 0's so the wave agrees.
            bi = __shfl(bi, 0);
#pragma unroll
            for (int b = 0; b < VEC; ++b) {
                const int c = c0 + b;
                const double h = (double)cb[bi * VEC + b];
                const double err = wr[c] - h;
                if (lane == (c & 63)) {
                    if (c < 64)
                        e0 = err;
                    else
                        e1 = err;
                }
                if (hat && lane == b) hat[(long)row * ld + c] = h;
            }
            if (lane == 0) idx[(long)row * ldi + g] = bi;
        }
    }
}

template <int VEC>
int launch(int32_t *idx, double *hat, const double *w, const double *prod, const double *lt, int ld, int ld_l, const float *lut,
           int m, int cols, int bits, hipStream_t stream) {
    const size_t lds = (size_t)(4 * VEC) << bits;
    if (lt) {
        const int need = (m + kLdlqWaves - 1) / kLdlqWaves;
        const int grid = need < qpal::kNumCU * 8 ? need : qpal::kNumCU * 8;
        hipLaunchKernelGGL(vq_ldlq_kernel<VEC>, dim3(grid), dim3(64 * kLdlqWaves), lds, stream, idx, hat, w, prod, lt, ld, ld_l, lut,
                           m, cols, bits);
    } else {
        const long per = (long)kNearestThreads * kNearestR;
        const long need = ((long)m * (cols / VEC) + per - 1) / per;
        const int grid = need < qpal::kNumCU * 16 ? (int)need : qpal::kNumCU * 16;
        hipLaunchKernelGGL(vq_nearest_kernel<VEC>, dim3(grid), dim3(kNearestThreads), lds, stream, idx, hat, w, ld, lut, m, cols,
                           bits);
    }
    return (int)hipGetLastError();
}

}  // namespace

extern "C" {

int qpal_vq_encode(int32_t *idx, double *hat_or_null, const double *w, const double *prod_or_null, const double *lt_or_null, int ld,
                   int ld_l, const float *lut, int m, int cols, int bits, int vec, void *stream) {
    if (!idx || !w || !lut) return QPAL_E_NULL;
    if (!lt_or_null && prod_or_null) return QPAL_E_NULL;  // prod belongs to the feedback path
    if ((vec != 1 && vec != 2 && vec != 4) || bits < 1 || bits > 12) return QPAL_E_PARAM;
    if (m < 1 || cols < vec || cols % vec || ld < cols || ld % vec) return QPAL_E_SHAPE;
    if (lt_or_null && (cols > kMaxBlockCols || ld_l < cols)) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(idx) & 3) || (reinterpret_cast<uintptr_t>(hat_or_null) & 7) ||
        (reinterpret_cast<uintptr_t>(w) & 7) || (reinterpret_cast<uintptr_t>(prod_or_null) & 7) ||
        (reinterpret_cast<uintptr_t>(lt_or_null) & 7) || (reinterpret_cast<uintptr_t>(lut) & 3))
        return QPAL_E_ALIGN;
    hipStream_t s = static_cast<hipStream_t>(stream);
    switch (vec) {
        case 1: return launch<1>(idx, hat_or_null, w, prod_or_null, lt_or_null, ld, ld_l, lut, m, cols, bits, s);
        case 2: return launch<2>(idx, hat_or_null, w, prod_or_null, lt_or_null, ld, ld_l, lut, m, cols, bits, s);
        default: return launch<4>(idx, hat_or_null, w, prod_or_null, lt_or_null, ld, ld_l, lut, m, cols, bits, s);
    }
}

}  // extern "C"
