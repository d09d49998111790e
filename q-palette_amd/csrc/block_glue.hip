// The glue of Qwen- and Gemma-shaped blocks between the existing launches of a step (blocks.py restates every rule in
// numpy float64).  All four work on fp32 rows that are already in memory, are one launch each and never synchronise.
//
//   qkv_prep_kernel<VEC>   one wave per (row, head) of q | k | v, four heads per workgroup, no LDS: lane l holds elements l, l + 64, ..
//                          of the head (VEC = hd / 64 coalesced dwords), adds the bias, and for q and k heads with norm weights
//                          reduces the sum of squares over the wave and scales by rsqrt(mean + eps) * w.  In place.
//   norm_add_kernel        one workgroup of 256 threads per row: float4 pass over y for the sum of squares (wave sums, then four
//                          partials through LDS), second pass h += y * inv * w (y comes from L2 the second time: n <= 16384).
//   glu_gelu_kernel        grid (tiles of 1024 columns, rows): act = gelu_tanh(gate) * up on float4s.
//   logit_cap_kernel       grid (tiles of 4096 logits, rows): l <- cap * tanh(l / cap) in place, float4s where the row allows.
// Both tanh users go through attn_common.h's soft_cap(): the clamped exp / rcp form whose error §32.2 states.
#include <hip/hip_runtime.h>

#include <cmath>

#include "attn_common.h"
#include "qpal_common.h"

namespace qpal {

namespace {

constexpr int kGlueThreads = 256, kGlueWaves = kGlueThreads / kWave;
constexpr int kGlueMaxRows = 65535;      // rows of one launch: a grid dimension (the steps have at most 128)
constexpr int kNormAddMaxN = 16384;
constexpr int kCapTile = kGlueThreads * 4 * 4;  // four float4 groups per thread

struct QkvPrepParams {
    float *q, *k, *v;
    long ld;
    int rows, nq, nkv, heads;  // heads: the heads of a row the launch visits (nq + nkv, + nkv more with a bias)
    const float *bias, *q_w, *k_w;
    float eps;
};

template <int VEC>
__global__ __launch_bounds__(kGlueThreads) void qkv_prep_kernel(const QkvPrepParams p) {
    constexpr int HD = VEC * kWave;
    const int lane = threadIdx.x & (kWave - 1);
    const long item = (long)blockIdx.x * kGlueWaves + (threadIdx.x >> 6);  // uniform in the wave
    if (item >= (long)p.rows * p.heads) return;
    const int r = (int)(item / p.heads), h = (int)(item % p.heads);
    float *base;
    const float *w;
    int hh;
    if (h < p.nq) {
        base = p.q, w = p.q_w, hh = h;
    } else if (h < p.nq + p.nkv) {
        base = p.k, w = p.k_w, hh = h - p.nq;
    } else {
        base = p.v, w = nullptr, hh = h - p.nq - p.nkv;
    }
    float *x = base + (long)r * p.ld + (long)hh * HD + lane;
    float t[VEC];
#pragma unroll
    for (int e = 0; e < VEC; e++) t[e] = x[e * kWave];
    if (p.bias) {
        const float *b = p.bias + (long)h * HD + lane;  // q | k | v order: head h of the row's nq + 2 nkv
#pragma unroll
        for (int e = 0; e < VEC; e++) t[e] += b[e * kWave];
    }
    if (w) {
        float ss = 0.f;
#pragma unroll
        for (int e = 0; e < VEC; e++) ss += t[e] * t[e];
        ss = wave_sum(ss);
        const float inv = rsqrtf(ss * (1.f / HD) + p.eps);  // a zero head: rsqrt(eps), finite, and 0 * inv * w = 0
#pragma unroll
        for (int e = 0; e < VEC; e++) t[e] = (t[e] * inv) * w[lane + e * kWave];
    }
#pragma unroll
    for (int e = 0; e < VEC; e++) x[e * kWave] = t[e];
}

struct NormAddParams {
    float *h;
    long ld_h;
    const float *y;
    long ld_y;
    const float *w;
    float eps;
    int n;
};

__global__ __launch_bounds__(kGlueThreads) void norm_add_kernel(const NormAddParams p) {
    __shared__ float s_part[kGlueWaves];
    const int tid = threadIdx.x, n4 = p.n >> 2;
    const float4 *y = reinterpret_cast<const float4 *>(p.y + (long)blockIdx.x * p.ld_y);
    float4 *h = reinterpret_cast<float4 *>(p.h + (long)blockIdx.x * p.ld_h);
    const float4 *w = reinterpret_cast<const float4 *>(p.w);
    float ss = 0.f;
    for (int j = tid; j < n4; j += kGlueThreads) {
        const float4 t = y[j];
        ss += (t.x * t.x + t.y * t.y) + (t.z * t.z + t.w * t.w);
    }
    ss = wave_sum(ss);
    if ((tid & (kWave - 1)) == 0) s_part[tid >> 6] = ss;
    __syncthreads();
    ss = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    const float inv = rsqrtf(ss / (float)p.n + p.eps);
    for (int j = tid; j < n4; j += kGlueThreads) {
        const float4 t = y[j], g = w[j];
        float4 o = h[j];
        o.x += (t.x * inv) * g.x;
        o.y += (t.y * inv) * g.y;
        o.z += (t.z * inv) * g.z;
        o.w += (t.w * inv) * g.w;
        h[j] = o;
    }
}

// gelu_tanh(g) = 0.5 g (1 + tanh(sqrt(2 / pi) (g + 0.044715 g^3)))
__device__ __forceinline__ float gelu_tanh(float g) {
    const float t = 0.7978845608f * (g + 0.044715f * (g * g * g));
    return (0.5f * g) * (1.f + soft_cap(t, 1.f, 1.f));
}

struct GluParams {
    float *act;
    long ld_act;
    const float *ug;
    long ld_ug;
    int inter;
};

__global__ __launch_bounds__(kGlueThreads) void glu_gelu_kernel(const GluParams p) {
    const int j = blockIdx.x * kGlueThreads + threadIdx.x;  // the float4 group of the row
    if (4 * j >= p.inter) return;
    const float *row = p.ug + (long)blockIdx.y * p.ld_ug;
    const float4 u = reinterpret_cast<const float4 *>(row)[j];
    const float4 g = reinterpret_cast<const float4 *>(row + p.inter)[j];
    reinterpret_cast<float4 *>(p.act + (long)blockIdx.y * p.ld_act)[j] =
        make_float4(gelu_tanh(g.x) * u.x, gelu_tanh(g.y) * u.y, gelu_tanh(g.z) * u.z, gelu_tanh(g.w) * u.w);
}

struct CapParams {
    float *logits;
    long ld;
    int vocab;
    float cap, inv_cap;
};

__global__ __launch_bounds__(kGlueThreads) void logit_cap_kernel(const CapParams p) {
    float *row = p.logits + (long)blockIdx.y * p.ld;
    const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
    const int base = blockIdx.x * kCapTile;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const int i0 = base + g * (kGlueThreads * 4) + 4 * threadIdx.x;
        if (vec && i0 + 4 <= p.vocab) {
            float4 t = *reinterpret_cast<float4 *>(row + i0);
            t.x = soft_cap(t.x, p.cap, p.inv_cap);
            t.y = soft_cap(t.y, p.cap, p.inv_cap);
            t.z = soft_cap(t.z, p.cap, p.inv_cap);
            t.w = soft_cap(t.w, p.cap, p.inv_cap);
            *reinterpret_cast<float4 *>(row + i0) = t;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (i0 + e < p.vocab) row[i0 + e] = soft_cap(row[i0 + e], p.cap, p.inv_cap);
        }
    }
}

inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }
inline bool eps_ok(float eps) { return eps > 0.f && eps <= 3.0e38f; }  // (a NaN fails the first comparison)

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" int qpal_qkv_prep(float *q, float *k, float *v, long ld, int rows, int nq, int nkv, int hd, const float *bias,
                             const float *q_norm_w, const float *k_norm_w, float eps, void *stream) {
    if (!q || !k || !v) return QPAL_E_NULL;
    if ((q_norm_w == nullptr) != (k_norm_w == nullptr)) return QPAL_E_PARAM;
    if (hd != 64 && hd != 128 && hd != 256) return QPAL_E_SHAPE;
    if (rows < 0 || rows > kGlueMaxRows || nq < 1 || nkv < 1 || nq > 1024 || nkv > 1024 || ld < (long)nq * hd) return QPAL_E_SHAPE;
    if (q_norm_w && !eps_ok(eps)) return QPAL_E_PARAM;
    if (misaligned(q, 4) || misaligned(k, 4) || misaligned(v, 4) || misaligned(bias, 4) || misaligned(q_norm_w, 4) || misaligned(k_norm_w, 4))
        return QPAL_E_ALIGN;
    if (rows == 0 || (!bias && !q_norm_w)) return QPAL_OK;  // nothing to do: nothing is launched
    const int heads = nq + nkv + (bias ? nkv : 0);           // v is visited for its bias only
    QkvPrepParams p{q, k, v, ld, rows, nq, nkv, heads, bias, q_norm_w, k_norm_w, eps};
    const dim3 grid((unsigned)(((long)rows * heads + kGlueWaves - 1) / kGlueWaves));
    const hipStream_t s = static_cast<hipStream_t>(stream);
    if (hd == 64) hipLaunchKernelGGL(qkv_prep_kernel<1>, grid, dim3(kGlueThreads), 0, s, p);
    else if (hd == 128) hipLaunchKernelGGL(qkv_prep_kernel<2>, grid, dim3(kGlueThreads), 0, s, p);
    else hipLaunchKernelGGL(qkv_prep_kernel<4>, grid, dim3(kGlueThreads), 0, s, p);
    return (int)hipGetLastError();
}

extern "C" int qpal_norm_add(float *h, long ld_h, const float *y, long ld_y, const float *w, float eps, int rows, int n, void *stream) {
    if (!h || !y || !w) return QPAL_E_NULL;
    if (rows < 0 || rows > kGlueMaxRows || n < 4 || n % 4 || n > kNormAddMaxN || ld_h < n || ld_y < n) return QPAL_E_SHAPE;
    if (!eps_ok(eps)) return QPAL_E_PARAM;
    if (misaligned(h, 16) || misaligned(y, 16) || misaligned(w, 16) || ld_h % 4 || ld_y % 4) return QPAL_E_ALIGN;
    // h and y are different rows: an overlap would let one thread read what another has already updated
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(h), b0 = reinterpret_cast<uintptr_t>(y);
    if (rows > 0 && a0 < b0 + 4 * ((uintptr_t)(rows - 1) * ld_y + n) && b0 < a0 + 4 * ((uintptr_t)(rows - 1) * ld_h + n)) return QPAL_E_PARAM;
    if (rows == 0) return QPAL_OK;
    NormAddParams p{h, ld_h, y, ld_y, w, eps, n};
    hipLaunchKernelGGL(norm_add_kernel, dim3((unsigned)rows), dim3(kGlueThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_glu_gelu_tanh(float *act, long ld_act, const float *ug, long ld_ug, int rows, int inter, void *stream) {
    if (!act || !ug) return QPAL_E_NULL;
    if (rows < 0 || rows > kGlueMaxRows || inter < 4 || inter % 4 || inter > (1 << 24) || ld_act < inter || ld_ug < 2L * inter) return QPAL_E_SHAPE;
    if (misaligned(act, 16) || misaligned(ug, 16) || ld_act % 4 || ld_ug % 4) return QPAL_E_ALIGN;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(act), b0 = reinterpret_cast<uintptr_t>(ug);
    if (rows > 0 && a0 < b0 + 4 * ((uintptr_t)(rows - 1) * ld_ug + 2 * (uintptr_t)inter) && b0 < a0 + 4 * ((uintptr_t)(rows - 1) * ld_act + inter))
        return QPAL_E_PARAM;
    if (rows == 0) return QPAL_OK;
    GluParams p{act, ld_act, ug, ld_ug, inter};
    const dim3 grid((unsigned)((inter / 4 + kGlueThreads - 1) / kGlueThreads), (unsigned)rows);
    hipLaunchKernelGGL(glu_gelu_kernel, grid, dim3(kGlueThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_logit_cap(float *logits, long ld, int rows, int vocab, float cap, void *stream) {
    if (!logits) return QPAL_E_NULL;
    if (rows < 0 || rows > kGlueMaxRows || vocab < 1 || vocab > (1 << 30) || ld < vocab) return QPAL_E_SHAPE;
    if (!(cap > 0.f && cap <= 3.0e38f)) return QPAL_E_PARAM;
    if (misaligned(logits, 4)) return QPAL_E_ALIGN;
    if (rows == 0) return QPAL_OK;
    CapParams p{logits, ld, vocab, cap, 1.f / cap};
    const dim3 grid((unsigned)(((long)vocab + kCapTile - 1) / kCapTile), (unsigned)rows);
    hipLaunchKernelGGL(logit_cap_kernel, grid, dim3(kGlueThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
