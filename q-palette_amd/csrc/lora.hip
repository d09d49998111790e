// Multi-adapter low-rank update (include/qpal.h: qpal_lora_apply):  out[i] += B[a] (A[a] xin[i]),  a = row_adapter[i],
// shrink and expand of one projection group (up to 3 column blocks) in ONE launch, no workspace, no atomics.
//
// One workgroup of 16 waves owns (row i, block p, column split s).  It leaves at once when the row has no adapter or the split has
// no columns.  Otherwise:
//   stage   the row's input under in_mode goes to LDS as fp32 (xs[k]): fp16 widened, fp32 as is or times the RMSNorm weight (the
//           sum of squares is taken in the same pass; the factor rsqrt(mean + eps) multiplies t, the shrink being linear), or
//           silu(gate) * up.  Nothing is rounded to fp16.
//   shrink  t[r] = sum_l A[a][p R + r][l] xs[l].  The work is cut into items of 8 rows of A x 64 chunks of 8 elements; wave w takes
//           items w, w + 16, ...: lane l one 16-byte load per row of A and 64 fp32 fmas, then a 6-step butterfly over the wave, and
//           lane r keeps the wave's running sum of row r.  The loads of the next item (and of the first one, ahead of the staging)
//           are issued before the current item is summed.  The 16 wave sums are added in wave order.  Every split of a block
//           recomputes t from L2: R k 2 bytes of A, no grid-wide wait.
//   expand  thread j of the split owns column j: sum_r B[a][boff_p + j][r] t[r] (R / 8 16-byte loads, the first column's issued
//           before t is complete), one fp32 read-modify-write.
// The thread -> element maps depend on nothing but (k, R): a row's bits depend on its input, its adapter and its out value only,
// and equal launches give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "launch.h"
#include "qpal.h"

namespace qpal {
namespace lora {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxR = 64, kMaxK = 32768, kMaxP = 3;
constexpr int kLdsTail = kWaves * kMaxR + kMaxR + kWaves;  // floats behind xs: wave partials, t, sums of squares

struct Params {
    float *out;
    long ld_out;
    const void *in;
    const _Float16 *rms_w;
    const _Float16 *A, *B;
    const int *row_adapter;
    float rms_eps;
    int k, R, N, P, m_total, cps;  // cps: columns per split (a multiple of 16)
    int blk_off[kMaxP], blk_m[kMaxP], boff[kMaxP];
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <int MODE, bool RMS>
__global__ __launch_bounds__(kThreads) void lora_kernel(const Params p) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int row = (int)blockIdx.z, pb = (int)blockIdx.y, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = p.row_adapter[row];
    if (a < 0 || a >= p.N) return;  // no adapter: none of the row's bytes are written
    const int m = p.blk_m[pb], j0 = (int)blockIdx.x * p.cps;
    if (j0 >= m) return;
    const int j1 = min(m, j0 + p.cps);
    const int k = p.k, R = p.R, nchunk = k >> 3;
    float *xs = sm, *part = sm + k, *tt = part + kWaves * kMaxR, *red = tt + kMaxR;

    // the rows of A of item `it`: rows 8 rg .. 8 rg + 7 of the block, chunk 64 cg + lane (clamped into k)
    const _Float16 *Ap = p.A + ((size_t)a * p.P + pb) * (size_t)R * k;
    auto loadA = [&](int item, half8_t (&av)[8]) {
        const int nrg_ = R >> 3, rg = item % nrg_, c = min((item / nrg_) * 64 + lane, nchunk - 1);
#pragma unroll
        for (int j = 0; j < 8; j++) av[j] = *reinterpret_cast<const half8_t *>(Ap + (size_t)(8 * rg + j) * k + 8 * c);
    };
    half8_t cur[8];
    loadA(wave, cur);  // (every wave has a first item, or a valid address to read: item % nrg and the clamp keep it inside A)

    // ---- stage: the row's input as fp32
    float ss = 0.0f;
    for (int c = tid; c < nchunk; c += kThreads) {
        f32x4_t lo, hi;
        if constexpr (MODE == QPAL_IN_F16) {
            const half8_t h = *reinterpret_cast<const half8_t *>(static_cast<const _Float16 *>(p.in) + (size_t)row * k + 8 * c);
            lo = f32x4_t{(float)h[0], (float)h[1], (float)h[2], (float)h[3]};
            hi = f32x4_t{(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
        } else if constexpr (MODE == QPAL_IN_F32) {
            const f32x4_t *x = reinterpret_cast<const f32x4_t *>(static_cast<const float *>(p.in) + (size_t)row * k + 8 * c);
            lo = x[0];
            hi = x[1];
            if constexpr (RMS) {
#pragma unroll
                for (int e = 0; e < 4; e++) ss = fmaf(lo[e], lo[e], ss);
#pragma unroll
                for (int e = 0; e < 4; e++) ss = fmaf(hi[e], hi[e], ss);
                if (p.rms_w) {
                    const half8_t w = *reinterpret_cast<const half8_t *>(p.rms_w + 8 * c);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        lo[e] *= (float)w[e];
                        hi[e] *= (float)w[4 + e];
                    }
                }
            }
        } else {
            const float *u = static_cast<const float *>(p.in) + (size_t)row * 2 * k + 8 * c;
            const f32x4_t *up = reinterpret_cast<const f32x4_t *>(u), *gt = reinterpret_cast<const f32x4_t *>(u + k);
            const f32x4_t u0 = up[0], u1 = up[1], g0 = gt[0], g1 = gt[1];
#pragma unroll
            for (int e = 0; e < 4; e++) {
                lo[e] = g0[e] / (1.0f + expf(-g0[e])) * u0[e];
                hi[e] = g1[e] / (1.0f + expf(-g1[e])) * u1[e];
            }
        }
        reinterpret_cast<f32x4_t *>(xs)[2 * c] = lo;
        reinterpret_cast<f32x4_t *>(xs)[2 * c + 1] = hi;
    }
    if constexpr (RMS) {
        ss = wave_sum(ss);
        if (lane == 0) red[wave] = ss;
    }
    __syncthreads();

    // ---- shrink
    const int nrg = R >> 3, nitems = nrg * ((nchunk + 63) >> 6);
    float mine = 0.0f;  // lane r: this wave's part of t[r]
    int it = wave;
    while (it < nitems) {
        const int nx = it + kWaves;
        half8_t nxt[8];
        if (nx < nitems) loadA(nx, nxt);
        else
#pragma unroll
            for (int j = 0; j < 8; j++) nxt[j] = cur[j];  // (no next item: nothing is read from it)
        const int rg = it % nrg, c = (it / nrg) * 64 + lane;
        f32x4_t lo = {0, 0, 0, 0}, hi = {0, 0, 0, 0};  // chunks past the end of k count as zeros (their loads were clamped)
        if (c < nchunk) {
            lo = reinterpret_cast<const f32x4_t *>(xs)[2 * c];
            hi = reinterpret_cast<const f32x4_t *>(xs)[2 * c + 1];
        }
#pragma unroll
        for (int j = 0; j < 8; j++) {
            float acc = 0.0f;
#pragma unroll
            for (int e = 0; e < 4; e++) acc = fmaf((float)cur[j][e], lo[e], acc);
#pragma unroll
            for (int e = 0; e < 4; e++) acc = fmaf((float)cur[j][4 + e], hi[e], acc);
            acc = wave_sum(acc);
            if (lane == 8 * rg + j) mine += acc;
        }
#pragma unroll
        for (int j = 0; j < 8; j++) cur[j] = nxt[j];
        it = nx;
    }
    if (lane < R) part[wave * kMaxR + lane] = mine;

    // the first column of this thread: its row of B and its out value are on their way while t is completed
    const _Float16 *Bp = p.B + ((size_t)a * p.m_total + p.boff[pb]) * (size_t)R;
    float *o = p.out + (size_t)row * (size_t)p.ld_out + p.blk_off[pb];
    const int jf = j0 + tid;
    half8_t bf[8];
    float old = 0.0f;
    if (jf < j1) {
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (8 * q < R) bf[q] = *reinterpret_cast<const half8_t *>(Bp + (size_t)jf * R + 8 * q);
        old = o[jf];
    }
    __syncthreads();
    if (tid < R) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < kWaves; w++) s += part[w * kMaxR + tid];
        if constexpr (RMS) {
            float q = 0.0f;
#pragma unroll
            for (int w = 0; w < kWaves; w++) q += red[w];
            s *= 1.0f / sqrtf(q / (float)k + p.rms_eps);
        }
        tt[tid] = s;
    }
    __syncthreads();

    // ---- expand: one thread per column, one owner per element of out
    if (jf < j1) {
        float s = 0.0f;
#pragma unroll
        for (int q = 0; q < 8; q++)
            if (8 * q < R) {
#pragma unroll
                for (int e = 0; e < 8; e++) s = fmaf((float)bf[q][e], tt[8 * q + e], s);
            }
        o[jf] = old + s;
    }
    for (int j = jf + kThreads; j < j1; j += kThreads) {
        const _Float16 *b = Bp + (size_t)j * R;
        float s = 0.0f;
        for (int r = 0; r < R; r += 8) {
            const half8_t bv = *reinterpret_cast<const half8_t *>(b + r);
#pragma unroll
            for (int e = 0; e < 8; e++) s = fmaf((float)bv[e], tt[r + e], s);
        }
        o[j] += s;
    }
}

}  // namespace lora
}  // namespace qpal

using namespace qpal::lora;

template <int MODE, bool RMS>
static int launch(const Params &p, dim3 grid, size_t lds, hipStream_t stream) {
    return qpal::launch_lds<lora_kernel<MODE, RMS>>(grid, dim3(kThreads), lds, (kMaxK + kLdsTail) * 4, stream, p);
}

extern "C" int qpal_lora_apply(float *out, long ld_out, const void *in, int in_mode, float rms_eps, const void *rms_weight,
                               const void *A, const void *B, const int *blk_off, const int *blk_m, int P, const int *row_adapter,
                               int rows, int k, int R, int N, void *stream) {
    if (!out || !in || !A || !B || !blk_off || !blk_m || !row_adapter) return QPAL_E_NULL;
    if (rows < 1 || rows > 128 || R < 8 || R > kMaxR || R % 8 || P < 1 || P > kMaxP || k < 64 || k > kMaxK || k % 64 || N < 1)
        return QPAL_E_SHAPE;
    if (in_mode != QPAL_IN_F16 && in_mode != QPAL_IN_F32 && in_mode != QPAL_IN_SWIGLU_F32) return QPAL_E_PARAM;
    const bool rms = rms_eps >= 0.0f;  // (false for NaN too)
    if (in_mode != QPAL_IN_F32 && (rms || rms_weight)) return QPAL_E_PARAM;  // the norm is defined on fp32 rows only
    if (!rms && rms_weight) return QPAL_E_PARAM;
    Params p;
    long m_total = 0, m_max = 0;
    for (int b = 0; b < P; b++) {
        if (blk_m[b] < 16 || blk_m[b] % 16 || blk_off[b] < 0 || (long)blk_off[b] + blk_m[b] > ld_out) return QPAL_E_SHAPE;
        for (int c = 0; c < b; c++)  // one owner per element of out: the blocks' columns must not meet
            if (blk_off[b] < blk_off[c] + blk_m[c] && blk_off[c] < blk_off[b] + blk_m[b]) return QPAL_E_SHAPE;
        p.blk_off[b] = blk_off[b];
        p.blk_m[b] = blk_m[b];
        p.boff[b] = (int)m_total;
        m_total += blk_m[b];
        m_max = blk_m[b] > m_max ? blk_m[b] : m_max;
    }
    for (int b = P; b < kMaxP; b++) p.blk_off[b] = p.blk_m[b] = p.boff[b] = 0;
    if ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(A) | reinterpret_cast<uintptr_t>(B) |
         reinterpret_cast<uintptr_t>(rms_weight)) & 15)
        return QPAL_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(row_adapter)) & 3) return QPAL_E_ALIGN;
    {   // out must not overlap in (the launch reads rows of `in` that other workgroups' columns of `out` would change)
        const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + ((size_t)(rows - 1) * (size_t)ld_out + (size_t)ld_out) * 4;
        const size_t in_row = in_mode == QPAL_IN_F16 ? (size_t)k * 2 : in_mode == QPAL_IN_F32 ? (size_t)k * 4 : (size_t)k * 8;
        const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), i1 = i0 + (size_t)rows * in_row;
        if (o0 < i1 && i0 < o1) return QPAL_E_PARAM;
    }
    p.out = out;
    p.ld_out = ld_out;
    p.in = in;
    p.rms_w = static_cast<const _Float16 *>(rms_weight);
    p.A = static_cast<const _Float16 *>(A);
    p.B = static_cast<const _Float16 *>(B);
    p.row_adapter = row_adapter;
    p.rms_eps = rms_eps;
    p.k = k, p.R = R, p.N = N, p.P = P, p.m_total = (int)m_total;
    // Columns per split.  Every split repeats the shrink (R k MACs, R k 2 bytes of A from L2), so splits only pay while the launch
    // has fewer workgroups than the chip has CUs: about 512 workgroups over all rows, 256 .. 4096 columns each.
    long cps = (m_total * rows / 512 + 15) & ~15L;
    cps = cps < 256 ? 256 : cps > 4096 ? 4096 : cps;
    p.cps = (int)cps;
    const dim3 grid((unsigned)((m_max + cps - 1) / cps), (unsigned)P, (unsigned)rows);
    const size_t lds = ((size_t)k + kLdsTail) * 4;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (in_mode == QPAL_IN_F16) return launch<QPAL_IN_F16, false>(p, grid, lds, s);
    if (in_mode == QPAL_IN_SWIGLU_F32) return launch<QPAL_IN_SWIGLU_F32, false>(p, grid, lds, s);
    return rms ? launch<QPAL_IN_F32, true>(p, grid, lds, s) : launch<QPAL_IN_F32, false>(p, grid, lds, s);
}
