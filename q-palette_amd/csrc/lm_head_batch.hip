// qpal_lm_head_logits: final RMSNorm + fp16 lm_head for up to 128 rows of the residual stream, on the matrix pipe.  The tail of a
// decode step at batch B (and of a sampled step at batch 1): as torch ops it is a norm (3 launches) and a hipBLASLt GEMM.
//
// The lm_head (vocab x k fp16: 1.05 GB for Llama-3.1-8B) is read from HBM once for all rows.  Workgroup = 16 waves = 256
// consecutive vocab rows; a wave owns 16 of them as the A side of v_mfma_f32_16x16x32_f16 and walks k in stages of 256 columns:
// its 16 x 256 weight block of the NEXT stage is requested (8 x 16 bytes per lane, non-temporal) before the current one is
// multiplied.  The B side is the normalised x: every stage the workgroup writes x[rows][256] as fp16 into LDS (rows padded to a
// multiple of 16 with ZEROS), each 16-row tile one MFMA column block.  Row stride 264 halves: the 16 lanes of an
// MFMA row group read 16 bytes each from 16 different bank quads.  D[weight row 4 q + r][batch row i] lands in lane (q, i): one
// writer per logit, no workspace, no atomics.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "qpal_common.h"

namespace qpal {

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float float4_t __attribute__((ext_vector_type(4)));

struct LmLogitsParams {
    const float *h;          // fp32 [rows][ld_h]
    long ld_h;
    const uint16_t *rms_w;   // fp16 [k] or null (w = 1)
    float rms_eps;           // 0: no norm (x = fp16(h), rms_w null)
    const uint16_t *w;       // fp16 [vocab][k]
    float *logits;           // fp32 [rows][ld_logits]
    long ld_logits;
    int rows, vocab, k;
};

constexpr int kLmStage = 256;              // columns of k per LDS stage
constexpr int kLmStride = kLmStage + 8;    // halves per staged row

template <int NBT>  // 16-row tiles of the batch: ceil(rows / 16)
__global__ __launch_bounds__(1024) void lm_head_logits_kernel(const LmLogitsParams p) {
    extern __shared__ __attribute__((aligned(16))) float lm_sh[];  // 1 / rms [NBT * 16] | x [NBT * 16][kLmStride] fp16
    float *inv_s = lm_sh;
    uint16_t *xs = reinterpret_cast<uint16_t *>(lm_sh + NBT * 16);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = p.k, nbt = NBT;
    // ---- 1 / rms of every row (every workgroup for itself: the rows come from L2)
    for (int r = wave; r < nbt * 16; r += 16) {
        float ss = 0.f;
        if (r < p.rows && p.rms_eps > 0.f) {
            const float *hr = p.h + (long)r * p.ld_h;
            for (int i = 4 * lane; i < k; i += 256) {
                const float4 v = *reinterpret_cast<const float4 *>(hr + i);
                ss += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
            }
        }
        ss = wave_sum(ss);
        if (lane == 0) inv_s[r] = p.rms_eps > 0.f ? __builtin_amdgcn_rsqf(ss / (float)k + p.rms_eps) : 1.0f;
    }
    // rows that do not exist: zeros, written once (no stage touches them)
    for (int i = tid; i < (nbt * 16 - p.rows) * (kLmStride / 2); i += 1024)
        reinterpret_cast<uint32_t *>(xs + p.rows * kLmStride)[i] = 0u;
    __syncthreads();

    const int mi = lane & 15, mq = lane >> 4;
    const int v0 = (blockIdx.x * 16 + wave) * 16;
    const bool act = v0 < p.vocab;  // (wave-uniform) a wave past the last vocab row only helps staging
    const int wr = v0 + mi < p.vocab ? v0 + mi : p.vocab - 1;
    const gptr<const uint16_t> wrow = as_global(p.w) + (long)wr * k + 8 * mq;
    float4_t acc[NBT];
#pragma unroll
    for (int t = 0; t < NBT; t++) acc[t] = float4_t{0.f, 0.f, 0.f, 0.f};
    u32x4 wcur[8], wnext[8];
#pragma unroll
    for (int kc = 0; kc < 8; kc++) wcur[kc] = wnext[kc] = u32x4{0u, 0u, 0u, 0u};
    if (act) {
#pragma unroll
        for (int kc = 0; kc < 8; kc++) wcur[kc] = __builtin_nontemporal_load((gptr<const u32x4>)(wrow + 32 * kc));
    }
    const int srow = tid >> 6, scol = 4 * (tid & 63);  // staging: 64 threads a row, 4 columns each
    const int nstage = k / kLmStage;
    // x of stage c: fp16(h * inv) [* rms_w in fp16], the arithmetic of lm_head_argmax_kernel
    auto stage_x = [&](const int c) {
        for (int r = srow; r < p.rows; r += 16) {
            const int col = c * kLmStage + scol;
            const float4 v = *reinterpret_cast<const float4 *>(p.h + (long)r * p.ld_h + col);
            const float inv = inv_s[r];
            _Float16 x0 = (_Float16)(v.x * inv), x1 = (_Float16)(v.y * inv), x2 = (_Float16)(v.z * inv), x3 = (_Float16)(v.w * inv);
            if (p.rms_w) {
                const uint16_t *wp = p.rms_w + col;
                x0 = x0 * __builtin_bit_cast(_Float16, wp[0]);
                x1 = x1 * __builtin_bit_cast(_Float16, wp[1]);
                x2 = x2 * __builtin_bit_cast(_Float16, wp[2]);
                x3 = x3 * __builtin_bit_cast(_Float16, wp[3]);
            }
            u32x2 o;
            o.x = __builtin_bit_cast(uint32_t, h2_t{x0, x1});
            o.y = __builtin_bit_cast(uint32_t, h2_t{x2, x3});
            *reinterpret_cast<u32x2 *>(xs + r * kLmStride + scol) = o;
        }
    };
    auto multiply = [&]() {
#pragma unroll
        for (int kc = 0; kc < 8; kc++) {
            const half8_t a = __builtin_bit_cast(half8_t, wcur[kc]);
#pragma unroll
            for (int t = 0; t < NBT; t++) {
                const u32x4 b = *reinterpret_cast<const u32x4 *>(xs + (t * 16 + mi) * kLmStride + 32 * kc + 8 * mq);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, __builtin_bit_cast(half8_t, b), acc[t], 0, 0, 0);
                // (at most four x fragments in flight: weights of two stages + 32 accumulators leave room for no more)
                if ((t & 3) == 3) __builtin_amdgcn_sched_barrier(0);
            }
        }
    };
    // every stage but the last requests the next stage's weights before it multiplies (the last one stands apart so that the
    // multiply of a prefetching stage waits for ITS weights only, with the eight younger loads still in flight)
    for (int c = 0; c + 1 < nstage; c++) {
        stage_x(c);
        __syncthreads();
        if (act) {
#pragma unroll
            for (int kc = 0; kc < 8; kc++)
                wnext[kc] = __builtin_nontemporal_load((gptr<const u32x4>)(wrow + (c + 1) * kLmStage + 32 * kc));
            multiply();
#pragma unroll
            for (int kc = 0; kc < 8; kc++) wcur[kc] = wnext[kc];
        }
        __syncthreads();
    }
    stage_x(nstage - 1);
    __syncthreads();
    if (!act) return;
    multiply();
    // ---- lane (mq, mi): logits of vocab rows v0 + 4 mq + r for batch row 16 t + mi
#pragma unroll
    for (int t = 0; t < NBT; t++) {
        const int b = t * 16 + mi;
        if (b < p.rows) {
            float *dst = p.logits + (long)b * p.ld_logits + v0 + 4 * mq;
#pragma unroll
            for (int r = 0; r < 4; r++)
                if (v0 + 4 * mq + r < p.vocab) dst[r] = acc[t][r];
        }
    }
}

}  // namespace qpal

using namespace qpal;

static size_t lm_logits_lds(int nbt) { return (size_t)nbt * 16 * (sizeof(float) + kLmStride * sizeof(uint16_t)); }

extern "C" int qpal_lm_head_logits(const float *h_f32, long ld_h, const void *rms_w_f16, float rms_eps, const void *w_f16,
                                   float *logits_f32, long ld_logits, int rows, int vocab, int k, void *stream) {
    if (!h_f32 || !w_f16 || !logits_f32) return QPAL_E_NULL;
    if (rows < 1 || rows > 128 || vocab < 1 || k < 512 || k > 8192 || k % 512 || ld_h < k || ld_logits < vocab) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(w_f16) & 15) || (reinterpret_cast<uintptr_t>(h_f32) & 15) || (rows > 1 && ld_h % 4) ||
        (reinterpret_cast<uintptr_t>(logits_f32) & 3) || (rms_w_f16 && (reinterpret_cast<uintptr_t>(rms_w_f16) & 7)))
        return QPAL_E_ALIGN;
    const bool norm = rms_eps > 0.f;  // no weight: w = 1, as in qpal_lm_head_argmax, x_rms and qpal_hadamard_rms
    LmLogitsParams p{h_f32, ld_h, norm ? static_cast<const uint16_t *>(rms_w_f16) : nullptr, norm ? rms_eps : 0.f,
                     static_cast<const uint16_t *>(w_f16), logits_f32, ld_logits, rows, vocab, k};
    const int grid = (vocab + 255) / 256;
    switch ((rows + 15) / 16) {
    // (128 rows: 66 KiB of LDS)
#define QPAL_LM_LOGITS(N_)                                                                                                  \
    case N_:                                                                                                                \
        return launch_lds<lm_head_logits_kernel<N_>>(dim3(grid), dim3(1024), lm_logits_lds(N_), (int)lm_logits_lds(N_), \
                                                     static_cast<hipStream_t>(stream), p);
        QPAL_LM_LOGITS(1) QPAL_LM_LOGITS(2) QPAL_LM_LOGITS(3) QPAL_LM_LOGITS(4)
        QPAL_LM_LOGITS(5) QPAL_LM_LOGITS(6) QPAL_LM_LOGITS(7) QPAL_LM_LOGITS(8)
#undef QPAL_LM_LOGITS
    }
    return QPAL_E_SHAPE;
}
