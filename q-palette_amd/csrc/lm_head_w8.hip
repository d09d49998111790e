// qpal_lm_head_w8: final RMSNorm + an 8-bit lm_head (OCP e4m3fn bytes, one fp32 scale per vocab row) for up to 128 rows of the
// residual stream, logits and / or the greedy token of every row in ONE launch; qpal_embed_rows_w8: the gather from such a table
// (DESIGN.md §38).
//
// Workgroup = 8 waves = 256 consecutive vocab rows.  A wave owns TWO 16-row weight tiles (32 vocab rows) as the A side of
// v_mfma_f32_16x16x32_f16 and walks k in stages of 256 columns.  One stage of both tiles is 128 bytes per lane: eight 16-byte
// non-temporal loads, requested for stage s + 1 before stage s is converted and multiplied.  A 16-byte load holds 16 consecutive k
// of one row; its low and its high 8 bytes are the A fragments of two MFMAs, converted in registers (exact: every e4m3 value is an
// fp16 value).  Lane (q, i) of tile T loads bytes 64 j + 16 q .. + 15 of row i, so MFMA (j, h) multiplies the columns
// 64 j + 16 q + 8 h + e (e < 8) in its slot (q, e): the k permutation lives in the ADDRESS of the x fragment a lane fetches from LDS
// (x itself is staged in natural order), and every fetched x fragment feeds both tiles.  The row scale meets the fp32 accumulators
// in the epilogue, never the weights.  D[weight row 4 q + r][batch row i] lands in lane (q, i): one writer per logit.
//
// The argmax: logit and vocab index as one 64-bit key (order-preserving image of the float above, ~index below, so the integer
// maximum is the largest logit at its lowest index), maximum over the lane's eight logits, over the workgroup through LDS, over
// the grid with an agent-scope atomic maximum into the workspace; the last workgroup to take a ticket writes the tokens and
// puts the workspace back to zeros.  An integer maximum does not depend on the order of arrival: two launches are bitwise equal.
#include <hip/hip_runtime.h>

#include "attn_common.h"
#include "kv8.h"
#include "launch.h"
#include "qpal_common.h"

namespace qpal {

typedef _Float16 w8_half8_t __attribute__((ext_vector_type(8)));
typedef float w8_float4_t __attribute__((ext_vector_type(4)));
typedef unsigned long long w8_key_t;

struct LmW8Params {
    const float *h;          // fp32 [rows][ld_h]
    long ld_h;
    const uint16_t *rms_w;   // fp16 [k] or null (w = 1)
    float rms_eps;           // 0: no norm (x = fp16(h), rms_w null)
    const uint8_t *w;        // e4m3fn [vocab][k]
    const float *scale;      // fp32 [vocab]
    float *logits;           // fp32 [rows][ld_logits] or null
    long ld_logits;
    long *token;             // int64 [rows] or null
    const long *active;      // int64 [rows] or null
    w8_key_t *keys;          // workspace: [128] keys, zero between launches
    unsigned *ticket;        // workspace: behind the keys, zero between launches
    int rows, vocab, k;
};

constexpr int kW8Stage = 256;             // columns of k per LDS stage
constexpr int kW8Stride = kW8Stage + 8;   // halves per staged row: 16 lanes of an MFMA row group hit 16 different bank quads
constexpr int kW8Waves = 8;
constexpr int kW8Threads = 64 * kW8Waves;
constexpr int kW8Rows = 32 * kW8Waves;    // vocab rows of a workgroup
constexpr long kW8WsBytes = 128 * (long)sizeof(w8_key_t) + 16;

// (logit, vocab index) -> key: a larger logit is a larger key, among equal logits (-0 = +0) the lower index; never 0
__device__ __forceinline__ w8_key_t w8_key(float val, int v) {
    uint32_t u = __builtin_bit_cast(uint32_t, val);
    if ((u << 1) == 0u) u = 0u;
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
    return ((w8_key_t)u << 32) | (w8_key_t)(0xffffffffu - (uint32_t)v);
}

template <int NBT>  // 16-row tiles of the batch: ceil(rows / 16)
__global__ __launch_bounds__(kW8Threads) void lm_head_w8_kernel(const LmW8Params p) {
    // 1 / rms [NBT * 16] | keys [NBT * 16] | flag (16 bytes) | x [NBT * 16][kW8Stride] fp16
    extern __shared__ __attribute__((aligned(16))) float w8_sh[];
    float *inv_s = w8_sh;
    w8_key_t *keys_s = reinterpret_cast<w8_key_t *>(w8_sh + NBT * 16);
    unsigned *flag = reinterpret_cast<unsigned *>(keys_s + NBT * 16);
    uint16_t *xs = reinterpret_cast<uint16_t *>(flag + 4);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = p.k, nbt = NBT;
    // ---- 1 / rms of every row (every workgroup for itself: the rows come from L2), the arithmetic of lm_head_logits_kernel
    for (int r = wave; r < nbt * 16; r += kW8Waves) {
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
    if (tid < nbt * 16) keys_s[tid] = 0ull;
    // rows that do not exist: zeros, written once (no stage touches them)
    for (int i = tid; i < (nbt * 16 - p.rows) * (kW8Stride / 2); i += kW8Threads)
        reinterpret_cast<uint32_t *>(xs + p.rows * kW8Stride)[i] = 0u;
    __syncthreads();

    const int mi = lane & 15, mq = lane >> 4;
    const int v0 = (blockIdx.x * kW8Waves + wave) * 32;
    const bool act = v0 < p.vocab;  // (wave-uniform) a wave past the last vocab row only helps staging
    // a tile row past the vocabulary reads the last row instead (never memory behind the table) and is never written
    gptr<const uint8_t> wrow[2];
#pragma unroll
    for (int T = 0; T < 2; T++) {
        const int wr = v0 + 16 * T + mi < p.vocab ? v0 + 16 * T + mi : p.vocab - 1;
        wrow[T] = as_global(p.w) + (long)wr * k + 16 * mq;
    }
    w8_float4_t acc[2][NBT];
#pragma unroll
    for (int T = 0; T < 2; T++)
#pragma unroll
        for (int t = 0; t < NBT; t++) acc[T][t] = w8_float4_t{0.f, 0.f, 0.f, 0.f};
    u32x4 wcur[2][4], wnext[2][4];
#pragma unroll
    for (int T = 0; T < 2; T++)
#pragma unroll
        for (int j = 0; j < 4; j++) wcur[T][j] = wnext[T][j] = u32x4{0u, 0u, 0u, 0u};
    auto request = [&](u32x4(&dst)[2][4], const int c) {
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int T = 0; T < 2; T++)
                dst[T][j] = __builtin_nontemporal_load((gptr<const u32x4>)(wrow[T] + c * kW8Stage + 64 * j));
    };
    if (act) request(wcur, 0);
    // the row scales of the lane's eight logits: in flight across the whole walk
    float sc[2][4];
#pragma unroll
    for (int T = 0; T < 2; T++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int v = v0 + 16 * T + 4 * mq + r;
            sc[T][r] = act ? p.scale[v < p.vocab ? v : p.vocab - 1] : 0.f;
        }
    const int srow = tid >> 6, scol = 4 * (tid & 63);  // staging: 64 threads a row, 4 columns each
    const int nstage = k / kW8Stage;
    // x of stage c: fp16(h * inv) [* rms_w in fp16], the arithmetic of lm_head_logits_kernel
    auto stage_x = [&](const int c) {
        for (int r = srow; r < p.rows; r += kW8Waves) {
            const int col = c * kW8Stage + scol;
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
            *reinterpret_cast<u32x2 *>(xs + r * kW8Stride + scol) = o;
        }
    };
    // load j, half h of both tiles: columns 64 j + 16 mq + 8 h .. + 7 of the stage against the same columns of x
    auto multiply = [&]() {
#pragma unroll
        for (int j = 0; j < 4; j++) {
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const u32x2 b0 = h ? u32x2{wcur[0][j].z, wcur[0][j].w} : u32x2{wcur[0][j].x, wcur[0][j].y};
                const u32x2 b1 = h ? u32x2{wcur[1][j].z, wcur[1][j].w} : u32x2{wcur[1][j].x, wcur[1][j].y};
                const w8_half8_t a0 = __builtin_bit_cast(w8_half8_t, e4m3_half8(b0));
                const w8_half8_t a1 = __builtin_bit_cast(w8_half8_t, e4m3_half8(b1));
#pragma unroll
                for (int t = 0; t < NBT; t++) {
                    const u32x4 b = *reinterpret_cast<const u32x4 *>(xs + (t * 16 + mi) * kW8Stride + 64 * j + 16 * mq + 8 * h);
                    const w8_half8_t xb = __builtin_bit_cast(w8_half8_t, b);
                    acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, xb, acc[0][t], 0, 0, 0);
                    acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, xb, acc[1][t], 0, 0, 0);
                }
            }
        }
    };
    // every stage but the last requests the next stage's weights before it converts and multiplies (the last one stands apart so
    // that the multiply of a prefetching stage waits for ITS weights only, with the eight younger loads still in flight)
    for (int c = 0; c + 1 < nstage; c++) {
        stage_x(c);
        __syncthreads();
        if (act) {
            request(wnext, c + 1);
            multiply();
#pragma unroll
            for (int T = 0; T < 2; T++)
#pragma unroll
                for (int j = 0; j < 4; j++) wcur[T][j] = wnext[T][j];
        }
        __syncthreads();
    }
    stage_x(nstage - 1);
    __syncthreads();
    if (act) {
        multiply();
        // ---- lane (mq, mi): logits of vocab rows v0 + 16 T + 4 mq + r for batch row 16 t + mi
#pragma unroll
        for (int t = 0; t < NBT; t++) {
            const int b = t * 16 + mi;
            if (b < p.rows) {
                w8_key_t best = 0ull;
#pragma unroll
                for (int T = 0; T < 2; T++)
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        const int v = v0 + 16 * T + 4 * mq + r;
                        if (v < p.vocab) {
                            const float val = acc[T][t][r] * sc[T][r];
                            if (p.logits) p.logits[(long)b * p.ld_logits + v] = val;
                            const w8_key_t key = w8_key(val, v);
                            best = key > best ? key : best;
                        }
                    }
                if (p.token && best) __hip_atomic_fetch_max(&keys_s[b], best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    if (!p.token) return;  // (uniform over the grid)
    // ---- the workgroup's best per row into the workspace, then the ticket: the last workgroup writes the tokens
    __syncthreads();
    if (tid < p.rows && keys_s[tid])
        __hip_atomic_fetch_max(as_global(p.keys + tid), keys_s[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (!ticket_last<__ATOMIC_ACQ_REL>(p.ticket, gridDim.x, flag, tid)) return;
    if (tid < p.rows) {
        const w8_key_t key = __hip_atomic_load(as_global(p.keys + tid), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(as_global(p.keys + tid), 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!p.active || p.active[tid] >= 0) p.token[tid] = (long)(0xffffffffu - (uint32_t)key);
    }
    if (tid == 0) __hip_atomic_store(as_global(p.ticket), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct EmbedW8Params {
    const uint8_t *w;     // e4m3fn [vocab][k]
    const float *scale;   // fp32 [vocab]
    const long *tokens;   // int64 [rows]
    float *out;           // fp32 [rows][ld_out]
    long ld_out;
    int vocab, k;
};

// one workgroup a row, a thread 16 bytes of it at a time: out = scale[t] * float(e4m3), one fp32 rounding
__global__ __launch_bounds__(256) void embed_rows_w8_kernel(const EmbedW8Params p) {
    const long t = p.tokens[blockIdx.x];
    const bool ok = t >= 0 && t < p.vocab;
    const float s = ok ? p.scale[t] : 0.f;
    float4 *dst = reinterpret_cast<float4 *>(p.out + (long)blockIdx.x * p.ld_out);
    for (int i = threadIdx.x; i < p.k / 16; i += 256) {
        u32x4 w = u32x4{0u, 0u, 0u, 0u};  // (the e4m3 byte 0 is +0)
        if (ok) w = *reinterpret_cast<const u32x4 *>(p.w + t * p.k + 16 * i);
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const kv8_float2_t lo = e4m3_float2<false>(w[d]), hi = e4m3_float2<true>(w[d]);
            dst[4 * i + d] = ok ? float4{s * lo[0], s * lo[1], s * hi[0], s * hi[1]} : float4{0.f, 0.f, 0.f, 0.f};
        }
    }
}

}  // namespace qpal

using namespace qpal;

static size_t lm_w8_lds(int nbt) {
    return (size_t)nbt * 16 * (sizeof(float) + sizeof(w8_key_t) + kW8Stride * sizeof(uint16_t)) + 16;
}

extern "C" long qpal_lm_head_w8_ws_bytes(int rows, int vocab) {
    return rows < 1 || rows > 128 || vocab < 1 ? 0 : kW8WsBytes;
}

extern "C" int qpal_lm_head_w8(const float *h_f32, long ld_h, const void *rms_w_f16, float rms_eps, const void *w_e4m3,
                               const float *scale_f32, float *logits_f32, long ld_logits, long *token, const long *active, void *ws,
                               long ws_bytes, int rows, int vocab, int k, void *stream) {
    if (!h_f32 || !w_e4m3 || !scale_f32 || (!logits_f32 && !token) || (token && !ws)) return QPAL_E_NULL;
    if (rows < 1 || rows > 128 || vocab < 1 || k < 512 || k > 8192 || k % 512 || ld_h < k || (logits_f32 && ld_logits < vocab) ||
        (token && ws_bytes < kW8WsBytes))
        return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(w_e4m3) & 15) || (reinterpret_cast<uintptr_t>(h_f32) & 15) || (rows > 1 && ld_h % 4) ||
        (reinterpret_cast<uintptr_t>(scale_f32) & 3) || (reinterpret_cast<uintptr_t>(logits_f32) & 3) ||
        (rms_w_f16 && (reinterpret_cast<uintptr_t>(rms_w_f16) & 7)) || (reinterpret_cast<uintptr_t>(token) & 7) ||
        (reinterpret_cast<uintptr_t>(active) & 7) || (token && (reinterpret_cast<uintptr_t>(ws) & 7)))
        return QPAL_E_ALIGN;
    const bool norm = rms_eps > 0.f;  // no weight: w = 1, as in qpal_lm_head_logits
    w8_key_t *keys = static_cast<w8_key_t *>(ws);
    LmW8Params p{h_f32, ld_h, norm ? static_cast<const uint16_t *>(rms_w_f16) : nullptr, norm ? rms_eps : 0.f,
                 static_cast<const uint8_t *>(w_e4m3), scale_f32, logits_f32, ld_logits, token, token ? active : nullptr,
                 token ? keys : nullptr, token ? reinterpret_cast<unsigned *>(keys + 128) : nullptr, rows, vocab, k};
    const int grid = (vocab + kW8Rows - 1) / kW8Rows;
    switch ((rows + 15) / 16) {
    // (128 rows: 68 KiB of LDS)
#define QPAL_LM_W8(N_)                                                                                                     \
    case N_:                                                                                                               \
        return launch_lds<lm_head_w8_kernel<N_>>(dim3(grid), dim3(kW8Threads), lm_w8_lds(N_), (int)lm_w8_lds(N_),          \
                                                 static_cast<hipStream_t>(stream), p);
        QPAL_LM_W8(1) QPAL_LM_W8(2) QPAL_LM_W8(3) QPAL_LM_W8(4)
        QPAL_LM_W8(5) QPAL_LM_W8(6) QPAL_LM_W8(7) QPAL_LM_W8(8)
#undef QPAL_LM_W8
    }
    return QPAL_E_SHAPE;
}

extern "C" int qpal_embed_rows_w8(const void *w_e4m3, const float *scale_f32, const long *tokens, float *out_f32, long ld_out,
                                  int rows, int vocab, int k, void *stream) {
    if (!w_e4m3 || !scale_f32 || !tokens || !out_f32) return QPAL_E_NULL;
    if (rows < 1 || rows > 128 || vocab < 1 || k < 16 || k % 16 || ld_out < k) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(w_e4m3) & 15) || (reinterpret_cast<uintptr_t>(scale_f32) & 3) ||
        (reinterpret_cast<uintptr_t>(tokens) & 7) || (reinterpret_cast<uintptr_t>(out_f32) & 15) || (rows > 1 && ld_out % 4))
        return QPAL_E_ALIGN;
    const EmbedW8Params p{static_cast<const uint8_t *>(w_e4m3), scale_f32, tokens, out_f32, ld_out, vocab, k};
    hipLaunchKernelGGL(embed_rows_w8_kernel, dim3(rows), dim3(256), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
