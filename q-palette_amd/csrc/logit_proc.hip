// qpal_logit_process / qpal_logit_observe: the stage between qpal_lm_head_logits and qpal_sample (DESIGN.md §22 has the contract
// word for word; logits.reference_process restates it in numpy fp32 and the kernel equals it bit for bit).
//
//   logit_process_kernel   grid (vocab tiles, rows), 256 threads, a tile = 4096 tokens of one row: four groups of four consecutive
//                          tokens per thread (group g of thread t: tokens base + 1024 g + 4 t ..), 16-byte loads of the logits and the
//                          counts where the three row bases allow, the same groups by single loads elsewhere and in the row's last
//                          group.  The tile's 128 mask words are loaded once (thread t < 128: word t, one word per 32 tokens) and
//                          the row's <= 15 extra tokens once (threads 0 .. 14), both into LDS; an extra reaches the compare loop
//                          through a scalar register and only when it lies in the tile.  The bias entries that fall into the tile are
//                          added by this workgroup after a barrier (one read-modify-write per entry by one thread): a word has one
//                          writer workgroup, and inside it the two writes are ordered by the barrier.
//   logit_observe_kernel   one thread per row: an integer atomicAdd on the (slot, token) counter — integer sums have no order, so
//                          equal launches leave equal bits.
// Penalty arithmetic: every operation rounded once, in the contract's order.  The compiler's default contracts a * b + c into a fused
// multiply-add, and __fmul_rn and friends do not stop it (they are plain operators inside a header that is compiled under that
// default): contraction is switched off for this translation unit, and the arithmetic is written with operators below the pragma.
#include <hip/hip_runtime.h>

#include "qpal_common.h"

#pragma clang fp contract(off)

namespace qpal {

constexpr int kProcThreads = 256, kProcGroups = 4, kProcTile = kProcThreads * 4 * kProcGroups;  // 4096 tokens = 128 mask words
constexpr int kProcMaxExtra = 15, kProcMaxRows = 128, kProcMaxBias = 1024, kObserveThreads = 256, kObserveMaxRows = 2048;

struct LogitProcParams {
    const float *in;
    long ld_in;
    float *out;
    long ld_out;
    int rows, vocab, slots;
    const int *row_slot;
    const long *ctr;
    const int *count;
    long ld_count;
    const float *repetition, *presence, *frequency;
    const uint32_t *mask;
    long ld_mask;
    const int *mask_on;
    const int *bias_id;
    const float *bias_val;
    const int *bias_n;
    int bias_slots;
    const long *tokens;
    const int *row0;
};

__global__ __launch_bounds__(kProcThreads) void logit_process_kernel(const LogitProcParams p) {
    __shared__ uint32_t s_mask[kProcTile / 32];
    __shared__ int s_extra[kProcMaxExtra + 1];
    const int r = blockIdx.y, tid = threadIdx.x, vocab = p.vocab;
    const int base = blockIdx.x * kProcTile;  // < vocab: the grid has ceil(vocab / tile) tiles
    // ---- the row (everything here is uniform in the workgroup)
    const int b = p.row_slot[r];
    if (p.ctr[r] < 0 || b < 0 || b >= p.slots) return;
    int n_extra = 0, first = 0;
    if (p.tokens) {
        first = p.row0[b];
        n_extra = r - first;
        if (first < 0 || n_extra < 0 || n_extra > kProcMaxExtra) return;  // no row of slot b's segment: inactive
    }
    const float rep = p.repetition[b], pres = p.presence[b], freq = p.frequency[b];
    const bool masked = p.mask_on[b] != 0;
    const float *in = p.in + (long)r * p.ld_in;
    float *out = p.out + (long)r * p.ld_out;
    const int *cnt = p.count + (long)b * p.ld_count;
    const bool vec = ((reinterpret_cast<uintptr_t>(in) | reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(cnt)) & 15) == 0;

    // ---- the loads of the tile, all in flight before anything waits
    float l[kProcGroups][4];
    int c[kProcGroups][4];
#pragma unroll
    for (int g = 0; g < kProcGroups; g++) {
        const int i0 = base + g * (kProcThreads * 4) + 4 * tid;
        if (vec && i0 + 4 <= vocab) {
            const float4 t = *reinterpret_cast<const float4 *>(in + i0);
            const int4 u = *reinterpret_cast<const int4 *>(cnt + i0);
            l[g][0] = t.x; l[g][1] = t.y; l[g][2] = t.z; l[g][3] = t.w;
            c[g][0] = u.x; c[g][1] = u.y; c[g][2] = u.z; c[g][3] = u.w;
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const bool ok = i0 + e < vocab;
                l[g][e] = ok ? in[i0 + e] : 0.f;
                c[g][e] = ok ? cnt[i0 + e] : 0;
            }
        }
    }
    if (masked && tid < kProcTile / 32) {
        const int w = (base >> 5) + tid;
        s_mask[tid] = w < ((vocab + 31) >> 5) ? p.mask[(long)b * p.ld_mask + w] : 0u;
    }
    if (tid < n_extra) {
        const long t = p.tokens[first + 1 + tid];
        s_extra[tid] = t >= 0 && t < vocab ? (int)t : -1;  // (a caller's draft may be no token of the model: it counts for nothing)
    }
    __syncthreads();

    // ---- 1. the guessed tokens in front of the row count as if they had been emitted
    for (int x = 0; x < n_extra; x++) {
        const int off = __builtin_amdgcn_readfirstlane(s_extra[x]) - base;
        if (off < 0 || off >= kProcTile) continue;  // (uniform) -1, or a token of another tile
        const int d = off - 4 * tid;
#pragma unroll
        for (int g = 0; g < kProcGroups; g++)
#pragma unroll
            for (int e = 0; e < 4; e++) c[g][e] += d == g * (kProcThreads * 4) + e ? 1 : 0;
    }
    // ---- 2. penalties, 3. mask; the store
#pragma unroll
    for (int g = 0; g < kProcGroups; g++) {
        const int i0 = base + g * (kProcThreads * 4) + 4 * tid;
        const uint32_t mw = masked ? s_mask[(i0 - base) >> 5] >> (i0 & 31) : 0xFu;  // the group's four bits: i0 % 4 == 0
#pragma unroll
        for (int e = 0; e < 4; e++) {
            float v = l[g][e];
            if (c[g][e] > 0 && v == v) {  // (a NaN passes through as it is)
                v = v > 0.f ? v / rep : v * rep;  // (the division is the correctly rounded one: hipcc's default)
                const float f = freq * (float)c[g][e];
                const float s = pres + f;
                v = v - s;
            }
            l[g][e] = (mw >> e) & 1u ? v : kNegInf;
        }
        if (vec && i0 + 4 <= vocab) {
            *reinterpret_cast<float4 *>(out + i0) = make_float4(l[g][0], l[g][1], l[g][2], l[g][3]);
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++)
                if (i0 + e < vocab) out[i0 + e] = l[g][e];
        }
    }
    // ---- 4. the sparse bias of the slot: the entries of this tile, on the values the tile's threads have just stored
    int nb = p.bias_slots > 0 ? p.bias_n[b] : 0;
    nb = nb < 0 ? 0 : (nb > p.bias_slots ? p.bias_slots : nb);
    if (nb == 0) return;  // (uniform)
    __syncthreads();      // the stores above are visible to the workgroup (a release / acquire pair at workgroup scope)
    const int end = base + kProcTile < vocab ? base + kProcTile : vocab;
    for (int j = tid; j < nb; j += kProcThreads) {
        const int id = p.bias_id[(long)b * p.bias_slots + j];
        if (id < base || id >= end) continue;
        const float v = out[id];
        if (v == v) out[id] = v + p.bias_val[(long)b * p.bias_slots + j];
    }
}

struct LogitObserveParams {
    int *count;
    long ld_count;
    int slots, vocab, n;
    const int *slot;
    int slot0;
    const long *tokens, *active;
};

__global__ __launch_bounds__(kObserveThreads) void logit_observe_kernel(const LogitObserveParams p) {
    const int r = blockIdx.x * kObserveThreads + threadIdx.x;
    if (r >= p.n) return;
    const int b = p.slot ? p.slot[r] : p.slot0;
    const long t = p.tokens[r];
    if (b < 0 || b >= p.slots || t < 0 || t >= p.vocab || (p.active && p.active[r] < 0)) return;
    atomicAdd(p.count + (long)b * p.ld_count + t, 1);
}

}  // namespace qpal

using namespace qpal;

static inline bool misaligned(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

extern "C" int qpal_logit_process(const float *logits, long ld_logits, float *out, long ld_out, int rows, int vocab,
                                  const int *row_slot, const long *ctr, int slots, const int *count, long ld_count,
                                  const float *repetition, const float *presence, const float *frequency, const unsigned *mask,
                                  long ld_mask, const int *mask_on, const int *bias_id, const float *bias_val, const int *bias_n,
                                  int bias_slots, const long *tokens, const int *row0, void *stream) {
    if (!logits || !out || !row_slot || !ctr || !count || !repetition || !presence || !frequency || !mask || !mask_on)
        return QPAL_E_NULL;
    if (bias_slots != 0 && (!bias_id || !bias_val || !bias_n)) return QPAL_E_NULL;
    if ((tokens == nullptr) != (row0 == nullptr)) return QPAL_E_NULL;
    if (rows < 1 || rows > kProcMaxRows || vocab < 1 || vocab > (1 << 30) || slots < 1 || slots > kProcMaxRows || ld_logits < vocab || ld_out < vocab ||
        ld_count < vocab || ld_mask < (vocab + 31) / 32 || bias_slots < 0 || bias_slots > kProcMaxBias)
        return QPAL_E_SHAPE;
    if (misaligned(logits, 4) || misaligned(out, 4) || misaligned(row_slot, 4) || misaligned(ctr, 8) || misaligned(count, 4) ||
        misaligned(repetition, 4) || misaligned(presence, 4) || misaligned(frequency, 4) || misaligned(mask, 4) ||
        misaligned(mask_on, 4) || misaligned(bias_id, 4) || misaligned(bias_val, 4) || misaligned(bias_n, 4) ||
        misaligned(tokens, 8) || misaligned(row0, 4))
        return QPAL_E_ALIGN;
    // in place means the same rows: out == logits with one stride; any other overlap would give a word two owners
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(logits), a1 = a0 + 4 * ((uintptr_t)(rows - 1) * ld_logits + vocab);
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(out), b1 = b0 + 4 * ((uintptr_t)(rows - 1) * ld_out + vocab);
    if (a0 == b0 ? (rows > 1 && ld_out != ld_logits) : (a0 < b1 && b0 < a1)) return QPAL_E_PARAM;
    LogitProcParams p{logits, ld_logits, out, ld_out, rows, vocab, slots, row_slot, ctr, count, ld_count, repetition, presence,
                      frequency, mask, ld_mask, mask_on, bias_id, bias_val, bias_n, bias_slots, tokens, row0};
    const dim3 grid((unsigned)(((long)vocab + kProcTile - 1) / kProcTile), (unsigned)rows);
    hipLaunchKernelGGL(logit_process_kernel, grid, dim3(kProcThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}

extern "C" int qpal_logit_observe(int *count, long ld_count, int slots, int vocab, const int *slot, int slot0, const long *tokens,
                                  const long *active, int n, void *stream) {
    if (!count || !tokens) return QPAL_E_NULL;
    if (n < 1 || n > kObserveMaxRows || vocab < 1 || vocab > (1 << 30) || slots < 1 || slots > kProcMaxRows || ld_count < vocab ||
        (!slot && (slot0 < 0 || slot0 >= slots)))
        return QPAL_E_SHAPE;
    if (misaligned(count, 4) || misaligned(slot, 4) || misaligned(tokens, 8) || misaligned(active, 8)) return QPAL_E_ALIGN;
    LogitObserveParams p{count, ld_count, slots, vocab, n, slot, slot0, tokens, active};
    hipLaunchKernelGGL(logit_observe_kernel, dim3((n + kObserveThreads - 1) / kObserveThreads), dim3(kObserveThreads), 0,
                       static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
