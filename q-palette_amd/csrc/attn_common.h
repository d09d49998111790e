// What the attention launches share (decoder_glue.hip's split-context kernel, attn_batch.hip, attn_prefill.h with attn_prefill.hip
// and attn_ragged.hip, attn_prefix.hip): the supported head shapes, the shape rule and the argument checks of the entry points,
// the preamble of the paged ones, and the agent-scope partial / ticket hand-over of the kernels that split a context.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "kv_paged.h"
#include "launch.h"
#include "qpal_common.h"

namespace qpal {

namespace {

constexpr int kAttnMaxRows = 128;  // the linears' fused batch

// THE list of (head_dim, query heads per kv head): f(integral_constant HD, integral_constant REP) of the pair, QPAL_E_SHAPE for any other
template <class F>
int for_hd_rep(int hd, int rep, F &&f) {
#define QPAL_HD_REP(HD_, REP_) \
    if (hd == HD_ && rep == REP_) return f(std::integral_constant<int, HD_>{}, std::integral_constant<int, REP_>{});
    QPAL_HD_REP(64, 1) QPAL_HD_REP(64, 2) QPAL_HD_REP(64, 4) QPAL_HD_REP(64, 8)
    QPAL_HD_REP(128, 1) QPAL_HD_REP(128, 2) QPAL_HD_REP(128, 4) QPAL_HD_REP(128, 8)
    QPAL_HD_REP(256, 1) QPAL_HD_REP(256, 2) QPAL_HD_REP(256, 4)
#undef QPAL_HD_REP
    return QPAL_E_SHAPE;
}

// f(CT{}) with the cache element type of kv_fmt: 0 fp16 (uint16_t), 1 e4m3fn (uint8_t)
template <class F>
int for_kv_fmt(int kv_fmt, F &&f) {
    return kv_fmt == 1 ? f(uint8_t{}) : f(uint16_t{});
}

// the shape rules every batched attention launch shares (rows: B of a decode launch, T of a one-sequence prefill, R of a ragged one)
inline int attn_shape(int rows, int nq, int nkv, int hd, long max_len) {
    if (rows < 1 || rows > kAttnMaxRows || nq < 1 || nkv < 1 || nq % nkv || (hd != 64 && hd != 128 && hd != 256)) return QPAL_E_SHAPE;
    const int rep = nq / nkv;
    if ((rep != 1 && rep != 2 && rep != 4 && rep != 8) || rep * hd > 1024) return QPAL_E_SHAPE;
    if (max_len < 4 || max_len % 4 || max_len >= (1L << 30)) return QPAL_E_SHAPE;
    return QPAL_OK;
}

// the argument checks those entry points share, behind the null checks and the geometry (need_ws: the workspace bytes of the
// launch; al4: every further pointer that must be 4-byte aligned, OR-ed — the block table, the shared launch's descriptors)
inline int attn_args(const void *q, const void *k, const void *v, long ld_qkv, const void *kcache, const void *vcache, const void *out_f16,
                     long ld_out, const void *pos, const void *inv_freq, int nq, int hd, size_t need_ws, const void *ws, long ws_bytes,
                     uintptr_t al4) {
    if (ld_qkv < (long)nq * hd || ld_out < (long)nq * hd) return QPAL_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(kcache) | reinterpret_cast<uintptr_t>(vcache)) & 15) return QPAL_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k) | reinterpret_cast<uintptr_t>(v) |
         reinterpret_cast<uintptr_t>(inv_freq) | reinterpret_cast<uintptr_t>(pos)) & 3)
        return QPAL_E_ALIGN;
    if (reinterpret_cast<uintptr_t>(out_f16) & 1) return QPAL_E_ALIGN;
    if (al4 & 3) return QPAL_E_ALIGN;
    if (need_ws) {
        if (!ws) return QPAL_E_NULL;
        if (ws_bytes < (long)need_ws) return QPAL_E_SHAPE;
        if (reinterpret_cast<uintptr_t>(ws) & 3) return QPAL_E_ALIGN;
    }
    return QPAL_OK;
}

// the preamble of a paged entry point: the null checks (any_null: the table first, then the siblings' pointers, so a null among
// q .. inv_freq wins over a paged shape error), the paged shape, then f(CT{}, shift, max_len) with the cache element type
template <class F>
int paged_entry(bool any_null, const PageArgs &pg, int kv_fmt, F &&f) {
    if (any_null) return QPAL_E_NULL;
    int shift;
    long max_len;
    const int rc = paged_shape(pg, kv_fmt, shift, max_len);
    if (rc != QPAL_OK) return rc;
    return for_kv_fmt(kv_fmt, [&](auto ct) { return f(ct, shift, max_len); });
}

// the score modifiers of the _score entry points: softcap 0 — none; sinks null — none, else fp32 [nq] on the device
struct ScoreMods {
    float softcap;
    const float *sinks;
};

// softcap as an argument: 0 or a finite value above it (anything else is QPAL_E_PARAM)
inline bool score_mods_ok(float softcap) {
    return softcap >= 0.f && softcap <= 3.0e38f;
}

// cap * tanh(s / cap) in fp32 with tanh(x) = 1 - 2 / (exp(2 x) + 1): one v_exp_f32 and one v_rcp_f32, no branch.  x is clamped to
// +-15, where the form has long reached +-1 in fp32 (tanh(15) = 1 - 2e-13), so exp never overflows; the absolute error of the
// tanh is a few 2^-24 (the rounding of exp(2 x) + 1 and of the subtraction from 1), of the result a few cap * 2^-24.
__device__ __forceinline__ float soft_cap(float s, float cap, float inv_cap) {
    const float x = fminf(fmaxf(s * inv_cap, -15.f), 15.f);
    return cap * (1.f - 2.f * __builtin_amdgcn_rcpf(__expf(2.f * x) + 1.f));
}

// partials that cross workgroups go out and come in at agent scope: the L2s of the XCDs are not coherent with each other
__device__ __forceinline__ void st_agent(float *p, float v) {
    __hip_atomic_store(as_global(reinterpret_cast<unsigned *>(p)), __builtin_bit_cast(unsigned, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ float ld_agent(const float *p) {
    return __builtin_bit_cast(float, __hip_atomic_load(as_global(reinterpret_cast<const unsigned *>(p)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
}

// The ticket hand-over of n workgroups that have left partials with st_agent (write-through): wait for the stores, then arrive
// at agent scope with memory order ORDER; true in every thread of the last workgroup to arrive, which sees the others' partials
// (ld_agent) and resets the ticket.  flag: a word of LDS.
template <int ORDER>
__device__ __forceinline__ bool ticket_last(unsigned *ticket, unsigned n, unsigned *flag, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned t = __hip_atomic_fetch_add(as_global(ticket), 1u, ORDER, __HIP_MEMORY_SCOPE_AGENT);
        *flag = t == n - 1 ? 1u : 0u;
    }
    __syncthreads();
    return *flag != 0u;
}

}  // namespace

}  // namespace qpal
