// What the attention launches share (decoder_glue.hip's split-context kernel, attn_batch.hip, attn_prefill.h with attn_prefill.hip,
// attn_ragged.hip and attn_prefill_wide.hip, attn_prefix.hip): the supported head shapes and the shape rule; the call and variant
// descriptors of the rope-append-attention entry points with their one preamble, variant dispatch (attn_launch) and argument
// checks (attn_args); the soft cap; and the agent-scope partial / ticket hand-over of the kernels that split a context.
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

// the score modifiers of the _score entry points: softcap 0 — none; sinks null — none, else fp32 [nq] on the device
struct ScoreMods {
    float softcap;
    const float *sinks;
};

// softcap as an argument: 0 or a finite value above it (anything else is QPAL_E_PARAM)
inline bool score_mods_ok(float softcap) {
    return softcap >= 0.f && softcap <= 3.0e38f;
}

// ---- the entry points: every launching extern "C" function fills an AttnCall and an AttnVariant, names its family
// and returns attn_launch's result

// what every entry point receives (pos: pos [B] of a decode launch, pos0 of a prefill, pos0 [S] of a ragged one; rows: B, T or R)
struct AttnCall {
    const float *q, *k, *v;
    long ld_qkv;
    void *kcache, *vcache, *out_f16;
    long ld_out;
    const long *pos;
    const float *inv_freq;
    int rows, nq, nkv, hd;
    float scale;
    void *ws;
    long ws_bytes;
    void *stream;
};

// the cache of a call and the variant of the launch, as far as the entry point's prototype can say them
struct AttnVariant {
    PageArgs pg{};            // table null: contiguous caches
    bool need_table = false;  // the _paged / _shared entry points: a null table is QPAL_E_NULL, not a contiguous cache
    int kv_fmt = 0;
    long max_len = 0;         // of contiguous caches; a paged launch's is max_pages * page_size
    long window = 0;          // 0: none
    ScoreMods mods{0.f, nullptr};
};

// the argument checks the launches share, behind attn_launch's and the geometry (need_ws: the workspace bytes of the launch; al4:
// the family's own pointers that must be 4-byte aligned, OR-ed — the block table and the sinks are taken from v)
inline int attn_args(const AttnCall &c, const AttnVariant &v, size_t need_ws, uintptr_t al4 = 0) {
    auto at = [](const void *p) { return reinterpret_cast<uintptr_t>(p); };
    if (c.ld_qkv < (long)c.nq * c.hd || c.ld_out < (long)c.nq * c.hd) return QPAL_E_SHAPE;
    if ((at(c.kcache) | at(c.vcache)) & 15) return QPAL_E_ALIGN;
    if ((at(c.q) | at(c.k) | at(c.v) | at(c.inv_freq) | at(c.pos)) & 3) return QPAL_E_ALIGN;
    if (at(c.out_f16) & 1) return QPAL_E_ALIGN;
    if ((al4 | at(v.pg.table) | at(v.mods.sinks)) & 3) return QPAL_E_ALIGN;
    if (need_ws) {
        if (!c.ws) return QPAL_E_NULL;
        if (c.ws_bytes < (long)need_ws) return QPAL_E_SHAPE;
        if (at(c.ws) & 3) return QPAL_E_ALIGN;
    }
    return QPAL_OK;
}

// THE preamble and variant dispatch of the entry points, in the order of the codes: a null pointer (the call's, the family's
// own, the table where the entry point needs one) QPAL_E_NULL; window < 0 or a bad softcap QPAL_E_PARAM; kv_fmt and the paged
// shape QPAL_E_SHAPE; then fam.launch<CT, PAGED, WIN, SC>(call, variant, log2(page_size), max_len) with the cache element type of
// kv_fmt, PAGED for a table, SC for a softcap or sinks (on the windowed body: WIN), WIN for a window.  A family says what it has kernels
// for — kContig: contiguous caches, kMods: windows and score modifiers — and nothing else of it is instantiated.
template <class Family>
int attn_launch(const AttnCall &c, const AttnVariant &v, const Family &fam) {
    const bool paged = v.pg.table != nullptr;
    if (!c.q || !c.k || !c.v || !c.kcache || !c.vcache || !c.out_f16 || !c.pos || !c.inv_freq || fam.any_null()) return QPAL_E_NULL;
    if ((v.need_table || !Family::kContig) && !paged) return QPAL_E_NULL;
    if (v.window < 0 || !score_mods_ok(v.mods.softcap)) return QPAL_E_PARAM;
    if (v.kv_fmt != 0 && v.kv_fmt != 1) return QPAL_E_SHAPE;
    int shift = 0;
    long max_len = v.max_len;
    if (paged) {
        const int rc = paged_shape(v.pg, v.kv_fmt, shift, max_len);
        if (rc != QPAL_OK) return rc;
    }
    const bool sc = v.mods.softcap != 0.f || v.mods.sinks, win = sc || v.window != 0;
    auto variant = [&](auto ct, auto pg) {
        using CT = decltype(ct);
        constexpr bool PAGED = decltype(pg)::value;
        if constexpr (Family::kMods) {
            if (sc) return fam.template launch<CT, PAGED, true, true>(c, v, shift, max_len);
            if (win) return fam.template launch<CT, PAGED, true, false>(c, v, shift, max_len);
        }
        return fam.template launch<CT, PAGED, false, false>(c, v, shift, max_len);
    };
    return for_kv_fmt(v.kv_fmt, [&](auto ct) {
        if constexpr (Family::kContig) {
            if (!paged) return variant(ct, std::false_type{});
        }
        return variant(ct, std::true_type{});
    });
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
