// The body of the prefill attention kernels, shared by attn_prefill.hip (ONE sequence per launch) and attn_ragged.hip (rows of
// several sequences per launch), and the host-side geometry both entry-point families size their grid and
// workspace with.  The header comment of attn_prefill.hip describes the kernel; RAGGED changes only where a workgroup's
// per-sequence values come from.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "attn_common.h"
#include "kv8.h"

namespace qpal {

namespace {

constexpr int kPfMaxT = kAttnMaxRows;
constexpr int kPfKT = 32;           // keys per tile
constexpr long kPfSplitFrom = 512;  // caches shorter than this: one chunk per (kv head, query tile), no workspace
constexpr long kPfMinChunk = 128;   // a chunk holds at least this many keys
constexpr int kPfMaxSplit = 16;
constexpr int kPfMaxTiles = 8;      // query tiles of a one-sequence launch: 128 rows / 16
constexpr int kPfRaggedTiles = kPfMaxT;  // ticket words per kv head of a ragged launch: ntile <= R <= 128, whatever (R, S)

template <class CT>
struct AttnPrefillParams {
    const float *q, *k, *v;  // fp32 rows [T][ld_qkv]: q [nq * HD], k / v [nkv * HD] inside a row
    long ld_qkv;
    CT *kcache, *vcache;        // fp16 (uint16_t) or e4m3fn (uint8_t) [nkv][max_len][HD]
    uint16_t *out;              // fp16 [T][ld_out]
    long ld_out;
    const long *pos0;           // int64, device
    const float *inv_freq;      // fp32 [HD / 2]
    int T, nkv;
    long max_len;
    float scale;
    unsigned *tickets;          // [nkv * kPfMaxTiles] (zero-filled once)
    float *part;                // [nkv * ntile * nsplit][rows of a tile][HD + 2] partials
    int nsplit, ntile;
    // PAGED only: kcache / vcache are the pools [num_pages][nkv][1 << page_shift][HD], max_len = max_pages << page_shift
    const int *table;           // int32 [max_pages] of this sequence, device
    int num_pages, page_shift;
    // WIN only (the _window entry points): the row at position n attends to [max(0, n - window + 1), n]
    long window;
    // SC only (the _score entry points): softcap 0 — no cap, else every score is softcap * tanh(score / softcap)
    // (inv_softcap = 1 / softcap); sinks null — none, else fp32 [nq], one logit per query head in the row's denominator
    float softcap, inv_softcap;
    const float *sinks;
};

// RAGGED: T = the rows R of q / k / v / out, pos0 = int64 [S], kcache / vcache = [B][nkv][max_len][HD] (PAGED: table = int32
// [B][ld_table]), tickets = [nkv * kPfRaggedTiles] (a fixed offset: one workspace serves launches of any R, S); segment s is rows row0[s] .. row0[s + 1] - 1 of sequence seq[s]
template <class CT>
struct AttnRaggedParams : AttnPrefillParams<CT> {
    const int *seq, *row0;  // int32 [S], [S + 1], device
    int S, B;
    long ld_table;
};

typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef __fp16 fp16x4_t __attribute__((vector_size(8)));
typedef __attribute__((address_space(3))) fp16x4_t *lds_half4_ptr;

constexpr int pf_qs(int rep) { return rep >= 4 ? 1 : 4 / rep; }  // 16-row query sub-tiles per workgroup: at least 4 waves

// eight consecutive dims [8 ch, 8 ch + 8) of a row after the rotary embedding at position pos, as fp16 (qpal_rope_kv's arithmetic)
template <int HD>
__device__ __forceinline__ u32x4 rope_chunk(const float *src, int ch, long pos, const float *inv_freq) {
    constexpr int HALF = HD / 2;
    const bool hi = 8 * ch >= HALF;
    const int i0 = 8 * ch - (hi ? HALF : 0);
    u32x4 val{0u, 0u, 0u, 0u};
#pragma unroll 1
    for (int e2 = 0; e2 < 4; e2++) {  // (rolled: one copy of cosf / sinf per call site)
        uint32_t w = 0;
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const int i = i0 + 2 * e2 + e;
            const float ang = (float)pos * inv_freq[i];
            const _Float16 c = (_Float16)cosf(ang), s = (_Float16)sinf(ang);
            const _Float16 x1 = (_Float16)src[i], x2 = (_Float16)src[i + HALF];
            const _Float16 o1 = x1 * c + (-x2) * s, o2 = x2 * c + x1 * s;
            w |= (uint32_t)__builtin_bit_cast(uint16_t, hi ? o2 : o1) << (16 * e);
        }
        val.x = e2 == 0 ? w : val.x;
        val.y = e2 == 1 ? w : val.y;
        val.z = e2 == 2 ? w : val.z;
        val.w = e2 == 3 ? w : val.w;
    }
    return val;
}

// RAGGED: the launch serves rows of several sequences (attn_ragged.hip)
//
// WIN (sliding window): the keys of a query tile are [kmin, kend) with kmin = lo(pos0 + t0), lo(n) = max(0, n -
// window + 1), and the chunk formulas run on kend - (kmin & ~31): a chunk still starts on a multiple of 32, so a 16-key half of a
// tile still lies in one page.  fetch() hands out zeros for n < kmin without touching the cache or a page (those rows may hold
// NaN, their pages may be gone: 0 * NaN in the second product would leak), the mask admits lo(qpos) <= n <= qpos per ROW, and a
// row with no admitted key in a tile or a whole chunk keeps m = -3e38, l = 0, O = 0, which the running rescale (alpha = 0 once a
// key arrives) and the merge (weight exp(-3e38 - M) = 0) meet today behind the diagonal.  window >= 1: a tile's own new rows lie
// at or above kmin, so they are fetched, and stored, as without a window.
//
// SC (score modifiers; built on the WIN body, window = max_len where the launch has none): the soft cap where sv =
// s * scale is formed, in front of the mask and the maximum; the sink of the row's head once per row — behind the last tile of a
// one-chunk row, or in the last arriver's merge — as one more term exp(sink - M) of the denominator, M = max(row maximum, sink).
// The running (m, l, O) and the partials in the workspace stay those of the keys alone.  Both are wave-uniform runtime tests; a
// sink of -inf leaves M, a rescale of exp(0) = 1 and a term of 0: the bits without sinks.
template <class CT, bool PAGED, bool RAGGED, int HD, int REP, bool WIN = false, bool SC = false>
__global__ __launch_bounds__(64 * REP * pf_qs(REP)) void attn_prefill_kernel(
    const std::conditional_t<RAGGED, AttnRaggedParams<CT>, AttnPrefillParams<CT>> p) {
    constexpr bool KV8 = kIsKv8<CT>;
    static_assert(!SC || WIN, "the score modifiers are built on the windowed body");
    using KR = std::conditional_t<KV8, u32x2, u32x4>;  // eight elements of a cache row as prefetched
    constexpr int QS = pf_qs(REP), NW = REP * QS, NT = 64 * NW, TQ = 16 * QS, R = 16 * NW;
    constexpr int HALF = HD / 2, KC = HD / 32, DT = HD / 16, CPR = HD / 8;
    constexpr int RS = 2 * HD + 16;                     // bytes of an LDS row (padded by one 16-byte access)
    constexpr int ROWS = R > 2 * kPfKT ? R : 2 * kPfKT;  // Q image [R] first, then K [32] | V [32] over it
    constexpr int NCH = 2 * kPfKT * CPR / NT;           // 16-byte chunks of a K + V tile per thread
    static_assert(2 * kPfKT * CPR % NT == 0, "the K + V tile is cut evenly over the threads");
    static_assert((size_t)ROWS * RS >= (size_t)(R * kPfMaxSplit + R) * sizeof(float), "the merge coefficients fit the tile image");
    static_assert(NT >= kPfMaxT, "RAGGED: one thread per segment of the launch");
    __shared__ __attribute__((aligned(16))) unsigned char sm[ROWS * RS];
    __shared__ unsigned flag;
    unsigned char *const Ks = sm, *const Vs = sm + kPfKT * RS;

    // a position: RAGGED has checked its segment's on the device (below 2^30) and keeps them in 32 bits — the same values, fewer
    // scalar registers (the paged hd 256 instantiations would otherwise spill some)
    using pos_t = std::conditional_t<RAGGED, int, long>;
    pos_t pos0;
    if constexpr (!RAGGED) {
        pos0 = *p.pos0;
        if (pos0 < 0 || pos0 > p.max_len - p.T) return;  // outside the cache: nothing is read or written, no ticket taken
    }
    const int per_kh = p.ntile * p.nsplit;
    const int kh = blockIdx.x / per_kh, rem = blockIdx.x - kh * per_kh;
    const int jg = rem / p.nsplit, split = rem - jg * p.nsplit;  // jg: the query tile's index in the launch
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mi = lane & 15, mq = lane >> 4;
    // T rows of ONE sequence at positions pos0 ..: the launch's (j = jg), or, RAGGED, those of the segment that holds tile jg —
    // tile j of it, its first row row_base of the launch's q / k / v / out, its sequence sq
    int T, j;
    [[maybe_unused]] int row_base = 0, sq = 0;
    if constexpr (RAGGED) {
        // thread s: the query tiles of segment s (inactive: none), then the tiles before it; the one whose range holds jg speaks
        __shared__ int seg_tiles[kPfMaxT];
        __shared__ int seg_sel[2];
        if (tid < kPfMaxT) {
            int n = 0;
            if (tid < p.S) {
                const int r0 = p.row0[tid], r1 = p.row0[tid + 1], b = p.seq[tid];
                const long ps = p.pos0[tid];
                if (r0 >= 0 && r1 > r0 && r1 <= p.T && (unsigned)b < (unsigned)p.B && ps >= 0 && ps <= p.max_len - (r1 - r0))
                    n = (r1 - r0 + TQ - 1) / TQ;
            }
            seg_tiles[tid] = n;
        }
        if (tid == 0) seg_sel[0] = -1;
        __syncthreads();
        if (tid < p.S) {
            int before = 0;
            for (int i = 0; i < p.S; i++) before += i < tid ? seg_tiles[i] : 0;
            if (jg >= before && jg < before + seg_tiles[tid]) seg_sel[0] = tid, seg_sel[1] = jg - before;
        }
        __syncthreads();
        const int s = __builtin_amdgcn_readfirstlane(seg_sel[0]);
        if (s < 0) return;  // no such tile: nothing is read or written, no ticket taken
        j = __builtin_amdgcn_readfirstlane(seg_sel[1]);
        row_base = p.row0[s];
        T = p.row0[s + 1] - row_base;
        sq = p.seq[s];
        pos0 = (pos_t)p.pos0[s];
    } else {
        T = p.T, j = jg;
    }
    const float *const qrows = RAGGED ? p.q + (long)row_base * p.ld_qkv : p.q;
    const float *const krows = RAGGED ? p.k + (long)row_base * p.ld_qkv : p.k;
    const float *const vrows = RAGGED ? p.v + (long)row_base * p.ld_qkv : p.v;
    uint16_t *const orows = RAGGED ? p.out + (long)row_base * p.ld_out : p.out;
    const int t0 = j * TQ, tend = t0 + TQ < T ? t0 + TQ : T;  // query rows of the tile: [t0, tend)
    const unsigned kend = (unsigned)pos0 + (unsigned)tend;    // its keys: [0, kend)  (positions are below 2^30)
    [[maybe_unused]] unsigned kmin = 0u;  // WIN: the first key any row of the tile admits
    if constexpr (WIN) {
        const long first = (long)pos0 + t0 - p.window + 1;
        kmin = first > 0 ? (unsigned)first : 0u;
    }
    const unsigned kbase = WIN ? kmin & ~31u : 0u;  // the chunks cut [kbase, kend)
    const unsigned span = kend - kbase;
    unsigned cld = (span + 31u) & ~31u;
    if (p.nsplit > 1) {
        cld = ((span + (unsigned)p.nsplit - 1u) / (unsigned)p.nsplit + 31u) & ~31u;
        if (cld < (unsigned)kPfMinChunk) cld = (unsigned)kPfMinChunk;
    }
    const int neff = (int)((span + cld - 1u) / cld);  // chunks that hold keys: the same in every workgroup of the tile
    if (split >= neff) return;
    const pos_t c0 = (WIN ? (pos_t)kbase : (pos_t)0) + (pos_t)split * cld;
    const pos_t c1 = c0 + cld < kend ? (pos_t)(c0 + cld) : (pos_t)kend;
    const int hh = wave % REP, qsub = wave / REP;
    const int head = kh * REP + hh;
    const int trow = t0 + qsub * 16 + mi;  // this lane's query row (a column of S^T)
    const pos_t qpos = pos0 + trow;
    [[maybe_unused]] pos_t qlo = 0;  // WIN: lo(qpos)
    if constexpr (WIN) qlo = (long)qpos >= p.window ? (pos_t)((long)qpos - p.window + 1) : (pos_t)0;
    long kvoff;
    if constexpr (PAGED) kvoff = 0;
    else if constexpr (RAGGED) kvoff = ((long)sq * p.nkv + kh) * p.max_len * HD;
    else kvoff = (long)kh * p.max_len * HD;
    const gptr<const CT> Kc = as_global(p.kcache) + kvoff, Vc = as_global(p.vcache) + kvoff;
    [[maybe_unused]] const int *table;  // PAGED: the sequence's block-table row
    if constexpr (RAGGED && PAGED) table = p.table + (long)sq * p.ld_table;
    else table = p.table;
    // PAGED: the page ids of keys kt0 .. kt0 + 15 and kt0 + 16 .. kt0 + 31 of the tile about to be fetched (the second only where
    // the chunk reaches it: entries past the launch's last position are never read)
    [[maybe_unused]] int pg0 = 0, pg1 = 0;
    auto tile_pages = [&]([[maybe_unused]] pos_t kt0) {
        if constexpr (PAGED) {
            if (kt0 < c1) {
                pg0 = table[kt0 >> p.page_shift];
                pg1 = kt0 + 16 < c1 ? table[(kt0 + 16) >> p.page_shift] : pg0;
            }
        }
    };
    tile_pages(c0);
    // element offset of row n (key rr of its tile) from the cache base, and whether a new row may be stored there
    auto row_off = [&](pos_t n, [[maybe_unused]] int rr, [[maybe_unused]] bool &ok) -> long {
        if constexpr (PAGED) {
            const int pg = rr < 16 ? pg0 : pg1;
            ok = page_ok(pg, p.num_pages);
            return paged_row<HD>(ok ? pg : 0, p.nkv, kh, p.page_shift, n);
        } else {
            return (long)n * HD;
        }
    };

    // ---- the wave's 16 query rows after the rotary embedding, through LDS into B fragments (rows >= T: zeros)
    for (int idx = lane; idx < 16 * HALF; idx += 64) {
        const int qi = idx / HALF, i = idx - qi * HALF;
        const int t = t0 + qsub * 16 + qi;
        uint16_t r1 = 0, r2 = 0;
        if (t < T) {
            const float *src = qrows + (long)t * p.ld_qkv + (long)head * HD;
            const float ang = (float)(pos0 + t) * p.inv_freq[i];
            const _Float16 c = (_Float16)cosf(ang), s = (_Float16)sinf(ang);
            const _Float16 x1 = (_Float16)src[i], x2 = (_Float16)src[i + HALF];
            const _Float16 o1 = x1 * c + (-x2) * s, o2 = x2 * c + x1 * s;
            r1 = __builtin_bit_cast(uint16_t, o1), r2 = __builtin_bit_cast(uint16_t, o2);
        }
        uint16_t *dst = reinterpret_cast<uint16_t *>(sm + (wave * 16 + qi) * RS);
        dst[i] = r1;
        dst[i + HALF] = r2;
    }
    __syncthreads();
    half8_t qf[KC];
#pragma unroll
    for (int kc = 0; kc < KC; kc++) qf[kc] = *reinterpret_cast<const half8_t *>(sm + (wave * 16 + mi) * RS + (32 * kc + 8 * mq) * 2);
    __syncthreads();  // the K / V tiles take the Q image's place

    // ---- one 16-byte chunk of the K | V tile at keys kt0 ..: cached rows from the cache, new rows from the inputs (and into the
    // cache where this tile owns them), rows past the chunk as zeros
    auto fetch = [&](pos_t kt0, KR(&regs)[NCH]) {
#pragma unroll
        for (int u = 0; u < NCH; u++) {
            const int idx = tid + u * NT;
            const int isv = idx / (kPfKT * CPR), rr = (idx / CPR) % kPfKT, ch = idx % CPR;
            const pos_t n = kt0 + rr;
            KR val{};
            if (n < c1 && (!WIN || n >= (pos_t)kmin)) {
                [[maybe_unused]] bool st_ok = true;  // (PAGED: a new row behind an entry outside the pool is not stored)
                if (n < pos0) {
                    val = *(gptr<const KR>)((isv ? Vc : Kc) + row_off(n, rr, st_ok) + 8 * ch);
                } else if constexpr (KV8) {
                    const int tn = (int)(n - pos0);  // < tend <= T
                    u32x4 h16;
                    if (isv) {
                        const float *src = vrows + (long)tn * p.ld_qkv + (long)kh * HD + 8 * ch;
                        uint16_t h[8];
#pragma unroll
                        for (int e = 0; e < 8; e++) h[e] = __builtin_bit_cast(uint16_t, (_Float16)src[e]);
                        h16 = u32x4{(uint32_t)h[0] | (uint32_t)h[1] << 16, (uint32_t)h[2] | (uint32_t)h[3] << 16,
                                    (uint32_t)h[4] | (uint32_t)h[5] << 16, (uint32_t)h[6] | (uint32_t)h[7] << 16};
                    } else {
                        h16 = rope_chunk<HD>(krows + (long)tn * p.ld_qkv + (long)kh * HD, ch, n, p.inv_freq);
                    }
                    val = e4m3_pack8(h16);  // quantised once: these bytes reach the cache and, converted back, the LDS image
                    {
                        const long noff = row_off(n, rr, st_ok);
                        if (tn >= t0 && (!PAGED || st_ok)) *reinterpret_cast<u32x2 *>((isv ? p.vcache : p.kcache) + kvoff + noff + 8 * ch) = val;
                    }
                } else {
                    const int tn = (int)(n - pos0);  // < tend <= T
                    if (isv) {
                        const float *src = vrows + (long)tn * p.ld_qkv + (long)kh * HD + 8 * ch;
                        uint16_t h[8];
#pragma unroll
                        for (int e = 0; e < 8; e++) h[e] = __builtin_bit_cast(uint16_t, (_Float16)src[e]);
                        val = u32x4{(uint32_t)h[0] | (uint32_t)h[1] << 16, (uint32_t)h[2] | (uint32_t)h[3] << 16,
                                    (uint32_t)h[4] | (uint32_t)h[5] << 16, (uint32_t)h[6] | (uint32_t)h[7] << 16};
                    } else {
                        val = rope_chunk<HD>(krows + (long)tn * p.ld_qkv + (long)kh * HD, ch, n, p.inv_freq);
                    }
                    {
                        const long noff = row_off(n, rr, st_ok);
                        if (tn >= t0 && (!PAGED || st_ok)) *reinterpret_cast<u32x4 *>((isv ? p.vcache : p.kcache) + kvoff + noff + 8 * ch) = val;
                    }
                }
            }
            regs[u] = val;
        }
    };
    auto commit = [&](const KR(&regs)[NCH]) {
#pragma unroll
        for (int u = 0; u < NCH; u++) {
            const int idx = tid + u * NT;
            const int row = idx / CPR, ch = idx % CPR;  // rows 0..31: K, 32..63: V
            if constexpr (KV8) *reinterpret_cast<u32x4 *>(sm + row * RS + 16 * ch) = e4m3_half8(regs[u]);
            else *reinterpret_cast<u32x4 *>(sm + row * RS + 16 * ch) = regs[u];
        }
    };

    float m_run = -3.0e38f, l_run = 0.f;  // l_run: this lane's share of its query's sum
    float4_t oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; dt++) oacc[dt] = float4_t{0.f, 0.f, 0.f, 0.f};
    KR regs[NCH];
    // per step: fetch tile k into registers (loads in flight), products of tile k - 1 from LDS, then tile k into LDS
    for (pos_t kt0 = c0;; kt0 += kPfKT) {
        const bool more = kt0 < c1;
        if (more) {
            fetch(kt0, regs);
            tile_pages(kt0 + kPfKT);  // the next tile's, behind this tile's row loads
        }
        if (kt0 > c0) {
            // S^T: lane holds keys kt0 + 16 kt + 4 mq + r of query mi
            float4_t s[2];
    #pragma unroll
            for (int kt = 0; kt < 2; kt++) {
                s[kt] = float4_t{0.f, 0.f, 0.f, 0.f};
    #pragma unroll
                for (int kc = 0; kc < KC; kc++) {
                    const half8_t a = *reinterpret_cast<const half8_t *>(Ks + (16 * kt + mi) * RS + (32 * kc + 8 * mq) * 2);
                    s[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[kc], s[kt], 0, 0, 0);
                }
            }
            float mx = -3.0e38f;
            bool ok[8];
            float sv[8];
    #pragma unroll
            for (int kt = 0; kt < 2; kt++)
    #pragma unroll
                for (int r = 0; r < 4; r++) {
                    const pos_t n = kt0 - kPfKT + 16 * kt + 4 * mq + r;
                    ok[4 * kt + r] = n <= qpos;  // causal (keys past the tile's last row lie past every row of it)
                    if constexpr (WIN) ok[4 * kt + r] = n <= qpos && n >= qlo;  // and the row's own lower edge
                    sv[4 * kt + r] = s[kt][r] * p.scale;
                    if constexpr (!SC) {
                        if (ok[4 * kt + r]) mx = fmaxf(mx, sv[4 * kt + r]);
                    }
                }
            if constexpr (SC) {  // the cap on the tile's eight scores behind ONE wave-uniform test, then the maximum in the same order
                if (p.softcap != 0.f) {
    #pragma unroll
                    for (int e = 0; e < 8; e++) sv[e] = soft_cap(sv[e], p.softcap, p.inv_softcap);
                }
    #pragma unroll
                for (int e = 0; e < 8; e++)
                    if (ok[e]) mx = fmaxf(mx, sv[e]);
            }
            mx = fmaxf(mx, lane_xor<16>(mx));
            mx = fmaxf(mx, lane_xor<32>(mx));
            const float m_new = fmaxf(m_run, mx);
            const float alpha = __expf(m_run - m_new);
            m_run = m_new;
            half8_t pf;
            float ls = 0.f;
    #pragma unroll
            for (int e = 0; e < 8; e++) {
                const _Float16 ph = (_Float16)(ok[e] ? __expf(sv[e] - m_new) : 0.f);
                pf[e] = ph;
                ls += (float)ph;
            }
            l_run = l_run * alpha + ls;
            // O^T[d][query] += V^T P^T: k slot (mq, e) = key 4 mq + e of the first 16 (e < 4), of the second 16 (e >= 4)
    #pragma unroll
            for (int dt = 0; dt < DT; dt++) {
                const unsigned char *va = Vs + (4 * mq + (mi >> 2)) * RS + (16 * dt + 4 * (mi & 3)) * 2;
                const half4_t lo = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_half4_ptr)(va)));
                const half4_t hi = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_half4_ptr)(va + 16 * RS)));
                const half8_t vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                oacc[dt] = oacc[dt] * alpha;
                oacc[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf, oacc[dt], 0, 0, 0);
            }
            __syncthreads();
        }
        if (!more) break;
        commit(regs);
        __syncthreads();
    }
    l_run += lane_xor<16>(l_run);
    l_run += lane_xor<32>(l_run);

    // lane holds O^T[d = 16 dt + 4 mq + r][query mi]
    if (neff == 1) {  // the only chunk
        if (trow < T) {
            uint16_t *orow = orows + (long)trow * p.ld_out + (long)head * HD;
            float inv = 1.f / l_run;
            [[maybe_unused]] float f = 1.f;  // SC: the rescale of the keys' sums to the maximum that includes the sink
            if constexpr (SC) {
                if (p.sinks) {  // the row is finished here: the sink joins the denominator
                    const float sk = p.sinks[head], M = fmaxf(m_run, sk);
                    f = __expf(m_run - M);
                    inv = 1.f / (l_run * f + __expf(sk - M));
                }
            }
#pragma unroll
            for (int dt = 0; dt < DT; dt++)
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    float o = oacc[dt][r];
                    if constexpr (SC) o *= f;
                    orow[16 * dt + 4 * mq + r] = __builtin_bit_cast(uint16_t, (_Float16)(o * inv));
                }
        }
        return;
    }
    const long slot = ((long)kh * p.ntile + jg) * p.nsplit;
    float *wsp = p.part + ((slot + split) * R + wave * 16 + mi) * (HD + 2);
    if (mq == 0) {
        st_agent(wsp, m_run);
        st_agent(wsp + 1, l_run);
    }
#pragma unroll
    for (int dt = 0; dt < DT; dt++)
#pragma unroll
        for (int r = 0; r < 4; r++) st_agent(wsp + 2 + 16 * dt + 4 * mq + r, oacc[dt][r]);
    // ---- ticket: the partial stores are agent-scope (write-through); wait for them, then arrive with an agent-scope release /
    // acquire so that the last arriver sees every other chunk's partials
    unsigned *ticket = p.tickets + kh * (RAGGED ? kPfRaggedTiles : kPfMaxTiles) + jg;
    if (!ticket_last<__ATOMIC_ACQ_REL>(ticket, (unsigned)neff, &flag, tid)) return;
    // ---- last arriver of this (kv head, query tile): merge in chunk order
    const float *base = p.part + slot * R * (HD + 2);
    float *cf = reinterpret_cast<float *>(sm);  // [R][neff] weights exp(m_s - M), then [R] sums
    if (tid < R) {
        float M = -3.0e38f;
        for (int sx = 0; sx < neff; sx++) M = fmaxf(M, ld_agent(base + ((long)sx * R + tid) * (HD + 2)));
        float L = 0.f;
        if constexpr (SC) {
            if (p.sinks) {  // once per row, in front of the chunks' terms
                const float sk = p.sinks[kh * REP + (tid >> 4) % REP];
                M = fmaxf(M, sk);
                L = __expf(sk - M);
            }
        }
        for (int sx = 0; sx < neff; sx++) {
            const float *pp = base + ((long)sx * R + tid) * (HD + 2);
            const float f = __expf(ld_agent(pp) - M);
            cf[tid * neff + sx] = f;
            L += ld_agent(pp + 1) * f;
        }
        cf[R * neff + tid] = L;
    }
    __syncthreads();
    for (int idx = tid; idx < R * HD; idx += NT) {
        const int row = idx / HD, d = idx - row * HD;
        const int w = row >> 4, t = t0 + (w / REP) * 16 + (row & 15);
        float v[kPfMaxSplit];
#pragma unroll
        for (int u = 0; u < kPfMaxSplit; u++) {  // (agent-scope loads issued together)
            const int sx = u < neff ? u : neff - 1;
            v[u] = ld_agent(base + ((long)sx * R + row) * (HD + 2) + 2 + d);
        }
        float o = 0.f;
#pragma unroll
        for (int u = 0; u < kPfMaxSplit; u++)
            if (u < neff) o += v[u] * cf[row * neff + u];
        if (t < T)
            orows[(long)t * p.ld_out + (long)(kh * REP + w % REP) * HD + d] = __builtin_bit_cast(uint16_t, (_Float16)(o / cf[R * neff + row]));
    }
    if (tid == 0) __hip_atomic_store(as_global(ticket), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct PrefillGeometry {
    int nsplit, ntile;
    size_t ws_bytes;
};

// chunks per query tile and the workspace of a launch of `ntile` query tiles per kv head with `tickets` ticket words.  ws_bytes
// is an upper bound of what ANY launch with at most ntile tiles and at most max_len positions needs (monotone in both).
inline void prefill_split(long ntile, long tickets, int nq, int nkv, int hd, long max_len, PrefillGeometry &g) {
    const int rep = nq / nkv, tq = 16 * pf_qs(rep);
    const long tiles = (long)nkv * ntile;
    const long cap = max_len < kPfSplitFrom ? 1 : (max_len + kPfMinChunk - 1) / kPfMinChunk;  // chunks the cache can feed
    const long lim = cap < kPfMaxSplit ? cap : kPfMaxSplit;
    long ns = (256 + tiles - 1) / tiles;  // ~one workgroup per compute unit over the whole launch
    if (ns > lim) ns = lim;
    g.nsplit = (int)ns, g.ntile = (int)ntile;
    if (cap > 1) {
        // slots: tiles * nsplit <= min(256 + tiles, tiles * lim), monotone in ntile and max_len
        const long a = 256 + tiles, b = tiles * lim;
        const long slots = a < b ? a : b;
        g.ws_bytes = ((size_t)tickets + (size_t)slots * tq * rep * (hd + 2)) * sizeof(float);
    }
}

// the positions a windowed launch is sized for: the longest span [kmin & ~31, kend) a query tile can have — window - 1 keys below
// the tile's first row, its 16 pf_qs(rep) rows, 31 keys down to the multiple of 32 — or max_len where that is shorter
inline long prefill_window_positions(long window, int rep, long max_len) {
    const long span = window + 16 * pf_qs(rep) + 30;
    return window >= max_len || span >= max_len ? max_len : span;
}

}  // namespace

}  // namespace qpal
