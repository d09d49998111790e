// Wide prompt prefill attention of ONE sequence (qpal_attn_rope_prefill_wide): 129 .. 256 new tokens at positions
// *pos0 .. *pos0 + T - 1 in TWO launches on one stream.  The contract is qpal_attn_rope_prefill's: rotary embedding of q and k,
// k and v appended at rows *pos0 + t, causal attention of row t over positions 0 .. *pos0 + t; *pos0 < 0 or *pos0 + T > max_len:
// neither launch does anything.
//
// 1. rope_append_wide_kernel: a thread owns eight consecutive dims of one head of one new row.  It rotates them with rope_chunk
//    (attn_prefill.h: qpal_rope_kv's arithmetic) — q as fp16 into the scratch [T][nq * hd] of the workspace, k into the cache — or
//    rounds v to fp16 into the cache; e4m3 caches take e4m3_pack8 of those fp16 values (kv8.h).  Every row is rotated ONCE.
// 2. attn_prefill_wide_kernel: every key, the new rows included, comes from the cache (stream order behind launch 1), so a new row
//    takes part at its stored, dequantised value by construction.
//    Workgroup = (kv head, tile of TQ query rows, chunk of that tile's keys), NW = REP * QS waves:
//        REP (query heads per kv head)    1     2     4     8
//        QS  (32-row sub-tiles)           4     4     2     1
//        NW  (waves)                      4     8     8     8
//        TQ  (query rows)               128   128    64    32
//    wave = (ONE query head, 32 query rows) = two groups of 16 MFMA columns, Q as B fragments in registers from the scratch.
//    Keys go in tiles of 64 through TWO LDS slots (K rows [64] | V rows [64], 2 hd + 16 bytes a row, the fp16 image whatever the
//    cache format): tile i + 1 travels global -> registers -> slot (i + 1) & 1 while tile i is multiplied out of slot i & 1; ONE
//    barrier per tile (a slot is overwritten one barrier behind its last reader).  Per tile and wave, g = 0, 1 the column groups:
//        S^T[g][key][query] = K Q^T     every K fragment read from LDS (ds_read_b128) feeds two v_mfma_f32_16x16x32_f16
//        online softmax per query       a column of S^T = one lane & 15: 16 registers and lanes ^ 16, ^ 32; ONE rescale per 64 keys
//        O^T[g][d][query] += V^T P^T    B = P^T from the S^T registers (attn_prefill.hip's slot order, per 32-key half), A = V^T by
//                                       ds_read_b64_tr_b16; every V fragment feeds two MFMAs
//    The causal mask runs only in tiles that reach past the wave's first row (a wave-uniform test); a wave skips the products of a
//    tile that lies wholly past its last row.  Rows >= T are zero columns, never stored, and a column's maximum is its own.
//    Chunks (multiples of 64 keys, at least 128) leave (max, sum, unnormalised out) per row in the workspace and take a ticket;
//    the last arriver merges in chunk order and resets the ticket: attn_prefill.h's pattern, bitwise reproducible, no host read.
#include "attn_prefill.h"

namespace qpal {

namespace {

constexpr int kPwMinT = kAttnMaxRows + 1, kPwMaxT = 2 * kAttnMaxRows;
constexpr int kPwKT = 64;  // keys per tile

constexpr int pw_qs(int rep) { return rep == 1 ? 4 : 8 / rep; }  // 32-row query sub-tiles per workgroup (the table above)

// ---- launch 1: the T new rows, rotated once
template <class CT, bool PAGED, int HD>
__global__ __launch_bounds__(256) void rope_append_wide_kernel(const AttnPrefillParams<CT> p, uint16_t *qs, int nq) {
    constexpr bool KV8 = kIsKv8<CT>;
    constexpr int CPR = HD / 8;
    const long pos0 = *p.pos0;
    if (pos0 < 0 || pos0 > p.max_len - p.T) return;
    const int heads = nq + 2 * p.nkv;
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= p.T * heads * CPR) return;
    const int ch = idx % CPR, h = (idx / CPR) % heads, t = idx / (CPR * heads);
    const long n = pos0 + t;
    if (h < nq) {
        const u32x4 val = rope_chunk<HD>(p.q + (long)t * p.ld_qkv + (long)h * HD, ch, n, p.inv_freq);
        *reinterpret_cast<u32x4 *>(qs + ((long)t * nq + h) * HD + 8 * ch) = val;
        return;
    }
    const bool isv = h >= nq + p.nkv;
    const int kh = h - nq - (isv ? p.nkv : 0);
    u32x4 val;
    if (isv) {
        const float *src = p.v + (long)t * p.ld_qkv + (long)kh * HD + 8 * ch;
        uint16_t e[8];
#pragma unroll
        for (int i = 0; i < 8; i++) e[i] = __builtin_bit_cast(uint16_t, (_Float16)src[i]);
        val = u32x4{(uint32_t)e[0] | (uint32_t)e[1] << 16, (uint32_t)e[2] | (uint32_t)e[3] << 16,
                    (uint32_t)e[4] | (uint32_t)e[5] << 16, (uint32_t)e[6] | (uint32_t)e[7] << 16};
    } else {
        val = rope_chunk<HD>(p.k + (long)t * p.ld_qkv + (long)kh * HD, ch, n, p.inv_freq);
    }
    long off;
    if constexpr (PAGED) {
        const int pg = p.table[n >> p.page_shift];
        if (!page_ok(pg, p.num_pages)) return;  // an entry outside the pool: the row is dropped
        off = paged_row<HD>(pg, p.nkv, kh, p.page_shift, n);
    } else {
        off = ((long)kh * p.max_len + n) * HD;
    }
    CT *dst = (isv ? p.vcache : p.kcache) + off + 8 * ch;
    if constexpr (KV8) *reinterpret_cast<u32x2 *>(dst) = e4m3_pack8(val);
    else *reinterpret_cast<u32x4 *>(dst) = val;
}

// ---- launch 2
template <class CT, bool PAGED, int HD, int REP>
__global__ __launch_bounds__(64 * REP * pw_qs(REP)) void attn_prefill_wide_kernel(const AttnPrefillParams<CT> p, const uint16_t *qs, int nq) {
    constexpr bool KV8 = kIsKv8<CT>;
    using KR = std::conditional_t<KV8, u32x2, u32x4>;  // eight elements of a cache row as prefetched
    constexpr int QS = pw_qs(REP), NW = REP * QS, NT = 64 * NW, TQ = 32 * QS, R = 32 * NW;
    constexpr int KC = HD / 32, DT = HD / 16, CPR = HD / 8;
    constexpr int RS = 2 * HD + 16;             // bytes of an LDS row (padded by one 16-byte access)
    constexpr int SLOT = 2 * kPwKT * RS;        // K [64] | V [64]
    constexpr int NCH = 2 * kPwKT * CPR / NT;   // 16-byte chunks of a K + V tile per thread
    static_assert(2 * kPwKT * CPR % NT == 0, "the K + V tile is cut evenly over the threads");
    static_assert((size_t)2 * SLOT >= (size_t)(R * kPfMaxSplit + R) * sizeof(float), "the merge coefficients fit the tile slots");
    static_assert(NT >= R, "one thread per row of the merge");
    __shared__ __attribute__((aligned(16))) unsigned char sm[2 * SLOT];
    __shared__ unsigned flag;

    const long pos0l = *p.pos0;
    if (pos0l < 0 || pos0l > p.max_len - p.T) return;  // outside the cache: nothing is read or written, no ticket taken
    const int pos0 = (int)pos0l;                       // (max_len < 2^30)
    const int T = p.T;
    const int per_kh = p.ntile * p.nsplit;
    const int kh = blockIdx.x / per_kh, rem = blockIdx.x - kh * per_kh;
    const int jg = rem / p.nsplit, split = rem - jg * p.nsplit;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int mi = lane & 15, mq = lane >> 4;
    const int t0 = jg * TQ, tend = t0 + TQ < T ? t0 + TQ : T;  // query rows of the tile: [t0, tend)
    const int kend = pos0 + tend;                              // its keys: [0, kend)
    int cld = (kend + kPwKT - 1) & ~(kPwKT - 1);
    if (p.nsplit > 1) {
        cld = ((kend + p.nsplit - 1) / p.nsplit + kPwKT - 1) & ~(kPwKT - 1);
        if (cld < (int)kPfMinChunk) cld = (int)kPfMinChunk;
    }
    const int neff = (kend + cld - 1) / cld;  // chunks that hold keys: the same in every workgroup of the tile
    if (split >= neff) return;
    const int c0 = split * cld, c1 = c0 + cld < kend ? c0 + cld : kend;
    const int hh = wave % REP, qsub = wave / REP;
    const int head = kh * REP + hh;
    const int tw = t0 + qsub * 32;                     // the wave's first query row
    const int qminw = pos0 + tw, qmaxw = qminw + 31;  // the positions of its first and last row

    const gptr<const CT> Kc = as_global((const CT *)p.kcache) + (PAGED ? 0L : (long)kh * p.max_len * HD);
    const gptr<const CT> Vc = as_global((const CT *)p.vcache) + (PAGED ? 0L : (long)kh * p.max_len * HD);
    // PAGED: the page ids of the four 16-key quarters of the tile about to be fetched (a tile starts at a multiple of 64, so a
    // quarter lies in one page), read one tile ahead of the rows and only where the chunk reaches
    [[maybe_unused]] int pg[4] = {0, 0, 0, 0};
    auto tile_pages = [&]([[maybe_unused]] int kt0) {
        if constexpr (PAGED) {
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (kt0 + 16 * u < c1) {
                    const int e = p.table[(kt0 + 16 * u) >> p.page_shift];
                    pg[u] = page_ok(e, p.num_pages) ? e : 0;  // an entry outside the pool reads page 0
                }
        }
    };
    // ---- one 16-byte chunk per (u) of the K | V tile at keys kt0 ..: rows of the chunk from the cache, rows past it as zeros
    auto fetch = [&](int kt0, KR(&regs)[NCH]) {
#pragma unroll
        for (int u = 0; u < NCH; u++) {
            const int idx = tid + u * NT;
            const int isv = idx / (kPwKT * CPR), rr = (idx / CPR) % kPwKT, ch = idx % CPR;
            const int n = kt0 + rr;
            KR val{};
            if (n < c1) {
                long off;
                if constexpr (PAGED) {
                    const int q4 = rr >> 4;
                    const int page = q4 == 0 ? pg[0] : q4 == 1 ? pg[1] : q4 == 2 ? pg[2] : pg[3];
                    off = paged_row<HD>(page, p.nkv, kh, p.page_shift, n);
                } else {
                    off = (long)n * HD;
                }
                val = *(gptr<const KR>)((isv ? Vc : Kc) + off + 8 * ch);
            }
            regs[u] = val;
        }
    };
    auto commit = [&](const KR(&regs)[NCH], unsigned char *slot) {
#pragma unroll
        for (int u = 0; u < NCH; u++) {
            const int idx = tid + u * NT;
            const int row = idx / CPR, ch = idx % CPR;  // rows 0..63: K, 64..127: V
            if constexpr (KV8) *reinterpret_cast<u32x4 *>(slot + row * RS + 16 * ch) = e4m3_half8(regs[u]);
            else *reinterpret_cast<u32x4 *>(slot + row * RS + 16 * ch) = regs[u];
        }
    };

    KR regs[NCH];
    tile_pages(c0);
    fetch(c0, regs);
    tile_pages(c0 + kPwKT);

    // ---- the wave's 2 x 16 rotated query rows as B fragments, straight from the scratch (rows >= T: zeros)
    half8_t qf[2][KC];
#pragma unroll
    for (int g = 0; g < 2; g++) {
        const int t = tw + 16 * g + mi;
#pragma unroll
        for (int kc = 0; kc < KC; kc++) {
            u32x4 w{0u, 0u, 0u, 0u};
            if (t < T) w = *(gptr<const u32x4>)(as_global(qs) + ((long)t * nq + head) * HD + 32 * kc + 8 * mq);
            qf[g][kc] = __builtin_bit_cast(half8_t, w);
        }
    }

    float m_run[2] = {-3.0e38f, -3.0e38f}, l_run[2] = {0.f, 0.f};  // l_run: this lane's share of its query's sum
    float4_t oacc[2][DT];
#pragma unroll
    for (int g = 0; g < 2; g++)
#pragma unroll
        for (int dt = 0; dt < DT; dt++) oacc[g][dt] = float4_t{0.f, 0.f, 0.f, 0.f};

    // the products of the 64-key tile at kt0 out of `slot`
    auto tile = [&](int kt0, const unsigned char *slot) {
        const unsigned char *const Ks = slot, *const Vs = slot + kPwKT * RS;
        // S^T: lane holds keys kt0 + 16 kt + 4 mq + r of queries tw + 16 g + mi
        float4_t s[2][4];
#pragma unroll
        for (int kt = 0; kt < 4; kt++) {
            s[0][kt] = s[1][kt] = float4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kc = 0; kc < KC; kc++) {
                const half8_t a = *reinterpret_cast<const half8_t *>(Ks + (16 * kt + mi) * RS + (32 * kc + 8 * mq) * 2);
                s[0][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[0][kc], s[0][kt], 0, 0, 0);
                s[1][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qf[1][kc], s[1][kt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int g = 0; g < 2; g++)
#pragma unroll
            for (int kt = 0; kt < 4; kt++) s[g][kt] = s[g][kt] * p.scale;
        // the causal mask, only in a tile that reaches past the wave's first row (wave-uniform); keys past the chunk's end lie
        // past every stored row
        if (kt0 + kPwKT - 1 > qminw) {
#pragma unroll
            for (int g = 0; g < 2; g++)
#pragma unroll
                for (int kt = 0; kt < 4; kt++)
#pragma unroll
                    for (int r = 0; r < 4; r++)
                        if (kt0 + 16 * kt + 4 * mq + r > qminw + 16 * g + mi) s[g][kt][r] = -__builtin_inff();
        }
        half8_t pf[2][2];  // P^T of the tile's two 32-key halves
#pragma unroll
        for (int g = 0; g < 2; g++) {
            float sv[16];
            float mx = -3.0e38f;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                sv[e] = s[g][e >> 2][e & 3];
                mx = fmaxf(mx, sv[e]);
            }
            mx = fmaxf(mx, lane_xor<16>(mx));
            mx = fmaxf(mx, lane_xor<32>(mx));
            const float m_new = fmaxf(m_run[g], mx);  // >= -3e38: exp(-inf - m_new) = 0 for a masked key
            const float alpha = __expf(m_run[g] - m_new);
            m_run[g] = m_new;
            float ls = 0.f;
#pragma unroll
            for (int e = 0; e < 16; e++) {
                const _Float16 ph = (_Float16)__expf(sv[e] - m_new);
                pf[g][e >> 3][e & 7] = ph;
                ls += (float)ph;
            }
            l_run[g] = l_run[g] * alpha + ls;
#pragma unroll
            for (int dt = 0; dt < DT; dt++) oacc[g][dt] = oacc[g][dt] * alpha;
        }
        // O^T[d][query] += V^T P^T per 32-key half: k slot (mq, e) = key 4 mq + e of its first 16 keys (e < 4), of its second (e >= 4)
#pragma unroll
        for (int dt = 0; dt < DT; dt++)
#pragma unroll
            for (int h = 0; h < 2; h++) {
                const unsigned char *va = Vs + (32 * h + 4 * mq + (mi >> 2)) * RS + (16 * dt + 4 * (mi & 3)) * 2;
                const half4_t lo = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_half4_ptr)(va)));
                const half4_t hi = __builtin_bit_cast(half4_t, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_half4_ptr)(va + 16 * RS)));
                const half8_t vf = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
                oacc[0][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[0][h], oacc[0][dt], 0, 0, 0);
                oacc[1][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pf[1][h], oacc[1][dt], 0, 0, 0);
            }
    };

    commit(regs, sm);
    __syncthreads();
    // per step: tile i + 1 into registers (loads in flight), the products of tile i out of slot i & 1, tile i + 1 into the other slot
    const int ntl = (c1 - c0 + kPwKT - 1) / kPwKT;
    for (int i = 0; i < ntl; i++) {
        const int kt0 = c0 + i * kPwKT;
        const bool more = i + 1 < ntl;
        if (more) {
            fetch(kt0 + kPwKT, regs);
            tile_pages(kt0 + 2 * kPwKT);
        }
        const unsigned char *slot = sm + (i & 1) * SLOT;
        if (kt0 <= qmaxw) tile(kt0, slot);  // (else: every key of the tile lies past every row of the wave)
        if (more) commit(regs, sm + ((i + 1) & 1) * SLOT);
        __syncthreads();
    }
#pragma unroll
    for (int g = 0; g < 2; g++) {
        l_run[g] += lane_xor<16>(l_run[g]);
        l_run[g] += lane_xor<32>(l_run[g]);
    }

    // lane holds O^T[g][d = 16 dt + 4 mq + r][query mi]
    if (neff == 1) {  // the only chunk
#pragma unroll
        for (int g = 0; g < 2; g++) {
            const int t = tw + 16 * g + mi;
            if (t < T) {
                uint16_t *orow = p.out + (long)t * p.ld_out + (long)head * HD;
                const float inv = 1.f / l_run[g];
#pragma unroll
                for (int dt = 0; dt < DT; dt++)
#pragma unroll
                    for (int r = 0; r < 4; r++) orow[16 * dt + 4 * mq + r] = __builtin_bit_cast(uint16_t, (_Float16)(oacc[g][dt][r] * inv));
            }
        }
        return;
    }
    const long slot0 = ((long)kh * p.ntile + jg) * p.nsplit;
#pragma unroll
    for (int g = 0; g < 2; g++) {
        float *wsp = p.part + ((slot0 + split) * R + wave * 32 + 16 * g + mi) * (HD + 2);
        if (mq == 0) {
            st_agent(wsp, m_run[g]);
            st_agent(wsp + 1, l_run[g]);
        }
#pragma unroll
        for (int dt = 0; dt < DT; dt++)
#pragma unroll
            for (int r = 0; r < 4; r++) st_agent(wsp + 2 + 16 * dt + 4 * mq + r, oacc[g][dt][r]);
    }
    // ---- ticket (attn_common.h), then the last arriver of this (kv head, query tile) merges in chunk order
    unsigned *ticket = p.tickets + kh * kPfMaxTiles + jg;
    if (!ticket_last<__ATOMIC_ACQ_REL>(ticket, (unsigned)neff, &flag, tid)) return;
    const float *base = p.part + slot0 * R * (HD + 2);
    float *cf = reinterpret_cast<float *>(sm);  // [R][neff] weights exp(m_s - M), then [R] sums
    if (tid < R) {
        float M = -3.0e38f;
        for (int sx = 0; sx < neff; sx++) M = fmaxf(M, ld_agent(base + ((long)sx * R + tid) * (HD + 2)));
        float L = 0.f;
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
        const int w = row >> 5, t = t0 + (w / REP) * 32 + (row & 31);
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
            p.out[(long)t * p.ld_out + (long)(kh * REP + w % REP) * HD + d] = __builtin_bit_cast(uint16_t, (_Float16)(o / cf[R * neff + row]));
    }
    if (tid == 0) __hip_atomic_store(as_global(ticket), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

struct WideGeometry {
    int nsplit, ntile;
    size_t part_off, qs_off, ws_bytes;  // tickets at 0 (where the 128-row launches keep theirs), partials, the q scratch
};

inline size_t up16(size_t n) { return (n + 15) & ~(size_t)15; }

// Launch geometry from (T, heads, max_len) only.  ws_bytes is monotone in T and max_len and never below the 128-row launches'
// workspace of the same heads and max_len, whose ticket words it shares: one workspace serves the wide chunks and the short last one.
int wide_geometry(int T, int nq, int nkv, int hd, long max_len, WideGeometry &g) {
    g = WideGeometry{0, 0, 0, 0, 0};
    if (T < kPwMinT || T > kPwMaxT) return QPAL_E_SHAPE;
    const int rc = attn_shape(kAttnMaxRows, nq, nkv, hd, max_len);
    if (rc != QPAL_OK) return rc;
    if (hd == 256) return QPAL_E_SHAPE;  // not built: two 128-row launches serve it
    const int rep = nq / nkv, tq = 32 * pw_qs(rep);
    const long ntile = (T + tq - 1) / tq, tiles = (long)nkv * ntile;
    const long cap = max_len < kPfSplitFrom ? 1 : (max_len + kPfMinChunk - 1) / kPfMinChunk;  // chunks the cache can feed
    const long lim = cap < kPfMaxSplit ? cap : kPfMaxSplit;
    long ns = (256 + tiles - 1) / tiles;  // ~one workgroup per compute unit
    if (ns > lim) ns = lim;
    g.nsplit = (int)ns, g.ntile = (int)ntile;
    // slots: tiles * nsplit <= min(256 + tiles, tiles * lim), monotone in T and max_len
    const long a = 256 + tiles, b = tiles * lim;
    const size_t part = cap > 1 ? (size_t)(a < b ? a : b) * tq * rep * (hd + 2) * sizeof(float) : 0;
    PrefillGeometry narrow{0, 0, 0};
    prefill_split(kPfMaxTiles / pf_qs(rep), (long)nkv * kPfMaxTiles, nq, nkv, hd, max_len, narrow);
    g.part_off = up16((size_t)nkv * kPfMaxTiles * sizeof(unsigned));
    const size_t body = g.part_off + up16(part);
    g.qs_off = up16(body > narrow.ws_bytes ? body : narrow.ws_bytes);
    g.ws_bytes = g.qs_off + up16((size_t)T * nq * hd * sizeof(uint16_t));
    return QPAL_OK;
}

// the wide family of attn_launch: no windows and no score modifiers; both launches on c.stream
struct PrefillWide {
    static constexpr bool kContig = true, kMods = false;

    bool any_null() const { return false; }

    template <class CT, bool PAGED, bool, bool>
    int launch(const AttnCall &c, const AttnVariant &v, int shift, long max_len) const {
        const int T = c.rows, nq = c.nq, nkv = c.nkv;
        WideGeometry g;
        int rc = wide_geometry(T, nq, nkv, c.hd, max_len, g);
        if (rc != QPAL_OK) return rc;
        rc = attn_args(c, v, g.ws_bytes);
        if (rc != QPAL_OK) return rc;
        if (reinterpret_cast<uintptr_t>(c.ws) & 15) return QPAL_E_ALIGN;  // the q scratch is read 16 bytes at a time
        unsigned char *wsb = static_cast<unsigned char *>(c.ws);
        uint16_t *qs = reinterpret_cast<uint16_t *>(wsb + g.qs_off);
        const int grid = nkv * g.ntile * g.nsplit, rope_grid = (T * (nq + 2 * nkv) * (c.hd / 8) + 255) / 256;
        AttnPrefillParams<CT> p{c.q, c.k, c.v, c.ld_qkv, static_cast<CT *>(c.kcache), static_cast<CT *>(c.vcache),
                                static_cast<uint16_t *>(c.out_f16), c.ld_out, c.pos, c.inv_freq, T, nkv, max_len, c.scale,
                                reinterpret_cast<unsigned *>(wsb), reinterpret_cast<float *>(wsb + g.part_off), g.nsplit, g.ntile};
        p.table = v.pg.table, p.num_pages = v.pg.num_pages, p.page_shift = shift;
        return for_hd_rep(c.hd, nq / nkv, [&](auto HD, auto REP) {
            if constexpr (HD() == 256) {
                return (int)QPAL_E_SHAPE;
            } else {
                hipLaunchKernelGGL((rope_append_wide_kernel<CT, PAGED, HD()>), dim3(rope_grid), dim3(256), 0,
                                   static_cast<hipStream_t>(c.stream), p, qs, nq);
                hipLaunchKernelGGL((attn_prefill_wide_kernel<CT, PAGED, HD(), REP()>), dim3(grid), dim3(64 * REP() * pw_qs(REP())), 0,
                                   static_cast<hipStream_t>(c.stream), p, static_cast<const uint16_t *>(qs), nq);
                return (int)hipGetLastError();
            }
        });
    }
};

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" long qpal_attn_prefill_wide_ws_bytes(int T, int nq, int nkv, int hd, long max_len) {
    WideGeometry g;
    if (wide_geometry(T, nq, nkv, hd, max_len, g) != QPAL_OK) return 0;
    return (long)g.ws_bytes;
}

extern "C" int qpal_attn_rope_prefill_wide(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                           void *out_f16, long ld_out, const long *pos0, const float *inv_freq, const int *block_row,
                                           int num_pages, int page_size, int max_pages, int kv_fmt, int T, int nq, int nkv, int hd,
                                           long max_len, float scale, void *ws, long ws_bytes, void *stream) {
    return attn_launch({q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos0, inv_freq, T, nq, nkv, hd, scale, ws, ws_bytes, stream},
                       {.pg = {block_row, max_pages, num_pages, page_size, max_pages}, .kv_fmt = kv_fmt, .max_len = max_len}, PrefillWide{});
}
