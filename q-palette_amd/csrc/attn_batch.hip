// Decode attention of B concurrent sequences in one launch (qpal_attn_rope_decode_batch): for every sequence b with 0 <= pos[b] <
// max_len, rotary embedding of its new q and k (qpal_rope_kv's convention: rotate_half, cos / sin of pos * inv_freq rounded to
// fp16, fp16 arithmetic), k and v appended to ITS cache at row pos[b], and softmax(q k^T * scale) v over its positions 0 .. pos[b].
// A sequence whose position lies outside the cache is inactive: nothing of it is read or written.
//
// Shape: the group form of decoder_glue.hip's split-context kernel with a batch dimension.  Workgroup = (sequence, kv head,
// chunk of that sequence's context) and serves all REP = nq / nkv query heads of its group, so a K / V row is read once per group
// and only rows <= pos[b] are read at all (bytes ~ sum_b (pos[b] + 1), not B * max_len).  The host fixes the grid from (B, nkv,
// max_len) alone — *pos is never read on the host, the launch stays graph-capturable with positions that change between
// replays — and every workgroup cuts the context that EXISTS for its sequence into at most `nsplit` chunks itself, leaving at
// once when its chunk is empty.  Small B with long contexts still spreads over the compute units; at large B (nsplit = 1) a
// sequence is one workgroup per kv head and nothing is merged.  Chunks of one (sequence, kv head) leave a partial (max, sum,
// unnormalised out) per head in the workspace and take a ticket; the last to arrive merges them in a fixed order (bitwise
// reproducible: no float atomics) and resets the ticket.
//
// The cache element type CT is a template parameter: uint16_t = fp16 (qpal_attn_rope_decode_batch), uint8_t = OCP e4m3fn
// (qpal_attn_rope_decode_batch_kv8, kv8.h).  The e4m3 instantiation differs at the load, convert and store sites
// only: a byte row is converted exactly to the fp16 values the matrix pipe and the value loop take today, the new row is quantised
// once and takes part at its stored value.  LDS layout, workspace and grid do not depend on CT.
//
// PAGED (qpal_attn_rope_decode_batch_paged, kv_paged.h): the caches are pools [num_pages][nkv][page_size][HD] and a
// sequence's position n lives in page table[b][n / page_size].  The instantiation differs in the address of a cache row only:
// every load and store site takes its row through paged_row(); the page ids of a step are loaded one step ahead of the rows they
// address (the first step's before the rotary embedding), so the lookup is not in front of the K / V loads.  Arithmetic, its order,
// LDS layout, workspace and grid are those of the contiguous launch with max_len = max_pages * page_size.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "attn_common.h"
#include "attn_prefix.h"
#include "kv8.h"

namespace qpal {

namespace {

constexpr int kBatchMax = kAttnMaxRows;
constexpr long kBatchSplitFrom = 512; // caches shorter than this: one chunk per (sequence, kv head), no workspace
constexpr long kBatchMinChunk = 128;  // a chunk holds at least this many positions (fewer: the merge costs more than it saves)
constexpr int kBatchNW = 16;          // waves per workgroup
constexpr int kBatchMaxSplit = 64;
constexpr size_t kBatchLdsMax = 160 * 1024;

template <class CT>
struct AttnBatchParams {
    const float *q, *k, *v;  // fp32 rows [B][ld_qkv]: q [nq * HD], k / v [nkv * HD] inside a row
    long ld_qkv;
    CT *kcache, *vcache;        // fp16 (uint16_t) or e4m3fn (uint8_t) [B][nkv][max_len][HD]
    uint16_t *out;              // fp16 [B][ld_out]
    long ld_out;
    const long *pos;            // int64 [B], device
    const float *inv_freq;      // fp32 [HD / 2]
    int nkv;
    long max_len;
    float scale;
    unsigned *tickets;          // [kBatchMax * nkv] (zero-filled once)
    float *part;                // [B * nkv * nsplit][REP][HD + 2] partials
    int nsplit, chunk;          // chunk: LDS score capacity per head (multiple of 64, nsplit * chunk >= max_len)
    // PAGED only: kcache / vcache are the pools [num_pages][nkv][1 << page_shift][HD], max_len = max_pages << page_shift
    const int *table;           // int32 [B][ld_table], device
    long ld_table;
    int num_pages, page_shift;
    // SHARED only (qpal_attn_rope_decode_batch_shared, attn_prefix.h): the sharing of the launch, its B, and the
    // merged prefix partials [B][nkv * REP][HD + 2] the prefix launch left in front of this one in the stream
    SharedPrefixArgs sp;
    int B;
    const float *pre;
    // WIN only (qpal_attn_rope_decode_batch_window): sequence b attends to [max(0, pos[b] - window + 1), pos[b]]
    long window;
    // SC only (qpal_attn_rope_decode_batch_score): softcap 0 — no cap, else every score is softcap * tanh(score /
    // softcap) (inv_softcap = 1 / softcap); sinks null — none, else fp32 [nq], one logit per query head in the row's denominator
    float softcap, inv_softcap;
    const float *sinks;
};

// SHARED (PAGED only): a member of a group (shared_prefix_len) attends to [grp_len, pos] through its own table row — the chunk
// formulas below applied to pos - start, so start = 0 is the plain launch — and every finishing path folds the row's prefix partial
// in, as the chunk in front of the row's own, before the division.  An ordinary slot takes the plain launch's arithmetic.
//
// WIN (sliding window): start = lo(pos) = max(0, pos - window + 1) in the same place, with no partial in front:
// the plain launch's arithmetic on the keys [lo, pos].  lo is arbitrary (SHARED's starts are page-aligned): every row address
// below is c0 + t with t relative to the chunk, the LDS scores are indexed by t alone, and the paged lookups take (c0 + t) >>
// page_shift per lane (scores) or per wave (values), so nothing depends on c0's alignment.  No row and no table entry below lo
// is read: the clamp of the rows past the chunk goes to c0 >= lo.  The host sizes nsplit and the LDS chunk for min(max_len,
// window rounded up to 4) positions, which rel = pos - lo never reaches.
//
// SC (score modifiers; built on the WIN body, window = max_len where the launch has none): the soft cap at the two
// places a score is scaled, in front of the maximum; the sink of head h once per row, where the row is finished — the only
// chunk's division or the last arriver's merge — as one more term exp(sink - M) of the denominator with M = max(row maximum,
// sink).  The partials in the workspace stay (m, l, O) of the keys alone.  Both are wave-uniform runtime tests (softcap == 0,
// sinks == nullptr); a sink of -inf gives M = the row's maximum, a rescale of exp(0) = 1 and a term of 0: the bits without sinks.
template <class CT, bool PAGED, int HD, int REP, bool SHARED = false, bool WIN = false, bool SC = false>
__global__ __launch_bounds__(64 * kBatchNW) void attn_rope_batch_kernel(const AttnBatchParams<CT> p) {
    constexpr bool KV8 = kIsKv8<CT>;
    constexpr int NW = kBatchNW, NT = 64 * NW, HALF = HD / 2;
    constexpr int LPR = HD / 8, DPL = HD / 64;
    static_assert(REP * HD <= 1024, "partial-out buffer: NW x REP x HD floats of LDS");
    static_assert(NW % REP == 0, "waves split evenly over the heads of a group");
    extern __shared__ float sh[];  // scores [REP][chunk] | q [REP][HD/2 dwords] | new k [HD/2 dwords] | new v [HD] | partial out [NW][REP][HD] | reduce [2 NW REP] | new-position scores, maxima, sums [3 REP] | flag
    const int CL = p.chunk;
    float *sc = sh;
    uint32_t *qh = reinterpret_cast<uint32_t *>(sh + REP * CL), *knh = qh + REP * HALF;
    float *vn = reinterpret_cast<float *>(knh + HALF), *po = vn + HD, *red = po + NW * REP * HD;
    float *park = red + 2 * NW * REP, *mxf = park + REP, *sumf = mxf + REP;
    unsigned *flag = reinterpret_cast<unsigned *>(sumf + REP);
    const int per_seq = p.nkv * p.nsplit;
    const int b = blockIdx.x / per_seq, rem = blockIdx.x - b * per_seq;
    const int kh = rem / p.nsplit, split = rem - kh * p.nsplit;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long pos = p.pos[b];
    if (pos < 0 || pos >= p.max_len) return;  // inactive sequence: nothing is read or written, no ticket taken
    // the context that exists, cut evenly over the splits (chunks of a multiple of 64 positions, at least kBatchMinChunk, at most
    // the LDS capacity); chunks 0 .. neff-1 hold positions <= pos, the last of them the new one
    // (32-bit unsigned divisions: positions are below max_len < 2^30)
    [[maybe_unused]] long start = 0;  // SHARED: the positions the prefix launch has served for this slot; WIN: lo(pos)
    static_assert(!(SHARED && WIN), "no window in the shared-prefix launches");
    static_assert(!SC || WIN, "the score modifiers are built on the windowed body");
    if constexpr (SHARED) {
        static_assert(PAGED, "groups share pages");
        int g;
        start = shared_prefix_len(p.sp, b, pos, p.B, p.page_shift, p.max_len, g);
    }
    if constexpr (WIN) start = pos >= p.window ? pos - p.window + 1 : 0;
    const long rel = (SHARED || WIN) ? pos - start : pos;
    long cld = CL;
    if (p.nsplit > 1) {
        cld = (long)((((unsigned)rel + (unsigned)p.nsplit) / (unsigned)p.nsplit + 63u) & ~63u);
        if (cld < kBatchMinChunk) cld = kBatchMinChunk;
        if (cld > CL) cld = CL;
    }
    const long c0 = ((SHARED || WIN) ? start : 0) + (long)split * cld;
    const int neff = (int)((unsigned)rel / (unsigned)cld) + 1;
    if (split >= neff) return;
    const bool owner = split == neff - 1;                    // this chunk holds the new position
    const long cend = pos < c0 + cld ? pos : c0 + cld;       // cached positions of the chunk: [c0, cend)
    const int nc = cend > c0 ? (int)(cend - c0) : 0;
    const long kvoff = PAGED ? 0 : ((long)b * p.nkv + kh) * p.max_len * HD;
    const gptr<const CT> K = as_global(p.kcache) + kvoff, V = as_global(p.vcache) + kvoff;
    // element offset of the new row from the cache base, and whether it is stored (PAGED: a page id outside the pool drops it)
    [[maybe_unused]] long newoff_pg = 0;
    [[maybe_unused]] bool new_ok = true;
    auto new_k_row = [&] {
        if constexpr (PAGED) return p.kcache + newoff_pg;
        else return p.kcache + kvoff + pos * HD;
    };
    auto new_off = [&] {
        if constexpr (PAGED) return newoff_pg;
        else return kvoff + pos * HD;
    };
    [[maybe_unused]] const int *tab = nullptr;
    [[maybe_unused]] int kpg[KV8 ? 4 : 2];  // PAGED: this lane's page ids of the next step of the score loop
    // offset of cached row c0 + t of this chunk: PAGED through page id `page` (outside the pool: page 0 is read instead)
    auto row_off = [&](long n, [[maybe_unused]] int page) {
        if constexpr (PAGED) return paged_row<HD>(page_ok(page, p.num_pages) ? page : 0, p.nkv, kh, p.page_shift, n);
        else return n * HD;
    };
    if constexpr (PAGED) {
        tab = p.table + (long)b * p.ld_table;
        if (owner) {
            const int pg = tab[pos >> p.page_shift];
            new_ok = page_ok(pg, p.num_pages);
            newoff_pg = paged_row<HD>(pg, p.nkv, kh, p.page_shift, pos);
        }
#pragma unroll
        for (int u = 0; u < (KV8 ? 4 : 2); u++) {  // (positions clamped to the chunk's first: entries <= pos only)
            const int t = (tid >> 6) * 16 + u * NW * 16 + (tid & 15);
            kpg[u] = tab[(c0 + (t < nc ? t : 0)) >> p.page_shift];
        }
    }
    const float *qrow = p.q + (long)b * p.ld_qkv, *krow = p.k + (long)b * p.ld_qkv, *vrow = p.v + (long)b * p.ld_qkv;
    uint16_t *orow = p.out + (long)b * p.ld_out + (long)kh * REP * HD;
    const long slot = ((long)b * p.nkv + kh) * p.nsplit;
    float *wsp = p.part + (slot + split) * REP * (HD + 2);
    unsigned *ticket = p.tickets + (long)b * p.nkv + kh;

    // ---- new token: rope of the group's REP query heads (+ k, v in the chunk that owns the new position)
    for (int idx = tid; idx < (REP + 1) * HALF; idx += NT) {
        const int hh = idx / HALF, i = idx - hh * HALF;
        const bool is_k = hh == REP;
        if (is_k && !owner) continue;
        const float *src = is_k ? krow + (long)kh * HD : qrow + (long)(kh * REP + hh) * HD;
        const float ang = (float)pos * p.inv_freq[i];
        const _Float16 c = (_Float16)cosf(ang), s = (_Float16)sinf(ang);
        const _Float16 x1 = (_Float16)src[i], x2 = (_Float16)src[i + HALF];
        const _Float16 o1 = x1 * c + (-x2) * s, o2 = x2 * c + x1 * s;
        uint16_t *dst16 = reinterpret_cast<uint16_t *>(is_k ? knh : qh + hh * HALF);
        if constexpr (KV8) {
            if (is_k) {  // quantised once: the bytes go to the cache, their fp16 image to this launch's scores
                const uint32_t b8 = e4m3_pack2(o1, o2), h2 = e4m3_half2<false>(b8);
                dst16[i] = (uint16_t)h2;
                dst16[i + HALF] = (uint16_t)(h2 >> 16);
                CT *dst = new_k_row();
                if (!PAGED || new_ok) {
                    dst[i] = (CT)b8;
                    dst[i + HALF] = (CT)(b8 >> 8);
                }
                continue;
            }
        }
        dst16[i] = __builtin_bit_cast(uint16_t, o1);
        dst16[i + HALF] = __builtin_bit_cast(uint16_t, o2);
        if constexpr (!KV8) {
            if (is_k && (!PAGED || new_ok)) {
                uint16_t *dst = new_k_row();
                dst[i] = __builtin_bit_cast(uint16_t, o1);
                dst[i + HALF] = __builtin_bit_cast(uint16_t, o2);
            }
        }
    }
    if (owner) {
        for (int d = tid; d < HD; d += NT) {
            const _Float16 hv = (_Float16)vrow[(long)kh * HD + d];
            if constexpr (KV8) {
                const uint32_t b8 = e4m3_pack2(hv, hv);
                vn[d] = e4m3_float2<false>(b8).x;
                if (!PAGED || new_ok) p.vcache[new_off() + d] = (CT)b8;
            } else {
                vn[d] = (float)hv;
                if (!PAGED || new_ok) p.vcache[new_off() + d] = __builtin_bit_cast(uint16_t, hv);
            }
        }
    }
    __syncthreads();

    // ---- scores on the matrix pipe: D[head][position] = Q[head][:] . K[position][:], v_mfma_f32_16x16x32_f16 with the group's
    // query heads as the (zero-padded) 16 rows of A and 16 cache rows as B (a B fragment: lane (column mi = position, mq = lane
    // >> 4) loads 8 consecutive dims 32 kc + 8 mq .. of its row, 16 bytes; e4m3: 8 bytes, converted in registers, and twice the
    // tiles in flight — the same bytes and registers in flight per wave)
    const int grp = lane / LPR, sl = lane % LPR;
    constexpr int U = KV8 ? 4 : 2;  // 16-row tiles in flight per wave
    using KB = std::conditional_t<KV8, u32x2, u32x4>;  // a lane's 8 dims of one row
    constexpr int KC = HD / 32;
    typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
    typedef float float4_t __attribute__((ext_vector_type(4)));
    const int mi = lane & 15, mq = lane >> 4;
    float mx4[4] = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};  // heads 4 mq + r
    {
        half8_t afr[KC];
#pragma unroll
        for (int kc = 0; kc < KC; kc++) {
            u32x4 a{0u, 0u, 0u, 0u};
            if (mi < REP) a = *reinterpret_cast<const u32x4 *>(qh + mi * HALF + 16 * kc + 4 * mq);
            afr[kc] = __builtin_bit_cast(half8_t, a);
        }
        for (int t0 = wave * 16; t0 < nc; t0 += NW * 16 * U) {
            KB kb[U][KC];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int t = t0 + u * NW * 16 + mi;
                const gptr<const CT> row = K + row_off(c0 + (t < nc ? t : 0), kpg[u]) + 8 * mq;
#pragma unroll
                for (int kc = 0; kc < KC; kc++) kb[u][kc] = *(gptr<const KB>)(row + 32 * kc);
            }
            if constexpr (PAGED) {  // the next step's page ids, behind this step's row loads
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const int t = t0 + (U + u) * NW * 16 + mi;
                    kpg[u] = tab[(c0 + (t < nc ? t : 0)) >> p.page_shift];
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int t = t0 + u * NW * 16 + mi;
                float4_t d{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kc = 0; kc < KC; kc++) {
                    if constexpr (KV8) d = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[kc], __builtin_bit_cast(half8_t, e4m3_half8(kb[u][kc])), d, 0, 0, 0);
                    else d = __builtin_amdgcn_mfma_f32_16x16x32_f16(afr[kc], __builtin_bit_cast(half8_t, kb[u][kc]), d, 0, 0, 0);
                }
                if (4 * mq < REP && t < nc) {
#pragma unroll
                    for (int r = 0; r < 4; r++) {
                        if (4 * mq + r < REP) {
                            float a = d[r] * p.scale;
                            if constexpr (SC) {
                                if (p.softcap != 0.f) a = soft_cap(a, p.softcap, p.inv_softcap);
                            }
                            sc[(4 * mq + r) * CL + t] = a;
                            mx4[r] = a > mx4[r] ? a : mx4[r];
                        }
                    }
                }
            }
        }
    }
    // rows in flight per wave (e4m3: a lane's DPL bytes, so twice the rows while their REP weights each stay within 32 registers)
    constexpr int UV16 = REP * DPL > 16 ? 2 : 4, UV = !KV8 ? UV16 : (2 * UV16 * REP > 32 ? 32 / REP : 2 * UV16);
    // PAGED: a row of the value loop belongs to one wave, so its page id is wave-uniform (a scalar load); ids one step ahead, the
    // first step's here: in front of the reductions
    [[maybe_unused]] int vpg[UV];
    [[maybe_unused]] const int wv = PAGED ? __builtin_amdgcn_readfirstlane(wave) : wave;
    auto v_pages = [&]([[maybe_unused]] int t0) {
        if constexpr (PAGED) {
#pragma unroll
            for (int u = 0; u < UV; u++) {
                const int t = t0 + u * NW;
                vpg[u] = tab[(c0 + (t < nc ? t : 0)) >> p.page_shift];
            }
        }
    };
    v_pages(wv);
    if (owner && wave == NW - 1) {  // the new position, from LDS (parked apart: the chunk's nc may equal CL)
        u32x4 kn = u32x4{0u, 0u, 0u, 0u};
        if (grp == 0) kn = *reinterpret_cast<const u32x4 *>(knh + 4 * sl);
#pragma unroll
        for (int h = 0; h < REP; h++) {
            const u32x4 qv = *reinterpret_cast<const u32x4 *>(qh + h * HALF + 4 * sl);
            float a = fdot2(kn.x, qv.x, 0.f);
            a = fdot2(kn.y, qv.y, a);
            a = fdot2(kn.z, qv.z, a);
            a = fdot2(kn.w, qv.w, a);
            a = group_sum<LPR>(a);
            a *= p.scale;
            if constexpr (SC) {
                if (p.softcap != 0.f) a = soft_cap(a, p.softcap, p.inv_softcap);
            }
            if (lane == 0) park[h] = a;
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {  // maximum over the 16 positions (lanes) of this lane's head group, per wave
        float m = mx4[r];
        m = group_max<16>(m);
        if (mi == 0 && 4 * mq + r < REP) red[(4 * mq + r) * NW + wave] = m;
    }
    __syncthreads();
    if (tid < REP) {
        float m = red[tid * NW];
#pragma unroll
        for (int w = 1; w < NW; w++) m = red[tid * NW + w] > m ? red[tid * NW + w] : m;
        if (owner) m = park[tid] > m ? park[tid] : m;
        mxf[tid] = m;
    }
    __syncthreads();
    {   // exponentials and their sums: wave -> (head wave % REP, part wave / REP of the chunk)
        constexpr int NP = NW / REP;
        const int hh = wave % REP, pw = wave / REP;
        const float m = mxf[hh];
        float sm = 0.f;
        for (int t = pw * 64 + lane; t < nc; t += 64 * NP) {
            const float e = __expf(sc[hh * CL + t] - m);
            sc[hh * CL + t] = e;
            sm += e;
        }
        sm = wave_sum(sm);
        if (lane == 0) red[NW * REP + wave] = sm;
    }
    __syncthreads();
    if (tid < REP) {
        constexpr int NP = NW / REP;
        float sm = 0.f;
#pragma unroll
        for (int pw = 0; pw < NP; pw++) sm += red[NW * REP + pw * REP + tid];
        const float wn = owner ? __expf(park[tid] - mxf[tid]) : 0.f;
        park[tid] = wn;  // from here on: the new position's softmax weight
        sumf[tid] = sm + wn;
    }

    // ---- values: wave w takes positions w, w + NW, ...; a lane owns DPL adjacent dims
    float acc[REP][DPL];
#pragma unroll
    for (int h = 0; h < REP; h++)
#pragma unroll
        for (int e = 0; e < DPL; e++) acc[h][e] = 0.f;
    for (int t0 = PAGED ? wv : wave; t0 < nc; t0 += NW * UV) {
        std::conditional_t<KV8, uint32_t, uint16_t> raw[UV][KV8 ? 1 : DPL];  // (e4m3: the DPL bytes in one register)
#pragma unroll
        for (int u = 0; u < UV; u++) {
            const int t = t0 + u * NW;
            const gptr<const CT> row = V + row_off(c0 + (t < nc ? t : 0), vpg[u]) + DPL * lane;
            if constexpr (KV8) {
                if constexpr (DPL == 1) raw[u][0] = row[0];
                else if constexpr (DPL == 2) raw[u][0] = *(gptr<const uint16_t>)row;
                else raw[u][0] = *(gptr<const uint32_t>)row;
            } else if constexpr (DPL == 1) raw[u][0] = row[0];
            else if constexpr (DPL == 2) { const uint32_t r = *(gptr<const uint32_t>)row; raw[u][0] = (uint16_t)r; raw[u][1] = (uint16_t)(r >> 16); }
            else { const u32x2 r = *(gptr<const u32x2>)row; raw[u][0] = (uint16_t)r.x; raw[u][1] = (uint16_t)(r.x >> 16); raw[u][2] = (uint16_t)r.y; raw[u][3] = (uint16_t)(r.y >> 16); }
        }
        v_pages(t0 + NW * UV);
#pragma unroll
        for (int u = 0; u < UV; u++) {
            const int t = t0 + u * NW;
            [[maybe_unused]] float vf[DPL];
            if constexpr (KV8) {
                const kv8_float2_t lo = e4m3_float2<false>(raw[u][0]);
                vf[0] = lo.x;
                if constexpr (DPL >= 2) vf[1] = lo.y;
                if constexpr (DPL == 4) {
                    const kv8_float2_t hi = e4m3_float2<true>(raw[u][0]);
                    vf[2] = hi.x, vf[3] = hi.y;
                }
            }
#pragma unroll
            for (int h = 0; h < REP; h++) {
                const float w = t < nc ? sc[h * CL + t] : 0.f;
#pragma unroll
                for (int e = 0; e < DPL; e++) {
                    if constexpr (KV8) acc[h][e] += w * vf[e];
                    else acc[h][e] += w * (float)__builtin_bit_cast(_Float16, raw[u][e]);
                }
            }
        }
    }
#pragma unroll
    for (int h = 0; h < REP; h++)
#pragma unroll
        for (int e = 0; e < DPL; e++) po[(wave * REP + h) * HD + DPL * lane + e] = acc[h][e];
    __syncthreads();  // (also orders park / sumf, written by the first REP threads above, before the reads below)
    for (int idx = tid; idx < REP * HD; idx += NT) {
        float v = 0.f;
#pragma unroll
        for (int w = 0; w < NW; w++) v += po[w * REP * HD + idx];
        const int h = idx / HD, d = idx - h * HD;
        if (owner) v += park[h] * vn[d];
        if constexpr (SHARED) {
            if (neff == 1 && start > 0) {  // the only chunk of a member: the prefix partial, then this one
                const float *pr = p.pre + ((long)b * p.nkv * REP + kh * REP + h) * (HD + 2);
                const float pm = pr[0], M = pm > mxf[h] ? pm : mxf[h];
                const float f0 = __expf(pm - M), f1 = __expf(mxf[h] - M);
                orow[idx] = __builtin_bit_cast(uint16_t, (_Float16)((pr[2 + d] * f0 + v * f1) / (pr[1] * f0 + sumf[h] * f1)));
                continue;
            }
        }
        if constexpr (SC) {
            if (neff == 1 && p.sinks) {  // the only chunk: the sink joins the denominator here
                const float sk = p.sinks[kh * REP + h], M = sk > mxf[h] ? sk : mxf[h];
                const float f = __expf(mxf[h] - M);
                orow[idx] = __builtin_bit_cast(uint16_t, (_Float16)((v * f) / (sumf[h] * f + __expf(sk - M))));
                continue;
            }
        }
        if (neff == 1) orow[idx] = __builtin_bit_cast(uint16_t, (_Float16)(v / sumf[h]));  // the only chunk
        else st_agent(wsp + h * (HD + 2) + 2 + d, v);
    }
    if (neff == 1) return;  // no partials, no ticket
    if (tid < REP) {
        st_agent(wsp + tid * (HD + 2), mxf[tid]);
        st_agent(wsp + tid * (HD + 2) + 1, sumf[tid]);
    }
    // ---- ticket: the partial stores are agent-scope (write-through); wait for them, then arrive with an agent-scope release /
    // acquire so that the last arriver sees every other chunk's partials
    if (!ticket_last<__ATOMIC_ACQ_REL>(ticket, (unsigned)neff, flag, tid)) return;
    // ---- last arriver of this (sequence, kv head): merge in chunk order (max / sum of every partial through LDS first, then the
    // out partials sixteen at a time: agent-scope loads are issued together, never one per iteration)
    const float *base = p.part + slot * REP * (HD + 2);
    float *ml = sh;  // [neff * REP][2]: the score buffer and what follows it are free now
    for (int i = tid; i < neff * REP; i += NT) {
        const float *pp = base + (long)i * (HD + 2);
        ml[2 * i] = ld_agent(pp);
        ml[2 * i + 1] = ld_agent(pp + 1);
    }
    __syncthreads();
    for (int idx = tid; idx < REP * HD; idx += NT) {
        const int h = idx / HD, d = idx - h * HD;
        float M = -3.0e38f;
        for (int s = 0; s < neff; s++) {
            const float m = ml[2 * (s * REP + h)];
            M = m > M ? m : M;
        }
        [[maybe_unused]] float es = 0.f;  // SC: the sink's term of the denominator, once per row
        if constexpr (SC) {
            if (p.sinks) {
                const float sk = p.sinks[kh * REP + h];
                M = sk > M ? sk : M;
                es = __expf(sk - M);
            }
        }
        float L = 0.f, o = 0.f;
        if constexpr (SHARED) {
            if (start > 0) {  // a member: the prefix partial is the chunk in front of the row's own
                const float *pr = p.pre + ((long)b * p.nkv * REP + kh * REP + h) * (HD + 2);
                const float pm = pr[0];
                M = pm > M ? pm : M;
                const float f = __expf(pm - M);
                L = pr[1] * f, o = pr[2 + d] * f;
            }
        }
        for (int s0 = 0; s0 < neff; s0 += 16) {
            float v[16];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int sx = s0 + u < neff ? s0 + u : neff - 1;
                v[u] = ld_agent(base + ((long)sx * REP + h) * (HD + 2) + 2 + d);
            }
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const int sx = s0 + u;
                if (sx < neff) {
                    const float f = __expf(ml[2 * (sx * REP + h)] - M);
                    L += ml[2 * (sx * REP + h) + 1] * f;
                    o += v[u] * f;
                }
            }
        }
        if constexpr (SC) L += es;
        orow[idx] = __builtin_bit_cast(uint16_t, (_Float16)(o / L));
    }
    if (tid == 0) __hip_atomic_store(as_global(ticket), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// LDS floats of the kernel's layout at score capacity `chunk`
size_t batch_lds_floats(int rep, int hd, long chunk) {
    const int nw = kBatchNW;
    return (size_t)rep * chunk + (size_t)rep * hd / 2 + hd / 2 + hd + (size_t)nw * rep * hd + 2 * (size_t)nw * rep + 3 * rep + 4;
}

template <class CT>
constexpr int kKvFmt = kIsKv8<CT> ? 1 : 0;  // the kv_fmt of a cache element type

// the positions a windowed launch is sized for: min(max_len, window rounded up to 4) (max_len is a multiple of 4, at least 4)
long window_positions(long window, long max_len) {
    return window >= max_len ? max_len : (window + 3) / 4 * 4;
}

struct BatchGeometry {
    int nsplit, chunk;
    size_t lds, ws_bytes;
};

// Launch geometry from (B, heads, max_len) only.  ws_bytes is an upper bound of what ANY launch with at most B sequences and at
// most max_len positions needs (monotone in both): one workspace serves every smaller launch of the same heads.
int batch_geometry(int B, int nq, int nkv, int hd, long max_len, BatchGeometry &g) {
    g = BatchGeometry{0, 0, 0, 0};
    const int rc = attn_shape(B, nq, nkv, hd, max_len);
    if (rc != QPAL_OK) return rc;
    const int rep = nq / nkv;
    const size_t budget = kBatchLdsMax / sizeof(float), fixed = batch_lds_floats(rep, hd, 0);
    const long cl_max = (long)((budget - fixed) / rep) / 64 * 64;  // the most positions one chunk's scores can hold
    if (cl_max < 64) return QPAL_E_SHAPE;
    const long ns_lds = (max_len + cl_max - 1) / cl_max;           // chunks the LDS forces
    if (ns_lds > kBatchMaxSplit) return QPAL_E_SHAPE;
    int ns = 1;
    if (max_len >= kBatchSplitFrom) {
        // ~one workgroup of 16 waves per compute unit over the whole launch
        long want = (256 + (long)B * nkv - 1) / ((long)B * nkv);
        if (want > kBatchMaxSplit) want = kBatchMaxSplit;
        ns = (int)(want > ns_lds ? want : ns_lds);
    } else {
        ns = (int)ns_lds;  // (1: a 512-position cache always fits)
    }
    long c = ((max_len + ns - 1) / ns + 63) / 64 * 64;
    if (c > cl_max) c = cl_max;
    ns = (int)((max_len + c - 1) / c);
    g.nsplit = ns, g.chunk = (int)c;
    g.lds = batch_lds_floats(rep, hd, c) * sizeof(float);
    if (max_len >= kBatchSplitFrom) {
        // slots: B nkv ns_lds where the LDS forces the split, else B nkv ceil(256 / (B nkv)) <= 256 + B nkv
        const long by_lds = (long)B * nkv * ns_lds, by_want = 256 + (long)B * nkv;
        const long slots = by_lds > by_want ? by_lds : by_want;
        g.ws_bytes = ((size_t)kBatchMax * nkv + (size_t)slots * rep * (hd + 2)) * sizeof(float);
    }
    return QPAL_OK;
}

// the entry points: the same checks, geometry and launch, the cache element type and the row addressing apart (PAGED: kcache /
// vcache are the pools, `pg` the block table, max_len = max_pages * page_size)
// the workspace of the shared launches: the plain launch's in front, then the prefix phase's tickets, chunk partials and merged
// partials (attn_prefix.h)
size_t shared_ws_bytes(const BatchGeometry &g, const PrefixGeometry &x) {
    return g.ws_bytes + (x.tickets + x.part + x.pre) * sizeof(float);
}

// sp: SHARED — the sharing of the launch; the prefix launch goes first, stream order is the only synchronisation between the two
// window: WIN — the geometry is that of min(max_len, window rounded up to 4) positions (a short window in a long cache takes no
// split and no merge floor); its workspace is never larger than the plain launch's of max_len
// mods: SC — the soft cap and the sinks; a launch without a window runs the windowed body with window = max_len
template <class CT, bool PAGED, bool SHARED = false, bool WIN = false, bool SC = false>
int attn_rope_decode_batch(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache, void *out_f16,
                           long ld_out, const long *pos, const float *inv_freq, int B, int nq, int nkv, int hd, long max_len,
                           float scale, void *ws, long ws_bytes, void *stream, const PageArgs *pg = nullptr, int shift = 0,
                           const SharedPrefixArgs *sp = nullptr, long window = 0, const ScoreMods *mods = nullptr) {
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !pos || !inv_freq) return QPAL_E_NULL;
    BatchGeometry g;
    long geo_len = max_len;
    if constexpr (WIN) {
        const int rcs = attn_shape(B, nq, nkv, hd, max_len);
        if (rcs != QPAL_OK) return rcs;
        if constexpr (SC) {
            if (window == 0) window = max_len;
        }
        geo_len = window_positions(window, max_len);
    }
    const int rc = batch_geometry(B, nq, nkv, hd, geo_len, g);
    if (rc != QPAL_OK) return rc;
    [[maybe_unused]] PrefixGeometry x{};
    [[maybe_unused]] const size_t plain_ws = g.ws_bytes;
    if constexpr (SHARED) {
        if (sp->G < 1 || sp->G > kPxMaxGroups) return QPAL_E_SHAPE;
        prefix_geometry(B, sp->G, nq, nkv, hd, max_len, x);
        g.ws_bytes = shared_ws_bytes(g, x);  // (checked below as the plain launch's is)
    }
    uintptr_t al4 = PAGED ? reinterpret_cast<uintptr_t>(pg->table) : 0;
    if constexpr (SC) al4 |= reinterpret_cast<uintptr_t>(mods->sinks);
    if constexpr (SHARED)
        al4 |= reinterpret_cast<uintptr_t>(sp->row_group) | reinterpret_cast<uintptr_t>(sp->grp_slot) | reinterpret_cast<uintptr_t>(sp->grp_len);
    const int rca = attn_args(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos, inv_freq, nq, hd, g.ws_bytes, ws, ws_bytes, al4);
    if (rca != QPAL_OK) return rca;
    float *wsf = static_cast<float *>(ws);
    if constexpr (SHARED) g.ws_bytes = plain_ws;  // from here on: the part of the workspace the suffix launch owns
    AttnBatchParams<CT> p{q, k, v, ld_qkv, static_cast<CT *>(kcache), static_cast<CT *>(vcache),
                          static_cast<uint16_t *>(out_f16), ld_out, pos, inv_freq, nkv, max_len, scale,
                          g.ws_bytes ? reinterpret_cast<unsigned *>(wsf) : nullptr, g.ws_bytes ? wsf + (long)kBatchMax * nkv : nullptr,
                          g.nsplit, g.chunk};
    if constexpr (PAGED) p.table = pg->table, p.ld_table = pg->ld_table, p.num_pages = pg->num_pages, p.page_shift = shift;
    if constexpr (WIN) p.window = window;
    if constexpr (SC) p.softcap = mods->softcap, p.inv_softcap = mods->softcap != 0.f ? 1.f / mods->softcap : 0.f, p.sinks = mods->sinks;
    const int grid = B * nkv * g.nsplit, rep = nq / nkv;
    if constexpr (SHARED) {
        float *xf = wsf + plain_ws / sizeof(float);
        p.sp = *sp, p.B = B, p.pre = xf + x.tickets + x.part;
        const PrefixLaunch a{q, ld_qkv, kcache, vcache, pos, inv_freq, *sp, pg->table, pg->ld_table, pg->num_pages, shift, B, nkv,
                             max_len, scale, reinterpret_cast<unsigned *>(xf), xf + x.tickets, xf + x.tickets + x.part, x.nsplit, x.ntile};
        const int rc2 = launch_attn_prefix(a, kKvFmt<CT>, hd, rep, stream);
        if (rc2 != QPAL_OK) return rc2;
    }
    return for_hd_rep(hd, rep, [&](auto HD, auto REP) {
        return launch_lds<attn_rope_batch_kernel<CT, PAGED, HD(), REP(), SHARED, WIN, SC>>(dim3(grid), dim3(64 * kBatchNW), g.lds, (int)kBatchLdsMax,
                                                                                   static_cast<hipStream_t>(stream), p);
    });
}

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" long qpal_attn_batch_ws_bytes(int B, int nq, int nkv, int hd, long max_len) {
    BatchGeometry g;
    if (batch_geometry(B, nq, nkv, hd, max_len, g) != QPAL_OK) return 0;
    return (long)g.ws_bytes;
}

extern "C" int qpal_attn_rope_decode_batch(const float *q, const float *k, const float *v, long ld_qkv, void *kcache_f16, void *vcache_f16,
                                           void *out_f16, long ld_out, const long *pos, const float *inv_freq, int B, int nq, int nkv,
                                           int hd, long max_len, float scale, void *ws, long ws_bytes, void *stream) {
    return attn_rope_decode_batch<uint16_t, false>(q, k, v, ld_qkv, kcache_f16, vcache_f16, out_f16, ld_out, pos, inv_freq, B, nq, nkv, hd,
                                            max_len, scale, ws, ws_bytes, stream);
}

extern "C" int qpal_attn_rope_decode_batch_kv8(const float *q, const float *k, const float *v, long ld_qkv, void *kcache_e4m3,
                                               void *vcache_e4m3, void *out_f16, long ld_out, const long *pos, const float *inv_freq,
                                               int B, int nq, int nkv, int hd, long max_len, float scale, void *ws, long ws_bytes,
                                               void *stream) {
    return attn_rope_decode_batch<uint8_t, false>(q, k, v, ld_qkv, kcache_e4m3, vcache_e4m3, out_f16, ld_out, pos, inv_freq, B, nq, nkv, hd,
                                           max_len, scale, ws, ws_bytes, stream);
}

extern "C" int qpal_attn_rope_decode_batch_paged(const float *q, const float *k, const float *v, long ld_qkv, void *kpool, void *vpool,
                                                 void *out_f16, long ld_out, const long *pos, const float *inv_freq,
                                                 const int *block_table, long ld_table, int num_pages, int page_size, int max_pages,
                                                 int kv_fmt, int B, int nq, int nkv, int hd, float scale, void *ws, long ws_bytes,
                                                 void *stream) {
    const PageArgs pg{block_table, ld_table, num_pages, page_size, max_pages};
    const bool any_null = !block_table || !q || !k || !v || !kpool || !vpool || !out_f16 || !pos || !inv_freq;
    return paged_entry(any_null, pg, kv_fmt, [&](auto ct, int shift, long max_len) {
        return attn_rope_decode_batch<decltype(ct), true>(q, k, v, ld_qkv, kpool, vpool, out_f16, ld_out, pos, inv_freq, B, nq, nkv, hd,
                                                          max_len, scale, ws, ws_bytes, stream, &pg, shift);
    });
}

extern "C" int qpal_attn_rope_decode_batch_window(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                                  void *out_f16, long ld_out, const long *pos, const float *inv_freq,
                                                  const int *block_table, long ld_table, int num_pages, int page_size, int max_pages,
                                                  int kv_fmt, int B, int nq, int nkv, int hd, long max_len, float scale, long window,
                                                  void *ws, long ws_bytes, void *stream) {
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !pos || !inv_freq) return QPAL_E_NULL;
    if (window < 0) return QPAL_E_PARAM;
    if (kv_fmt != 0 && kv_fmt != 1) return QPAL_E_SHAPE;
    auto launch = [&](auto ct, auto paged, auto win, long len, const PageArgs *pg, int shift) {
        return attn_rope_decode_batch<decltype(ct), paged(), false, win()>(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos, inv_freq, B, nq,
                                                                          nkv, hd, len, scale, ws, ws_bytes, stream, pg, shift, nullptr,
                                                                          window);
    };
    using T = std::true_type;
    using F = std::false_type;
    if (!block_table) {  // contiguous caches [B][nkv][max_len][hd]
        return for_kv_fmt(kv_fmt, [&](auto ct) {
            return window ? launch(ct, F{}, T{}, max_len, nullptr, 0) : launch(ct, F{}, F{}, max_len, nullptr, 0);
        });
    }
    const PageArgs pg{block_table, ld_table, num_pages, page_size, max_pages};
    return paged_entry(false, pg, kv_fmt, [&](auto ct, int shift, long len) {
        return window ? launch(ct, T{}, T{}, len, &pg, shift) : launch(ct, T{}, F{}, len, &pg, shift);
    });
}

extern "C" int qpal_attn_rope_decode_batch_score(const float *q, const float *k, const float *v, long ld_qkv, void *kcache, void *vcache,
                                                 void *out_f16, long ld_out, const long *pos, const float *inv_freq,
                                                 const int *block_table, long ld_table, int num_pages, int page_size, int max_pages,
                                                 int kv_fmt, int B, int nq, int nkv, int hd, long max_len, float scale, long window,
                                                 float softcap, const float *sinks, void *ws, long ws_bytes, void *stream) {
    if (!q || !k || !v || !kcache || !vcache || !out_f16 || !pos || !inv_freq) return QPAL_E_NULL;
    if (window < 0 || !score_mods_ok(softcap)) return QPAL_E_PARAM;
    if (softcap == 0.f && !sinks)
        return qpal_attn_rope_decode_batch_window(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos, inv_freq, block_table, ld_table,
                                                  num_pages, page_size, max_pages, kv_fmt, B, nq, nkv, hd, max_len, scale, window, ws,
                                                  ws_bytes, stream);
    if (kv_fmt != 0 && kv_fmt != 1) return QPAL_E_SHAPE;
    const ScoreMods mods{softcap, sinks};
    auto launch = [&](auto ct, auto paged, long len, const PageArgs *pg, int shift) {
        return attn_rope_decode_batch<decltype(ct), paged(), false, true, true>(q, k, v, ld_qkv, kcache, vcache, out_f16, ld_out, pos, inv_freq,
                                                                               B, nq, nkv, hd, len, scale, ws, ws_bytes, stream, pg, shift,
                                                                               nullptr, window, &mods);
    };
    if (!block_table)  // contiguous caches [B][nkv][max_len][hd]
        return for_kv_fmt(kv_fmt, [&](auto ct) { return launch(ct, std::false_type{}, max_len, nullptr, 0); });
    const PageArgs pg{block_table, ld_table, num_pages, page_size, max_pages};
    return paged_entry(false, pg, kv_fmt, [&](auto ct, int shift, long len) { return launch(ct, std::true_type{}, len, &pg, shift); });
}

extern "C" long qpal_attn_prefix_ws_bytes(int B, int G, int nq, int nkv, int hd, long max_len) {
    BatchGeometry g;
    if (batch_geometry(B, nq, nkv, hd, max_len, g) != QPAL_OK || G < 1 || G > kPxMaxGroups) return 0;
    PrefixGeometry x;
    prefix_geometry(B, G, nq, nkv, hd, max_len, x);
    return (long)shared_ws_bytes(g, x);
}

extern "C" int qpal_attn_rope_decode_batch_shared(const float *q, const float *k, const float *v, long ld_qkv, void *kpool, void *vpool,
                                                  void *out_f16, long ld_out, const long *pos, const float *inv_freq,
                                                  const int *block_table, long ld_table, int num_pages, int page_size, int max_pages,
                                                  int kv_fmt, const int *row_group, const int *grp_slot, const int *grp_len, int G, int B,
                                                  int nq, int nkv, int hd, float scale, void *ws, long ws_bytes, void *stream) {
    const PageArgs pg{block_table, ld_table, num_pages, page_size, max_pages};
    const SharedPrefixArgs sp{row_group, grp_slot, grp_len, G};
    const bool any_null = !block_table || !row_group || !grp_slot || !grp_len || !q || !k || !v || !kpool || !vpool || !out_f16 || !pos || !inv_freq;
    return paged_entry(any_null, pg, kv_fmt, [&](auto ct, int shift, long max_len) {
        return attn_rope_decode_batch<decltype(ct), true, true>(q, k, v, ld_qkv, kpool, vpool, out_f16, ld_out, pos, inv_freq, B, nq, nkv,
                                                                hd, max_len, scale, ws, ws_bytes, stream, &pg, shift, &sp);
    });
}
