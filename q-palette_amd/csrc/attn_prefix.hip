// Prefix phase of shared-prefix decode attention (qpal_attn_rope_decode_batch_shared): the slots of a group share
// the pages of their first grp_len positions, so those K / V rows are read ONCE per group, kv head and chunk instead of once per
// slot, and the (slot, query head) rows of the group against one K / V stream are a real matrix product.
//
// Shape: attn_prefill.h's flash loop (keys on the M side of the matrix pipe, 32-key tiles through LDS once per workgroup, fp16
// softmax weights as the B operand of the value product, e4m3 bytes converted exactly on their way into LDS) with other rows and
// no causal mask.  Workgroup = (kv head, tile of 64 rows of ONE group, chunk of [0, grp_len)); wave = 16 rows; a row is (member
// slot in slot order, query head of the kv head's group) and carries its own position: q is rotated at pos[b] with the decode
// kernel's fp16 arithmetic.  Every workgroup finds its group and its rows itself by a scan of row_group / pos through
// shared_prefix_len() (B <= 128: one thread per slot, ballots): the host fixes grid and workspace from (B, G, heads, max_len) and
// reads none of the three tensors, so the launch is capturable with groups, lengths and positions rewritten between replays.
// A row's arithmetic touches its own column of S^T only: its partial does not depend on which other rows share its tile.
//
// A chunk leaves (max, sum, unnormalised out[hd]) per row, addressed by (slot, query head); chunks of one (kv head, tile) take a
// ticket and the last to arrive merges them in chunk order into the merged partial the suffix launch folds in (no float atomics,
// the merger resets the ticket): the pattern of attn_batch.hip and attn_prefill.h.
#include "attn_prefill.h"
#include "attn_prefix.h"

namespace qpal {

namespace {

constexpr int kPxSlots = 128;  // B of a launch (attn_batch.hip's kBatchMax)

template <class CT>
struct AttnPrefixParams {
    PrefixLaunch a;
    const CT *kpool, *vpool;
};

template <class CT, int HD, int REP>
__global__ __launch_bounds__(256) void attn_prefix_kernel(const AttnPrefixParams<CT> pp) {
    const PrefixLaunch &p = pp.a;
    constexpr bool KV8 = kIsKv8<CT>;
    using KR = std::conditional_t<KV8, u32x2, u32x4>;  // eight elements of a cache row as prefetched
    constexpr int NW = 4, NT = 64 * NW, R = kPxRows, MPT = R / REP;  // MPT: members of a tile
    constexpr int HALF = HD / 2, KC = HD / 32, DT = HD / 16, CPR = HD / 8;
    constexpr int RS = 2 * HD + 16;                    // bytes of an LDS row (padded by one 16-byte access)
    constexpr int ROWS = R > 2 * kPfKT ? R : 2 * kPfKT;  // Q image [R] first, then K [32] | V [32] over it
    constexpr int NCH = 2 * kPfKT * CPR / NT;          // 16-byte chunks of a K + V tile per thread
    static_assert(R == 16 * NW && R % REP == 0 && 2 * kPfKT * CPR % NT == 0, "rows and tiles are cut evenly");
    static_assert(R * HD % (4 * NT) == 0 && R * kPxMaxSplit % NT == 0, "the merge is cut evenly over the threads");
    static_assert(NT >= kPxSlots && kPxMaxGroups <= 64, "one thread per slot, one per group");
    constexpr size_t MERGE = (size_t)2 * R * kPxMaxSplit * sizeof(float);  // the merge's maxima / weights and sums
    __shared__ __attribute__((aligned(16))) unsigned char sm[(size_t)ROWS * RS > MERGE ? (size_t)ROWS * RS : MERGE];
    __shared__ unsigned flag;
    __shared__ int s_cnt[2][kPxMaxGroups];  // members of every group among slots 0..63 and 64..127
    __shared__ int s_sel[2];                // the group and the row tile of this workgroup
    __shared__ int s_mem[R];                // the slots of the tile's members, in slot order
    __shared__ int s_rid[R];                // merge: row -> slot * nq + head, -1 past the group's rows
    unsigned char *const Ks = sm, *const Vs = sm + kPfKT * RS;

    const int per_kh = p.ntile * p.nsplit;
    const int kh = blockIdx.x / per_kh, rem = blockIdx.x - kh * per_kh;
    const int jt = rem / p.nsplit, split = rem - jt * p.nsplit;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int mi = lane & 15, mq = lane >> 4;
    const int nq = p.nkv * REP;

    // ---- the groups of the launch: thread b = slot b's group by THE rule, its rank among the group's members by ballots
    int gid = -1, rank = 0;
    if (tid == 0) s_sel[0] = -1;
    if (tid < kPxSlots) {
        if (tid < p.B) shared_prefix_len(p.sp, tid, p.pos[tid], p.B, p.page_shift, p.max_len, gid);
        for (int gg = 0; gg < p.sp.G; gg++) {
            const unsigned long long m = __ballot(gid == gg);
            if (gid == gg) rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
            if (lane == 0) s_cnt[wave][gg] = __popcll(m);
        }
    }
    __syncthreads();
    if (gid >= 0 && wave == 1) rank += s_cnt[0][gid];
    if (tid < p.sp.G) {  // thread g: the tiles of group g and of the groups before it
        int before = 0, mine = 0;
        for (int i = 0; i <= tid; i++) {
            const int t = ((s_cnt[0][i] + s_cnt[1][i]) * REP + R - 1) / R;
            if (i < tid) before += t;
            else mine = t;
        }
        if (jt >= before && jt < before + mine) s_sel[0] = tid, s_sel[1] = jt - before;
    }
    __syncthreads();
    const int g = __builtin_amdgcn_readfirstlane(s_sel[0]);
    if (g < 0) return;  // no such tile: nothing is read or written, no ticket taken
    const int rt = __builtin_amdgcn_readfirstlane(s_sel[1]);
    const int nrows = (s_cnt[0][g] + s_cnt[1][g]) * REP;  // rows of the group; the tile's: [rt * R, rt * R + R)
    if (gid == g && rank >= rt * MPT && rank < (rt + 1) * MPT) s_mem[rank - rt * MPT] = tid;
    const unsigned len = (unsigned)p.sp.grp_len[g];  // (a member passed the rule: 0 < len, a page multiple, below max_len < 2^30)
    unsigned cld = (len + 31u) & ~31u;
    if (p.nsplit > 1) {
        cld = ((len + (unsigned)p.nsplit - 1u) / (unsigned)p.nsplit + 31u) & ~31u;
        if (cld < (unsigned)kPxMinChunk) cld = (unsigned)kPxMinChunk;
    }
    const int neff = (int)((len + cld - 1u) / cld);  // chunks that hold keys: the same in every workgroup of the tile
    if (split >= neff) return;
    const int c0 = (int)(split * cld);
    const int c1 = (unsigned)c0 + cld < len ? (int)(c0 + cld) : (int)len;
    const gptr<const CT> Kc = as_global(pp.kpool), Vc = as_global(pp.vpool);
    const int *table = p.table + (long)p.sp.grp_slot[g] * p.ld_table;
    // the page ids of keys kt0 .. kt0 + 15 and kt0 + 16 .. kt0 + 31 of the tile about to be fetched (kt0 is a multiple of 32, a
    // page holds at least 16 positions; the second only where the chunk reaches it)
    int pg0 = 0, pg1 = 0;
    auto tile_pages = [&](int kt0) {
        if (kt0 < c1) {
            pg0 = table[kt0 >> p.page_shift];
            pg1 = kt0 + 16 < c1 ? table[(kt0 + 16) >> p.page_shift] : pg0;
        }
    };
    tile_pages(c0);
    __syncthreads();  // s_mem

    // ---- the wave's 16 rows after the rotary embedding at each row's own position, through LDS into B fragments
    // (REP > 1: cos / sin once per (member, i) through LDS — the heads of a member sit at one position, and the reduction of a
    // large angle is the longest part of this prologue; the rotation itself keeps the decode kernel's expression)
    [[maybe_unused]] __shared__ uint32_t s_cs[REP > 1 ? MPT * HALF : 1];
    if constexpr (REP > 1) {
        for (int idx = tid; idx < MPT * HALF; idx += NT) {
            const int mw = idx / HALF, i = idx - mw * HALF;
            uint32_t w = 0;
            if ((rt * MPT + mw) * REP < nrows) {
                const float ang = (float)p.pos[s_mem[mw]] * p.inv_freq[i];
                const _Float16 c = (_Float16)cosf(ang), s = (_Float16)sinf(ang);
                w = (uint32_t)__builtin_bit_cast(uint16_t, c) | (uint32_t)__builtin_bit_cast(uint16_t, s) << 16;
            }
            s_cs[idx] = w;
        }
        __syncthreads();
    }
    for (int idx = lane; idx < 16 * HALF; idx += 64) {
        const int qi = idx / HALF, i = idx - qi * HALF;
        const int lr = wave * 16 + qi;
        uint16_t r1 = 0, r2 = 0;
        if (rt * R + lr < nrows) {
            const int b = s_mem[lr / REP];
            const float *src = p.q + (long)b * p.ld_qkv + (long)(kh * REP + lr % REP) * HD;
            _Float16 c, s;
            if constexpr (REP > 1) {
                const uint32_t w = s_cs[(lr / REP) * HALF + i];
                c = __builtin_bit_cast(_Float16, (uint16_t)w), s = __builtin_bit_cast(_Float16, (uint16_t)(w >> 16));
            } else {
                const float ang = (float)p.pos[b] * p.inv_freq[i];
                c = (_Float16)cosf(ang), s = (_Float16)sinf(ang);
            }
            const _Float16 x1 = (_Float16)src[i], x2 = (_Float16)src[i + HALF];
            const _Float16 o1 = x1 * c + (-x2) * s, o2 = x2 * c + x1 * s;
            r1 = __builtin_bit_cast(uint16_t, o1), r2 = __builtin_bit_cast(uint16_t, o2);
        }
        uint16_t *dst = reinterpret_cast<uint16_t *>(sm + lr * RS);
        dst[i] = r1;
        dst[i + HALF] = r2;
    }
    __syncthreads();
    half8_t qf[KC];
#pragma unroll
    for (int kc = 0; kc < KC; kc++) qf[kc] = *reinterpret_cast<const half8_t *>(sm + (wave * 16 + mi) * RS + (32 * kc + 8 * mq) * 2);
    __syncthreads();  // the K / V tiles take the Q image's place

    // one 16-byte chunk of the K | V tile at keys kt0 ..: rows of the chunk from the pool, rows past it as zeros
    auto fetch = [&](int kt0, KR(&regs)[NCH]) {
#pragma unroll
        for (int u = 0; u < NCH; u++) {
            const int idx = tid + u * NT;
            const int isv = idx / (kPfKT * CPR), rr = (idx / CPR) % kPfKT, ch = idx % CPR;
            const int n = kt0 + rr;
            KR val{};
            if (n < c1) {
                const int pg = rr < 16 ? pg0 : pg1;
                val = *(gptr<const KR>)((isv ? Vc : Kc) + paged_row<HD>(page_ok(pg, p.num_pages) ? pg : 0, p.nkv, kh, p.page_shift, n) + 8 * ch);
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

    float m_run = -3.0e38f, l_run = 0.f;  // l_run: this lane's share of its row's sum
    float4_t oacc[DT];
#pragma unroll
    for (int dt = 0; dt < DT; dt++) oacc[dt] = float4_t{0.f, 0.f, 0.f, 0.f};
    KR regs[NCH];
    // per step: fetch tile k into registers (loads in flight), products of tile k - 1 from LDS, then tile k into LDS
    for (int kt0 = c0;; kt0 += kPfKT) {
        const bool more = kt0 < c1;
        if (more) {
            fetch(kt0, regs);
            tile_pages(kt0 + kPfKT);  // the next tile's, behind this tile's row loads
        }
        if (kt0 > c0) {
            // S^T: lane holds keys kt0 - 32 + 16 kt + 4 mq + r of row mi
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
                    const int n = kt0 - kPfKT + 16 * kt + 4 * mq + r;
                    ok[4 * kt + r] = n < c1;  // every key of the chunk lies below every member's position
                    sv[4 * kt + r] = s[kt][r] * p.scale;
                    if (ok[4 * kt + r]) mx = fmaxf(mx, sv[4 * kt + r]);
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
            // O^T[d][row] += V^T P^T: k slot (mq, e) = key 4 mq + e of the first 16 (e < 4), of the second 16 (e >= 4)
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

    // ---- lane holds O^T[d = 16 dt + 4 mq + r][row mi]: the partial of row (slot, query head)
    const int lrow = wave * 16 + mi;
    const bool live = rt * R + lrow < nrows;
    const long rid = live ? (long)s_mem[lrow / REP] * nq + kh * REP + lrow % REP : 0;
    const long rows_all = (long)p.B * nq;
    if (neff == 1) {  // the only chunk: it is the merged partial
        if (live) {
            float *dst = p.pre + rid * (HD + 2);
            if (mq == 0) dst[0] = m_run, dst[1] = l_run;
#pragma unroll
            for (int dt = 0; dt < DT; dt++)
#pragma unroll
                for (int r = 0; r < 4; r++) dst[2 + 16 * dt + 4 * mq + r] = oacc[dt][r];
        }
        return;
    }
    if (live) {
        float *wsp = p.part + ((long)split * rows_all + rid) * (HD + 2);
        if (mq == 0) {
            st_agent(wsp, m_run);
            st_agent(wsp + 1, l_run);
        }
#pragma unroll
        for (int dt = 0; dt < DT; dt++)
#pragma unroll
            for (int r = 0; r < 4; r++) st_agent(wsp + 2 + 16 * dt + 4 * mq + r, oacc[dt][r]);
    }
    if (mq == 0) s_rid[lrow] = live ? (int)rid : -1;
    // ---- ticket: the partial stores are agent-scope (write-through); wait for them, then arrive with an agent-scope release /
    // acquire so that the last arriver sees every other chunk's partials
    unsigned *ticket = p.tickets + (long)kh * p.ntile + jt;
    if (!ticket_last<__ATOMIC_ACQ_REL>(ticket, (unsigned)neff, &flag, tid)) return;
    // ---- last arriver of this (kv head, tile): merge in chunk order
    // (agent-scope loads are issued in batches, never one per iteration: a round trip each would be the launch's longest part)
    float *cf = reinterpret_cast<float *>(sm);  // [R][neff]: the maxima, then in their place the weights exp(m_s - M); [R][neff] sums
    float *ls = cf + R * kPxMaxSplit;
    const long cstride = rows_all * (HD + 2);   // from a chunk's partials to the next chunk's
    {
        constexpr int UM = R * kPxMaxSplit / NT;  // (row, chunk) pairs per thread
        float mv[UM], lv[UM];
#pragma unroll
        for (int u = 0; u < UM; u++) {
            const int i = tid + u * NT, row = i / neff, sx = i - row * neff;
            const int r = row < R ? s_rid[row] : -1;
            const float *pc = p.part + (long)(r < 0 ? 0 : r) * (HD + 2) + (long)sx * cstride;
            mv[u] = ld_agent(pc);
            lv[u] = ld_agent(pc + 1);
        }
#pragma unroll
        for (int u = 0; u < UM; u++) {
            const int i = tid + u * NT;
            if (i < R * neff) cf[i] = mv[u], ls[i] = lv[u];
        }
    }
    __syncthreads();
    if (tid < R && s_rid[tid] >= 0) {
        float M = -3.0e38f;
        for (int sx = 0; sx < neff; sx++) M = fmaxf(M, cf[tid * neff + sx]);
        float L = 0.f;
        for (int sx = 0; sx < neff; sx++) {
            const float f = __expf(cf[tid * neff + sx] - M);
            cf[tid * neff + sx] = f;
            L += ls[tid * neff + sx] * f;
        }
        float *dst = p.pre + (long)s_rid[tid] * (HD + 2);
        dst[0] = M, dst[1] = L;
    }
    __syncthreads();
    for (int idx0 = tid; idx0 < R * HD; idx0 += 4 * NT) {  // four outputs per thread and step: 32 loads in flight
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        int row[4], rr[4];
#pragma unroll
        for (int j = 0; j < 4; j++) row[j] = (idx0 + j * NT) / HD, rr[j] = s_rid[row[j]];
        for (int s0 = 0; s0 < neff; s0 += 8) {
            float v[4][8];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float *base = p.part + (long)(rr[j] < 0 ? 0 : rr[j]) * (HD + 2) + 2 + (idx0 + j * NT - row[j] * HD);
#pragma unroll
                for (int u = 0; u < 8; u++) v[j][u] = ld_agent(base + (long)(s0 + u < neff ? s0 + u : neff - 1) * cstride);
            }
#pragma unroll
            for (int j = 0; j < 4; j++)
#pragma unroll
                for (int u = 0; u < 8; u++)
                    if (s0 + u < neff) o[j] += v[j][u] * cf[row[j] * neff + s0 + u];
        }
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (rr[j] >= 0) p.pre[(long)rr[j] * (HD + 2) + 2 + (idx0 + j * NT - row[j] * HD)] = o[j];
    }
    if (tid == 0) __hip_atomic_store(as_global(ticket), 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <class CT>
int launch_prefix(const PrefixLaunch &a, int hd, int rep, void *stream) {
    const AttnPrefixParams<CT> p{a, static_cast<const CT *>(a.kpool), static_cast<const CT *>(a.vpool)};
    const int grid = a.nkv * a.ntile * a.nsplit;
    return for_hd_rep(hd, rep, [&](auto HD, auto REP) {
        hipLaunchKernelGGL((attn_prefix_kernel<CT, HD(), REP()>), dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), p);
        return (int)hipGetLastError();
    });
}

}  // namespace

int launch_attn_prefix(const PrefixLaunch &a, int kv_fmt, int hd, int rep, void *stream) {
    return kv_fmt == 1 ? launch_prefix<uint8_t>(a, hd, rep, stream) : launch_prefix<uint16_t>(a, hd, rep, stream);
}

}  // namespace qpal
