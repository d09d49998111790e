// Routed fused decode + skinny GEMM for mixture-of-experts layers: qpal_moe_gemm.
//
// qpal_moe_gemv (moe_gemv.hip) makes one pass over an expert's weights per table entry, i.e. per 8 routed rows.  Here the work item is
// (CHUNK, block of 8 supertile rows): a chunk is a run of consecutive table entries of one expert with contiguous positions, up to
// max_run <= 128 rows, and its rows are the batch columns of up to 8 groups of 16 of tc_gemm16.h's fragment mapping — the trellis of
// a weight row is read and decoded ONCE for all of them.  The structure is the dense lockstep kernel's (tc_gemm.h): the 8 waves of a
// workgroup own 8 different supertile rows of the chunk's expert and walk the whole K range in lockstep, stream 1 then stream 2; the
// step's [rows][128] tile of x is gathered once per workgroup (x_index -> registers -> LDS, one step ahead, two slots, one barrier
// per step); a wave sees its whole K range, so there is no cross-wave reduction, no split-K and no atomics: a row's result is a
// function of the shapes alone, whatever shares its chunk.  What differs from the dense kernel: the expert's weight rows come from
// the per-projection device tables (buffer descriptors per wave and stream, as moe_gemv builds them), the KV of a wave's row is a
// runtime value (dispatch_kv: a block of rows may straddle up | gate), the batch rows are gathered through x_index, and the number
// of 16-row groups is chosen per chunk (wave-uniform: moe_gemm_body<1 / 2 / 4 / 8>), so a group without rows costs no MFMAs.
#include "tc_gemm16.h"

namespace qpal {

namespace {

constexpr int kMoeS = 9;  // codebooks of 512 pairs: KV 2..8, one 64 KiB image
using MoeImage = TcqCodec<kMoeS, 8>;
constexpr int kMgWaves = 8;                 // waves = supertile rows of a workgroup
constexpr int kMgThreads = 64 * kMgWaves;
constexpr int kMgMaxGroups = 8;             // groups of 16 batch rows: 128 rows per chunk
constexpr int kMgSlot = kMgMaxGroups * kG16Group;  // bytes of one tile slot (32 KiB), two slots

struct MoeGemmProj {
    const uint64_t *c1, *c2, *wscale;  // device tables [E] of device pointers
    int nrows, kv, kv2, out_col;
};

struct MoeGemmParams {
    float *out;
    long ldo;
    int out_rows;
    int nproj;
    MoeGemmProj pj[2];
    const uint16_t *x;
    long ldx;
    int x_rows;
    const int *x_index, *group_expert, *group_first, *group_count, *ngroups;
    int max_groups, E, max_run;
    int nsc1, nsc2, st1, st2, col2;
    const void *tab;
    float oscale;
};

// one entry of the group table, with the guards of qpal_moe_gemv (an entry that fails one belongs to no chunk)
struct MoeEntry {
    int e, first, count;
    bool ok;
};
__device__ __forceinline__ MoeEntry moe_entry(const MoeGemmParams &p, int j, int ng) {
    MoeEntry t{-1, 0, 0, false};
    if (j < 0 || j >= ng) return t;
    t.e = p.group_expert[j], t.first = p.group_first[j], t.count = p.group_count[j];
    t.ok = (unsigned)t.e < (unsigned)p.E && t.count >= 1 && t.count <= 8 && t.first >= 0 && t.first <= p.out_rows - t.count;
    return t;
}
// entry b continues the sequence of entry a (its predecessor in the table)
__device__ __forceinline__ bool moe_follows(const MoeEntry &a, const MoeEntry &b) {
    return a.ok && b.ok && a.e == b.e && b.first == a.first + a.count;
}

// Rows of the chunk entry g leads, 0 where it leads none (wave- and workgroup-uniform: scalar loads only).  The chunks of a
// sequence are cut greedily from its start: an entry joins the chunk in front of it while the chunk stays within max_run rows.  So
// g walks back to the start of its sequence — for a route-built table at most 16 entries (128 rows in entries of 8) — replays the
// cuts up to itself, and, where a cut falls on it, collects the entries behind it.
__device__ __forceinline__ int moe_chunk_rows(const MoeGemmParams &p, int g, int ng, MoeEntry &lead) {
    lead = moe_entry(p, g, ng);
    if (!lead.ok) return 0;
    int s = g;
    MoeEntry a = lead;
    while (s > 0) {
        const MoeEntry prev = moe_entry(p, s - 1, ng);
        if (!moe_follows(prev, a)) break;
        a = prev;
        s--;
    }
    int start = s, sum = a.count;
    for (int j = s + 1; j <= g; j++) {
        const int c = p.group_count[j];
        if (sum + c > p.max_run) start = j, sum = c;
        else sum += c;
    }
    if (start != g) return 0;
    int rows = lead.count;
    MoeEntry last = lead;
    for (int j = g + 1; j < ng; j++) {
        const MoeEntry nx = moe_entry(p, j, ng);
        if (!moe_follows(last, nx) || rows + nx.count > p.max_run) break;
        rows += nx.count;
        last = nx;
    }
    return rows;
}

// which stream a global step of a row belongs to, and which x columns it covers (tc_gemm.h: gemm_where)
struct MoeStep {
    int col_base, col_end;
};
__device__ __forceinline__ MoeStep moe_where(const MoeGemmParams &p, int g) {
    const bool on2 = g >= p.st1;
    const int s = on2 ? g - p.st1 : g;
    return MoeStep{(on2 ? p.col2 : 0) + s * 128, on2 ? p.col2 + p.nsc2 * 32 : p.nsc1 * 32};
}

// One chunk (expert e, positions first .. first + rows - 1, rows <= 16 NG) against the blocks of 8 supertile rows this workgroup owns.
template <int NG>
__device__ __forceinline__ void moe_gemm_body(const MoeGemmParams &p, uint32_t *lut, unsigned char *xt, int e, int first, int rows_c,
                                              int tid, int lane, int wave) {
    using Map = G16Map<NG>;
    constexpr int NT = kMgThreads;
    constexpr int NCH = NG * 256;                  // 16-byte chunks of one step's x tile
    constexpr int CPT = (NCH + NT - 1) / NT;       // chunks per thread
    const uint32_t laneoff = (uint32_t)(lane & (MoeImage::C - 1)) << 2;
    const int T = p.st1 + p.st2;
    const int rows0 = p.pj[0].nrows, rows = rows0 + (p.nproj > 1 ? p.pj[1].nrows : 0);

    // this thread's chunks of a tile: id -> (batch row b = id >> 4, column block q); the byte offset of the batch row's source row
    // inside x, kBufDead where the row is absent (past the chunk, or an index outside x: zeros)
    const buf_rsrc_t rs_x = gemm_rsrc(p.x, (int)((long)p.x_rows * p.ldx * 2));
    uint32_t xvo[CPT];
    u32x4 xr[CPT];
#pragma unroll
    for (int r = 0; r < CPT; r++) {
        const int id = tid + r * NT, b = id >> 4;
        xvo[r] = kBufDead;
        if (id < NCH && b < rows_c) {
            const int src = p.x_index ? p.x_index[first + b] : first + b;
            if ((unsigned)src < (unsigned)p.x_rows) xvo[r] = (uint32_t)((long)src * p.ldx * 2) + 16u * g16_chunk_q(id & 15);
        }
    }
    auto load_x = [&](int g) {  // (a dead chunk, or columns past the end of the stream: beyond the descriptor's range, zeros)
        const MoeStep st = moe_where(p, g);
#pragma unroll
        for (int r = 0; r < CPT; r++) {
            const int q = g16_chunk_q((tid + r * NT) & 15);
            const bool ok = xvo[r] != kBufDead && st.col_base + 8 * q < st.col_end;
            xr[r] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, ok ? xvo[r] + (uint32_t)st.col_base * 2u : kBufDead, 0, 0);
        }
    };
    auto store_x = [&](unsigned char *buf) {
#pragma unroll
        for (int r = 0; r < CPT; r++) {
            const int id = tid + r * NT;
            if (id < NCH) Map::store_chunk(buf, id >> 4, g16_chunk_q(id & 15), xr[r]);
        }
    };

    for (int blk = blockIdx.x; blk * kMgWaves < rows; blk += gridDim.x) {
        const int vr = blk * kMgWaves + wave;
        const bool live = vr < rows;  // (wave-uniform: a row past the end only keeps the staging and the barriers company)
        const bool second = live && vr >= rows0;
        const int sr = live ? (second ? vr - rows0 : vr) : 0;
        const MoeGemmProj &pj = second ? p.pj[1] : p.pj[0];

        load_x(0);
        store_x(xt);
        typename Map::Accum acc;
        acc.zero();
        __syncthreads();

        // the steps [ga, gb) of ONE stream: tile of step g + 1 requested first, then the next weights; the step; the tile into the
        // slot that was last read one step ago, i.e. before the latest barrier
        auto run = [&](auto kc, const uint32_t *stream, int nsc, int ga, int gb) {
            using CK = TcqCodec<kMoeS, decltype(kc)::value>;
            constexpr int NW = CK::NW;
            const buf_rsrc_t rs = gemm_rsrc(stream + (long)sr * nsc * 16 * NW, live ? nsc * 64 * NW : 0);
            uint32_t wa[NW], wb[NW];
            load_step_w_buf<NW>(rs, 0, lane, wa);
            auto one_step = [&](int g, uint32_t(&wc)[NW], uint32_t(&wn)[NW]) {
                load_x(g + 1 < T ? g + 1 : g);
                load_step_w_buf<NW>(rs, g + 1 < gb ? g + 1 - ga : g - ga, lane, wn);
                __builtin_amdgcn_sched_barrier(0);
                if (live) Map::template step<CK>(lut, laneoff, wc, xt + (g & 1) * kMgSlot, lane, acc);
                store_x(xt + ((g + 1) & 1) * kMgSlot);
                __syncthreads();
            };
            int g = ga;
            for (; g + 1 < gb; g += 2) {
                one_step(g, wa, wb);
                one_step(g + 1, wb, wa);
            }
            if (g < gb) one_step(g, wa, wb);
        };
        // (every wave passes the same T barriers, whichever KV its row has)
        dispatch_kv<kMoeS>(pj.kv, [&](auto kc) { run(kc, reinterpret_cast<const uint32_t *>(pj.c1[e]), p.nsc1, 0, p.st1); });
        if (p.st2 > 0)
            dispatch_kv<kMoeS>(pj.kv2, [&](auto kc) { run(kc, reinterpret_cast<const uint32_t *>(pj.c2[e]), p.nsc2, p.st1, T); });

        // ---- epilogue (tc_gemm.h's): one group of 16 batch rows at a time through a per-wave [16][32] fp32 scratch that overlays the
        // tiles (the last step ended on a barrier), out as 128-byte runs
        float *scr = reinterpret_cast<float *>(xt) + wave * (Map::SCRATCH / 4);
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));  // the epilogue's addresses are computed HERE: hoisted over the steps they sat in registers
        const int q4 = lane_e >> 4, c = lane_e & 15, r32 = lane_e & 31;
        float osc = p.oscale;
        if (pj.wscale && live) osc *= (float)__builtin_bit_cast(_Float16, as_global(reinterpret_cast<const uint16_t *>(pj.wscale[e]))[sr * 32 + r32]);
        static_for<0, NG>([&](auto gc) {
            constexpr int grp = decltype(gc)::value;
            Map::template scatter<grp>(scr, acc, q4, c);  // (wave-private scratch: LDS operations of one wave complete in order)
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const int bl = 2 * i + (lane_e >> 5), b = 16 * grp + bl;
                const float v = scr[bl * 32 + r32] * osc;
                if (live && b < rows_c) p.out[(long)(first + b) * p.ldo + pj.out_col + sr * 32 + r32] = v;
            }
        });
        __syncthreads();  // the scratch is the next block's first tile
    }
}

__global__ __launch_bounds__(kMgThreads) void moe_gemm_kernel(const MoeGemmParams p) {
    // ONE block, the codebook image first: at LDS address 0 a gather address is one v_and_or_b32 (tc_gemm.h)
    __shared__ __attribute__((aligned(16))) unsigned char smem[MoeImage::LDS_DWORDS * 4 + 2 * kMgSlot];
    uint32_t *const lut = reinterpret_cast<uint32_t *>(smem);
    unsigned char *const xt = smem + MoeImage::LDS_DWORDS * 4;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.y;
    int ng = *p.ngroups;
    ng = ng < p.max_groups ? ng : p.max_groups;
    if (g >= ng) return;
    MoeEntry lead;
    const int rows_c = moe_chunk_rows(p, g, ng, lead);
    if (rows_c == 0) return;
    MoeImage::build(lut, p.tab, tid, kMgThreads);  // (the first barrier of the body publishes it)
    if (rows_c <= 16) moe_gemm_body<1>(p, lut, xt, lead.e, lead.first, rows_c, tid, lane, wave);
    else if (rows_c <= 32) moe_gemm_body<2>(p, lut, xt, lead.e, lead.first, rows_c, tid, lane, wave);
    else if (rows_c <= 64) moe_gemm_body<4>(p, lut, xt, lead.e, lead.first, rows_c, tid, lane, wave);
    else moe_gemm_body<8>(p, lut, xt, lead.e, lead.first, rows_c, tid, lane, wave);
}

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" int qpal_moe_gemm(float *out, long ldo, int out_rows, const qpal_moe_proj *proj, int nproj, const void *x_f16, long ldx,
                             int x_rows, const int *x_index, const int *group_expert, const int *group_first, const int *group_count,
                             const int *ngroups, int max_groups, int E, int k, const void *tlut, int S, float oscale, int max_run,
                             void *stream) {
    if (!out || !proj || !x_f16 || !group_expert || !group_first || !group_count || !ngroups || !tlut) return QPAL_E_NULL;
    if (nproj < 1 || nproj > 2) return QPAL_E_SHAPE;
    const bool split = proj[0].kv2 != 0;
    if (k <= 0 || k % 32 || (split && k % 64) || out_rows < 1 || x_rows < 1 || max_groups < 1 || E < 1 || E > 256 || ldx < k || ldx % 4)
        return QPAL_E_SHAPE;
    if (max_run < 1 || max_run > 16 * kMgMaxGroups || max_groups > 65535) return QPAL_E_SHAPE;
    if ((long)x_rows * ldx * 2 >= (1l << 31)) return QPAL_E_SHAPE;  // x is read through one buffer descriptor
    for (int j = 0; j < nproj; j++) {
        const qpal_moe_proj &q = proj[j];
        if (!q.c1 || (q.kv2 && !q.c2)) return QPAL_E_NULL;
        if (q.m <= 0 || q.m % 32 || q.out_col < 0 || (long)q.out_col + q.m > ldo) return QPAL_E_SHAPE;
        if ((q.kv2 != 0) != split) return QPAL_E_PARAM;  // one row geometry per launch
    }
    if (S != kMoeS) return QPAL_E_PARAM;  // (S 10 / 11: no any-KV image shared by KV 2..8)
    for (int j = 0; j < nproj; j++) {
        const qpal_moe_proj &q = proj[j];
        if (q.kv < TcqAny<kMoeS>::kMinKV || q.kv > TcqAny<kMoeS>::kMaxKV) return QPAL_E_PARAM;
        if (q.kv2 && (q.kv2 != q.kv + 1 || q.kv2 > TcqAny<kMoeS>::kMaxKV)) return QPAL_E_PARAM;
    }
    if ((reinterpret_cast<uintptr_t>(x_f16) & 7) || (reinterpret_cast<uintptr_t>(tlut) & 3)) return QPAL_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(x_index) | reinterpret_cast<uintptr_t>(group_expert) |
         reinterpret_cast<uintptr_t>(group_first) | reinterpret_cast<uintptr_t>(group_count) | reinterpret_cast<uintptr_t>(ngroups)) & 3)
        return QPAL_E_ALIGN;
    MoeGemmParams p{};
    p.out = out, p.ldo = ldo, p.out_rows = out_rows, p.nproj = nproj;
    int rows = 0;
    for (int j = 0; j < nproj; j++) {
        const qpal_moe_proj &q = proj[j];
        if ((reinterpret_cast<uintptr_t>(q.c1) | reinterpret_cast<uintptr_t>(q.c2) | reinterpret_cast<uintptr_t>(q.wscale)) & 7) return QPAL_E_ALIGN;
        p.pj[j] = MoeGemmProj{static_cast<const uint64_t *>(q.c1), static_cast<const uint64_t *>(q.c2), static_cast<const uint64_t *>(q.wscale),
                              q.m / 32, q.kv, q.kv2, q.out_col};
        rows += q.m / 32;
    }
    p.x = static_cast<const uint16_t *>(x_f16), p.ldx = ldx, p.x_rows = x_rows, p.x_index = x_index;
    p.group_expert = group_expert, p.group_first = group_first, p.group_count = group_count, p.ngroups = ngroups;
    p.max_groups = max_groups, p.E = E, p.max_run = max_run;
    const int k1 = split ? k / 2 : k;
    p.nsc1 = k1 / 32, p.nsc2 = split ? k1 / 32 : 0;
    p.st1 = (p.nsc1 + 3) / 4, p.st2 = (p.nsc2 + 3) / 4, p.col2 = k1;
    p.tab = tlut, p.oscale = oscale == 0.0f ? 1.0f : oscale;
    // one workgroup per (entry, block of 8 supertile rows): only a chunk's first entry works, and the experts in use supply the
    // parallelism — every block of rows gets its own workgroup (it builds the image once: 64 KiB against >= 8 rows of decode)
    const int nblk = (rows + kMgWaves - 1) / kMgWaves;
    const int gx = nblk < 4096 ? nblk : 4096;
    hipLaunchKernelGGL(moe_gemm_kernel, dim3(gx, max_groups), dim3(kMgThreads), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
