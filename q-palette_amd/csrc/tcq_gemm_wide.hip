// Wide fused decode + skinny GEMM: qpal_tcq_gemm_wide, 129 .. 256 batch rows in ONE pass over the packed weights.
//
// The lockstep kernels (tc_gemm.h with tc_gemm16.h's mapping) stop at 128 batch rows: beside the 64 KiB codebook image they keep two
// (or four) [n][128] tiles of x in LDS, and at 256 rows one such tile is 64 KiB — two do not fit into 160 KiB.  Here the tile of a
// step is staged in HALVES: a half-step is the two column blocks kj = 2 h, 2 h + 1 of every supertile of the step (columns
// 32 sup + 16 h .. + 15, sup = 0..3: 64 columns), 32 KiB at 256 rows, two slots — 128 KiB with the image.  The structure is otherwise
// the lockstep one: the 8 waves of a workgroup own 8 different supertile rows and walk the same K range; a wave loads the packed
// words of a 128-column step ONCE, keeps them in registers across the barrier between the two half-steps and decodes column blocks
// 0, 1 in the first and 2, 3 in the second — every weight is decoded exactly once per launch; an A fragment then feeds one
// v_mfma_f32_16x16x32_f16 per group of 16 batch rows (NG = 12 or 16 groups: 96 / 128 accumulator registers).  The next half tile
// travels global -> registers -> LDS one half-step ahead; one workgroup barrier per half-step.
//
// Half tile layout, per group of 16 batch rows 2 KiB: the 16-byte piece (batch row b, supertile sup, column block kj = 2 h + jh) lives at
//   (b >> 4) * 2048 + (2 sup + jh) * 256 + ((b + g16_rot(4 sup + kj)) & 15) * 16
// — tc_gemm16.h's blocks of 256 bytes and its rotation, so a ds_read_b128 of an MFMA's B fragment meets every bank once.  The rotation
// takes only four values over the 8 pieces of one batch row (supertiles 0, 1 and 2, 3 share it: they share a read), so the eight lanes
// of a staging store are two batch rows b, b + 2 with four pieces each: eight different 16-byte windows (wide_chunk below).
//
// K is split over workgroups where a launch has few rows (host: wide_split, the lockstep kernels' rule: a power of two, cuts at
// step boundaries, towards 192 items of at least 4 steps): the partial sums meet in fp32 atomics on an output the entry point has cleared with a small kernel (or on the live
// output of an accumulating job).  Persistent workgroups walk the item list of up to 4 jobs that share x.
#include "gemm_wide.h"

namespace qpal {

namespace {

constexpr int kWdS = 9;  // codebooks of 512 pairs: KV 2..8, one 64 KiB image
using WdImage = TcqCodec<kWdS, 8>;

struct WideJob {
    float *out;
    long ldo;
    const uint32_t *c1, *c2;
    const uint16_t *wscale;
    const void *tab;
    float oscale;
    int nrows;  // supertile rows (m / 32)
    int accumulate;
};

struct WideParams {
    WideJob job[kWdMaxJobs];
    int item_end[kWdMaxJobs];  // items of jobs 0..j; item = (block of 8 supertile rows, K split)
    int njobs;
    const uint16_t *x;  // fp16 [n][k]
    int n, k;
    int nsc1, nsc2, st1, st2, col2;  // supertile columns / steps of the two streams, first column of stream 2
    int kv1, kv2;
    int lsk;  // log2 of the K split
};

template <int NG>
__global__ __launch_bounds__(kWdThreads) void tcq_gemm_wide_kernel(const WideParams p) {
    static_assert(NG % 4 == 0 && NG * 16 >= kWdMinN && NG * 16 <= kWdMaxN);
    using Map = G16Map<NG>;  // accumulators and the epilogue's scatter
    constexpr int NT = kWdThreads;
    constexpr int SLOT = NG * kWdGroup;
    constexpr int NCH = NG * 128;   // 16-byte chunks of a half tile
    constexpr int CPT = NCH / NT;   // chunks per thread (3 / 4)
    static_assert(NCH % NT == 0 && 2 * SLOT >= kWdWaves * Map::SCRATCH);
    // ONE block, the codebook image first: at LDS address 0 a gather address is one v_and_or_b32 (tc_gemm.h)
    __shared__ __attribute__((aligned(16))) unsigned char smem[WdImage::LDS_DWORDS * 4 + 2 * SLOT];
    uint32_t *const lut = reinterpret_cast<uint32_t *>(smem);
    unsigned char *const xt = smem + WdImage::LDS_DWORDS * 4;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t laneoff = (uint32_t)(lane & (WdImage::C - 1)) << 2;
    const int T = p.st1 + p.st2;
    const int total = p.item_end[kWdMaxJobs - 1];
    const void *cur_tab = nullptr;

    // this thread's chunks of a half tile: the byte offset of (batch row, supertile, jh) inside x without the step's column base;
    // a batch row >= n lies beyond the descriptor's range: zeros
    const buf_rsrc_t rs_x = gemm_rsrc(p.x, p.n * p.k * 2);
    uint32_t xvo[CPT];
    u32x4 xr[CPT];
#pragma unroll
    for (int r = 0; r < CPT; r++) {
        const WideChunk ch = wide_chunk(tid + r * NT);
        xvo[r] = ch.b < p.n ? (uint32_t)(ch.b * p.k + 32 * ch.sup + 8 * ch.jh) * 2u : kBufDead;
    }
    // half h of global step g: x columns col_base(g) + 32 sup + 16 h + 8 jh
    auto load_x = [&](int g, int h) __attribute__((always_inline)) {
        const bool on2 = g >= p.st1;
        const uint32_t col = (uint32_t)((on2 ? p.col2 + (g - p.st1) * 128 : g * 128) + 16 * h) * 2u;
#pragma unroll
        for (int r = 0; r < CPT; r++) xr[r] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xvo[r] != kBufDead ? xvo[r] + col : kBufDead, 0, 0);
    };
    auto store_x = [&](auto hc, unsigned char *buf) __attribute__((always_inline)) {
        // (chunk r is chunk 0's piece of batch row b + 64 r: four groups further, the same rotation)
        int t = tid;
        asm volatile("" : "+v"(t));  // the store address is computed HERE: hoisted out of the item loop it sat in a register through the steps
        const WideChunk ch = wide_chunk(t);
        unsigned char *dst = buf + wide_x_off<decltype(hc)::value>(ch.b, ch.sup, ch.jh);
#pragma unroll
        for (int r = 0; r < CPT; r++) *reinterpret_cast<u32x4 *>(dst + r * (NT / 128) * kWdGroup) = xr[r];
    };
    constexpr std::integral_constant<int, 0> h0{};
    constexpr std::integral_constant<int, 1> h1{};

    for (int gitem = blockIdx.x; gitem < total; gitem += gridDim.x) {
        int j = 0, item_begin = 0;
#pragma unroll
        for (int i = 0; i < kWdMaxJobs - 1; i++) {
            if (gitem >= p.item_end[i]) {
                j = i + 1;
                item_begin = p.item_end[i];
            }
        }
        const WideJob jb = p.job[j];
        const int item = gitem - item_begin;
        const int rg = item >> p.lsk, ks = item & ((1 << p.lsk) - 1);
        const int g0 = (T * ks) >> p.lsk, g1 = (T * (ks + 1)) >> p.lsk;  // (host: T >= 4 << lsk, never empty)
        const int sr = rg * kWdWaves + wave;
        const bool live = sr < jb.nrows;  // (wave-uniform: a row past the end only keeps the staging and the barriers company)
        const int srow = live ? sr : 0;

        load_x(g0, 0);
        if (jb.tab != cur_tab) {  // workgroup-uniform; the barrier that ended the last item freed the image
            WdImage::build(lut, jb.tab, tid, NT);
            cur_tab = jb.tab;
        }
        store_x(h0, xt);
        typename Map::Accum acc;
        acc.zero();
        __syncthreads();

        // the steps [ga, gb) of ONE stream.  A step: half 1's tile and the next step's words requested; half 0 from slot 0; half 1's
        // tile into slot 1 (last read one half-step ago, before the latest barrier); barrier; the next step's first half requested;
        // half 1 from slot 1 with the SAME words; that tile into slot 0; barrier.
        auto run = [&](auto kc, const uint32_t *stream, int nsc, int s0, int ga, int gb) __attribute__((always_inline)) {
            using CK = TcqCodec<kWdS, decltype(kc)::value>;
            constexpr int NW = CK::NW;
            const buf_rsrc_t rs = gemm_rsrc(stream + (long)srow * nsc * 16 * NW, live ? nsc * 64 * NW : 0);
            uint32_t wa[NW], wb[NW];
            load_step_w_buf<NW>(rs, ga - s0, lane, wa);
            auto one_step = [&](int g, uint32_t(&wc)[NW], uint32_t(&wn)[NW]) __attribute__((always_inline)) {
                load_x(g, 1);
                load_step_w_buf<NW>(rs, (g + 1 < gb ? g + 1 : g) - s0, lane, wn);
                if (live) wide_half<CK, NG, 0>(lut, laneoff, wc, xt, lane, acc.v);
                store_x(h1, xt + SLOT);
                __syncthreads();
                load_x(g + 1 < g1 ? g + 1 : g, 0);
                if (live) wide_half<CK, NG, 1>(lut, laneoff, wc, xt + SLOT, lane, acc.v);
                store_x(h0, xt);
                __syncthreads();
            };
            int g = ga;
            for (; g + 1 < gb; g += 2) {
                one_step(g, wa, wb);
                one_step(g + 1, wb, wa);
            }
            if (g < gb) one_step(g, wa, wb);
        };
        // (every wave passes the same barriers: the KV of a launch is one value per stream)
        const int mid = g1 < p.st1 ? g1 : (g0 > p.st1 ? g0 : p.st1);
        if (g0 < mid) dispatch_kv<kWdS>(p.kv1, [&](auto kc) __attribute__((always_inline)) { run(kc, jb.c1, p.nsc1, 0, g0, mid); });
        if (mid < g1) dispatch_kv<kWdS>(p.kv2, [&](auto kc) __attribute__((always_inline)) { run(kc, jb.c2, p.nsc2, p.st1, mid, g1); });

        // ---- epilogue (tc_gemm.h's): one group of 16 batch rows at a time through a per-wave [16][32] fp32 scratch that overlays the
        // tiles (the last half-step ended on a barrier), out as 128-byte runs
        float *scr = reinterpret_cast<float *>(xt) + wave * (Map::SCRATCH / 4);
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));  // the epilogue's addresses are computed HERE, not kept in registers through the steps
        const int q4 = lane_e >> 4, c = lane_e & 15, r32 = lane_e & 31;
        float osc = jb.oscale;
        if (jb.wscale && live) osc *= (float)__builtin_bit_cast(_Float16, as_global(jb.wscale)[sr * 32 + r32]);
        auto epilogue = [&](auto mode_c) __attribute__((always_inline)) {
            constexpr int mode = decltype(mode_c)::value;  // 0: store, 1: out += (residual add), 2: split-K atomics
            static_for<0, NG>([&](auto gc) {
                constexpr int grp = decltype(gc)::value;
                Map::template scatter<grp>(scr, acc, q4, c);  // (wave-private scratch: LDS operations of one wave complete in order)
#pragma unroll
                for (int i = 0; i < 8; i++) {
                    const int bl = 2 * i + (lane_e >> 5), b = 16 * grp + bl;
                    const float v = scr[bl * 32 + r32] * osc;
                    if (live && b < p.n) {
                        float *dst = jb.out + (long)b * jb.ldo + (long)sr * 32 + r32;
                        if constexpr (mode == 2) atomicAdd(dst, v);
                        else if constexpr (mode == 1) *dst += v;
                        else *dst = v;
                    }
                }
            });
        };
        if (p.lsk > 0) epilogue(std::integral_constant<int, 2>{});
        else if (jb.accumulate) epilogue(std::integral_constant<int, 1>{});
        else epilogue(std::integral_constant<int, 0>{});
        __syncthreads();  // the scratch is the next item's first half tile
    }
}

// rows 0 .. n - 1 of every output a split launch adds into (a kernel, not a memset node: the launch may be recorded into a graph)
__global__ __launch_bounds__(256) void tcq_gemm_wide_clear(const WideClear c) {
    if (!c.out[blockIdx.y]) return;
    float *row = c.out[blockIdx.y] + (long)blockIdx.x * c.ldo[blockIdx.y];
    for (int i = threadIdx.x; i < c.cols[blockIdx.y]; i += 256) row[i] = 0.f;
}

}  // namespace

void launch_gemm_wide_clear(const WideClear &c, int n, int njobs, hipStream_t stream) {
    hipLaunchKernelGGL(tcq_gemm_wide_clear, dim3(n, njobs), dim3(256), 0, stream, c);
}

}  // namespace qpal

using namespace qpal;

extern "C" int qpal_tcq_gemm_wide(const qpal_tcq_job *jobs, int njobs, int n, int S, int KV1, int KV2, void *stream) {
    if (!jobs) return QPAL_E_NULL;
    if (njobs < 1 || njobs > kWdMaxJobs || n < kWdMinN || n > kWdMaxN) return QPAL_E_SHAPE;
    const int k = jobs[0].k;
    const int step = KV2 ? 256 : 128;  // whole 128-column steps in every stream
    if (k <= 0 || k % step || (long)n * k * 2 >= (1l << 31)) return QPAL_E_SHAPE;  // (x is read through one buffer descriptor)
    for (int j = 0; j < njobs; j++) {
        const qpal_tcq_job &q = jobs[j];
        if (q.m <= 0 || q.m % 32 || q.k != k || (q.ldo != 0 && q.ldo < q.m)) return QPAL_E_SHAPE;
    }
    if (S != kWdS || KV1 < TcqAny<kWdS>::kMinKV || KV1 > TcqAny<kWdS>::kMaxKV) return QPAL_E_PARAM;
    if (KV2 && (KV2 < TcqAny<kWdS>::kMinKV || KV2 > TcqAny<kWdS>::kMaxKV)) return QPAL_E_PARAM;
    for (int j = 0; j < njobs; j++) {
        const qpal_tcq_job &q = jobs[j];
        if (!q.out || !q.c1 || !q.x || !q.tlut || (KV2 && !q.c2)) return QPAL_E_NULL;
        // no rotation, RMSNorm, activation or per-job codec in this launch; one x for all jobs
        if (q.x_had || q.x_su || q.x_f32 || q.x_rms_eps != 0.0f || q.x_rms_w || q.act_out || q.act_su || q.x_hadk || q.x_K || q.kv || q.kv2 ||
            q.x != jobs[0].x)
            return QPAL_E_PARAM;
        if ((reinterpret_cast<uintptr_t>(q.x) & 15) || (reinterpret_cast<uintptr_t>(q.wscale) & 1)) return QPAL_E_ALIGN;
        if ((reinterpret_cast<uintptr_t>(q.out) | reinterpret_cast<uintptr_t>(q.c1) | reinterpret_cast<uintptr_t>(q.c2) |
             reinterpret_cast<uintptr_t>(q.tlut)) & 3)
            return QPAL_E_ALIGN;
    }
    WideParams p{};
    p.njobs = njobs, p.x = static_cast<const uint16_t *>(jobs[0].x), p.n = n, p.k = k;
    const int k1 = KV2 ? k / 2 : k;
    p.nsc1 = k1 / 32, p.nsc2 = KV2 ? k1 / 32 : 0;
    p.st1 = p.nsc1 / 4, p.st2 = p.nsc2 / 4, p.col2 = k1;
    p.kv1 = KV1, p.kv2 = KV2;
    int nblk = 0;
    for (int j = 0; j < njobs; j++) nblk += (jobs[j].m / 32 + kWdWaves - 1) / kWdWaves;
    p.lsk = wide_split(nblk, p.st1 + p.st2);
    int items = 0;
    bool clear = false;
    WideClear wc{};
    for (int j = 0; j < kWdMaxJobs; j++) {
        if (j < njobs) {
            const qpal_tcq_job &q = jobs[j];
            p.job[j] = WideJob{q.out, q.ldo ? q.ldo : q.m, static_cast<const uint32_t *>(q.c1), static_cast<const uint32_t *>(q.c2),
                               static_cast<const uint16_t *>(q.wscale), q.tlut, q.oscale == 0.0f ? 1.0f : q.oscale, q.m / 32, q.accumulate};
            items += ((q.m / 32 + kWdWaves - 1) / kWdWaves) << p.lsk;
            clear = clear || !q.accumulate;
            if (!q.accumulate) wc.out[j] = p.job[j].out, wc.ldo[j] = p.job[j].ldo, wc.cols[j] = q.m;
        }
        p.item_end[j] = items;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p.lsk > 0 && clear) launch_gemm_wide_clear(wc, n, njobs, st);
    const int grid = items < kWdGrid ? items : kWdGrid;
    if (n <= 192) hipLaunchKernelGGL(tcq_gemm_wide_kernel<12>, dim3(grid), dim3(kWdThreads), 0, st, p);
    else hipLaunchKernelGGL(tcq_gemm_wide_kernel<16>, dim3(grid), dim3(kWdThreads), 0, st, p);
    return (int)hipGetLastError();
}
