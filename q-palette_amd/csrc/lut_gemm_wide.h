// Wide fused decode + skinny GEMM for the VQ/SQ (tensor-core packing) layers: 129 .. 256 batch rows in ONE pass over
// the packed weights.  The geometry is tcq_gemm_wide.hip's (gemm_wide.h): 8 waves = 8 supertile rows walk one K range in lockstep, the
// x tile of a 128-column step is staged in two halves of 64 columns (two slots of NG * 2 KiB, one barrier per half-step), a wave
// loads the packed words of a step once, keeps them in registers across the barrier and decodes column blocks 0, 1 in the first
// half and 2, 3 in the second; an exchanged A fragment feeds one v_mfma_f32_16x16x32_f16 per group of 16 batch rows.
//
// What differs from the TCQ unit:
//   - every (bits, vec) of lut_table.inc is its OWN kernel (x NG = 12 / 16): no codec branch inside a kernel, so the words of two
//     steps (2 NW <= 32 registers) and the accumulators (8 NG) fit without scratch — the resource table is in §43;
//   - the codebook image is LutCodec<bits, vec, 16>: at most 64 KiB beside the 64 KiB of tiles (the codebooks of 2^10 .. 2^12
//     entries keep 16 / 8 / 4 bank-spread copies, half of what the 128-row kernels give them);
//   - `lut` is a per-job field: the image is rebuilt where a workgroup's next item belongs to a job with another codebook (the
//     barrier that ends an item has freed it), never otherwise;
//   - one stream per layer.
#pragma once
#include "gemm_wide.h"

namespace qpal {

constexpr int kLutWideCapLog2 = 16;  // image <= 64 KiB

struct LutWideJob {
    float *out;
    long ldo;
    const uint32_t *qw;
    const uint16_t *wscale;
    const void *lut;
    float oscale;
    int nrows;  // supertile rows (m / 32)
    int accumulate;
};

struct LutWideParams {
    LutWideJob job[kWdMaxJobs];
    int item_end[kWdMaxJobs];  // items of jobs 0..j; item = (block of 8 supertile rows, K split)
    const uint16_t *x;         // fp16 [n][k]
    int n, k;
    int T;    // steps of 128 columns
    int lsk;  // log2 of the K split
};

// one launcher per (NG, vec) translation unit (lut_gemm_wide_inst.inc); QPAL_E_PARAM for a (bits, vec) outside lut_table.inc
int launch_lut_gemm_wide_ng12_v1(const LutWideParams &p, int bits, int grid, hipStream_t stream);
int launch_lut_gemm_wide_ng12_v2(const LutWideParams &p, int bits, int grid, hipStream_t stream);
int launch_lut_gemm_wide_ng16_v1(const LutWideParams &p, int bits, int grid, hipStream_t stream);
int launch_lut_gemm_wide_ng16_v2(const LutWideParams &p, int bits, int grid, hipStream_t stream);

template <class Codec, int NG>
__global__ __launch_bounds__(kWdThreads) void lut_gemm_wide_kernel(const LutWideParams p) {
    static_assert(NG % 4 == 0 && NG * 16 >= kWdMinN && NG * 16 <= kWdMaxN);
    using Map = G16Map<NG>;  // accumulators and the epilogue's scatter
    constexpr int NT = kWdThreads, NW = Codec::NW;
    constexpr int SLOT = NG * kWdGroup;
    constexpr int NCH = NG * 128;   // 16-byte chunks of a half tile
    constexpr int CPT = NCH / NT;   // chunks per thread (3 / 4)
    constexpr int IMAGE = Codec::LDS_DWORDS * 4;
    static_assert(NCH % NT == 0 && 2 * SLOT >= kWdWaves * Map::SCRATCH && IMAGE % 16 == 0 && IMAGE + 2 * SLOT <= 160 * 1024);
    // ONE block, the codebook image first: at LDS address 0 a gather address is the shifted index | the lane's copy
    __shared__ __attribute__((aligned(16))) unsigned char smem[IMAGE + 2 * SLOT];
    uint32_t *const lut = reinterpret_cast<uint32_t *>(smem);
    unsigned char *const xt = smem + IMAGE;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t laneoff = (uint32_t)(lane & (Codec::C - 1)) << 2;
    const int total = p.item_end[kWdMaxJobs - 1];
    const void *cur_lut = nullptr;

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
    // half h of step g: x columns 128 g + 32 sup + 16 h + 8 jh
    auto load_x = [&](int g, int h) __attribute__((always_inline)) {
        const uint32_t col = (uint32_t)(g * 128 + 16 * h) * 2u;
#pragma unroll
        for (int r = 0; r < CPT; r++) xr[r] = __builtin_amdgcn_raw_buffer_load_b128(rs_x, xvo[r] != kBufDead ? xvo[r] + col : kBufDead, 0, 0);
    };
    auto store_x = [&](auto hc, unsigned char *buf) __attribute__((always_inline)) {
        // (chunk r is chunk 0's piece of batch row b + 64 r: four groups further, the same rotation)
        int t = tid;
        asm volatile("" : "+v"(t));  // the store address is computed HERE, not kept in a register through the steps
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
        const LutWideJob jb = p.job[j];
        const int item = gitem - item_begin;
        const int rg = item >> p.lsk, ks = item & ((1 << p.lsk) - 1);
        const int g0 = (p.T * ks) >> p.lsk, g1 = (p.T * (ks + 1)) >> p.lsk;  // (host: T >= 4 << lsk where lsk > 0, T >= 1: never empty)
        const int sr = rg * kWdWaves + wave;
        const bool live = sr < jb.nrows;  // (wave-uniform: a row past the end only keeps the staging and the barriers company)
        const int srow = live ? sr : 0;
        const int nsc = p.T * 4;
        const buf_rsrc_t rs = gemm_rsrc(jb.qw + (long)srow * nsc * 16 * NW, live ? nsc * 64 * NW : 0);

        load_x(g0, 0);
        uint32_t wa[NW], wb[NW];
        load_step_w_buf<NW>(rs, g0, lane, wa);
        if (jb.lut != cur_lut) {  // workgroup-uniform; the barrier that ended the last item freed the image
            Codec::build(lut, jb.lut, tid, NT);
            cur_lut = jb.lut;
        }
        store_x(h0, xt);
        typename Map::Accum acc;
        acc.zero();
        __syncthreads();

        // A step: half 1's tile and the next step's words requested; half 0 from slot 0; half 1's tile into slot 1 (last read one
        // half-step ago, before the latest barrier); barrier; the next step's first half requested; half 1 from slot 1 with the SAME
        // words; that tile into slot 0; barrier.
        auto one_step = [&](int g, uint32_t(&wc)[NW], uint32_t(&wn)[NW]) __attribute__((always_inline)) {
            const int gn = g + 1 < g1 ? g + 1 : g;
            load_x(g, 1);
            load_step_w_buf<NW>(rs, gn, lane, wn);
            if (live) wide_half<Codec, NG, 0>(lut, laneoff, wc, xt, lane, acc.v);
            store_x(h1, xt + SLOT);
            __syncthreads();
            load_x(gn, 0);
            if (live) wide_half<Codec, NG, 1>(lut, laneoff, wc, xt + SLOT, lane, acc.v);
            store_x(h0, xt);
            __syncthreads();
        };
        int g = g0;
        for (; g + 1 < g1; g += 2) {
            one_step(g, wa, wb);
            one_step(g + 1, wb, wa);
        }
        if (g < g1) one_step(g, wa, wb);

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

}  // namespace qpal
