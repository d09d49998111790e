// What the wide dequant GEMMs share (tcq_gemm_wide.hip: DESIGN.md §39, lut_gemm_wide.hip: §43): the half-step geometry of the x
// tile, one half-step of MFMAs for any codec of tc_gemm16.h's fragment mapping, the K split and the kernel that clears an output
// in front of a split launch.  The layout is described at the head of tcq_gemm_wide.hip.
#pragma once
#include "tc_gemm16.h"

namespace qpal {

constexpr int kWdWaves = 8;             // waves = supertile rows of a workgroup
constexpr int kWdThreads = 64 * kWdWaves;
constexpr int kWdGroup = kG16Group / 2;  // bytes of a half tile per 16 batch rows
constexpr int kWdMaxJobs = 4;
constexpr int kWdMinN = 129, kWdMaxN = 256;
constexpr int kWdGrid = 256;            // one workgroup per CU

// chunk id of a half tile -> (batch row, supertile, column block half jh): ids 8 i .. 8 i + 7 — the lanes of one staging store — are
// batch rows b, b + 2 x supertiles {lo, lo + 2} x jh {0, 1}
struct WideChunk {
    int b, sup, jh;
};
__device__ __forceinline__ WideChunk wide_chunk(int id) {
    const int l = id & 7, rest = id >> 3, r7 = rest >> 1;
    return WideChunk{(r7 & 1) + 4 * (r7 >> 1) + 2 * (l >> 2), (l & 2) + (rest & 1), l & 1};
}
template <int H>
__device__ __forceinline__ int wide_x_off(int b, int sup, int jh) {
    return (b >> 4) * kWdGroup + (2 * sup + jh) * 256 + (((b + g16_rot(4 * sup + 2 * H + jh)) & 15) << 4);
}

// Half H of a step: column blocks kj = 2 H + jh.  Per kj the two A fragments (msub 0, 1) are decoded and exchanged once and feed
// 2 NG MFMAs; the B fragments come two groups at a time, one pair ahead.
template <class Codec, int NG, int H>
__device__ __forceinline__ void wide_half(const uint32_t *lut, uint32_t laneoff, const uint32_t (&w)[Codec::NW], const unsigned char *xt, int lane,
                                          float4_t (&acc)[NG][2]) {
    int lane_x = lane;
    asm volatile("" : "+v"(lane_x));  // (the B fragments' addresses are computed here, not kept in registers across the half-steps)
    const int sup = lane_x >> 4, c = lane_x & 15;
    static_for<0, 2>([&](auto jc) {
        constexpr int jh = decltype(jc)::value, kj = 2 * H + jh;
        u32x4 a0, a1;
        g16_xchg2(g16_pairs_t<Codec, 2 * kj>(lut, laneoff, w), g16_pairs_t<Codec, 2 * kj + 1>(lut, laneoff, w), a0, a1);
        const unsigned char *xl = xt + wide_x_off<H>(c, sup, jh);
        // (the order is pinned: left to itself the scheduler requests the B fragments of all NG groups at once and spills)
        u32x4 xb[2], xn[2];
        static_for<0, 2>([&](auto gc) { xb[decltype(gc)::value] = *reinterpret_cast<const u32x4 *>(xl + decltype(gc)::value * kWdGroup); });
        static_for<0, NG / 2>([&](auto bc) {
            constexpr int g2 = 2 * decltype(bc)::value;
            if constexpr (g2 + 2 < NG)
                static_for<0, 2>([&](auto gc) { xn[decltype(gc)::value] = *reinterpret_cast<const u32x4 *>(xl + (g2 + 2 + decltype(gc)::value) * kWdGroup); });
            __builtin_amdgcn_sched_barrier(0);
            static_for<0, 2>([&](auto gc) { g16_mfma(acc[g2 + decltype(gc)::value][0], a0, xb[decltype(gc)::value]); });
            static_for<0, 2>([&](auto gc) { g16_mfma(acc[g2 + decltype(gc)::value][1], a1, xb[decltype(gc)::value]); });
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (g2 + 2 < NG) static_for<0, 2>([&](auto gc) { xb[decltype(gc)::value] = xn[decltype(gc)::value]; });
        });
    });
}

// K split of a launch with nblk blocks of 8 supertile rows and T steps per row: the lockstep kernels' rule (qpal_capi.hip plan_gemm) —
// doubled while the launch has fewer than kWdWantItems items and every split keeps kWdMinSteps steps.  A launch that rule leaves
// whole is left whole here too: the same chain of MFMAs per (row, batch row), the same bits as two 128-row passes.
constexpr int kWdWantItems = 192, kWdMinSteps = 4;
inline int wide_split(int nblk, int T) {
    int lsk = 0;
    while ((nblk << lsk) < kWdWantItems && (T >> (lsk + 1)) >= kWdMinSteps && lsk < 5) lsk++;
    return lsk;
}

// Rows 0 .. n - 1 of every output a split launch adds into (a kernel, not a memset node: the launch may be recorded into a graph).
// out == nullptr: an accumulating job, left as it is.  (tcq_gemm_wide.hip)
struct WideClear {
    float *out[kWdMaxJobs];
    long ldo[kWdMaxJobs];
    int cols[kWdMaxJobs];
};
void launch_gemm_wide_clear(const WideClear &c, int n, int njobs, hipStream_t stream);

}  // namespace qpal
