// Fused decode + skinny GEMM for batches 9..128, second fragment mapping (round 5): the MFMA's 16 rows are 16 REAL rows of W.
//
// tc_gemm.h inherited the GEMV's mapping: a wave-lane holds the weights of two reference lanes = one tile row x one column HALF
// (4 of every 8 columns), so an MFMA's 16 rows were (8 tile rows x 2 column halves) and its 16 columns (8 batch rows x 2 halves):
// only the products whose halves agree are valid.  The matrix pipe did twice the needed work, the accumulators took 16 VGPRs per 8
// batch rows (128 at batch 64: 256-VGPR kernels, two waves per SIMD), and a pass over the weights could carry 64 batch rows at most
// (65 rows = two passes: the 64 -> 65 cliff).
//
// Here lanes p and p ^ 1 of a DPP row — the two column halves of tile row p >> 1 — EXCHANGE half of their decoded pairs: the even
// lane keeps its pairs of tile row r (jl = 0) and takes the odd lane's, the odd lane keeps its pairs of row r + 8 (jl = 1) and takes
// the even lane's.  Each then holds 8 CONSECUTIVE columns of one row: an A fragment of v_mfma_f32_16x16x32_f16 whose rows are the
// 16 rows (r, r + 8 for r = 0..7) of a 16-row block and whose K is (4 supertiles x 8 columns); the B fragment is 8 consecutive
// columns of one batch row, 16 batch rows per MFMA.  Per step and 16 batch rows: 8 MFMAs (was 16), 8 accumulator VGPRs (was 32);
// the exchange costs one v_cndmask_b32_dpp per decoded pair (32 per step, full-rate VALU).  One pass carries 128 batch rows.
//
// Everything else is tc_gemm.h's: the 8 waves of a workgroup own 8 supertile rows and walk one K range in lockstep, the step's
// [n][128] tile of x is staged once per workgroup (global -> registers -> LDS, two steps ahead where four slots fit), split-K over
// workgroups with atomics only where a layer has too few rows.  Same arithmetic per (row, batch) up to the K split and the order
// of the eight column blocks inside a step.  Replaces, for bs > 8, the reference's decode-to-HBM + cuBLAS path
// (lib/linear/tcq_linear.py:75-84, vq_linear.py:60-66).
#pragma once
#include "tc_gemm.h"

namespace qpal {

constexpr int kG16Group = 4096;  // bytes of one step's x tile per 16 batch rows: [sup 4][ksub, jh 4][slot 16][16 B]

// x tile layout.  The 16-byte piece (batch row b, columns 8 q .. 8 q + 7 of the step; q = 4 sup + 2 ksub + jh) lives at
//   (b >> 4) * 4096 + q * 256 + ((b + q) & 15) * 16:
// the 16 batch rows' pieces of one q form a 256-byte block — the lanes (sup, c) of a 16-lane group of a ds_read_b128 cover 64
// banks exactly once — and the rotation by q spreads the 8 lanes of a ds_write_b128 group (one batch row, 8 values of q) over the
// banks as well (without it they all hit one 16-byte window: 8-way conflicts on every staging store).
// (round 5, second version) The rotation is g(q) = (q & 3) + 4 (q >> 3), not q itself.  A ds_read_b128 is served in
// four groups of 16 lanes that are NOT 16 consecutive lanes (MI355X_MICROARCH.md, LDS: {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ...):
// a group mixes batch rows {0-3, 12-15} of column block q with rows {4-11} of block q + 4, so the two blocks must share one rotation
// or four of the sixteen 16-byte windows collide (measured: SQ_LDS_BANK_CONFLICT 54 % of the LDS cycles of a batch-64 step).  The
// staging stores keep their eight lanes of one batch row on eight different windows by taking the column blocks in the order
// 0-3, 8-11 | 4-7, 12-15 (g16_chunk_q).
__device__ __forceinline__ int g16_rot(int q) { return (q & 3) + 4 * (q >> 3); }
__device__ __forceinline__ int g16_chunk_q(int j) { return (j & 3) | ((j & 4) << 1) | ((j & 8) >> 1); }  // staging lane j of a batch row -> its column block
__device__ __forceinline__ int g16_x_off(int b, int q) { return (b >> 4) * kG16Group + q * 256 + (((b + g16_rot(q)) & 15) << 4); }

// The four decoded pairs an A fragment is made of — tile group G = ksub * 2 + msub, column block JH.  Pair index I = jl + 2 jh + 4 isB
// (tc_kernels.h gemv_step); a lane's pairs (jl, jh) are columns 4 u + 0..3 (isB = 0: +0, 1; isB = 1: +2, 3) of tile row (p >> 1) + 8 jl.
struct G16Pairs {
    uint32_t p0a, p0b, p1a, p1b;  // p0: tile row r (jl = 0), p1: tile row r + 8 (jl = 1)
};
template <class Codec, int G, int JH>
__device__ __forceinline__ G16Pairs g16_pairs(const uint32_t *lut, uint32_t laneoff, const uint32_t (&w)[Codec::NW]) {
    uint32_t nh = 0u;
    if constexpr (Codec::kNeedsNext) nh = row16_next(Codec::template head<G>(w));  // (one per G: CSE)
    return G16Pairs{Codec::template pair<G, 0 + 2 * JH>(lut, laneoff, w, nh), Codec::template pair<G, 0 + 2 * JH + 4>(lut, laneoff, w, nh),
                    Codec::template pair<G, 1 + 2 * JH>(lut, laneoff, w, nh), Codec::template pair<G, 1 + 2 * JH + 4>(lut, laneoff, w, nh)};
}
// The exchange.  Even lane (u = 0): row r, columns 0..3 own (p0), 4..7 the partner's p0; odd lane: row r + 8, columns 0..3 the
// partner's p1, 4..7 own (p1).  "The partner's" = lane ^ 1 = DPP quad_perm [1, 0, 3, 2], folded into the select: v_cndmask_b32_dpp
// computes vcc ? src1 : dpp(src0) — ONE full-rate instruction per pair.  (Written as a move + a select the compiler emitted both: 64
// more vector instructions per step.)  Hazards the assembler does not see inside an asm: a DPP operand written by the VALU
// instruction right in front needs two wait states (s_nop 1); SALU writes of VCC are interlocked.  Two fragments are exchanged
// under one pair of lane masks.
__device__ __forceinline__ void g16_xchg2(const G16Pairs &q, const G16Pairs &r, u32x4 &a, u32x4 &b) {
    uint32_t x, y, z, w_, x2, y2, z2, w2;
    asm("s_nop 1\n\t"
        "s_mov_b64 vcc, %[even]\n\t"
        "v_cndmask_b32_dpp %[x], %[p1a], %[p0a], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[y], %[p1b], %[p0b], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[x2], %[r1a], %[r0a], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[y2], %[r1b], %[r0b], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "s_not_b64 vcc, vcc\n\t"
        "v_cndmask_b32_dpp %[z], %[p0a], %[p1a], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[w], %[p0b], %[p1b], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[z2], %[r0a], %[r1a], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
        "v_cndmask_b32_dpp %[w2], %[r0b], %[r1b], vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
        : [x] "=&v"(x), [y] "=&v"(y), [z] "=&v"(z), [w] "=&v"(w_), [x2] "=&v"(x2), [y2] "=&v"(y2), [z2] "=&v"(z2), [w2] "=&v"(w2)
        : [p0a] "v"(q.p0a), [p0b] "v"(q.p0b), [p1a] "v"(q.p1a), [p1b] "v"(q.p1b), [r0a] "v"(r.p0a), [r0b] "v"(r.p0b), [r1a] "v"(r.p1a),
          [r1b] "v"(r.p1b), [even] "s"(0x5555555555555555ull)
        : "vcc", "scc");
    a = u32x4{x, y, z, w_};
    b = u32x4{x2, y2, z2, w2};
}

__device__ __forceinline__ void g16_mfma(float4_t &acc, const u32x4 &a, const u32x4 &b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(half8_t, a), __builtin_bit_cast(half8_t, b), acc, 0, 0, 0);
}

// One step: 8 A fragments t = 2 kj + msub (kj = 2 ksub + jh), each feeding NG MFMAs — acc[grp][msub] accumulates the 16 rows
// 16 msub + (r, r + 8) x 16 batch rows; per kj the B fragments of the NG batch groups (8 consecutive columns of batch row 16 grp + c).
// Software-pipelined: a wave issues in order, and left to the compiler a fragment is decode -> wait for the
// gathers -> exchange -> NG MFMAs; here the pairs of fragment t + 1 are decoded and gathered in front of the MFMAs of fragment t and
// exchanged behind them (the MFMAs cover the gather latency), and the B fragments of kj + 1 are read behind the last use of kj's.
template <class Codec, int T>
__device__ __forceinline__ G16Pairs g16_pairs_t(const uint32_t *lut, uint32_t laneoff, const uint32_t (&w)[Codec::NW]) {
    constexpr int kj = T >> 1, msub = T & 1, ksub = kj >> 1, jh = kj & 1;
    return g16_pairs<Codec, ksub * 2 + msub, jh>(lut, laneoff, w);
}
template <class Codec, int NG>
__device__ __forceinline__ void g16_step(const uint32_t *lut, uint32_t laneoff, const uint32_t (&w)[Codec::NW], const unsigned char *xt, int lane,
                                         float4_t (&acc)[NG][2]) {
    const int sup = lane >> 4, c = lane & 15;
    auto xoff = [&](int kj) { return (4 * sup + kj) * 256 + (((c + g16_rot(4 * sup + kj)) & 15) << 4); };
    // fragment PAIRS (msub 0, 1 of one column block): one VCC flip and one DPP wait per two exchanges, 2 NG MFMAs in a row
    u32x4 xb[NG], xn[NG];
    static_for<0, NG>([&](auto gc) { xb[decltype(gc)::value] = *reinterpret_cast<const u32x4 *>(xt + decltype(gc)::value * kG16Group + xoff(0)); });
    u32x4 a0, a1;
    g16_xchg2(g16_pairs_t<Codec, 0>(lut, laneoff, w), g16_pairs_t<Codec, 1>(lut, laneoff, w), a0, a1);
    static_for<0, 4>([&](auto kc) {
        constexpr int kj = decltype(kc)::value;
        G16Pairs n0{}, n1{};
        if constexpr (kj < 3) {
            n0 = g16_pairs_t<Codec, 2 * kj + 2>(lut, laneoff, w);
            n1 = g16_pairs_t<Codec, 2 * kj + 3>(lut, laneoff, w);
            static_for<0, NG>([&](auto gc) { xn[decltype(gc)::value] = *reinterpret_cast<const u32x4 *>(xt + decltype(gc)::value * kG16Group + xoff(kj + 1)); });
        }
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, NG>([&](auto gc) { g16_mfma(acc[decltype(gc)::value][0], a0, xb[decltype(gc)::value]); });
        static_for<0, NG>([&](auto gc) { g16_mfma(acc[decltype(gc)::value][1], a1, xb[decltype(gc)::value]); });
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (kj < 3) {
            g16_xchg2(n0, n1, a0, a1);
            static_for<0, NG>([&](auto gc) { xb[decltype(gc)::value] = xn[decltype(gc)::value]; });
        }
    });
}

// The mapping as tc_gemm_kernel takes it (tc_gemm.h: GemmHalves): groups of 16 batch rows.
template <int NG>
struct G16Map {
    static constexpr int ROWS = 16, GROUPS = NG;
    static constexpr int XBUF = NG * kG16Group;
    static constexpr int SCRATCH = 2048;
    struct Accum {
        float4_t v[NG][2];
        __device__ __forceinline__ void zero() {
            static_for<0, NG>([&](auto gc) {
                v[decltype(gc)::value][0] = float4_t{0.f, 0.f, 0.f, 0.f};
                v[decltype(gc)::value][1] = float4_t{0.f, 0.f, 0.f, 0.f};
            });
        }
    };
    static constexpr bool Q_PERMUTED = true;
    static __device__ __forceinline__ int chunk_q(int j) { return g16_chunk_q(j); }
    static __device__ __forceinline__ void store_chunk(unsigned char *buf, int b, int q, const u32x4 &v) {
        *reinterpret_cast<u32x4 *>(buf + g16_x_off(b, q)) = v;
    }
    static constexpr bool ZERO_IN_REG = false;  // dead chunks: zeros selected at the store (store_x, tc_gemm.h)
    template <class Codec>
    static __device__ __forceinline__ void step(const uint32_t *lut, uint32_t laneoff, const uint32_t (&w)[Codec::NW], const unsigned char *xt,
                                                int lane, Accum &acc) {
        g16_step<Codec, NG>(lut, laneoff, w, xt, lane, acc.v);
    }
    // acc.v[GRP][msub]: lane (q4, c) holds D[i = 4 q4 + e][c], e = 0..3: batch row 16 GRP + c, MFMA row i = A lane
    // p = 2 r + u -> row 16 msub + (i >> 1) + 8 (i & 1) of the supertile: e = 0, 1, 2, 3 are rows 2 q4, 2 q4 + 8, 2 q4 + 1, 2 q4 + 9 (+ 16 msub)
    template <int GRP>
    static __device__ __forceinline__ void scatter(float *scr, const Accum &acc, int q4, int c) {
        static_for<0, 2>([&](auto mc) {
            constexpr int msub = decltype(mc)::value;
            const float4_t d = acc.v[GRP][msub];
            float *dst = scr + c * 32 + 16 * msub + 2 * q4;
            *reinterpret_cast<float2 *>(dst) = float2{d[0], d[2]};      // rows 2 q4, 2 q4 + 1
            *reinterpret_cast<float2 *>(dst + 8) = float2{d[1], d[3]};  // rows 2 q4 + 8, 2 q4 + 9
        });
    }
};

// the mapping of a launch with NBG batch groups of 8 rows: 1, 2 (batches <= 8 / 16) keep the GEMV's mapping — with one group of 16 rows an
// A fragment feeds ONE MFMA and the exchange is pure cost: measured -3 % at batch 16 —, 4, 8, 10, 16 run in groups of 16 rows
template <int NBG>
using gemm_map = std::conditional_t<NBG <= 2, GemmHalves<NBG>, G16Map<NBG / 2>>;

}  // namespace qpal
