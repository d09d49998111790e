// Routed fused decode + GEMV for mixture-of-experts layers: qpal_moe_gemv.
//
// The fused GEMV of tc_kernels.h takes every weight pointer as a kernel argument planned on the host; an expert is chosen on the
// device, per row and step.  Here a work item is (group g of the route's table, block of supertile rows of expert
// group_expert[g]'s matrix): the group's at most 8 rows are the 8 batch columns of ONE MFMA batch group (Acc<1>,
// gemv_step_any<Codec, 1>), so the trellis is decoded once for all of them; the weight, second-stream and Wscale pointers come
// from per-projection device tables indexed by the group's expert; x rows come through x_index and the output row is the sorted
// position.  The geometry is a function of the shapes only: the 16 waves of a workgroup are RP = 16 / KS rows x KS parts of K, a
// row's lead wave sums the parts through LDS in wave order (run_sum) — no float atomics, no split-K across workgroups — and a
// row's result depends neither on which other rows share its group nor on n.
#include "tc_kernels.h"

namespace qpal {

namespace {

constexpr int kMoeS = 9;  // codebooks of 512 pairs: KV 2..8, one 64 KiB image
using MoeImage = TcqCodec<kMoeS, 8>;

struct MoeGemvProj {
    const uint64_t *c1, *c2, *wscale;  // device tables [E] of device pointers
    int nrows, kv, kv2, out_col;
};

struct MoeGemvParams {
    float *out;
    long ldo;
    int out_rows;
    int nproj;
    MoeGemvProj pj[2];
    const uint16_t *x;
    long ldx;
    int x_rows;
    const int *x_index, *group_expert, *group_first, *group_count, *ngroups;
    int max_groups, E;
    int nsc1, nsc2, st1, st2, col2;
    int lg_ks;  // log2 of the parts a row's steps are cut into
    const void *tab;
    float oscale;
};

// parts of K per row: every wave keeps at least four steps
inline int moe_lg_ks(int steps) {
    int lg = 0;
    while (lg < 4 && (8 << lg) <= steps) lg++;
    return lg;
}

// steps [s0, s1) of one stream of one supertile row, the group's x rows fetched through this lane's row pointer (null: zeros)
template <class CK>
__device__ __forceinline__ void moe_run(const uint32_t *lut, uint32_t laneoff, const uint32_t *rowbase, int nsc, const uint16_t *xrow,
                                        int s0, int s1, int lane, Acc<1> &acc) {
    constexpr int NW = CK::NW;
    const buf_rsrc_t rs = gemm_rsrc(rowbase, nsc * 64 * NW);
    uint32_t w[NW], wb[NW];
    load_step_w_buf<NW>(rs, s0, lane, w);
    auto step_x = [&](int s, u32x4(&xb)[1][2]) {
        const int sc = s * 4 + (lane >> 4);
        if (xrow && sc < nsc) {
            const uint16_t *row = xrow + sc * 32;
#pragma unroll
            for (int ksub = 0; ksub < 2; ksub++) {
                const u32x2 lo = *reinterpret_cast<const u32x2 *>(row + 16 * ksub);
                const u32x2 hi = *reinterpret_cast<const u32x2 *>(row + 16 * ksub + 8);
                xb[0][ksub] = u32x4{lo.x, lo.y, hi.x, hi.y};
            }
        } else {
            xb[0][0] = xb[0][1] = u32x4{0u, 0u, 0u, 0u};
        }
    };
    for (int s = s0; s < s1; s += 2) {
        {
            load_step_w_buf<NW>(rs, s + 1 < s1 ? s + 1 : s, lane, wb);
            __builtin_amdgcn_sched_barrier(0);
            u32x4 xb[1][2];
            step_x(s, xb);
            gemv_step_any<CK, 1>(lut, laneoff, w, xb, acc);
        }
        if (s + 1 < s1) {
            load_step_w_buf<NW>(rs, s + 2 < s1 ? s + 2 : s + 1, lane, w);
            __builtin_amdgcn_sched_barrier(0);
            u32x4 xb[1][2];
            step_x(s + 1, xb);
            gemv_step_any<CK, 1>(lut, laneoff, wb, xb, acc);
        }
    }
}

__global__ __launch_bounds__(1024) void moe_gemv_kernel(const MoeGemvParams p) {
    __shared__ __attribute__((aligned(16))) uint32_t lut[MoeImage::LDS_DWORDS];
    __shared__ float red[16 * 8 * 32];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = blockIdx.y;
    int ng = *p.ngroups;
    ng = ng < p.max_groups ? ng : p.max_groups;
    if (g >= ng) return;
    const int e = p.group_expert[g], first = p.group_first[g], count = p.group_count[g];
    if ((unsigned)e >= (unsigned)p.E || count < 1 || count > 8 || first < 0 || first + count > p.out_rows) return;
    const uint32_t laneoff = (uint32_t)(lane & (MoeImage::C - 1)) << 2;
    MoeImage::build(lut, p.tab, tid, 1024);
    // this lane's x row: MFMA column c = 2 b + u is batch row b, column half u
    const int b_l = (lane & 15) >> 1;
    const uint16_t *xrow = nullptr;
    if (b_l < count) {
        const int xr = p.x_index ? p.x_index[first + b_l] : first + b_l;
        if ((unsigned)xr < (unsigned)p.x_rows) xrow = p.x + (long)xr * p.ldx + 4 * (lane & 1);
    }
    __syncthreads();
    const int ks = 1 << p.lg_ks, rp = 16 >> p.lg_ks, steps = p.st1 + p.st2;
    const int rows0 = p.pj[0].nrows, rows = rows0 + (p.nproj > 1 ? p.pj[1].nrows : 0);
    const int pt = wave & (ks - 1);
    for (int blk = blockIdx.x; blk * rp < rows; blk += gridDim.x) {
        const int vr = blk * rp + (wave >> p.lg_ks);
        const bool work = vr < rows;  // (wave-uniform)
        const bool second = vr >= rows0;
        const int sr = second ? vr - rows0 : vr;
        const uint64_t *t1 = second ? p.pj[1].c1 : p.pj[0].c1, *t2 = second ? p.pj[1].c2 : p.pj[0].c2;
        const int kv1 = second ? p.pj[1].kv : p.pj[0].kv, kv2 = second ? p.pj[1].kv2 : p.pj[0].kv2;
        Acc<1> acc;
        static_for<0, 4>([&](auto ac) { acc.v[0][decltype(ac)::value] = float4_t{0.f, 0.f, 0.f, 0.f}; });
        if (work) {
            const int v0 = (pt * steps) >> p.lg_ks, v1 = ((pt + 1) * steps) >> p.lg_ks;
            for (int st = 0; st < 2; st++) {  // a wave's part may reach into both streams of a column-split matrix: one run each
                const int base = st ? p.st1 : 0, nst = st ? p.st2 : p.st1;
                const int s0 = v0 - base > 0 ? v0 - base : 0, s1 = v1 - base < nst ? v1 - base : nst;
                if (s0 >= s1) continue;
                const int nsc = st ? p.nsc2 : p.nsc1;
                const uint32_t *c = reinterpret_cast<const uint32_t *>((st ? t2 : t1)[e]);
                const uint16_t *xr = xrow ? xrow + (st ? p.col2 : 0) : nullptr;
                dispatch_kv<kMoeS>(st ? kv2 : kv1, [&](auto kc) {
                    using CK = TcqCodec<kMoeS, decltype(kc)::value>;
                    moe_run<CK>(lut, laneoff, c + (long)sr * nsc * 16 * CK::NW, nsc, xr, s0, s1, lane, acc);
                });
            }
        }
        // lane (q = lane >> 4, c = 2 b + u), register r of acc[msub * 2 + jl] = D[4 q + r][c], valid where r & 1 == u: the even lane's
        // r = 0 / 2 plus its odd neighbour's r = 1 / 3 are the two column halves of tile rows 2 q and 2 q + 1 (tc_gemv_kernel)
        {
            const int q = lane >> 4;
            const bool writer = (lane & 1) == 0 && b_l < count && work;
            float *dst = red + (wave * 8 + b_l) * 32 + 2 * q;
            static_for<0, 4>([&](auto ac) {  // rows 16 msub + 8 jl + 2 q + {0, 1}
                constexpr int a = decltype(ac)::value;
                const float4_t d = acc.v[0][a];
                const float r0 = d[0] + lane_xor<1>(d[1]);
                const float r1 = d[2] + lane_xor<1>(d[3]);
                if (writer) {
                    dst[8 * a] = r0;
                    dst[8 * a + 1] = r1;
                }
            });
        }
        __syncthreads();
        if (work && pt == 0) {  // the row's lead wave: the parts in wave order, lanes 0..31 the even batch rows, 32..63 the odd ones
            const int fr = lane & 31;
            const MoeGemvProj &pj = second ? p.pj[1] : p.pj[0];
            float osc = p.oscale;
            if (pj.wscale) osc *= (float)__builtin_bit_cast(_Float16, as_global(reinterpret_cast<const uint16_t *>(pj.wscale[e]))[sr * 32 + fr]);
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int b = (lane >> 5) + 2 * i;
                if (b < count) {
                    const float v = run_sum<false>(red + (wave * 8 + b) * 32 + fr, 8 * 32, ks);
                    p.out[(long)(first + b) * p.ldo + pj.out_col + sr * 32 + fr] = v * osc;
                }
            }
        }
        __syncthreads();  // (the next block of rows reuses `red`)
    }
}

}  // namespace

}  // namespace qpal

using namespace qpal;

extern "C" int qpal_moe_gemv(float *out, long ldo, int out_rows, const qpal_moe_proj *proj, int nproj, const void *x_f16, long ldx,
                             int x_rows, const int *x_index, const int *group_expert, const int *group_first, const int *group_count,
                             const int *ngroups, int max_groups, int E, int k, const void *tlut, int S, float oscale, void *stream) {
    if (!out || !proj || !x_f16 || !group_expert || !group_first || !group_count || !ngroups || !tlut) return QPAL_E_NULL;
    if (nproj < 1 || nproj > 2) return QPAL_E_SHAPE;
    const bool split = proj[0].kv2 != 0;
    if (k <= 0 || k % 32 || (split && k % 64) || out_rows < 1 || x_rows < 1 || max_groups < 1 || E < 1 || E > 256 || ldx < k || ldx % 4)
        return QPAL_E_SHAPE;
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
    MoeGemvParams p{};
    p.out = out, p.ldo = ldo, p.out_rows = out_rows, p.nproj = nproj;
    int rows = 0;
    for (int j = 0; j < nproj; j++) {
        const qpal_moe_proj &q = proj[j];
        if ((reinterpret_cast<uintptr_t>(q.c1) | reinterpret_cast<uintptr_t>(q.c2) | reinterpret_cast<uintptr_t>(q.wscale)) & 7) return QPAL_E_ALIGN;
        p.pj[j] = MoeGemvProj{static_cast<const uint64_t *>(q.c1), static_cast<const uint64_t *>(q.c2), static_cast<const uint64_t *>(q.wscale),
                              q.m / 32, q.kv, q.kv2, q.out_col};
        rows += q.m / 32;
    }
    p.x = static_cast<const uint16_t *>(x_f16), p.ldx = ldx, p.x_rows = x_rows, p.x_index = x_index;
    p.group_expert = group_expert, p.group_first = group_first, p.group_count = group_count, p.ngroups = ngroups;
    p.max_groups = max_groups, p.E = E;
    const int k1 = split ? k / 2 : k;
    p.nsc1 = k1 / 32, p.nsc2 = split ? k1 / 32 : 0;
    p.st1 = (p.nsc1 + 3) / 4, p.st2 = (p.nsc2 + 3) / 4, p.col2 = k1;
    p.lg_ks = moe_lg_ks(p.st1 + p.st2);
    p.tab = tlut, p.oscale = oscale == 0.0f ? 1.0f : oscale;
    const int rp = 16 >> p.lg_ks, nblk = (rows + rp - 1) / rp;
    int gx = 512 / max_groups;  // ~two workgroups per CU when every group is in use: each builds the codebook image once
    gx = gx < 1 ? 1 : gx;
    gx = gx < nblk ? gx : nblk;
    if (max_groups > 65535) return QPAL_E_SHAPE;
    hipLaunchKernelGGL(moe_gemv_kernel, dim3(gx, max_groups), dim3(1024), 0, static_cast<hipStream_t>(stream), p);
    return (int)hipGetLastError();
}
