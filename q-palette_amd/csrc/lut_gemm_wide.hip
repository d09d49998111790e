// qpal_lut_gemm_wide: the entry point of the VQ/SQ wide dequant GEMM (lut_gemm_wide.h) — its checks, in
// qpal_tcq_gemm_wide's order, the K split (wide_split) and the launch.  The kernels are built in lut_gemm_wide_ng*_v*.hip.
#include "lut_gemm_wide.h"

using namespace qpal;

extern "C" int qpal_lut_gemm_wide(const qpal_lut_job *jobs, int njobs, int n, int bits, int vec, void *stream) {
    if (!jobs) return QPAL_E_NULL;
    if (njobs < 1 || njobs > kWdMaxJobs || n < kWdMinN || n > kWdMaxN) return QPAL_E_SHAPE;
    const int k = jobs[0].k;
    if (k <= 0 || k % 128 || (long)n * k * 2 >= (1l << 31)) return QPAL_E_SHAPE;  // (x is read through one buffer descriptor)
    for (int j = 0; j < njobs; j++) {
        const qpal_lut_job &q = jobs[j];
        if (q.m <= 0 || q.m % 32 || q.k != k || (q.ldo != 0 && q.ldo < q.m)) return QPAL_E_SHAPE;
    }
    bool known = false;
#define QPAL_LUT(B_, V_) known = known || (bits == B_ && vec == V_);
#include "lut_table.inc"
#undef QPAL_LUT
    if (!known) return QPAL_E_PARAM;
    for (int j = 0; j < njobs; j++) {
        const qpal_lut_job &q = jobs[j];
        if (!q.out || !q.qweight || !q.x || !q.lut) return QPAL_E_NULL;
        // no rotation, RMSNorm or activation in this launch; one x for all jobs
        if (q.x_had || q.x_su || q.x_f32 || q.x_rms_eps != 0.0f || q.x_rms_w || q.act_out || q.act_su || q.x_hadk || q.x_K || q.x != jobs[0].x)
            return QPAL_E_PARAM;
        if ((reinterpret_cast<uintptr_t>(q.x) & 15) || (reinterpret_cast<uintptr_t>(q.wscale) & 1)) return QPAL_E_ALIGN;
        if ((reinterpret_cast<uintptr_t>(q.out) | reinterpret_cast<uintptr_t>(q.qweight) | reinterpret_cast<uintptr_t>(q.lut)) & 3) return QPAL_E_ALIGN;
    }
    LutWideParams p{};
    p.x = static_cast<const uint16_t *>(jobs[0].x), p.n = n, p.k = k, p.T = k / 128;
    int nblk = 0;
    for (int j = 0; j < njobs; j++) nblk += (jobs[j].m / 32 + kWdWaves - 1) / kWdWaves;
    p.lsk = wide_split(nblk, p.T);
    int items = 0;
    bool clear = false;
    WideClear wc{};
    for (int j = 0; j < kWdMaxJobs; j++) {
        if (j < njobs) {
            const qpal_lut_job &q = jobs[j];
            p.job[j] = LutWideJob{q.out, q.ldo ? q.ldo : q.m, static_cast<const uint32_t *>(q.qweight), static_cast<const uint16_t *>(q.wscale),
                                  q.lut, q.oscale == 0.0f ? 1.0f : q.oscale, q.m / 32, q.accumulate};
            items += ((q.m / 32 + kWdWaves - 1) / kWdWaves) << p.lsk;
            clear = clear || !q.accumulate;
            if (!q.accumulate) wc.out[j] = p.job[j].out, wc.ldo[j] = p.job[j].ldo, wc.cols[j] = q.m;
        }
        p.item_end[j] = items;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (p.lsk > 0 && clear) launch_gemm_wide_clear(wc, n, njobs, st);
    const int grid = items < kWdGrid ? items : kWdGrid;
    if (n <= 192) return vec == 1 ? launch_lut_gemm_wide_ng12_v1(p, bits, grid, st) : launch_lut_gemm_wide_ng12_v2(p, bits, grid, st);
    return vec == 1 ? launch_lut_gemm_wide_ng16_v1(p, bits, grid, st) : launch_lut_gemm_wide_ng16_v2(p, bits, grid, st);
}
