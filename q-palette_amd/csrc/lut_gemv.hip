// VQ/SQ tensor-core-format fused decode+GEMV kernels (batch 1..8) + launcher.
#include "gemv_launch.h"
#include "lut_kernels_api.h"

namespace qpal {

int launch_lut_tc_gemv(const TcMultiParams &p, int bits, int vec, int nbg, int grid, hipStream_t stream) {
    for (int j = 0; j < p.njobs; j++)
        if (p.job[j].x_rot) return nbg == 1 ? launch_lut_tc_gemv_rot(p, bits, vec, grid, stream) : QPAL_E_SHAPE;
#define QPAL_LUT(B_, V_)                                                             \
    if (bits == B_ && vec == V_)                                                     \
        return nbg == 1 ? launch_gemv<LutCodec<B_, V_>, void, 1>(p, grid, stream)    \
             : nbg == 2 ? launch_gemv<LutCodec<B_, V_>, void, 2>(p, grid, stream)    \
                        : launch_lut_tc_gemv_wide(p, bits, vec, nbg, grid, stream);
#include "lut_table.inc"
#undef QPAL_LUT
    return QPAL_E_PARAM;
}

}  // namespace qpal
