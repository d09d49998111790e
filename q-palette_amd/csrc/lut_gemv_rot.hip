// VQ/SQ tensor-core-format GEMV kernels that also apply the incoherence rotation to x while staging it.
#include "gemv_launch.h"
#include "lut_kernels_api.h"

namespace qpal {

int launch_lut_tc_gemv_rot(const TcMultiParams &p, int bits, int vec, int grid, hipStream_t stream) {
    if (p.job[0].x_rot == kK28) return launch_lut_tc_gemv_rot28(p, bits, vec, grid, stream);
#define QPAL_LUT(B_, V_) \
    if (bits == B_ && vec == V_) return launch_gemv<LutCodec<B_, V_>, void, 1, 1>(p, grid, stream);
#include "lut_table.inc"
#undef QPAL_LUT
    return QPAL_E_PARAM;
}

}  // namespace qpal
