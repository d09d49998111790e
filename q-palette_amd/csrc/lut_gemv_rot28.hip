// VQ/SQ tensor-core-format GEMV kernels whose x staging applies the 14336-wide rotation of rot_k28.h (codecs whose codebook image
// can lend it 40 KiB of LDS; the host refuses the others: qpal_capi.hip rot_k28_ok).
#include "gemv_launch.h"
#include "lut_kernels_api.h"

namespace qpal {

int launch_lut_tc_gemv_rot28(const TcMultiParams &p, int bits, int vec, int grid, hipStream_t stream) {
#define QPAL_LUT(B_, V_)                                                                                           \
    if (bits == B_ && vec == V_) {                                                                                 \
        if constexpr (LutCodec<B_, V_>::LDS_DWORDS * 4 >= kP28 * kTbRow) {                                         \
            return launch_gemv<LutCodec<B_, V_>, void, 1, 2>(p, grid, stream);                                     \
        } else {                                                                                                   \
            return QPAL_E_SHAPE;                                                                                   \
        }                                                                                                          \
    }
#include "lut_table.inc"
#undef QPAL_LUT
    return QPAL_E_PARAM;
}

}  // namespace qpal
