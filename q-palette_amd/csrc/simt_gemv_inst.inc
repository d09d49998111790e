// Instantiates the SIMT-format GEMV kernels for one batch width QPAL_NB.
#include "launch.h"
#include "lut_kernels_api.h"

namespace qpal {

#define QPAL_CAT2(a, b) a##b
#define QPAL_CAT(a, b) QPAL_CAT2(a, b)

int QPAL_CAT(launch_simt_gemv_nb, QPAL_NB)(const SimtParams &p, int bits, int vec, const SimtGeometry &g, hipStream_t stream) {
#define QPAL_SIMT(B_, V_)                                                                               \
    if (bits == B_ && vec == V_) {                                                                      \
        if constexpr (QPAL_NB == 1) {                                                                   \
            if (g.x_lds) {  /* dynamic LDS beside a static image: lift the 64 KiB default once per device */ \
                constexpr auto kern = simt_gemv_kernel<B_, V_, 1, true>;                                \
                const int rc = lds_opt_in<kern>(160 * 1024 - SimtCodec<B_, V_>::LDS_DWORDS * 4);        \
                if (rc != 0) return rc;                                                                 \
                hipLaunchKernelGGL(kern, dim3(g.grid), dim3(g.threads), g.dyn_lds, stream, p, g.split);          \
                return (int)hipGetLastError();                                                          \
            }                                                                                           \
        }                                                                                               \
        hipLaunchKernelGGL((simt_gemv_kernel<B_, V_, QPAL_NB, false>), dim3(g.grid), dim3(g.threads), 0, stream, p, g.split); \
        return (int)hipGetLastError();                                                                  \
    }
#include "simt_table.inc"
#undef QPAL_SIMT
    return QPAL_E_PARAM;
}

}  // namespace qpal
