// TCQ fused decode+GEMV for launches whose jobs have DIFFERENT KV (same codebook size S): one kernel per S that switches
// to the job's decode loop per work item (tc_kernels.h: TcqAny).  Single-stream layers, batch <= 8.
#include "gemv_launch.h"
#include "tcq_kernels_api.h"

namespace qpal {

int launch_tcq_gemv_any(const TcMultiParams &p, int S, int grid, hipStream_t stream) {
    if (S == 9) return launch_gemv<TcqAny<9>, void, 1>(p, grid, stream);
    if (S == 10) return launch_gemv<TcqAny<10>, void, 1>(p, grid, stream);
    if (S == 11) return launch_gemv<TcqAny<11>, void, 1>(p, grid, stream);
    return QPAL_E_PARAM;
}

}  // namespace qpal
