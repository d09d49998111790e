// The one launch of the fused decode+GEMV kernel: every tc_gemv_kernel instantiation of the TCQ and the VQ/SQ units starts here.
#pragma once
#include "tc_kernels.h"
#ifdef QPAL_STAMPS
#include "gemv_stamps.h"
#endif

namespace qpal {

template <class C1, class C2, int NBG, int ROT = 0>
static int launch_gemv(const TcMultiParams &mp, int grid, hipStream_t stream) {
    const TcEarly e = early_args(mp, grid);
    auto launch = [&](const TcMultiParams &q) {
        hipLaunchKernelGGL((tc_gemv_kernel<C1, C2, NBG, ROT>), dim3(grid), dim3(64 * gemv_waves<NBG>()), 0, stream, e.x, e.tab, e.n, e.k, e.on, e.ie, e.su, e.rw, q);
    };
#ifdef QPAL_STAMPS
    if (stamped_launch(mp, grid, ROT, launch)) return (int)hipGetLastError();
#endif
    launch(mp);
    return (int)hipGetLastError();
}

}  // namespace qpal
