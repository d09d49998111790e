// Host side of a launch with dynamic LDS, shared by every translation unit that has one.
#pragma once
#include <hip/hip_runtime.h>

namespace qpal {

// More than 64 KiB of dynamic LDS needs an opt-in, per KERNEL and per DEVICE (function attributes belong to the device's code
// object); idempotent, races are harmless.  The latch is keyed on the kernel's VALUE: a latch keyed on the kernel's type is
// shared by every kernel with the same parameter list, and only the first of them to ask is ever opted in.
template <auto Kern>
static int lds_opt_in(int lds_max) {
    static bool attr_set[64] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = -1;
    if (dev < 0 || !attr_set[dev]) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(Kern), hipFuncAttributeMaxDynamicSharedMemorySize, lds_max);
        if (e != hipSuccess) return (int)e;
        if (dev >= 0) attr_set[dev] = true;
    }
    return 0;
}

// Launches Kern with `lds` bytes of dynamic LDS, opted in to `lds_max` where the launch needs it; the HIP error as int.
template <auto Kern, class... Params>
static int launch_lds(dim3 grid, dim3 block, size_t lds, int lds_max, hipStream_t stream, const Params &...p) {
    if (lds > 64 * 1024) {
        const int rc = lds_opt_in<Kern>(lds_max);
        if (rc != 0) return rc;
    }
    hipLaunchKernelGGL(Kern, grid, block, lds, stream, p...);
    return (int)hipGetLastError();
}

}  // namespace qpal
