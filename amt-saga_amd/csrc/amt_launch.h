// THE launch of a kernel that needs more dynamic LDS than the default limit, and the compute-unit count: both kept per
// device and safe under concurrent callers (the book-keeping: amt_launch_core.h).
#pragma once
#include "amt_common.h"
#include "amt_launch_core.h"

#define AMT_LDS_CQT (159 * 1024)     /* the dynamic-LDS ceiling the CQT kernels ask for */
#define AMT_LDS_CONV (80 * 1024)     /* ... and the split-bf16 / split-fp16 tiled convolutions */

inline amt_lds_limits &amt_lds_granted() { static amt_lds_limits limits; return limits; }

// Kern<<<grid, block, lds, st>>>(args...) with Kern's dynamic-LDS limit on the current device at least lds_cap bytes (0:
// it stays within the default, nothing is raised): raised on Kern's first launch on a device and when a larger cap comes
template <auto Kern, class... Args>
static int amt_launch(size_t lds_cap, dim3 grid, dim3 block, size_t lds, hipStream_t st, Args... args) {
    if (lds_cap) {
        int dev = 0;
        AMT_HIP_CHECK(hipGetDevice(&dev));
        const void *fn = reinterpret_cast<const void *>(Kern);
        const int rc = amt_lds_granted().request(dev, fn, lds_cap, [&](size_t bytes) -> int {
            AMT_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            return AMT_OK;
        });
        if (rc != AMT_OK) return rc;
    }
    Kern<<<grid, block, lds, st>>>(args...);
    AMT_LAUNCH_CHECK();
    return AMT_OK;
}

// compute units of the current device, asked once per device; 256 where the runtime will not say
inline int amt_cu_count() {
    static std::mutex mu; static std::map<int, int> counts;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::lock_guard<std::mutex> hold(mu);
    int &cus = counts[dev];
    if (cus <= 0 && (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)) cus = 256;
    return cus;
}
