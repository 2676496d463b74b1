// Host-side launch helpers shared by every csrc/*.hip: the dynamic-LDS opt-in per (kernel, device), the CU count per device, the storage-type
// switch. The parts that need no HIP (knob reader, once-mask) are in launch_host.h.
#pragma once
#include "common.h"
#include "launch_host.h"

// Launches that ask for more than 64 KiB of dynamic LDS need hipFuncAttributeMaxDynamicSharedMemorySize raised on the kernel, on EVERY device that
// runs it. Call this in front of the launch of `Kernel` with the bytes the launch asks for: at or below 64 KiB nothing happens; above, the attribute
// is set once per (kernel, current device; more than once only under racing first launches) -- to `max_bytes` where the launcher's request varies from call to call (the largest it ever makes), else
// to `bytes`. Returns 0 or the hipError_t of the failed call, which the launcher returns like a failed launch (positive = hipError_t). A kernel's
// first launch is never under stream capture (every captured path runs eagerly first), so the attribute call is never captured either.
template <auto Kernel>
inline int mg_lds_opt_in(size_t bytes, size_t max_bytes = 0) {
    if (bytes <= 64 * 1024) return 0;
    static mg_once_mask once;
    int dev = -1;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return (int)e;
    if (once.is_done(dev)) return 0;
    // the device is remembered only once the attribute is in place: threads that race here each make the (idempotent) call, none launches before
    // it, and a failed call is tried again by the next launch
    e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(max_bytes > bytes ? max_bytes : bytes));
    if (e != hipSuccess) return (int)e;
    once.first_time(dev);
    return 0;
}
#define MG_RETURN_IF(...)                                \
    do {                                           \
        const int rc__ = (__VA_ARGS__);            \
        if (rc__) return rc__;                     \
    } while (0)
// The launch form of it: hipLaunchKernelGGL behind the opt-in for the same kernel and the same bytes (the kernel in parentheses when its template
// arguments hold commas). Launchers whose request varies per call (token_side.hip) call mg_lds_opt_in with their cap themselves.
#define MG_LAUNCH_LDS(kernel, grid, block, lds, st, ...)                    \
    do {                                                                    \
        MG_RETURN_IF(mg_lds_opt_in<kernel>(lds));                                 \
        hipLaunchKernelGGL(kernel, grid, block, lds, st, __VA_ARGS__);      \
    } while (0)

// multiProcessorCount of the current device, asked once per device; 256 (an MI355X) when the runtime does not say
inline int mg_cu_count() {
    static std::atomic<int> ncu[MG_MAX_DEVICES] = {};
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MG_MAX_DEVICES) return 256;
    int n = ncu[dev].load(std::memory_order_relaxed);
    if (n == 0) {
        hipDeviceProp_t prop;
        n = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
        ncu[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}

// The storage-type switch: the statements run with `T` naming the element type of `code`. A code that is neither bf16 nor f16 is fp32 storage, as the
// ladders this replaces had it; MG_WITH_DTYPE_OR is for the sites that refuse such a code and return `bad`. A macro, not a generic lambda: the three
// branches instantiate their kernels where the ladder did (the order of the kernels in the code object stays put), and a `return` in the statements
// leaves the launcher.
#define MG_WITH_DTYPE(code, T, ...)                                         \
    do {                                                                    \
        if ((code) == MG_BF16) { using T = bf16raw; __VA_ARGS__; }          \
        else if ((code) == MG_F16) { using T = f16raw; __VA_ARGS__; }       \
        else { using T = float; __VA_ARGS__; }                              \
    } while (0)
#define MG_WITH_DTYPE_OR(code, bad, T, ...)                                 \
    do {                                                                    \
        if (!MG_IS16(code) && (code) != MG_F32) return (bad);               \
        MG_WITH_DTYPE(code, T, __VA_ARGS__);                                \
    } while (0)
