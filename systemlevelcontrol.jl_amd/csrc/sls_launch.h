// sls_launch.h — the optional event pair of the column kernels' launchers (declared in sls_internal.h; bodies in sls_kernels.hip,
// sls_wave_kernel.hip, sls_twisted4_kernel.hip, sls_tile_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

namespace sls {

// Events that the kernel's own dispatch packet completes (hipExtLaunchKernelGGL, flags 0: in order): `start` takes the
// dispatch's begin timestamp and `stop` its end, so hipEventElapsedTime over the pair is the kernel alone, and `stop` is an
// event to wait on like a recorded one — but no marker packet is queued in front of or behind the kernel.  Either may be NULL.
// A launcher given no LaunchEvents launches with hipLaunchKernelGGL; grid, block, LDS, stream and argument are the same.
struct LaunchEvents { hipEvent_t start, stop; };

}  // namespace sls
