// rsl_launch.h — the one checked kernel launch and the per-device launch facts of every launcher (host side only).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <tuple>

#include "rsl_launch_limits.h"

namespace rsl {

struct GridXY {  // the few 2-D grids (rsl_eval.hip, rsl_nci.hip)
  long long x, y;
};

// Launches `kernel` on grid x threads with `lds` bytes of dynamic LDS and returns the launch's error;
// hipErrorInvalidValue, and no launch, for a grid outside launch_in_range.  More than 64 KiB of dynamic LDS is opted
// into here.  `args` convert to the kernel's parameter types, so a wrong argument list does not compile.
template <typename... KArgs, typename... Args>
hipError_t launch(hipStream_t st, void (*kernel)(KArgs...), GridXY grid, long long threads, size_t lds, Args&&... args) {
  if (!launch_in_range(grid.x, grid.y, threads)) return hipErrorInvalidValue;
  if (lds > 64 * 1024) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid.x, (unsigned)grid.y), dim3((unsigned)threads), lds, st,
                     static_cast<KArgs>(args)...);
  return hipGetLastError();
}
template <typename... KArgs, typename... Args>
hipError_t launch(hipStream_t st, void (*kernel)(KArgs...), long long gx, long long threads, size_t lds,
                  Args&&... args) {
  return launch(st, kernel, GridXY{gx, 1}, threads, lds, static_cast<Args&&>(args)...);
}

// Facts of the current device, queried once each and kept behind one mutex (handles launch from several threads).
struct DeviceFacts {
  std::mutex mu;
  std::map<int, int> cus;                                          // device -> CU count
  std::map<std::tuple<int, const void*, int, size_t>, int> occ;  // (device, kernel, threads, lds) -> workgroups per CU
};
inline DeviceFacts& device_facts() {
  static DeviceFacts f;
  return f;
}

// CUs of the current device; 256 (an MI355X), uncached, where the runtime does not say.
inline int cu_count() {
  int dev = 0, ncu = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 256;
  DeviceFacts& f = device_facts();
  std::lock_guard<std::mutex> lock(f.mu);
  if (auto it = f.cus.find(dev); it != f.cus.end()) return it->second;
  if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || ncu < 1) return 256;
  return f.cus[dev] = ncu;
}

// Workgroups of `kernel` (threads, lds bytes of dynamic LDS) that one CU of the current device holds; 1, uncached,
// where the runtime does not say.
template <typename... KArgs>
int occupancy(void (*kernel)(KArgs...), int threads, size_t lds) {
  int dev = 0, nb = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 1;
  const auto key = std::make_tuple(dev, reinterpret_cast<const void*>(kernel), threads, lds);
  DeviceFacts& f = device_facts();
  std::lock_guard<std::mutex> lock(f.mu);
  if (auto it = f.occ.find(key); it != f.occ.end()) return it->second;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, threads, lds) != hipSuccess || nb < 1) return 1;
  return f.occ[key] = nb;
}

// The workgroups of `kernel` resident on the current device at once: the grid of a persistent or grid-striding kernel,
// before the caller's own clamps.
template <typename... KArgs>
long long resident_blocks(void (*kernel)(KArgs...), int threads, size_t lds) {
  return (long long)occupancy(kernel, threads, lds) * cu_count();
}

}  // namespace rsl
