// rsl_launch_limits.h — the range rule of rsl::launch (rsl_launch.h), free of HIP so a host test compiles it alone.
#pragma once

namespace rsl {

// A launch the device can take: gx workgroups in [1, 2^31 - 1] (gridDim.x), gy in [1, 65535] (gridDim.y), 1 to 1024
// threads each.  The counts are 64-bit so that a product that outgrew 32 bits is refused, not truncated.
inline bool launch_in_range(long long gx, long long gy, long long threads) {
  return gx >= 1 && gx <= 0x7fffffffLL && gy >= 1 && gy <= 65535 && threads >= 1 && threads <= 1024;
}

}  // namespace rsl
