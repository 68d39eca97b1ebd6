// rsl_cloud.h — the point cloud as the device code sees it: the one statement of the rows a frame owns and of the
// points that count.  The specification is "The point cloud" in include/rsl.h, whose RSL_POINT_COLS and RSL_POINT_* are
// the row layout on both sides of the ABI.  rsl_refine.hip writes the rows; rsl_register.hip and rsl_map.hip read them
// through the two functions below.
// Loads, conversions and comparisons only: rsl_map.hip is compiled with fp contraction off and promises cells that are
// bit-equal to a numpy restatement, so nothing a contraction could touch belongs in this file.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rsl.h"

namespace rsl {

// What every consumer is handed: points f32 [*][RSL_POINT_COLS], seg i64 [F + 1], the row count n the segments are
// clamped to, and the optional weight f32 [*].  The first member of RegProblem and MapProblem, built by cloud_view
// (rsl_api.hip).
struct CloudView {
  const float* points;
  const long long* seg;
  long long n;
  int F;
  const float* weight;  // nullable = 1
};

// The rows [b, e) of frame f: both ends of the segment clamped to [0, n], empty (e = b) when it descends.
__device__ __forceinline__ void cloud_frame(const CloudView& c, long f, long long& b, long long& e) {
  const long long lo = c.seg[f], hi = c.seg[f + 1];
  b = lo < 0 ? 0 : (lo > c.n ? c.n : lo);
  e = hi < 0 ? 0 : (hi > c.n ? c.n : hi);
  if (e < b) e = b;
}

// x and y of row i, and the weight the point counts with: 1 without a weight array; 0 when x or y is not finite or the
// weight is not > 0 (a NaN weight is not).
__device__ __forceinline__ float cloud_point(const float* points, const float* weight, long long i, float& x,
                                             float& y) {
  x = points[i * RSL_POINT_COLS + RSL_POINT_X];
  y = points[i * RSL_POINT_COLS + RSL_POINT_Y];
  const float w = weight ? weight[i] : 1.f;
  return (isfinite(x) && isfinite(y) && w > 0.f) ? w : 0.f;
}

}  // namespace rsl
