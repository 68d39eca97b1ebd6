// rsl_detect_common.h — the detection rule that k_detect (rsl_detect.hip), k_detect_cfar (rsl_cfar.hip),
// k_detect_oscfar (rsl_oscfar.hip) and the fused Doppler + detection tile body dd_tile_compute share: the 3x3 'reflect'
// local-maximum test over a power tile in LDS and the output stage of one 64-cell word of a range row.
// dd_tile_compute_reg keeps its own register form of the body (column maxima in registers, neighbours by DPP,
// tile-compact peak powers): it shares the rule, not the code.  What only the two CFAR kernels share is in
// rsl_cfar_common.h.
//
// The rule (dechirp.py:215-278 on fp32 power p; log10 is monotone): cell (i, j) is a peak iff p >= every existing 3x3
// neighbour, i_lo <= i <= i_hi and p > thr_f, where thr_f = threshold_as_float(thr_p) is the largest float <= the fp64
// threshold, so that p > thr_f <=> (double)p > thr_p for every float p.
#pragma once
#include "rsl_common.h"

namespace rsl {

// The fp32 power p of a map element: |z|^2 of a c64 RDS value, or the value itself where the map already holds powers
// (rsl_detect_power: the antenna-summed map of rsl_power_integrate).  The only place a detector's element type shows.
RSL_DEV float cell_power(float2 z) { return cabs2(z); }
RSL_DEV float cell_power(float p) { return p; }

// The largest of the 3x3 window around column j of row `mid` (the cell itself included), rows of C powers in LDS.
// 'reflect' edges: a neighbour outside the map repeats a cell of the window.  So the row above (has_up false) or below
// (has_dn false) is read as `mid` again, which keeps the row loads unconditional, and the column left of 0 or right of
// C - 1 is left out (constant offsets from the three row addresses).  The cell is a local maximum iff its power >= the
// result.
RSL_DEV float window_max3(const float* up, const float* mid, const float* dn, int j, int C, bool has_up, bool has_dn) {
  const float* u = has_up ? up : mid;
  const float* d = has_dn ? dn : mid;
  float m = fmaxf(fmaxf(u[j], mid[j]), d[j]);
  if (j > 0) m = fmaxf(m, fmaxf(fmaxf(u[j - 1], mid[j - 1]), d[j - 1]));
  if (j + 1 < C) m = fmaxf(m, fmaxf(fmaxf(u[j + 1], mid[j + 1]), d[j + 1]));
  return m;
}

// Output stage of word w of row `row` = (frame * A + antenna) * S + i, called by a whole wave: lane l holds cell
// j = 64 w + l (in: j < C), its power p and its decision pk (false where !in).  Stores the dB map value, the mask word
// (the wave's ballot) and the peak's power at its rank within the row (row-compact: slot cnt + peaks of the lower
// lanes), and adds the word's peaks to the row's running count cnt.
RSL_DEV void detect_store_word(bool pk, float p, bool in, size_t row, int w, int W, int C,
                               unsigned long long* __restrict__ mask, float* __restrict__ dbmap,
                               float* __restrict__ pk_pow, int& cnt) {
  const int lane = threadIdx.x & 63;
  if (dbmap && in) dbmap[row * C + w * 64 + lane] = 10.f * log10f(p + 1e-12f);
  const unsigned long long b = __ballot(pk);
  if (lane == 0) mask[row * W + w] = b;
  if (pk_pow && pk) pk_pow[row * C + cnt + lanes_below(b)] = p;
  cnt += __popcll(b);
}

// ... and of the row, after its last word.
RSL_DEV void detect_store_count(size_t row, int cnt, int* __restrict__ row_count) {
  if ((threadIdx.x & 63) == 0) row_count[row] = cnt;
}

}  // namespace rsl
