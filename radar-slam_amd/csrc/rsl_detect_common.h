// rsl_detect_common.h — the detection rule that k_detect (rsl_detect.hip), k_detect_cfar (rsl_cfar.hip),
// k_detect_oscfar (rsl_oscfar.hip) and the fused Doppler + detection tile body dd_tile_compute share: the 3x3 'reflect'
// local-maximum test over a power tile in LDS and the output stage of one 64-cell word of a range row.
// dd_tile_compute_reg keeps its own register form of the body (column maxima in registers, neighbours by DPP,
// tile-compact peak powers): it shares the rule, not the code.  The two CFAR kernels also share their strip walk: the
// strip of a workgroup, the power rows with their wrapped Doppler halo, and the launcher's rows per strip.
//
// The rule (dechirp.py:215-278 on fp32 power p; log10 is monotone): cell (i, j) is a peak iff p >= every existing 3x3
// neighbour, i_lo <= i <= i_hi and p > thr_f, where thr_f = threshold_as_float(thr_p) is the largest float <= the fp64
// threshold, so that p > thr_f <=> (double)p > thr_p for every float p.
#pragma once
#include "rsl_common.h"

namespace rsl {

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

// The strip walk of the CFAR kernels: workgroup b decides the rows i0 .. i0 + Re - 1 of map fa (frame * A + antenna),
// strips of R range rows.
struct CfarStrip {
  size_t fa;
  int i0, Re;
};
RSL_DEV CfarStrip cfar_strip(int S, int R) {
  const int nstrip = (S + R - 1) / R;
  const int i0 = (int)(blockIdx.x % nstrip) * R;
  return {blockIdx.x / nstrip, i0, min(R, S - i0)};
}
// Rows per strip: 128 (halo re-read 1.16x at hr = 10); 32 when that leaves the device short of workgroups.
inline int cfar_strip_rows(int F, int A, int S) { return (long long)F * A * ((S + 127) / 128) < 1024 ? 32 : 128; }

// One wave's share of a step's rows: the fp32 powers of the strip rows u = u0, u0 + 4, u0 + 8, ... < u1 (u0 = the
// step's first row + the wave's index; strip row u is range row ibase + u of the map `base`, c64 [S][C]) into their
// rows of the LDS ring PW [NP][PS], PS = C + 2 hd: ring row u % NP, whose first and last hd cells repeat the other end
// of the row (Doppler wraps); a row outside the map holds `outside`.  Four rows at a time, their loads issued together
// (a row outside the map, or past u1, re-reads a row of the map and drops the value): one load in flight per wave
// leaves the kernel waiting on memory latency.
RSL_DEV void power_rows_halo(float* PW, int NP, int PS, const float2* __restrict__ base, int ibase, int u0, int u1,
                             int S, int C, int hd, float outside) {
  for (int ub = u0; ub < u1; ub += 16) {
    const float2* src[4];
    float* dst[4];
    bool valid[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
      const int u = ub + 4 * m, i = ibase + u;
      valid[m] = i >= 0 && i < S;
      src[m] = base + (size_t)min(max(i, 0), S - 1) * C;
      dst[m] = u < u1 ? PW + (size_t)(u % NP) * PS : nullptr;
    }
    for (int j = threadIdx.x & 63; j < C; j += 64) {
      float2 z[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) z[m] = src[m][j];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        float* pr = dst[m];
        if (!pr) continue;
        const float p = valid[m] ? cabs2(z[m]) : outside;
        pr[hd + j] = p;
        if (j < hd) pr[hd + C + j] = p;         // right halo: columns 0 .. hd-1
        if (j >= C - hd) pr[j - (C - hd)] = p;  // left halo: columns C-hd .. C-1
      }
    }
  }
}

}  // namespace rsl
