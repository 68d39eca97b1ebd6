// rsl_cfar_common.h — what the CFAR family (k_detect_cfar in rsl_cfar.hip, k_detect_oscfar in rsl_oscfar.hip) shares
// on top of the detection rule of rsl_detect_common.h: the window, the strip of a workgroup, the power rows with their
// wrapped Doppler halo, and the one launcher (rows per step against the LDS, rows per strip, the argument tail).  A
// detector of the family adds its kernel, a constexpr LDS-size function and a static_assert that the function fits
// kCfarLdsMax at the limits of include/rsl.h.  The kernel files include this inside their no-packed-fp32-ops region;
// rsl_api.hip takes CfarWindow from it and instantiates none of the device code.
#pragma once
#include "rsl_common.h"
#include "rsl_detect_common.h"
#include "rsl_internal.h"

namespace rsl {

constexpr size_t kCfarLdsMax = 160 * 1024;  // LDS of one gfx950 CU

// The window of a cell under test: guard half-sizes gr x gd around it, training half-sizes tr x td around those
// (range x Doppler; Doppler wraps, range truncates at the map's edges).
struct CfarWindow {
  int gr, gd, tr, td;
  RSL_HD constexpr int hr() const { return gr + tr; }
  RSL_HD constexpr int hd() const { return gd + td; }
  RSL_HD constexpr int hh() const { return hr() > 1 ? hr() : 1; }  // rows a strip loads beyond each end: 3x3 needs one
  RSL_HD constexpr int nfull() const { return 2 * hd() + 1; }      // cells of a window row
  RSL_HD constexpr int nguard() const { return 2 * gd + 1; }       // ... of which the guard box takes these
  // n(i): the training cells that exist for range row i of S.  >= 1 (2 hr + 1 <= S), <= 33 * 33 - 1 = 1088.
  RSL_HD constexpr int cells(int i, int S) const {
    const int lo = i, hi = S - 1 - i;
    const int vh = (lo < hr() ? lo : hr()) + 1 + (hi < hr() ? hi : hr());
    const int vg = (lo < gr ? lo : gr) + 1 + (hi < gr ? hi : gr);
    return vh * nfull() - vg * nguard();
  }
};

// The strip walk: workgroup b decides the rows i0 .. i0 + Re - 1 of map fa (frame * A + antenna), strips of R range
// rows.
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
// step's first row + the wave's index; strip row u is range row ibase + u of the map `base`, [S][C] of c64 values or
// of fp32 powers: cell_power) into their
// rows of the LDS ring PW [NP][PS], PS = C + 2 hd: ring row u % NP, whose first and last hd cells repeat the other end
// of the row (Doppler wraps); a row outside the map holds `outside`.  Four rows at a time, their loads issued together
// (a row outside the map, or past u1, re-reads a row of the map and drops the value): one load in flight per wave
// leaves the kernel waiting on memory latency.
template <class T>
RSL_DEV void power_rows_halo(float* PW, int NP, int PS, const T* __restrict__ base, int ibase, int u0, int u1, int S,
                             int C, int hd, float outside) {
  for (int ub = u0; ub < u1; ub += 16) {
    const T* src[4];
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
      T z[4];
#pragma unroll
      for (int m = 0; m < 4; ++m) z[m] = src[m][j];
#pragma unroll
      for (int m = 0; m < 4; ++m) {
        float* pr = dst[m];
        if (!pr) continue;
        const float p = valid[m] ? cell_power(z[m]) : outside;
        pr[hd + j] = p;
        if (j < hd) pr[hd + C + j] = p;         // right halo: columns 0 .. hd-1
        if (j >= C - hd) pr[j - (C - hd)] = p;  // left halo: columns C-hd .. C-1
      }
    }
  }
}

// The launcher of the family.  `kernel` takes (map, S, C, W, window, extra..., thr_f, i_lo, i_hi, R, RB, mask,
// row_count, dbmap, pk_pow) and lds_bytes(C, window, RB) bytes of dynamic LDS, one workgroup of 256 per strip.  The
// F * A maps are c64 RDS maps (T = float2) or fp32 power maps (T = float).
template <class T, typename... KArgs, typename... Extra>
hipError_t launch_cfar_strips(hipStream_t st, void (*kernel)(KArgs...), size_t (*lds_bytes)(int, CfarWindow, int),
                              const T* rds, int F, int A, int S, int C, CfarWindow win, const DetectArgs& d,
                              Extra... extra) {
  if (F <= 0 || A <= 0 || S <= 0 || C <= 0) return hipSuccess;
  const int W = (C + 63) / 64;
  // rows per step: the largest of 16 / 8 / 4 whose LDS leaves room for three workgroups per CU, else 4
  int RB = 4;
  if (lds_bytes(C, win, 16) <= 48 * 1024) RB = 16;
  else if (lds_bytes(C, win, 8) <= 48 * 1024) RB = 8;
  const size_t lds = lds_bytes(C, win, RB);
  if (lds > kCfarLdsMax) return hipErrorInvalidValue;
  const int R = cfar_strip_rows(F, A, S);
  const long long nblk = (long long)F * A * ((S + R - 1) / R);
  return launch(st, kernel, nblk, 256, lds, rds, S, C, W, win, extra..., threshold_as_float(d.thr_p), d.i_lo, d.i_hi, R,
                RB, d.mask, d.row_count, d.dbmap, d.pk_pow);
}

}  // namespace rsl
