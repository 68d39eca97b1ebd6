// rsl_refine.hip — the point cloud's last stage for gfx950 (rsl_cell_refine, include/rsl.h): for every detected cell
// the sub-bin range and Doppler offsets from the five powers around it, the azimuth at the vertex of the parabola
// through the three beamforming values around the scan's argmax (over sin(theta): the beam is symmetric there, not in
// theta), and the position in physical units.
//
// One cell per thread, as k_cell_extras (rsl_doa.hip): the same plane-strided signature gather (A 8-B reads), then
// five 4-B power reads (cell, range +-1, Doppler +-1 with wrap), 3 A 8-B steering reads (rows g-1 .. g+1 of the c64
// table, contiguous, cache resident: the table is G A 8 bytes), about 12 A fp64 FMAs, and one 32-B row (two 16-B
// stores) plus one double out.  Without a power map the four neighbour powers are formed from the RDS as
// rsl_power_integrate forms them (cabs2 per antenna, added in antenna order in fp32): 4 A more strided reads, a path
// for short per-call lists.  Every decision of the offset estimators compares fp32 powers, so it does not depend on
// the lane mapping or on the rounding of the fp64 arithmetic behind it.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "../../include/rsl.h"
#include "rsl_common.h"
#include "rsl_doa_common.h"
#include "rsl_internal.h"

namespace rsl {

namespace {

constexpr int kRefineMaxA = 32;

// The antenna-summed power of one cell from the RDS, bit for bit rsl_power_integrate's: z points at antenna 0.
RSL_DEV float refine_cell_power(const float2* __restrict__ z, int A, size_t plane) {
  float acc = 0.f;
  for (int m = 0; m < A; ++m) acc += cabs2(z[(size_t)m * plane]);
  return acc;
}

RSL_DEV double clamp_half(double v) { return fmin(0.5, fmax(-0.5, v)); }

// The offset of the peak from the centre bin in [-0.5, 0.5], from the powers below, at and above it.
RSL_DEV double refine_offset(int mode, float pm, float p0, float pp) {
  if (mode == RSL_REFINE_LOG) {
    if (!(pm > 0.f && p0 > 0.f && pp > 0.f)) return 0.0;
    const double lm = log((double)pm), l0 = log((double)p0), lp = log((double)pp);
    const double den = lm - 2.0 * l0 + lp;
    if (!(den < 0.0)) return 0.0;
    return clamp_half(0.5 * (lm - lp) / den);
  }
  if (mode == RSL_REFINE_RECT || mode == RSL_REFINE_HANN) {
    if (!(p0 > 0.f) || pm == pp) return 0.0;
    const double q = (double)fmaxf(pm, pp);
    const double r = sqrt(q / (double)p0);
    const double s = pp > pm ? 1.0 : -1.0;
    const double v = mode == RSL_REFINE_RECT ? r / (1.0 + r) : fmax(0.0, (2.0 * r - 1.0) / (r + 1.0));
    return s * fmin(0.5, v);
  }
  return 0.0;
}

// origin + step * bin with both operations rounded (no fused multiply-add): a label is then the same double wherever
// it is evaluated, also where it cancels (with d0 = -fs / 2 and d_step = fs / (C - 1), bin C / 2 - 1 with a clamped
// offset of +0.5 is 0 Hz up to the rounding of the product, which a fused form would not make).
RSL_DEV double axis_label(double origin, double step, double bin) {
#pragma clang fp contract(off)
  const double t = step * bin;
  return origin + t;
}

}  // namespace

// NA > 0: antenna count fixed at compile time (registers only); NA == 0: runtime A (<= kRefineMaxA).
template <int NA>
__global__ __launch_bounds__(256) void k_cell_refine(CellList cl, const float* __restrict__ power,
                                                     const int* __restrict__ gidx, const double* __restrict__ az_table,
                                                     const float2* __restrict__ steer, int G, int range_mode,
                                                     int doppler_mode, double r0, double r_step, double d0,
                                                     double d_step, float4* __restrict__ out_points,
                                                     double* __restrict__ out_az) {
  constexpr int MA = NA > 0 ? NA : kRefineMaxA;
  const int A = NA > 0 ? NA : cl.A;
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= cl.count()) return;
  const size_t plane = cl.plane();
  const int S = cl.S, C = cl.C;
  const int f = cl.frame[c], rc = cl.rc[c];
  const int i = rc / C, j = rc - i * C;
  const int jm = j > 0 ? j - 1 : C - 1, jp = j + 1 < C ? j + 1 : 0;  // the Doppler axis wraps
  const bool inner = i > 0 && i + 1 < S;                              // the range axis truncates
  const float2* base = cl.rds + (size_t)f * cl.fstride() + (size_t)rc;
  float2 zf[MA];
#pragma unroll
  for (int m = 0; m < MA; ++m)
    if (m < A) zf[m] = base[(size_t)m * plane];

  // 1. the five powers
  float p0, prm = 0.f, prp = 0.f, pdm, pdp;
  if (power) {
    const float* prow = power + (size_t)f * plane + (size_t)i * C;
    p0 = prow[j];
    pdm = prow[jm];
    pdp = prow[jp];
    if (inner) {
      prm = prow[(ptrdiff_t)j - C];
      prp = prow[(size_t)j + C];
    }
  } else {
    p0 = 0.f;
#pragma unroll
    for (int m = 0; m < MA; ++m)
      if (m < A) p0 += cabs2(zf[m]);
    const float2* row = cl.rds + (size_t)f * cl.fstride() + (size_t)i * C;
    pdm = refine_cell_power(row + jm, A, plane);
    pdp = refine_cell_power(row + jp, A, plane);
    if (inner) {
      prm = refine_cell_power(base - C, A, plane);
      prp = refine_cell_power(base + C, A, plane);
    }
  }

  // 2. the offsets
  const double dr = inner ? refine_offset(range_mode, prm, p0, prp) : 0.0;
  const double dd = refine_offset(doppler_mode, pdm, p0, pdp);

  // 3. the azimuth: vertex of the parabola through B_k = |a_k^H z|^2, k = g-1, g, g+1, over u_k = sin(az_table[k])
  const int g = gidx[c];
  double az;
  if (g < 0 || g >= G) {
    az = __builtin_nan("");
  } else {
    az = az_table[g];
    if (g > 0 && g + 1 < G) {
      const float2* a = steer + (size_t)(g - 1) * A;
      double br[3] = {0.0, 0.0, 0.0}, bi[3] = {0.0, 0.0, 0.0};
#pragma unroll
      for (int m = 0; m < MA; ++m) {
        if (m < A) {
          const double zr = zf[m].x, zi = zf[m].y;
#pragma unroll
          for (int k = 0; k < 3; ++k) {
            const float2 s = a[(size_t)k * A + m];
            const double ar = s.x, ai = s.y;
            br[k] += ar * zr + ai * zi;  // conj(a) z
            bi[k] += ar * zi - ai * zr;
          }
        }
      }
      const double b0 = br[0] * br[0] + bi[0] * bi[0];
      const double b1 = br[1] * br[1] + bi[1] * bi[1];
      const double b2 = br[2] * br[2] + bi[2] * bi[2];
      const double u0 = sin(az_table[g - 1]), u1 = sin(az), u2 = sin(az_table[g + 1]);
      const double d01 = (b1 - b0) / (u1 - u0);
      const double d12 = (b2 - b1) / (u2 - u1);
      const double cc = (d12 - d01) / (u2 - u0);
      if (cc < 0.0 && isfinite(cc)) {
        const double lo = 0.5 * (u0 + u1), hi = 0.5 * (u1 + u2);
        const double us = fmin(hi, fmax(lo, lo - 0.5 * d01 / cc));
        az = asin(us);
      }
    }
  }

  // 4. the outputs, computed in fp64 and rounded once
  if (out_az) out_az[c] = az;
  if (out_points) {
    const double range = axis_label(r0, r_step, (double)i + dr);
    const double dop = axis_label(d0, d_step, (double)j + dd);
    const double x = range * cos(az), y = range * sin(az);
    const double db = 10.0 * log10((double)p0 + 1e-12);
    static_assert(RSL_POINT_COLS == 8 && RSL_POINT_RANGE == 0 && RSL_POINT_DOPPLER == 1 && RSL_POINT_AZ == 2 &&
                      RSL_POINT_X == 3 && RSL_POINT_Y == 4 && RSL_POINT_POWER_DB == 5 && RSL_POINT_RANGE_OFFSET == 6 &&
                      RSL_POINT_DOPPLER_OFFSET == 7, "the two 16-byte stores below write the row in this order");
    float4* row = out_points + (size_t)c * 2;
    row[0] = make_float4((float)range, (float)dop, (float)az, (float)x);
    row[1] = make_float4((float)y, (float)db, (float)dr, (float)dd);
  }
}

hipError_t launch_cell_refine(hipStream_t st, CellList cl, const float* power, const int* gidx, const double* az_table,
                              const float2* steer, int G, int range_mode, int doppler_mode, const double* axes4,
                              float* out_points, double* out_az) {
  if (cl.A > kRefineMaxA || cl.A < 2) return hipErrorInvalidValue;
  if (cl.n_host <= 0) return hipSuccess;
  const long long nb = (cl.n_host + 255) / 256;
  const double r0 = axes4[0], r_step = axes4[1], d0 = axes4[2], d_step = axes4[3];
  auto go = [&](auto na) {
    return launch(st, k_cell_refine<decltype(na)::value>, nb, 256, 0, cl, power, gidx, az_table, steer, G, range_mode,
                  doppler_mode, r0, r_step, d0, d_step, reinterpret_cast<float4*>(out_points), out_az);
  };
  const bool fixed = cl.A == 4 || cl.A == 8 || cl.A == 16;  // antenna counts with an instance of their own
  return with_int<0, 4, 8, 16>(fixed ? cl.A : 0, go);
}

}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
