// rsl_vel_common.h — what the velocity solvers share (k_velocity in rsl_vel.hip, k_velocity_robust in
// rsl_vel_robust.hip, k_velocity_consensus in rsl_vel_consensus.hip), each step said once:
//   vel_load       kVelU cells of one thread, all loads issued first
//   vel_moments    one cell into the 7 moments [n, cc, cs, ss, cy, sy, yy]
//   vel_frame      the frame prologue: the cos / sin table in LDS and the frame's clamped cell range (k_velocity and
//                  k_velocity_robust; k_velocity_consensus keeps these lines open-coded and says why)
//   qcost, box_solve, vel_solve_bcast   the quadratic cost, the 2x2 box solve, and thread 0's solve into LDS
//   rv_cells       the cell loop of a pass (grid-index or azimuth path) around a callback
//   rv_resid       the residual of a cell, with explicit fma
// The workgroup sums of the 7 moments (and k_velocity's R2 and maximum, the consensus solver's winner) are
// rsl_reduce.h's, which this header includes for the three solvers.
// The robust solver starts from k_velocity's solution, and the consensus solver falls back on it; all take it from these
// functions, in the same order of operations.  Every helper is force-inlined and holds the expression text of the
// kernels it came from: under fp-contract the compiler picks per kernel which products it fuses into an fma, so a
// helper that is rewritten (an explicit fma, other brackets) may change a kernel's last bit.
#pragma once
#include "rsl_common.h"
#include "rsl_reduce.h"

namespace rsl {

constexpr int kVelU = 8;

// kVelU cells i0 + u * stride (u < kVelU; stride = the block size) of one thread, all loads issued first (the loop is
// HBM-latency bound otherwise); cells at or past e read as weight 0, grid index 0
RSL_DEV void vel_load(long long i0, long long e, unsigned stride, const int* __restrict__ gidx,
                      const double* __restrict__ y, const unsigned* __restrict__ amask, int (&gv)[kVelU],
                      double (&yv)[kVelU], unsigned (&mv)[kVelU]) {
#pragma unroll
  for (int u = 0; u < kVelU; ++u) {
    const long long i = i0 + (long long)u * stride;
    const bool ok = i < e;
    const long long ii = ok ? i : i0;  // i0 < e: always a valid address
    gv[u] = gidx[ii];
    yv[u] = y[ii];
    mv[u] = amask ? amask[ii] : 1u;
    if (!ok) {
      gv[u] = 0;
      yv[u] = 0.0;
      mv[u] = 0u;
    }
  }
}

// One cell of weight w, direction (c, s) and phase yi into the 7 moments v = [n, cc, cs, ss, cy, sy, yy].
RSL_DEV void vel_moments(double (&v)[7], double w, double c, double s, double yi) {
  v[0] += w;
  v[1] += w * c * c;
  v[2] += w * c * s;
  v[3] += w * s * s;
  v[4] += w * c * yi;
  v[5] += w * s * yi;
  v[6] += w * yi * yi;
}

// Frame prologue of a workgroup of kThreads.  gidx path (tab, the kernel's own flag: passing the pointer instead
// changes the register allocation of the whole kernel): cs_tab[0..G) = cos, cs_tab[G..2G) = sin of the grid azimuths,
// then a barrier.  Returns the cells [b, e) of frame f, both ends clamped to nmax, the arrays' length (an overflowed
// capacity-sized list ends at its capacity).
template <int kThreads>
RSL_DEV void vel_frame(bool tab, const double* az_table, int G, const long long* seg, long long nmax, long f,
                       double* cs_tab, long long& b, long long& e) {
  if (tab) {
    for (int g = threadIdx.x; g < G; g += kThreads) sincos(az_table[g], &cs_tab[G + g], &cs_tab[g]);
    __syncthreads();
  }
  b = seg[f] < nmax ? seg[f] : nmax;
  e = seg[f + 1] < nmax ? seg[f + 1] : nmax;
}

RSL_DEV double qcost(double vx, double vy, double k, double ridge, const double* m) {
  // m: [n, cc, cs, ss, cy, sy, yy]
  const double kx = k * vx, ky = k * vy;
  return m[6] - 2.0 * (kx * m[4] + ky * m[5]) + kx * kx * m[1] + 2.0 * kx * ky * m[2] + ky * ky * m[3] +
         ridge * (vx * vx + vy * vy);
}

// The minimiser of the convex quadratic of the moments m over the box [lx, hx] x [ly, hy]: the interior
// normal-equation solution when feasible, else the best of the four edge minimisers (1-D clamp).
RSL_DEV double2 box_solve(const double* m, double k, double ridge, double lx, double hx, double ly, double hy) {
  const double H00 = k * k * m[1] + ridge, H01 = k * k * m[2], H11 = k * k * m[3] + ridge;
  const double b0 = k * m[4], b1 = k * m[5];
  const double det = H00 * H11 - H01 * H01;
  double bx = 0.0, by = 0.0;
  bool done = false;
  if (det > 1e-300) {
    const double vx = (H11 * b0 - H01 * b1) / det, vy = (H00 * b1 - H01 * b0) / det;
    if (vx >= lx && vx <= hx && vy >= ly && vy <= hy) {
      bx = vx;
      by = vy;
      done = true;
    }
  }
  if (!done) {
    double bc = INFINITY;
    for (int edge = 0; edge < 4; ++edge) {
      const int fix = edge >> 1;  // 0: vx fixed, 1: vy fixed
      const double val = (fix == 0) ? ((edge & 1) ? hx : lx) : ((edge & 1) ? hy : ly);
      double x;
      if (fix == 0) {
        x = H11 > 0 ? (b1 - H01 * val) / H11 : 0.0;
        x = fmin(fmax(x, ly), hy);
      } else {
        x = H00 > 0 ? (b0 - H01 * val) / H00 : 0.0;
        x = fmin(fmax(x, lx), hx);
      }
      const double vx = fix == 0 ? val : x, vy = fix == 0 ? x : val;
      const double cst = qcost(vx, vy, k, ridge, m);
      if (cst < bc) {
        bc = cst;
        bx = vx;
        by = vy;
      }
    }
  }
  return make_double2(bx, by);
}

// Thread 0: the box solve on the moments mom into bc[0..1].  The barrier that publishes bc is the caller's: each call
// site orders different reads with it.
RSL_DEV void vel_solve_bcast(const double* mom, double k, double ridge, double lx, double hx, double ly, double hy,
                             double* bc) {
  if (threadIdx.x == 0) {
    const double2 x = box_solve(mom, k, ridge, lx, hx, ly, hy);
    bc[0] = x.x;
    bc[1] = x.y;
  }
}

// -- the passes over a frame's cells: one workgroup of kThreads per frame ---------------------------------------------

// fn(i, ok, m, c, s, y) for the cells of [b, e) owned by this thread; gidx path: cells past e come as ok = false with
// m = 0, y = 0 (they add 0 to every sum).
template <int kThreads, class Fn>
RSL_DEV void rv_cells(const double* __restrict__ az, const int* __restrict__ gidx, const double* __restrict__ y,
                      const unsigned* __restrict__ amask, const double* cs_tab, int G, long long b, long long e,
                      Fn&& fn) {
  if (gidx) {
    const long long step = (long long)kThreads * kVelU;
    for (long long i0 = b + threadIdx.x; i0 < e; i0 += step) {
      int gv[kVelU];
      double yv[kVelU];
      unsigned mv[kVelU];
      vel_load(i0, e, kThreads, gidx, y, amask, gv, yv, mv);
#pragma unroll
      for (int u = 0; u < kVelU; ++u) {
        const long long i = i0 + (long long)u * kThreads;
        fn(i, i < e, __popc(mv[u]), cs_tab[gv[u]], cs_tab[G + gv[u]], yv[u]);
      }
    }
  } else {
    for (long long i = b + threadIdx.x; i < e; i += kThreads) {
      double s, c;
      sincos(az[i], &s, &c);
      fn(i, true, amask ? __popc(amask[i]) : 1, c, s, y[i]);
    }
  }
}

// The residual, with explicit fma: every pass (select, score, moments, output) must see the same bits for a cell.
RSL_DEV double rv_resid(double yi, double k, double vx, double vy, double c, double s) {
  return fma(-k, fma(vx, c, vy * s), yi);
}

}  // namespace rsl
