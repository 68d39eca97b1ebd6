// rsl_vel.hip — K8: batched box-constrained (ridge) least-squares velocity solve, fp64.  gfx950.
//
// Replaces VelocitySolver.two_step_optimization (reference src/velocity_solver/velocity_solver.py:178-307),
// which runs differential_evolution (seed 42) over cost = sum (y - 4 pi dt / lambda * (v + w x p).d)^2
// (velocity_solver.py:65-176).  With elevation 0 and p = r d (velocity_solver.py:334-339), (w x p).d = 0 and
// d_z = 0: only (v_x, v_y) enter, linearly.  The cost is a convex quadratic over the box
// [-50,50]^2, so its exact minimiser is the interior normal-equation solution when feasible, else the
// best of the four edge minimisers (1-D clamp).  ``ridge`` adds ridge*(vx^2+vy^2)
// (velocity_solver_improved.py:261 without the wrap).  Items carry a multiplicity (popcount of the
// antenna mask of a deduplicated cell) so duplicate per-antenna detections count as in the reference.
// The cell loader, the moments, the frame prologue and the 2x2 box solve are rsl_vel_common.h's, the workgroup
// reductions rsl_reduce.h's.
#include "rsl_common.h"
#include "rsl_internal.h"
#include "rsl_vel_common.h"

namespace rsl {

constexpr int kVelThreads = 512;  // k_velocity's only launch shape
constexpr int kVelWaves = kVelThreads / 64;

// Order-preserving key of a finite or infinite double (NaN never enters): min / max of keys = min / max of values.
RSL_DEV unsigned long long okey(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
RSL_DEV double unkey(unsigned long long k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// One workgroup per frame.  gidx path (the chain): one pass over the cells.  Besides the 7 moments it keeps, per grid
// index g, the smallest and largest phase of the cells with weight > 0 (LDS min / max on order-preserving keys:
// exact and order-independent).  All cells of index g share the prediction p_g = k (vx c_g + vy s_g), so the
// residual y - p_g of largest magnitude is that of the group's smallest or largest y: max |residual| comes from 2G
// values instead of a second pass over the cells (bit-identical: same p_g, same subtraction).  The residual sum
// of squares is the quadratic form of the moments; it is used when its terms do not cancel (R2 >= 1e-6 of their
// magnitude sum, i.e. < 1e-9 relative rounding), else (a near-perfect fit) R2 is summed per cell in a second pass,
// as it is for the az path and whenever per-cell residuals / predictions are requested.
__global__ __launch_bounds__(kVelThreads) void k_velocity(
    const double* __restrict__ az, const int* __restrict__ gidx, const double* __restrict__ az_table, int G,
    const double* __restrict__ y, const unsigned* __restrict__ amask, const long long* __restrict__ seg, long long nmax,
    double k, double ridge, double lx, double hx, double ly, double hy, double* __restrict__ out,
    double* __restrict__ resid, double* __restrict__ pred) {
  __shared__ double red[kVelWaves * 7];  // wave partials of the moments, then of R2 and the maximum
  __shared__ double mom[7];
  __shared__ double sol[3];
  extern __shared__ double cs_tab[];  // [2G] cos, sin of the grid azimuths, then [2G] min / max phase keys (gidx path)
  const bool tab = gidx != nullptr;  // with it, per-group extremes: 32 G B of LDS (rsl_velocity admits G <= 2048)
  unsigned long long* ymn = reinterpret_cast<unsigned long long*>(cs_tab + 2 * G);
  unsigned long long* ymx = ymn + G;
  for (int g = threadIdx.x; tab && g < G; g += kVelThreads) {
    ymn[g] = ~0ull;
    ymx[g] = 0ull;  // no key is 0 (that would be a NaN's bits): 0 marks an empty group
  }
  const long f = blockIdx.x;
  long long b, e;
  vel_frame<kVelThreads>(tab, az_table, G, seg, nmax, f, cs_tab, b, e);  // its barrier publishes the keys too
  // the first pass is not an rv_cells callback: the extremes need the grid index and the raw mask
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  if (tab) {
    for (long long i0 = b + threadIdx.x; i0 < e; i0 += (long long)kVelThreads * kVelU) {
      int gv[kVelU];
      double yv[kVelU];
      unsigned mv[kVelU];
      vel_load(i0, e, kVelThreads, gidx, y, amask, gv, yv, mv);
#pragma unroll
      for (int u = 0; u < kVelU; ++u) {
        vel_moments(v, (double)__popc(mv[u]), cs_tab[gv[u]], cs_tab[G + gv[u]], yv[u]);
        if (mv[u] != 0u && yv[u] == yv[u]) {  // weight > 0, not NaN (fmax ignores a NaN residual)
          const unsigned long long kk = okey(yv[u]);
          atomicMin(&ymn[gv[u]], kk);
          atomicMax(&ymx[gv[u]], kk);
        }
      }
    }
  } else {
    for (long long i = b + threadIdx.x; i < e; i += kVelThreads) {
      double s, c;
      sincos(az[i], &s, &c);
      vel_moments(v, amask ? (double)__popc(amask[i]) : 1.0, c, s, y[i]);
    }
  }
  wg_sums<kVelWaves>(v, red, mom);
  __syncthreads();  // publishes mom; red is free again
  if (threadIdx.x == 0) {
    // the moments in registers, read once for the solve and the residual form below: which product the compiler fuses
    // into each fma of that form (the last bit of the cost) follows the order of these reads
    double m[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) m[q] = mom[q];
    const double2 bv = box_solve(m, k, ridge, lx, hx, ly, hy);
    const double bx = bv.x, by = bv.y;
    sol[0] = bx;
    sol[1] = by;
    // residual sum of squares from the moments, kept when its terms do not cancel (gidx path only)
    const double kx = k * bx, ky = k * by;
    const double q = m[6] - 2.0 * (kx * m[4] + ky * m[5]) + kx * kx * m[1] + 2.0 * kx * ky * m[2] + ky * ky * m[3];
    const double mag = m[6] + 2.0 * (fabs(kx * m[4]) + fabs(ky * m[5])) + kx * kx * m[1] + 2.0 * fabs(kx * ky * m[2]) +
                       ky * ky * m[3];
    sol[2] = (tab && q >= 1e-6 * mag) ? q : -1.0;
  }
  __syncthreads();
  const double vx = sol[0], vy = sol[1], r2m = sol[2];
  double r2 = 0.0, rmax = 0.0;
  // The second pass keeps its own loops although it has the shape of an rv_cells callback: as one, the compiler fuses
  // vx * c + vy * s the other way round on the gidx path (fma(vy, s, vx c) for fma(vx, c, vy s)), and the residuals
  // and predictions change in the last bit.
  auto acc2 = [&](long long i, double w, double c, double s, double yi) {
    const double pr = k * (vx * c + vy * s);
    const double r = yi - pr;
    r2 += w * r * r;
    if (w > 0) rmax = fmax(rmax, fabs(r));
    if (resid) resid[i] = r;
    if (pred) pred[i] = pr;
  };
  if (tab) {
    if (r2m < 0.0 || resid || pred) {
      for (long long i0 = b + threadIdx.x; i0 < e; i0 += (long long)kVelThreads * kVelU) {
        int gv[kVelU];
        double yv[kVelU];
        unsigned mv[kVelU];
        vel_load(i0, e, kVelThreads, gidx, y, amask, gv, yv, mv);
#pragma unroll
        for (int u = 0; u < kVelU; ++u)
          if (i0 + (long long)u * kVelThreads < e)
            acc2(i0 + (long long)u * kVelThreads, (double)__popc(mv[u]), cs_tab[gv[u]], cs_tab[G + gv[u]], yv[u]);
      }
    }
  } else {
    for (long long i = b + threadIdx.x; i < e; i += kVelThreads) {
      double s, c;
      sincos(az[i], &s, &c);
      acc2(i, amask ? (double)__popc(amask[i]) : 1.0, c, s, y[i]);
    }
  }
  if (tab) {
    rmax = 0.0;  // from the per-group extremes (same values as the per-cell maximum)
    for (int g = threadIdx.x; g < G; g += kVelThreads) {
      const unsigned long long hi = ymx[g];
      if (hi == 0ull) continue;
      const double pr = k * (vx * cs_tab[g] + vy * cs_tab[G + g]);
      rmax = fmax(rmax, fmax(fabs(unkey(ymn[g]) - pr), fabs(unkey(hi) - pr)));
    }
  }
  // Two one-value reductions back to back on the same red.  The first may write it because the barrier behind the
  // moments' fold above came after that fold's reads; the second because of the barrier between the two, which comes
  // after thread 0 has folded R2s.  Nothing writes red after the second.
  const double R2s = wg_one<kVelWaves, Red::Sum>(r2, red, 0.0);
  const double R2 = r2m >= 0.0 ? r2m : R2s;
  __syncthreads();
  const double RM = wg_one<kVelWaves, Red::Max>(rmax, red, -1.0);
  if (threadIdx.x == 0) {
    double* o = out + f * 8;
    o[0] = vx;
    o[1] = vy;
    o[2] = R2 + ridge * (vx * vx + vy * vy);               // cost at the optimum
    o[3] = mom[0] > 0 ? sqrt(R2 / mom[0]) : 0.0;           // rmse (velocity_solver.py:283)
    o[4] = RM;                                             // max |residual| (velocity_solver.py:284)
    o[5] = mom[0];                                         // number of targets (with multiplicity)
    o[6] = mom[1] * mom[3] - mom[2] * mom[2];              // normal-matrix determinant / k^4
    o[7] = 0.0;
  }
}

hipError_t launch_velocity(hipStream_t st, const VelProblem& p, double* out, double* resid, double* pred) {
  if (p.F <= 0) return hipSuccess;
  const size_t lds = p.gidx ? sizeof(double) * 4 * (size_t)p.G : 0;
  return launch(st, k_velocity, p.F, kVelThreads, lds, p.az, p.gidx, p.az_table, p.G, p.y, p.amask, p.seg, p.n, p.k,
                p.ridge, p.lx, p.hx, p.ly, p.hy, out, resid, pred);
}

}  // namespace rsl
