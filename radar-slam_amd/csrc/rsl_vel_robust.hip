// rsl_vel_robust.hip — K8r: batched robust (Huber / Tukey IRLS) box-constrained velocity solve, fp64.  gfx950.
//
// The model, the inputs and the start x0 are those of k_velocity (rsl_vel.hip): residual r_i = y_i - k (vx c_i + vy s_i),
// multiplicity m_i = popcount(amask_i), x0 = the box-constrained ridge LS solution.  Each iteration re-weights the
// cells with the loss's weight u_i(|r_i| / (c sigma)) and solves the same 2x2 box problem with weights m_i u_i
// (iteratively re-weighted least squares; the estimator's contract is the doc comment of rsl_velocity_robust in
// include/rsl.h).  sigma is given, or 1.4826 x the lower weighted median of (float)|r_i|: a 3-pass radix select
// (11 / 11 / 10 bits) on the uint32 pattern of the non-negative float, with integer LDS histograms of the
// multiplicities, so the result is exact and independent of the lane order.
//
// One 512-thread workgroup per frame.  Every pass streams the frame's (gidx, y, amask) again (16 B per cell): a fixed
// scale costs 1 pass per iteration, the estimated scale 4; the LS start and the output pass add 2.  The workgroup
// re-reads its own lines, so all passes after the first are served by L2 / Infinity Cache.
//
// The start comes from k_velocity's own source: the frame prologue, the cell loader, the moments and the 2x2 box solve
// are the helpers of rsl_vel_common.h, the reduction is rsl_reduce.h's, in both kernels.  Same source, not guaranteed
// the same bits: under fp-contract the compiler chooses per kernel which products it fuses into an fma, so the two starts may differ
// in the last place (tests/test_gpu_vel_robust.py::test_ls_equivalence holds them within 1e-13).
#include "rsl_common.h"
#include "rsl_internal.h"
#include "rsl_vel_common.h"
#include "../../include/rsl.h"

namespace rsl {
namespace {

constexpr int kRvThreads = 512;
constexpr int kRvWaves = kRvThreads / 64;
constexpr int kRvBins = 2048;  // histogram bins of one radix-select pass (11-bit digit), 4 per thread
constexpr int kRvPer = kRvBins / kRvThreads;
typedef unsigned long long u64;

// LDS carve (doubles / u64, after the optional [2G] cos / sin table)
constexpr int kRvRed = 0;                    // [kRvWaves * 7] wave partials
constexpr int kRvMom = kRvRed + kRvWaves * 7;  // [8] reduced sums
constexpr int kRvBc = kRvMom + 8;            // [2] solution broadcast
constexpr int kRvSel = kRvBc + 2;            // [2] selected digit, remaining rank
constexpr int kRvWtot = kRvSel + 2;          // [kRvWaves] wave totals of the histogram scan
constexpr int kRvHist = kRvWtot + kRvWaves;  // [kRvBins]
constexpr int kRvLds = kRvHist + kRvBins;

// u(a), a = |r|, cut-off t = c sigma.  t = 0 (sigma = 0): 1 where the fit is exact, else 0, for both losses.
RSL_DEV double rv_weight(int loss, double a, double t) {
  if (loss == RSL_LOSS_HUBER) return a <= t ? 1.0 : t / a;
  if (a < t) {
    const double q = a / t, w = 1.0 - q * q;
    return w * w;
  }
  return (t == 0.0 && a == 0.0) ? 1.0 : 0.0;
}

RSL_DEV double rv_rho(int loss, double a, double t) {
  if (loss == RSL_LOSS_HUBER) return a <= t ? a * a : 2.0 * t * a - t * t;
  if (a < t) {
    const double q = a / t, w = 1.0 - q * q;
    return (t * t / 3.0) * (1.0 - w * w * w);
  }
  return t * t / 3.0;
}

}  // namespace

__global__ __launch_bounds__(kRvThreads) void k_velocity_robust(
    const double* __restrict__ az, const int* __restrict__ gidx, const double* __restrict__ az_table, int G,
    const double* __restrict__ y, const unsigned* __restrict__ amask, const long long* __restrict__ seg, long long nmax,
    double k, double ridge, double lx, double hx, double ly, double hy, int loss, double c_tune, double scale, int iters,
    double tol, double* __restrict__ out, float* __restrict__ weight, double* __restrict__ resid) {
  extern __shared__ __attribute__((aligned(16))) double rv_lds[];
  const bool tab = gidx != nullptr;
  double* cs_tab = rv_lds;  // [2G] cos, sin of the grid azimuths (gidx path)
  double* wk = rv_lds + (tab ? 2 * G : 0);
  double* red = wk + kRvRed;
  double* mom = wk + kRvMom;
  double* bc = wk + kRvBc;
  u64* sel = reinterpret_cast<u64*>(wk + kRvSel);
  u64* wtot = reinterpret_cast<u64*>(wk + kRvWtot);
  u64* hist = reinterpret_cast<u64*>(wk + kRvHist);
  const int t = threadIdx.x;
  const long f = blockIdx.x;
  long long b, e;
  vel_frame<kRvThreads>(tab, az_table, G, seg, nmax, f, cs_tab, b, e);

  // x0: the plain LS solve of k_velocity
  {
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    rv_cells<kRvThreads>(az, gidx, y, amask, cs_tab, G, b, e,
                         [&](long long, bool, int m, double c, double s, double yi) {
      vel_moments(v, (double)m, c, s, yi);
    });
    wg_sums<kRvWaves>(v, red, mom);
    __syncthreads();  // publishes mom; red is free again (so at every fold below)
  }
  const double W = mom[0];  // sum of the multiplicities: an exact integer
  vel_solve_bcast(mom, k, ridge, lx, hx, ly, hy, bc);
  __syncthreads();
  double vx = bc[0], vy = bc[1];

  const bool fixed = scale > 0.0;
  double sigma = fixed ? scale : 0.0;
  int it = 0;
  bool conv = !(W > 0.0);  // empty segment or all multiplicities 0
  for (int j = 1; !conv && j <= iters; ++j) {
    if (!fixed) {
      // lower weighted median of (float)|r|: the key of rank ceil(W / 2) among the multiplicities
      unsigned prefix = 0;
      u64 rank = ((u64)W + 1) / 2;
      for (int pass = 0; pass < 3; ++pass) {
        const int shift = pass == 0 ? 21 : pass == 1 ? 10 : 0, bits = pass == 2 ? 10 : 11;
#pragma unroll
        for (int q = 0; q < kRvPer; ++q) hist[t * kRvPer + q] = 0;
        if (t == 0) {
          sel[0] = 0;
          sel[1] = rank;
        }
        __syncthreads();
        rv_cells<kRvThreads>(az, gidx, y, amask, cs_tab, G, b, e,
                             [&](long long, bool ok, int m, double c, double s, double yi) {
          if (!ok || m == 0) return;
          const unsigned key = __float_as_uint((float)fabs(rv_resid(yi, k, vx, vy, c, s)));
          if (pass == 0 || (key >> (shift + bits)) == prefix)
            atomicAdd(&hist[(key >> shift) & ((1u << bits) - 1u)], (u64)m);
        });
        __syncthreads();
        u64 h[kRvPer], sum = 0;
#pragma unroll
        for (int q = 0; q < kRvPer; ++q) {
          h[q] = hist[t * kRvPer + q];
          sum += h[q];
        }
        u64 inc = sum;
        for (int off = 1; off < 64; off <<= 1) {
          const u64 up = __shfl_up(inc, off);
          if ((t & 63) >= off) inc += up;
        }
        if ((t & 63) == 63) wtot[t >> 6] = inc;
        __syncthreads();
        for (int w = 0; w < (t >> 6); ++w) inc += wtot[w];
        u64 cum = inc - sum;
        if (cum < rank && rank <= inc) {  // exactly one thread: its bins hold the rank
          int d = kRvPer - 1;
          bool found = false;
#pragma unroll
          for (int q = 0; q < kRvPer; ++q)
            if (!found) {
              if (cum + h[q] >= rank) {
                d = q;
                found = true;
              } else {
                cum += h[q];
              }
            }
          sel[0] = (u64)(t * kRvPer + d);
          sel[1] = rank - cum;
        }
        __syncthreads();
        prefix = (prefix << bits) | (unsigned)sel[0];
        rank = sel[1];
        __syncthreads();  // sel is rewritten at the top of the next pass
      }
      sigma = 1.4826 * (double)__uint_as_float(prefix);
    }
    if (sigma == 0.0) {
      conv = true;
      break;
    }
    const double tc = c_tune * sigma;
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    rv_cells<kRvThreads>(az, gidx, y, amask, cs_tab, G, b, e,
                         [&](long long, bool, int m, double c, double s, double yi) {
      const double w = m == 0 ? 0.0 : (double)m * rv_weight(loss, fabs(rv_resid(yi, k, vx, vy, c, s)), tc);
      vel_moments(v, w, c, s, yi);
    });
    // all 7 in one pass: as 7 one-value sums (21 barriers for these 2) the Huber solve at a fixed scale took 2.376
    // instead of 2.210 ms per 2000 cfg2 frames
    wg_sums<kRvWaves>(v, red, mom);
    __syncthreads();
    if (!(mom[0] != 0.0)) {  // every weight is 0: keep x
      conv = true;
      break;
    }
    vel_solve_bcast(mom, k, ridge, lx, hx, ly, hy, bc);
    __syncthreads();
    const double nx = bc[0], ny = bc[1];
    const double dx = fmax(fabs(nx - vx), fabs(ny - vy));
    vx = nx;
    vy = ny;
    it = j;
    if (tol > 0.0 && dx <= tol) conv = true;
    __syncthreads();  // bc is rewritten by the next iteration's solve
  }
  if (tol == 0.0) conv = true;

  // output pass at the returned x, with the last sigma
  const double tc = c_tune * sigma;
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  rv_cells<kRvThreads>(az, gidx, y, amask, cs_tab, G, b, e,
                       [&](long long i, bool ok, int m, double c, double s, double yi) {
    if (!ok) return;
    const double r = rv_resid(yi, k, vx, vy, c, s), a = fabs(r);
    const double u = rv_weight(loss, a, tc);
    if (weight) weight[i] = (float)u;
    if (resid) resid[i] = r;
    if (m == 0) return;
    const double w = (double)m;
    v[0] += w * rv_rho(loss, a, tc);
    v[1] += w * u * r * r;
    v[2] += w * u;
    if (loss == RSL_LOSS_HUBER ? a <= tc : (a < tc || (tc == 0.0 && a == 0.0))) v[3] += w;
  });
  wg_sums<kRvWaves>(v, red, mom);
  __syncthreads();
  if (t == 0) {
    double* o = out + f * 8;
    o[0] = vx;
    o[1] = vy;
    o[2] = mom[0] + ridge * (vx * vx + vy * vy);
    o[3] = mom[2] > 0 ? sqrt(mom[1] / mom[2]) : 0.0;
    o[4] = mom[3];
    o[5] = W;
    o[6] = sigma;
    o[7] = conv ? (double)it : -(double)it;
  }
}

hipError_t launch_velocity_robust(hipStream_t st, const VelProblem& p, int loss, double c, double scale, int iters,
                                  double tol, double* out, float* weight, double* resid) {
  if (p.F <= 0) return hipSuccess;
  const size_t lds = sizeof(double) * ((p.gidx ? 2 * (size_t)p.G : 0) + kRvLds);
  return launch(st, k_velocity_robust, p.F, kRvThreads, lds, p.az, p.gidx, p.az_table, p.G, p.y, p.amask, p.seg, p.n,
                p.k, p.ridge, p.lx, p.hx, p.ly, p.hy, loss, c, scale, iters, tol, out, weight, resid);
}

}  // namespace rsl
