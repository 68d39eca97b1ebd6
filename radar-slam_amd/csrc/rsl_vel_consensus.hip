// rsl_vel_consensus.hip — K8c: batched consensus (RANSAC) box-constrained velocity solve, fp64.  gfx950.
//
// The model and the inputs are those of k_velocity / k_velocity_robust: residual r_i = y_i - k (vx c_i + vy s_i),
// multiplicity m_i = popcount(amask_i).  The estimator's contract is the doc comment of rsl_velocity_consensus in
// include/rsl.h: hyps two-cell hypotheses drawn with Philox, each scored by the multiplicity of the cells within
// t = c scale of it, the best one refined by box-constrained LS on its inliers.  It does not start from the LS fit, so
// it finds the largest coherent population even where that is a minority of the frame.
//
// One 256-thread workgroup per frame, a lane per hypothesis: thread t owns the hypotheses t, t + 256, ... (at most
// kCvMaxPer = 16 at RSL_CONSENSUS_MAX_H), each as (vx, vy, count) in registers.  The frame's cells are staged into LDS
// in chunks of kCvChunk as (c, s, y, m) through the shared cell loader, and every lane walks the chunk reading the same
// LDS address (a broadcast: no bank conflict), so the cells are streamed from memory once for all hypotheses and there
// is no per-hypothesis reduction.  The winner is one workgroup-wide max over the 64-bit key (count + 1, hyps - 1 - h);
// an invalid hypothesis has key 0.  The loader, moments, residual and box solve of the LS fallback, the
// refinement passes and the output pass are rsl_vel_common.h's, the reductions rsl_reduce.h's; every pass, scoring included, evaluates the
// residual with the one rv_resid, so score, refinement and output see the same bits for a cell.
//
// Scoring is bound by fp64 VALU issue (mul + 2 fma + compare per cell and hypothesis), not by memory.  Measured on
// 2000 cfg2 frames of 35.5 k cells: 4.17 / 4.53 / 12.3 ms at 64 / 256 / 1024 hypotheses, against 2.39 ms
// for k_velocity_robust (Tukey, given sigma); below 256 hypotheses the spare waves idle, so 64 cost what 256 do.
#include "rsl_common.h"
#include "rsl_internal.h"
#include "rsl_philox.h"
#include "rsl_vel_common.h"
#include "../../include/rsl.h"

namespace rsl {
namespace {

constexpr int kCvThreads = 256;
constexpr int kCvWaves = kCvThreads / 64;
constexpr int kCvChunk = 1024;  // cells staged per trip of the scoring loop: 28 B each, 28 KB of LDS
constexpr int kCvMaxPer = RSL_CONSENSUS_MAX_H / kCvThreads;
typedef unsigned long long u64;
static_assert(kCvChunk % kCvThreads == 0 && kCvChunk <= kCvThreads * kVelU, "a chunk is one trip of the cell loader");
static_assert(RSL_CONSENSUS_MAX_H == 4096, "the winner's key keeps h in its low 12 bits");

// LDS carve (doubles / u64, after the optional [2G] cos / sin table)
constexpr int kCvRed = 0;                      // [kCvWaves * 7] wave partials
constexpr int kCvMom = kCvRed + kCvWaves * 7;  // [8] reduced sums
constexpr int kCvBc = kCvMom + 8;              // [2] solution broadcast
constexpr int kCvKey = kCvBc + 2;              // [kCvWaves * 2] wave partials: maximum key, count of valid hypotheses
constexpr int kCvWin = kCvKey + kCvWaves * 2;  // [2] the winner's key, the number of valid hypotheses
constexpr int kCvC = kCvWin + 2;               // [kCvChunk] cos
constexpr int kCvS = kCvC + kCvChunk;          // [kCvChunk] sin
constexpr int kCvY = kCvS + kCvChunk;          // [kCvChunk] y
constexpr int kCvM = kCvY + kCvChunk;          // [kCvChunk] int multiplicities (kCvChunk / 2 doubles)
constexpr int kCvLds = kCvM + kCvChunk / 2;

// (x * n) >> 32 for a 32-bit draw x and 0 <= n < 2^63: a uniform index below n
RSL_DEV long long cv_index(unsigned x, long long n) {
  const u64 un = (u64)n;
  return (long long)((u64)x * (un >> 32) + (((u64)x * (un & 0xffffffffull)) >> 32));
}

template <int kPer>
__global__ __launch_bounds__(kCvThreads) void k_velocity_consensus(
    const double* __restrict__ az, const int* __restrict__ gidx, const double* __restrict__ az_table, int G,
    const double* __restrict__ y, const unsigned* __restrict__ amask, const long long* __restrict__ seg, long long nmax,
    double k, double ridge, double lx, double hx, double ly, double hy, double tc, int hyps, double min_det, int refine,
    unsigned k0, unsigned k1, long long frame0, double* __restrict__ out, float* __restrict__ weight,
    double* __restrict__ resid) {
  extern __shared__ __attribute__((aligned(16))) double cv_lds[];
  const bool tab = gidx != nullptr;
  double* cs_tab = cv_lds;  // [2G] cos, sin of the grid azimuths (gidx path)
  double* wk = cv_lds + (tab ? 2 * G : 0);
  double* red = wk + kCvRed;
  double* mom = wk + kCvMom;
  double* bc = wk + kCvBc;
  u64* keyw = reinterpret_cast<u64*>(wk + kCvKey);
  u64* win = reinterpret_cast<u64*>(wk + kCvWin);
  double* lc = wk + kCvC;
  double* ls = wk + kCvS;
  double* ly_ = wk + kCvY;
  int* lm = reinterpret_cast<int*>(wk + kCvM);
  const int t = threadIdx.x;
  // vel_frame's text, open-coded: this kernel keeps wave-uniform values in VGPR lanes, and with the prologue inlined
  // from the helper the compiler places them differently throughout (the other two kernels compile as before with it)
  if (tab) {
    for (int g = t; g < G; g += kCvThreads) sincos(az_table[g], &cs_tab[G + g], &cs_tab[g]);
    __syncthreads();
  }
  const long f = blockIdx.x;
  const long long b = seg[f] < nmax ? seg[f] : nmax, e0 = seg[f + 1] < nmax ? seg[f + 1] : nmax;
  const long long e = e0 > b ? e0 : b;
  const long long nf = e - b;

  // one cell by its index, with the loader's values: the grid table's entry, or sincos of its azimuth
  auto cell = [&](long long i, double& c, double& s, double& yi, int& m) {
    if (tab) {
      const int g = gidx[i];
      c = cs_tab[g];
      s = cs_tab[G + g];
    } else {
      sincos(az[i], &s, &c);
    }
    yi = y[i];
    m = amask ? __popc(amask[i]) : 1;
  };

  // draw and solve this thread's hypotheses
  double hvx[kPer], hvy[kPer];
  bool hok[kPer];
  const u64 fr = (u64)(frame0 + f);
#pragma unroll
  for (int q = 0; q < kPer; ++q) {
    const int h = t + q * kCvThreads;
    hvx[q] = 0.0;
    hvy[q] = 0.0;
    hok[q] = false;
    if (h < hyps && nf >= 2) {
      const uint4 x = philox4x32_10(make_uint4((unsigned)h, (unsigned)fr, (unsigned)(fr >> 32), 0u), k0, k1);
      const long long i = cv_index(x.x, nf);
      long long j = cv_index(x.y, nf - 1);
      j += (j >= i);
      double ci, si, yi, cj, sj, yj;
      int mi, mj;
      cell(b + i, ci, si, yi, mi);
      cell(b + j, cj, sj, yj, mj);
      const double det = ci * sj - cj * si;
      const double vx = (yi * sj - yj * si) / (k * det), vy = (ci * yj - cj * yi) / (k * det);
      hok[q] = mi > 0 && mj > 0 && fabs(det) >= min_det && vx >= lx && vx <= hx && vy >= ly && vy <= hy;
      if (hok[q]) {
        hvx[q] = vx;
        hvy[q] = vy;
      }
    }
  }

  // score: the multiplicity within the cut-off of every hypothesis, the cells broadcast from LDS chunk by chunk
  u64 cnt[kPer];
#pragma unroll
  for (int q = 0; q < kPer; ++q) cnt[q] = 0;
  for (long long cb = b; cb < e; cb += kCvChunk) {
    const long long ce = cb + kCvChunk < e ? cb + kCvChunk : e;
    rv_cells<kCvThreads>(az, gidx, y, amask, cs_tab, G, cb, ce,
                         [&](long long i, bool ok, int m, double c, double s, double yi) {
                           if (!ok) return;
                           const int l = (int)(i - cb);
                           lc[l] = c;
                           ls[l] = s;
                           ly_[l] = yi;
                           lm[l] = m;
                         });
    __syncthreads();
    const int nc = (int)(ce - cb);
    unsigned part[kPer];  // at most kCvChunk * 32 per chunk
#pragma unroll
    for (int q = 0; q < kPer; ++q) part[q] = 0u;
    for (int l = 0; l < nc; ++l) {
      const double c = lc[l], s = ls[l], yi = ly_[l];
      const unsigned m = (unsigned)lm[l];
#pragma unroll
      for (int q = 0; q < kPer; ++q) part[q] += fabs(rv_resid(yi, k, hvx[q], hvy[q], c, s)) <= tc ? m : 0u;
    }
#pragma unroll
    for (int q = 0; q < kPer; ++q) cnt[q] += part[q];
    __syncthreads();  // the chunk is rewritten by the next trip
  }

  // the winner: the largest count, ties to the lowest h; and the number of valid hypotheses
  u64 kn[2] = {0, 0};  // key, valid count
#pragma unroll
  for (int q = 0; q < kPer; ++q)
    if (hok[q]) {
      const u64 kq = ((cnt[q] + 1) << 12) | (u64)(hyps - 1 - (t + q * kCvThreads));
      kn[0] = kq > kn[0] ? kq : kn[0];
      ++kn[1];
    }
  const u64 mine = kn[0];
  wg_partials<Red::Max, Red::Sum>(kn, keyw);  // integers: exact in any order
  if (t == 0) {
    win[0] = wg_fold<kCvWaves, 2, Red::Max>(keyw, 0, (u64)0);
    win[1] = wg_fold<kCvWaves, 2, Red::Sum>(keyw, 1, (u64)0);
  }
  __syncthreads();
  const u64 best = win[0];
  const int n_valid = (int)win[1];
  const int best_h = best ? hyps - 1 - (int)(best & 0xfffull) : -1;
  if (best) {
    if (mine == best)  // exactly one thread: h is part of the key
#pragma unroll
      for (int q = 0; q < kPer; ++q)
        if (t + q * kCvThreads == best_h) {
          bc[0] = hvx[q];
          bc[1] = hvy[q];
        }
  } else {
    // no valid hypothesis: the plain LS solve of k_velocity
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    rv_cells<kCvThreads>(az, gidx, y, amask, cs_tab, G, b, e,
                         [&](long long, bool, int m, double c, double s, double yi) {
                           vel_moments(v, (double)m, c, s, yi);
                         });
    wg_sums<kCvWaves>(v, red, mom);
    __syncthreads();  // publishes mom; red is free again (so at every fold below)
    vel_solve_bcast(mom, k, ridge, lx, hx, ly, hy, bc);
  }
  __syncthreads();
  double vx = bc[0], vy = bc[1];

  // refinement: box-constrained LS on the inliers of x
  for (int j = 0; j < refine; ++j) {
    double v[7] = {0, 0, 0, 0, 0, 0, 0};
    rv_cells<kCvThreads>(az, gidx, y, amask, cs_tab, G, b, e,
                         [&](long long, bool, int m, double c, double s, double yi) {
                           const double w = fabs(rv_resid(yi, k, vx, vy, c, s)) <= tc ? (double)m : 0.0;
                           vel_moments(v, w, c, s, yi);
                         });
    wg_sums<kCvWaves>(v, red, mom);  // its barrier also orders the reads of bc above before the write below
    __syncthreads();
    if (!(mom[0] != 0.0)) break;  // no inlier: keep x
    vel_solve_bcast(mom, k, ridge, lx, hx, ly, hy, bc);
    __syncthreads();
    vx = bc[0];
    vy = bc[1];
  }

  // output pass at the returned x
  double v[7] = {0, 0, 0, 0, 0, 0, 0};
  rv_cells<kCvThreads>(az, gidx, y, amask, cs_tab, G, b, e,
                       [&](long long i, bool ok, int m, double c, double s, double yi) {
                         if (!ok) return;
                         const double r = rv_resid(yi, k, vx, vy, c, s);
                         const bool in = fabs(r) <= tc;
                         if (weight) weight[i] = in ? 1.0f : 0.0f;
                         if (resid) resid[i] = r;
                         const double w = (double)m;
                         v[0] += w * (in ? r * r : tc * tc);
                         v[1] += in ? w * r * r : 0.0;
                         v[2] += in ? w : 0.0;
                         v[3] += w;
                       });
  wg_sums<kCvWaves>(v, red, mom);
  __syncthreads();
  if (t == 0) {
    double* o = out + f * 8;
    o[0] = vx;
    o[1] = vy;
    o[2] = mom[0] + ridge * (vx * vx + vy * vy);
    o[3] = mom[2] > 0 ? sqrt(mom[1] / mom[2]) : 0.0;
    o[4] = mom[2];
    o[5] = mom[3];
    o[6] = (double)best_h;
    o[7] = (double)n_valid;
  }
}

}  // namespace

hipError_t launch_velocity_consensus(hipStream_t st, const VelProblem& p, double c, double scale, int hyps,
                                     double min_det, int refine, unsigned long long seed, long long frame0, double* out,
                                     float* weight, double* resid) {
  if (p.F <= 0) return hipSuccess;
  const size_t lds = sizeof(double) * ((p.gidx ? 2 * (size_t)p.G : 0) + kCvLds);
  const int per = (hyps + kCvThreads - 1) / kCvThreads;
  auto go = [&](auto kern) {
    return launch(st, kern, p.F, kCvThreads, lds, p.az, p.gidx, p.az_table, p.G, p.y, p.amask, p.seg, p.n, p.k, p.ridge,
                  p.lx, p.hx, p.ly, p.hy, c * scale, hyps, min_det, refine, (unsigned)seed, (unsigned)(seed >> 32),
                  frame0, out, weight, resid);
  };
  // hypotheses per thread, in registers: the smallest instantiation that holds hyps
  if (per <= 1) return go(k_velocity_consensus<1>);
  if (per <= 4) return go(k_velocity_consensus<4>);
  return go(k_velocity_consensus<kCvMaxPer>);
}

}  // namespace rsl
