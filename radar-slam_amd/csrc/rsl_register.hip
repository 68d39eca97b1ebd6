// rsl_register.hip — scan registration for gfx950 (rsl_scan_register, include/rsl.h): the yaw increment and the
// displacement between the point clouds of consecutive frames, by a yaw search and an MM / IRLS descent on the biweight
// kernel correlation of the two clouds.
//
// One workgroup of 256 threads per frame pair; the whole coarse and fine loop runs inside the kernel, so a call with
// F = 2 uses one CU.  A wave takes current points in turn (the point, its transform and its reference window are
// uniform over the wave); its lanes stride over the contiguous reference slice of that window.  A pair reads the
// reference's x and y from its 32-byte point row and its weight: there is no packed copy, the function owns no scratch.
// Coarse scores are held 16 candidates at a time in registers (the pairs are walked once per 16 candidates; a pair
// farther from the start pose than h_coarse plus the arc the search can move the point is skipped for all of them).
// Every sum is fp64, per thread in a fixed order and then through rsl_reduce.h (8 values per pass): no atomics, the
// rows are run-to-run bit-identical.  The culling (binary search on rc for the range rows that can hold a partner)
// only removes pairs outside the kernel's support: the result is defined by the support alone.  The rows' first points
// are looked up once per workgroup into an LDS table (up to 4096 range rows), so a window costs two LDS reads.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "../../include/rsl.h"
#include "rsl_common.h"
#include "rsl_internal.h"
#include "rsl_reduce.h"

namespace rsl {

namespace {

constexpr int kRegThreads = 256;
constexpr int kRegWaves = kRegThreads / 64;
constexpr int kRegChunk = 16;                      // coarse candidates held in registers per walk over the pairs
constexpr int kRegCand = 2 * RSL_REG_MAX_K + 1;    // the most candidates
constexpr int kRegU = 4;                           // reference points a lane loads before it computes
constexpr int kRegRows = 4096;                     // range rows the LDS row table holds (16 KiB)
constexpr int kRegScore = (kRegCand + kRegChunk - 1) / kRegChunk * kRegChunk;

struct RegCloud {
  const float* pts;  // rows of rsl_cloud.h
  const float* w;    // nullable
  const int* rc;     // nullable
  long long b, e;    // the cloud's rows, inside the arrays
};

// Point i of a cloud: cloud_point's coordinates and weight promoted to fp64.
RSL_DEV double reg_point(const RegCloud& c, long long i, double& x, double& y) {
  float xf, yf;
  const float wf = cloud_point(c.pts, c.w, i, xf, yf);
  x = (double)xf;
  y = (double)yf;
  return (double)wf;
}

// First index of [b, e) whose rc is >= key (rc ascends inside a frame); e if there is none.
RSL_DEV long long reg_lower(const int* __restrict__ rc, long long b, long long e, long long key) {
  while (b < e) {
    const long long m = b + ((e - b) >> 1);
    if ((long long)rc[m] < key) b = m + 1; else e = m;
  }
  return b;
}

// The reference rows that can hold a point with a range inside [lo, hi]: the range rows whose label interval
// r0 + r_step (i -+ 0.5) meets it, one more row on each side.  Without rc: the whole cloud.  rows (LDS, nullable):
// rows[i] = the offset from q.b of the first point of range row i or above, i = 0 .. nrows (rows[nrows] = all);
// without it the two ends are found by binary search, 2 x log2(n) dependent loads per call.
RSL_DEV void reg_window(const RegCloud& q, int C, double r0, double inv_step, double lo, double hi, const int* rows,
                        int nrows, long long& jb, long long& je) {
  jb = q.b;
  je = q.e;
  if (!q.rc) return;
  const double big = 2147483648.0;
  const double a = fmax(-2.0, fmin(ceil((lo - r0) * inv_step - 0.5) - 1.0, big));
  const double b = fmax(-2.0, fmin(floor((hi - r0) * inv_step + 0.5) + 1.0, big));
  const long long ia = (long long)a, ib = (long long)b + 1;
  if (rows) {
    jb = q.b + (ia <= 0 ? 0 : rows[ia < nrows ? ia : nrows]);
    je = q.b + rows[ib <= 0 ? 0 : (ib < nrows ? ib : nrows)];
    if (je < jb) je = jb;
    return;
  }
  jb = reg_lower(q.rc, q.b, q.e, ia * C);
  je = reg_lower(q.rc, jb, q.e, ib * C);
}

// kRegU reference points j0 + 64 u (u < kRegU) of one lane, all loads issued first (the walk is load-latency bound
// otherwise); points at or past e come with weight 0.  The lane meets its points in the same order as one at a time.
RSL_DEV void reg_load(const RegCloud& q, long long j0, long long e, double (&x)[kRegU], double (&y)[kRegU],
                      double (&u)[kRegU]) {
#pragma unroll
  for (int k = 0; k < kRegU; ++k) {
    const long long j = j0 + 64ll * k;
    u[k] = reg_point(q, j < e ? j : j0, x[k], y[k]);  // j0 < e: always a valid row
    if (j >= e) u[k] = 0.0;
  }
}

}  // namespace

__global__ __launch_bounds__(kRegThreads) void k_scan_register(RegProblem p, double* __restrict__ out,
                                                               double* __restrict__ omega) {
  __shared__ double red[kRegWaves * 8];
  __shared__ double ct[kRegCand], sn[kRegCand], score[kRegScore];
  __shared__ double bc[8];
  __shared__ int rowtab[kRegRows + 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long f = blockIdx.x;
  double* o = out + f * 8;

  if (t == 0 && omega && f == 0) {  // the last row has no successor in this call
    double* w = omega + (size_t)(p.cloud.F - 1) * 3;
    w[0] = w[1] = w[2] = 0.0;
  }
  const bool has_prev = p.prev_points != nullptr;
  if (f == 0 && !has_prev) {  // uniform over the workgroup: nobody reaches a barrier
    if (t == 0) {
      for (int q = 0; q < 7; ++q) o[q] = 0.0;
      o[7] = 2.0;
    }
    return;
  }

  RegCloud P{p.cloud.points, p.cloud.weight, p.rc, 0, 0};
  cloud_frame(p.cloud, f, P.b, P.e);
  RegCloud Q;
  if (f == 0) {
    long long m = p.prev_n;
    if (p.prev_n_dev && *p.prev_n_dev < m) m = *p.prev_n_dev;
    Q = RegCloud{p.prev_points, p.prev_weight, p.prev_rc, 0, m < 0 ? 0 : m};
  } else {
    Q = P;  // the same arrays, the rows of the frame before
    cloud_frame(p.cloud, f - 1, Q.b, Q.e);
  }

  // the reference's range rows -> first point, once per workgroup (every thread computes the same bounds)
  const int* rows = nullptr;
  int nrows = 0;
  if (Q.rc && Q.e > Q.b && Q.e - Q.b < 0x7fffffffll) {
    const long long last = Q.rc[Q.e - 1];  // rc ascends: the largest
    if (last >= 0 && last / p.C + 1 <= kRegRows) {
      nrows = (int)(last / p.C + 1);
      rows = rowtab;
    }
  }
  if (rows) {
    for (int r = t; r <= nrows; r += kRegThreads)
      rowtab[r] = (int)(reg_lower(Q.rc, Q.b, Q.e, (long long)r * p.C) - Q.b);
    __syncthreads();
  }

  double th = 0.0, tx = 0.0, ty = 0.0;
  if (p.init) {
    const double a = p.init[f * 3], b = p.init[f * 3 + 1], c = p.init[f * 3 + 2];
    th = isfinite(a) ? a : 0.0;
    tx = isfinite(b) ? b : 0.0;
    ty = isfinite(c) ? c : 0.0;
  }
  const double inv_step = p.inv_step;

  // ---- coarse stage: the yaw candidates at the start translation
  const int ncand = 2 * p.K + 1;
  const double th0 = th;
  for (int k = t; k < ncand; k += kRegThreads) sincos(th0 + (double)(k - p.K) * p.dtheta, &sn[k], &ct[k]);
  __syncthreads();
  {
    const double hc2 = p.h_coarse * p.h_coarse, inv_hc2 = 1.0 / hc2;
    const double tnorm = sqrt(tx * tx + ty * ty);
    const double c0 = ct[p.K], s0 = sn[p.K];
    for (int k0 = 0; k0 < ncand; k0 += kRegChunk) {
      double acc[kRegChunk];
#pragma unroll
      for (int c = 0; c < kRegChunk; ++c) acc[c] = 0.0;
      for (long long i = P.b + wave; i < P.e; i += kRegWaves) {
        double px, py;
        const double w = reg_point(P, i, px, py);
        if (!(w > 0.0)) continue;
        const double pn = sqrt(px * px + py * py);
        long long jb, je;
        reg_window(Q, p.C, p.r0, inv_step, pn - tnorm - p.h_coarse, pn + tnorm + p.h_coarse, rows, nrows, jb, je);
        // no candidate moves the point farther from its place at the start yaw than the arc K dtheta |p|
        const double reach = (p.h_coarse + pn * (double)p.K * p.dtheta) * (1.0 + 1e-9);
        const double reach2 = reach * reach;
        const double cx = c0 * px - s0 * py + tx, cy = s0 * px + c0 * py + ty;
        for (long long j0 = jb + lane; j0 < je; j0 += 64 * kRegU) {
          double qxs[kRegU], qys[kRegU], us[kRegU];
          reg_load(Q, j0, je, qxs, qys, us);
#pragma unroll
          for (int v = 0; v < kRegU; ++v) {
            const double qx = qxs[v], qy = qys[v], u = us[v];
            if (!(u > 0.0)) continue;
            const double ex = cx - qx, ey = cy - qy;
            if (!(ex * ex + ey * ey < reach2)) continue;
            const double wu = w * u;
#pragma unroll
            for (int c = 0; c < kRegChunk; ++c) {
              const int k = k0 + c;
              if (k < ncand) {
                const double dx = ct[k] * px - sn[k] * py + tx - qx;
                const double dy = sn[k] * px + ct[k] * py + ty - qy;
                const double a = fmax(0.0, 1.0 - (dx * dx + dy * dy) * inv_hc2);
                acc[c] += wu * (a * a * a);
              }
            }
          }
        }
      }
#pragma unroll
      for (int half = 0; half < kRegChunk / 8; ++half) {
        double v[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] = acc[half * 8 + q];
        wg_partials<Red::Sum>(v, red);
        if (t < 8) score[k0 + half * 8 + t] = wg_fold<kRegWaves, 8, Red::Sum>(red, t, 0.0);
        __syncthreads();  // red is free again; score is published
      }
    }
  }
  if (t == 0) {
    int best = 0;
    double sb = score[0], tot = 0.0;
    for (int k = 0; k < ncand; ++k) {
      tot += score[k];
      if (score[k] > sb) {
        sb = score[k];
        best = k;
      }
    }
    bc[0] = (double)best;
    bc[1] = sb;
    bc[2] = tot;
  }
  __syncthreads();
  const double s_best = bc[1], s_tot = bc[2];
  const double ratio = s_tot > 0.0 ? s_best / s_tot : 0.0;
  if (!(s_best > 0.0)) {  // no pair inside the coarse radius at any candidate: the start values stand
    if (t == 0) {
      o[0] = th0;
      o[1] = tx;
      o[2] = ty;
      o[3] = o[4] = o[5] = o[6] = 0.0;
      o[7] = 1.0;
      if (omega && f > 0) {
        double* w = omega + (size_t)(f - 1) * 3;
        w[0] = w[1] = 0.0;
        w[2] = th0 / p.dt;
      }
    }
    return;
  }
  th = th0 + (double)((int)bc[0] - p.K) * p.dtheta;
  __syncthreads();  // bc is rewritten below

  // ---- fine stage: MM / IRLS steps on the squared biweight kernel, the radius shrinking from h_coarse to h
  double Wl = 0.0, El = 0.0, flag = 0.0;
  int done = 0;
  double hcur = p.h_coarse;
  for (int it = 0; it < p.iters; ++it, hcur *= p.shrink) {
    const double h = fmax(p.h, hcur);
    const double inv_h2 = 1.0 / (h * h);
    double s, c;
    sincos(th, &s, &c);
    double v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (long long i = P.b + wave; i < P.e; i += kRegWaves) {
      double px, py;
      const double w = reg_point(P, i, px, py);
      if (!(w > 0.0)) continue;
      const double mx = c * px - s * py + tx, my = s * px + c * py + ty;
      const double rho = sqrt(mx * mx + my * my);
      long long jb, je;
      reg_window(Q, p.C, p.r0, inv_step, rho - h, rho + h, rows, nrows, jb, je);
      for (long long j0 = jb + lane; j0 < je; j0 += 64 * kRegU) {
        double qxs[kRegU], qys[kRegU], us[kRegU];
        reg_load(Q, j0, je, qxs, qys, us);
#pragma unroll
        for (int k = 0; k < kRegU; ++k) {
          const double qx = qxs[k], qy = qys[k], u = us[k];
          if (!(u > 0.0)) continue;
          const double dx = mx - qx, dy = my - qy;
          const double d2 = dx * dx + dy * dy;
          const double a = 1.0 - d2 * inv_h2;
          if (!(a > 0.0)) continue;
          const double g = w * u * (a * a);
          v[0] += g;
          v[1] += g * px;
          v[2] += g * py;
          v[3] += g * qx;
          v[4] += g * qy;
          v[5] += g * (px * qx + py * qy);
          v[6] += g * (px * qy - py * qx);
          v[7] += g * d2;
        }
      }
    }
    wg_partials<Red::Sum>(v, red);
    if (t == 0) {
      double m[8];
      for (int q = 0; q < 8; ++q) m[q] = wg_fold<kRegWaves, 8, Red::Sum>(red, q, 0.0);
      bc[3] = m[0];
      bc[4] = m[7];
      if (!(m[0] > p.w_min)) {
        bc[5] = 1.0;  // too little support: keep T
      } else {
        const double W = m[0];
        const double Dc = m[5] - (m[1] * m[3] + m[2] * m[4]) / W;
        const double Xc = m[6] - (m[1] * m[4] - m[2] * m[3]) / W;
        const double nth = atan2(Xc, Dc);
        double ns, nc;
        sincos(nth, &ns, &nc);
        const double ntx = m[3] / W - (nc * m[1] - ns * m[2]) / W;
        const double nty = m[4] / W - (ns * m[1] + nc * m[2]) / W;
        const double ch = fmax(fabs(nth - th), fmax(fabs(ntx - tx), fabs(nty - ty)));
        bc[0] = nth;
        bc[1] = ntx;
        bc[2] = nty;
        bc[5] = (h == p.h && ch < p.tol) ? 2.0 : 0.0;  // 2: converged
      }
    }
    __syncthreads();  // publishes bc; red is free again
    Wl = bc[3];
    El = bc[4];
    const double stop = bc[5];
    if (stop != 1.0) {
      th = bc[0];
      tx = bc[1];
      ty = bc[2];
      done = it + 1;
    } else {
      flag = 1.0;
    }
    __syncthreads();  // bc is rewritten by the next step
    if (stop != 0.0) break;
  }

  if (t == 0) {
    o[0] = th;
    o[1] = tx;
    o[2] = ty;
    o[3] = Wl;
    o[4] = Wl > 0.0 ? sqrt(El / Wl) : 0.0;
    o[5] = ratio;
    o[6] = (double)done;
    o[7] = flag;
    if (omega && f > 0) {
      double* w = omega + (size_t)(f - 1) * 3;
      w[0] = w[1] = 0.0;
      w[2] = th / p.dt;
    }
  }
}

hipError_t launch_scan_register(hipStream_t st, const RegProblem& p, double* out, double* omega) {
  if (p.cloud.F <= 0) return hipSuccess;
  return launch(st, k_scan_register, p.cloud.F, kRegThreads, 0, p, out, omega);
}

}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
