// rsl_aux.hip — per-call kernels behind the reference's fine-grained methods.  gfx950.
//
//  k_preprocess_rows : dechirp_signal / apply_window / remove_dc / process_chirp (dechirp.py:85-166):
//                      rows * table, then optional complex-mean removal.
//  k_phase_model     : compute_phase_difference_model + cost_function (velocity_solver.py:65-176,
//                      velocity_solver_improved.py:173-266 with the wrap and ridge), general 6-DoF.
//  k_bvls            : two_step_optimization (velocity_solver.py:178-307) for arbitrary positions /
//                      angles: the model k (v + w x p).d = k [d, p x d] . [v; w] is linear in the 6
//                      unknowns, so the DE box problem is a bounded linear least-squares problem, solved
//                      exactly by an active-set (Stark-Parker BVLS) on the 6x6 normal equations in fp64.
#include "rsl_common.h"
#include "rsl_internal.h"
#include "rsl_phase_common.h"
#include "rsl_reduce.h"

namespace rsl {

constexpr int kAuxWaves = 256 / 64;  // every kernel of this file runs 256 threads

__global__ __launch_bounds__(256) void k_preprocess_rows(const float2* __restrict__ in, int S,
                                                         const float2* __restrict__ table, int dc,
                                                         float2* __restrict__ out) {
  const long r = blockIdx.x;
  const float2* src = in + (size_t)r * S;
  float2* dst = out + (size_t)r * S;
  double a[2] = {0.0, 0.0};  // fp64 mean accumulation: re, im
  for (int s = threadIdx.x; s < S; s += 256) {
    const float2 v = cmul(src[s], table[s]);
    dst[s] = v;
    a[0] += v.x;
    a[1] += v.y;
  }
  if (!dc) return;
  __shared__ double red[kAuxWaves * 2], mean[2];
  wg_partials<Red::Sum>(a, red);
  if (threadIdx.x == 0) {
    mean[0] = wg_fold<kAuxWaves, 2, Red::Sum>(red, 0, 0.0) / S;
    mean[1] = wg_fold<kAuxWaves, 2, Red::Sum>(red, 1, 0.0) / S;
  }
  __syncthreads();
  const double mx = mean[0], my = mean[1];
  for (int s = threadIdx.x; s < S; s += 256) {
    const float2 v = dst[s];
    dst[s] = make_float2((float)(v.x - mx), (float)(v.y - my));
  }
}

hipError_t launch_preprocess_rows(hipStream_t st, const float2* in, long rows, int S, const float2* table, int dc,
                                  float2* out) {
  if (rows <= 0 || S <= 0) return hipSuccess;
  return launch(st, k_preprocess_rows, rows, 256, 0, in, S, table, dc, out);
}

// ---------------------------------------------------------------------------------------------
// pos f64 [N,3], ang f64 [N,2], x f64 [6] (v, w); y f64 [N] nullable; out_pred/out_resid nullable;
// cost_out f64 [1] = sum r^2 (+ ridge |x|^2), r wrapped to (-pi, pi] when wrap != 0.  One block.
__global__ __launch_bounds__(256) void k_phase_model(const double* __restrict__ pos, const double* __restrict__ ang,
                                                     long n, const double* __restrict__ x, double k,
                                                     const double* __restrict__ y, int wrap, double ridge,
                                                     double* __restrict__ pred, double* __restrict__ resid,
                                                     double* __restrict__ cost_out) {
  __shared__ double red[kAuxWaves];
  double acc = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    double J[6];
    jacobian_row(pos + 3 * i, ang + 2 * i, J);
    double p = 0.0;
    for (int c = 0; c < 6; ++c) p += J[c] * x[c];
    p *= k;
    if (pred) pred[i] = p;
    if (y) {
      double r = y[i] - p;
      if (wrap) r = atan2(sin(r), cos(r));
      if (resid) resid[i] = r;
      acc += r * r;
    }
  }
  const double sum = wg_one<kAuxWaves, Red::Sum>(acc, red, 0.0);
  if (threadIdx.x == 0 && cost_out) {
    double reg = 0.0;
    for (int c = 0; c < 6; ++c) reg += x[c] * x[c];
    cost_out[0] = sum + ridge * reg;
  }
}

hipError_t launch_phase_model(hipStream_t st, const double* pos, const double* ang, long n, const double* x, double k,
                              const double* y, int wrap, double ridge, double* pred, double* resid, double* cost) {
  return launch(st, k_phase_model, 1, 256, 0, pos, ang, n, x, k, y, wrap, ridge, pred, resid, cost);
}

// ---------------------------------------------------------------------------------------------
// Solve H_FF z = g_F for the free set F (n <= 6) by Gaussian elimination with partial pivoting;
// singular directions (pivot <= eps * scale) get 0 (minimum-norm on exactly-null columns).
RSL_DEV void solve_free(const double H[6][6], const double* g, const int* freev, int nf, double* z) {
  double M[6][7];
  double scale = 0.0;
  for (int a = 0; a < nf; ++a) scale = fmax(scale, fabs(H[freev[a]][freev[a]]));
  for (int a = 0; a < nf; ++a) {
    for (int b = 0; b < nf; ++b) M[a][b] = H[freev[a]][freev[b]];
    M[a][nf] = g[a];
  }
  int piv_ok[6];
  for (int col = 0; col < nf; ++col) {
    int best = col;
    for (int r = col + 1; r < nf; ++r)
      if (fabs(M[r][col]) > fabs(M[best][col])) best = r;
    if (best != col)
      for (int c = 0; c <= nf; ++c) {
        const double t = M[col][c];
        M[col][c] = M[best][c];
        M[best][c] = t;
      }
    piv_ok[col] = fabs(M[col][col]) > 1e-13 * (scale > 0 ? scale : 1.0);
    if (!piv_ok[col]) continue;
    for (int r = col + 1; r < nf; ++r) {
      const double f = M[r][col] / M[col][col];
      for (int c = col; c <= nf; ++c) M[r][c] -= f * M[col][c];
    }
  }
  for (int col = nf - 1; col >= 0; --col) {
    if (!piv_ok[col]) {
      z[col] = 0.0;
      continue;
    }
    double s = M[col][nf];
    for (int c = col + 1; c < nf; ++c) s -= M[col][c] * z[c];
    z[col] = s / M[col][col];
  }
}

// BVLS on the reduced moments m (21 of the upper triangle of J'J, then 6 of J'y; J scaled by k) over the first nv
// unknowns; one thread.  xout [nv].
RSL_DEV void bvls_solve(const double* m, int nv, double ridge, const double* __restrict__ lo,
                        const double* __restrict__ hi, double* xout) {
  double H[6][6], b[6];
  {
    int t = 0;
    for (int a = 0; a < 6; ++a)
      for (int c = a; c < 6; ++c) {
        H[a][c] = H[c][a] = m[t++];
      }
    for (int a = 0; a < 6; ++a) {
      b[a] = m[21 + a];
      H[a][a] += ridge;
    }
  }
  // BVLS (Stark & Parker): state 0 free, -1 at lower, +1 at upper.  Start with all at bound nearest 0
  // (0 itself when inside the box: treat as free start).
  double x[6];
  int state[6];
  for (int a = 0; a < nv; ++a) {
    x[a] = fmin(fmax(0.0, lo[a]), hi[a]);
    state[a] = 0;
  }
  for (int it = 0; it < 100; ++it) {
    // solve on the free set with bound variables fixed
    int freev[6], nf = 0;
    for (int a = 0; a < nv; ++a)
      if (state[a] == 0) freev[nf++] = a;
    double g[6], z[6];
    for (int ai = 0; ai < nf; ++ai) {
      const int a = freev[ai];
      double s = b[a];
      for (int c = 0; c < nv; ++c)
        if (state[c] != 0) s -= H[a][c] * x[c];
      g[ai] = s;
    }
    solve_free(H, g, freev, nf, z);
    // move toward z; stop at the first bound crossed
    double alpha = 1.0;
    int hit = -1, hit_state = 0;
    for (int ai = 0; ai < nf; ++ai) {
      const int a = freev[ai];
      const double d = z[ai] - x[a];
      if (z[ai] < lo[a]) {
        const double t = (lo[a] - x[a]) / d;
        if (t < alpha) { alpha = t; hit = a; hit_state = -1; }
      } else if (z[ai] > hi[a]) {
        const double t = (hi[a] - x[a]) / d;
        if (t < alpha) { alpha = t; hit = a; hit_state = 1; }
      }
    }
    if (alpha < 0) alpha = 0;
    for (int ai = 0; ai < nf; ++ai) {
      const int a = freev[ai];
      x[a] = x[a] + alpha * (z[ai] - x[a]);
    }
    if (hit >= 0) {
      x[hit] = hit_state < 0 ? lo[hit] : hi[hit];
      state[hit] = hit_state;
      continue;
    }
    // KKT: gradient of 0.5|r|^2 wrt x is -(b - H x); release the bound variable that violates most
    int rel = -1;
    double worst = 0.0;
    for (int a = 0; a < nv; ++a) {
      if (state[a] == 0) continue;
      double gr = b[a];
      for (int c = 0; c < nv; ++c) gr -= H[a][c] * x[c];  // descent direction component
      const double viol = state[a] < 0 ? gr : -gr;          // at lower: wants to increase if gr > 0
      if (viol > worst * (1.0 + 1e-12) && viol > 1e-12 * (fabs(b[a]) + 1.0)) {
        worst = viol;
        rel = a;
      }
    }
    if (rel < 0) break;
    state[rel] = 0;
  }
  for (int a = 0; a < nv; ++a) xout[a] = x[a];
}

// One block: normal equations of min |y - k J x|^2 + ridge |x|^2 over nv (3 or 6) unknowns, then BVLS on thread 0, then
// the cost at the solution as a per-target sum of squares over the workgroup.
// out f64 [nv + 1] = x, cost.
__global__ __launch_bounds__(256) void k_bvls(const double* __restrict__ pos, const double* __restrict__ ang, long n,
                                              const double* __restrict__ y, double k, int nv, double ridge,
                                              const double* __restrict__ lo, const double* __restrict__ hi,
                                              double* __restrict__ out) {
  __shared__ double red[kAuxWaves * 27];
  __shared__ double xs[6];
  double acc[27];
  for (int c = 0; c < 27; ++c) acc[c] = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    double J[6];
    jacobian_row(pos + 3 * i, ang + 2 * i, J);
    for (int c = 0; c < 6; ++c) J[c] *= k;
    int t = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = a; b < 6; ++b) acc[t++] += J[a] * J[b];  // 21
    for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * y[i];  // 6
  }
  // all 27 in one pass, 1 barrier: with one-value sums, then of 3 barriers each, for these and the cost (28 in all)
  // k_bvls took 49.8 instead of 47.6 us at 26 targets
  double m[27];
  wg_sums<kAuxWaves>(acc, red, m);
  if (threadIdx.x == 0) bvls_solve(m, nv, ridge, lo, hi, xs);
  __syncthreads();  // publishes xs; red is free again for the cost's sum
  // The cost as the reference's sum of squares (step1_result.fun), in k_phase_model's operation order.  The moment form
  // y'y - 2 b.x + x'Hx cancels at a near-exact fit: its error is ~1e-15 y'y whatever the residual (-3e-8 ... +6e-8 was
  // returned at exact fits of 3 to 300 targets, where the sum of squares is ~1e-23).
  double q = 0.0;
  for (long i = threadIdx.x; i < n; i += 256) {
    double J[6];
    jacobian_row(pos + 3 * i, ang + 2 * i, J);
    double p = 0.0;
    for (int c = 0; c < nv; ++c) p += J[c] * xs[c];
    const double r = y[i] - p * k;
    q += r * r;
  }
  const double sum = wg_one<kAuxWaves, Red::Sum>(q, red, 0.0);
  if (threadIdx.x != 0) return;
  double reg = 0.0;
  for (int a = 0; a < nv; ++a) {
    out[a] = xs[a];
    reg += xs[a] * xs[a];
  }
  out[nv] = sum + ridge * reg;
}

hipError_t launch_bvls(hipStream_t st, const double* pos, const double* ang, long n, const double* y, double k, int nv,
                       double ridge, const double* lo, const double* hi, double* out) {
  return launch(st, k_bvls, 1, 256, 0, pos, ang, n, y, k, nv, ridge, lo, hi, out);
}

}  // namespace rsl
