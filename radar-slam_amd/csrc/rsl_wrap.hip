// rsl_wrap.hip — K9: greedy cross-frame target association and the wrapped-phase (regularised) ego-motion
// solve of the reference's "Improved" and "Advanced" solvers.  gfx950 / CDNA4, fp64 throughout.
//
// Replaces (reference src/algorithms/):
//   velocity_solver_improved.py  associate_targets_across_frames :74-129, cost_function :223-266,
//                                two_step_optimization :325-477 (differential_evolution, seed 42);
//   advanced_velocity_optimization.py  compute_regularized_cost_function :153-223,
//                                run_single_optimization / run_robust_optimization :343-524.
//
// Association: for each current target in order, the nearest not-yet-used previous target with
// Euclidean (x, y) distance < thr (strict), ties to the lowest index — exactly the reference's greedy loop.
// It is sequential across current targets, so one workgroup runs it per problem, with a block-wide
// (distance, index) argmin per step.
//
// Wrapped solve: the cost sum_i wrap(y_i - k J_i . x)^2 + R(x), J_i = [d_i, p_i x d_i], is piecewise
// quadratic with one basin per 2 pi / k of radial velocity (0.0195 m/s at 77 GHz, dt 0.1 s): the reference
// runs DE over the box and reports whichever basin DE settles in.  Here every thread runs a projected
// Gauss-Newton descent (the data Hessian 2 k^2 sum J J^T is constant, precomputed) from one start of a dense
// (v_x, v_y) grid over the box, with backtracking on the true cost, and a reduction keeps the lowest cost.
// "Projected" means: each iteration solves the Newton system on the free coordinates only -- a coordinate is held
// while it sits exactly on a bound and the total gradient points out of the box there; the others get the step of the
// reduced Hessian -- and the trial points x + step d are clamped to the box.  The descent so ends at the minimiser
// over the box of the piece it is in (a KKT point), not at the clamped unconstrained minimiser, which differs from it
// whenever a bound is active and the Hessian is not diagonal.  With no bound active the step is the plain one.
// Parity contract: cost <= the reference's DE cost (the argmin itself is not unique).
#include "rsl_common.h"
#include "rsl_internal.h"
#include "rsl_phase_common.h"

namespace rsl {

// ---------------------------------------------------------------------------------------------------------
// Greedy association (one block of 256 threads per problem).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_associate(const double* __restrict__ cur, int nc,
                                                   const double* __restrict__ prev, int np, double thr,
                                                   unsigned* __restrict__ used, int* __restrict__ match,
                                                   double* __restrict__ dist) {
  __shared__ double sd[256];
  __shared__ long si[256];
  const int t = threadIdx.x;
  for (int j = t; j < (np + 31) / 32; j += 256) used[j] = 0u;
  __syncthreads();
  for (int i = 0; i < nc; ++i) {
    const double cx = cur[2 * i], cy = cur[2 * i + 1];
    double bd = INFINITY;
    int bj = -1;
    for (int j = t; j < np; j += 256) {
      if ((used[j >> 5] >> (j & 31)) & 1u) continue;
      const double dx = cx - prev[2 * j], dy = cy - prev[2 * j + 1];
      const double d = sqrt(dx * dx + dy * dy);  // scipy cdist 'euclidean'
      if (d < thr && d < bd) {  // strict: the first (lowest) j wins ties within the thread's stripe
        bd = d;
        bj = j;
      }
    }
    block_argmin<256>(bd, bj, sd, si);
    if (t == 0) {
      const int j = (int)si[0];
      match[i] = j;
      dist[i] = j >= 0 ? sd[0] : INFINITY;
      if (j >= 0) used[j >> 5] |= 1u << (j & 31);
    }
    __syncthreads();
  }
}

hipError_t launch_associate(hipStream_t st, const double* cur, int nc, const double* prev, int np, double thr,
                            unsigned* used_scratch, int* match, double* dist) {
  if (nc <= 0) return hipSuccess;
  return launch(st, k_associate, 1, 256, 0, cur, nc, prev, np, thr, used_scratch, match, dist);
}

// ---------------------------------------------------------------------------------------------------------
// Wrapped multi-start solve.
// ---------------------------------------------------------------------------------------------------------
constexpr double kPi = 3.14159265358979323846;

// np.arctan2(np.sin(r), np.cos(r)): r reduced to [-pi, pi]
RSL_DEV double wrap_pi(double r) { return r - 2.0 * kPi * rint(r * (0.5 / kPi)); }

struct WrapProblem {
  const double* J;  // [N][6] = [d, p x d]
  const double* y;  // [N]
  long n;
  double k;
  int mode;         // 0 = Improved (0.01 |v|^2 + 0.01 |w|^2), 1 = Advanced (piecewise penalties)
  double w, vmax, wmax;
  const double* prev;  // [6] or null (Advanced temporal term)
  double lo[6], hi[6];
  int nv;           // 3: w fixed at 0, 6: full
};

// R(x) of the reference cost functions (exactly the reference's formulas).
RSL_DEV double reg_cost(const WrapProblem& P, const double* x) {
  if (P.mode == 0) {  // velocity_solver_improved.py:258-262
    double s = 0.0, s2 = 0.0;
    for (int a = 0; a < 3; ++a) s += x[a] * x[a];
    for (int a = 3; a < 6; ++a) s2 += x[a] * x[a];
    return 0.01 * s + 0.01 * s2;
  }
  // advanced_velocity_optimization.py:190-219
  const double vm = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double wm = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
  double r = 0.0;
  if (vm > P.vmax * 0.8) r += P.w * (vm - P.vmax * 0.8) * (vm - P.vmax * 0.8);
  if (wm > P.wmax * 0.8) r += P.w * (wm - P.wmax * 0.8) * (wm - P.wmax * 0.8);
  if (P.prev) {
    double s = 0.0;
    for (int a = 0; a < 6; ++a) s += (x[a] - P.prev[a]) * (x[a] - P.prev[a]);
    r += P.w * 0.1 * s;
  }
  if (vm > 20 && wm > 5) r += P.w * 0.01 * ((vm - 20) * (wm - 5));
  r += P.w * 10.0 * (x[2] * x[2]);
  return r;
}

// Gradient and a positive semi-definite (Gauss-Newton) Hessian of R.
RSL_DEV void reg_grad_hess(const WrapProblem& P, const double* x, double* g, double (*H)[6]) {
  for (int a = 0; a < 6; ++a) {
    g[a] = 0.0;
    for (int b = 0; b < 6; ++b) H[a][b] = 0.0;
  }
  if (P.mode == 0) {
    for (int a = 0; a < 6; ++a) {
      g[a] = 0.02 * x[a];
      H[a][a] = 0.02;
    }
    return;
  }
  const double vm = sqrt(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
  const double wm = sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5]);
  const double av = P.vmax * 0.8, aw = P.wmax * 0.8;
  if (vm > av) {
    const double c = 2.0 * P.w * (vm - av) / vm;
    for (int a = 0; a < 3; ++a) {
      g[a] += c * x[a];
      for (int b = 0; b < 3; ++b) H[a][b] += 2.0 * P.w * x[a] * x[b] / (vm * vm);
    }
  }
  if (wm > aw) {
    const double c = 2.0 * P.w * (wm - aw) / wm;
    for (int a = 3; a < 6; ++a) {
      g[a] += c * x[a];
      for (int b = 3; b < 6; ++b) H[a][b] += 2.0 * P.w * x[a] * x[b] / (wm * wm);
    }
  }
  if (P.prev) {
    for (int a = 0; a < 6; ++a) {
      g[a] += 0.2 * P.w * (x[a] - P.prev[a]);
      H[a][a] += 0.2 * P.w;
    }
  }
  if (vm > 20 && wm > 5) {
    for (int a = 0; a < 3; ++a) g[a] += P.w * 0.01 * (wm - 5) * x[a] / vm;
    for (int a = 3; a < 6; ++a) g[a] += P.w * 0.01 * (vm - 20) * x[a] / wm;
  }
  g[2] += 20.0 * P.w * x[2];
  H[2][2] += 20.0 * P.w;
}

// sum_i wrap(y_i - k J_i . x)^2; with GRAD also its gradient g[6] = -2k sum J r (g is not read otherwise).
template <bool GRAD>
RSL_DEV double data_cost(const WrapProblem& P, const double* x, double* g) {
  double c = 0.0;
  double gg[6] = {0, 0, 0, 0, 0, 0};
  for (long i = 0; i < P.n; ++i) {
    const double* Ji = P.J + 6 * i;
    double pred = 0.0;
#pragma unroll
    for (int a = 0; a < 6; ++a) pred += Ji[a] * x[a];
    const double r = wrap_pi(P.y[i] - P.k * pred);
    c += r * r;
    if (GRAD) {
#pragma unroll
      for (int a = 0; a < 6; ++a) gg[a] += Ji[a] * r;
    }
  }
  if (GRAD)
    for (int a = 0; a < 6; ++a) g[a] = -2.0 * P.k * gg[a];
  return c;
}

// One backtracking step of a projected descent over the first NX coordinates: x + step d clamped to the box, step
// 1, 1/2, ... (six trials), and the first trial whose cost(xn) is below f replaces x and f.  True while the descent
// should go on: a trial was taken and it gained more than 1e-13 (1 + f).
template <int NX, class Cost>
RSL_DEV bool backtrack(const WrapProblem& P, double* x, const double* d, double& f, Cost cost) {
  double step = 1.0, fn = f, xn[NX];
  bool ok = false;
  for (int ls = 0; ls < 6; ++ls) {
    for (int a = 0; a < NX; ++a) xn[a] = fmin(fmax(x[a] + step * d[a], P.lo[a]), P.hi[a]);
    fn = cost(xn);
    if (fn < f) {
      ok = true;
      break;
    }
    step *= 0.5;
  }
  if (!ok) return false;
  const double df = f - fn;
  for (int a = 0; a < NX; ++a) x[a] = xn[a];
  f = fn;
  return !(df <= 1e-13 * (1.0 + f));
}

// The free set of a projected step over the first nx coordinates, bit a per coordinate: a coordinate is held (its bit
// clear) while it sits on a bound of the box and the total gradient g points out of the box there, so that the
// descent direction would only be clamped back.  A held coordinate is released as soon as its gradient turns inward.
RSL_DEV unsigned free_set(const WrapProblem& P, const double* x, const double* g, int nx) {
  unsigned fr = 0u;
  for (int a = 0; a < nx; ++a) {
    const bool held = (x[a] <= P.lo[a] && g[a] > 0.0) || (x[a] >= P.hi[a] && g[a] < 0.0);
    if (!held) fr |= 1u << a;
  }
  return fr;
}

// Solve H d = -g on the free coordinates among the first nv (fr: free_set; Cholesky of the reduced Hessian with a tiny
// diagonal floor), d = 0 on the held ones and on [nv..5].  A held coordinate's row and column of L stay 0, so with
// every coordinate free the operations are those of the plain nv x nv solve, in its order.
RSL_DEV void newton_step(const double (*H)[6], const double* g, int nv, unsigned fr, double* d) {
  double L[6][6];
  for (int a = 0; a < 6; ++a)
    for (int b = 0; b < 6; ++b) L[a][b] = 0.0;
  for (int a = 0; a < nv; ++a) {
    if (!((fr >> a) & 1u)) continue;
    for (int b = 0; b <= a; ++b) {
      if (!((fr >> b) & 1u)) continue;
      double s = H[a][b];
      for (int q = 0; q < b; ++q) s -= L[a][q] * L[b][q];
      if (a == b) {
        L[a][a] = sqrt(s > 1e-12 ? s : 1e-12);
      } else {
        L[a][b] = s / L[b][b];
      }
    }
  }
  double z[6];
  for (int a = 0; a < nv; ++a) {
    z[a] = 0.0;
    if (!((fr >> a) & 1u)) continue;
    double s = -g[a];
    for (int q = 0; q < a; ++q) s -= L[a][q] * z[q];
    z[a] = s / L[a][a];
  }
  for (int a = nv - 1; a >= 0; --a) {
    d[a] = 0.0;
    if (!((fr >> a) & 1u)) continue;
    double s = z[a];
    for (int q = a + 1; q < nv; ++q) s -= L[q][a] * d[q];
    d[a] = s / L[a][a];
  }
  for (int a = nv; a < 6; ++a) d[a] = 0.0;
}

// One start per thread: x0 = (grid v_x, grid v_y, extra / 0 ...), projected Gauss-Newton with backtracking.
__global__ __launch_bounds__(256) void k_wrapped_ms(WrapProblem P, const double* __restrict__ Hd /* 6x6 */,
                                                    int gn, const double* __restrict__ extra, int nextra,
                                                    int iters, double* __restrict__ out /* [nstart][8] */) {
  const long s = (long)blockIdx.x * 256 + threadIdx.x;
  const long nstart = (long)gn * gn + nextra;
  if (s >= nstart) return;
  double x[6] = {0, 0, 0, 0, 0, 0};
  if (s < (long)gn * gn) {
    const int ix = (int)(s % gn), iy = (int)(s / gn);
    x[0] = P.lo[0] + (P.hi[0] - P.lo[0]) * (ix + 0.5) / gn;
    x[1] = P.lo[1] + (P.hi[1] - P.lo[1]) * (iy + 0.5) / gn;
  } else {
    for (int a = 0; a < 6; ++a) x[a] = extra[(s - (long)gn * gn) * 6 + a];
  }
  for (int a = 0; a < 6; ++a) {
    if (a >= P.nv) x[a] = 0.0;
    x[a] = fmin(fmax(x[a], P.lo[a]), P.hi[a]);
  }
  double g[6], H[6][6], d[6];
  double f = data_cost<true>(P, x, g) + reg_cost(P, x);
  const auto cost = [&](const double* xn) { return data_cost<false>(P, xn, nullptr) + reg_cost(P, xn); };
  for (int it = 0; it < iters; ++it) {
    double gr[6];
    reg_grad_hess(P, x, gr, H);
    for (int a = 0; a < 6; ++a) {
      g[a] += gr[a];
      for (int b = 0; b < 6; ++b) H[a][b] += Hd[a * 6 + b];
    }
    newton_step(H, g, P.nv, free_set(P, x, g, P.nv), d);
    if (!backtrack<6>(P, x, d, f, cost)) break;
    data_cost<true>(P, x, g);  // gradient at the new point
  }
  double* o = out + s * 8;
  for (int a = 0; a < 6; ++a) o[a] = x[a];
  o[6] = f;
  o[7] = (double)s;
}

// Argmin over starts (lowest cost, then lowest start index): one block.
__global__ __launch_bounds__(1024) void k_wrapped_best(const double* __restrict__ res, long nstart,
                                                      double* __restrict__ best) {
  __shared__ double sc[1024];
  __shared__ long si[1024];
  const int t = threadIdx.x;
  double bc = INFINITY;
  long bi = -1;
  for (long s = t; s < nstart; s += 1024) {
    const double c = res[s * 8 + 6];
    if (c < bc) {
      bc = c;
      bi = s;
    }
  }
  block_argmin<1024>(bc, bi, sc, si);
  if (t == 0) {
    const long b = si[0];
    for (int a = 0; a < 8; ++a) best[a] = b >= 0 ? res[b * 8 + a] : 0.0;
  }
}

// Data Hessian 2 k^2 sum J J^T (fp64), one block.  Its sums are not rsl_reduce.h's on purpose: here 21 threads add the
// 256 per-thread values of part in thread order, another order of additions than the wave tree.  Moving it would
// change the last bits of Hd, and with them possibly the basin a wrapped search ends in.
__global__ __launch_bounds__(256) void k_wrapped_hess(const double* __restrict__ J, long n, double k,
                                                      double* __restrict__ Hd) {
  __shared__ double part[256][21];
  const int t = threadIdx.x;
  double acc[21];
  for (int q = 0; q < 21; ++q) acc[q] = 0.0;
  for (long i = t; i < n; i += 256) {
    const double* Ji = J + 6 * i;
    int q = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b <= a; ++b) acc[q++] += Ji[a] * Ji[b];
  }
  for (int q = 0; q < 21; ++q) part[t][q] = acc[q];
  __syncthreads();
  if (t < 21) {
    double s = 0.0;
    for (int u = 0; u < 256; ++u) s += part[u][t];
    int q = 0;
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b <= a; ++b, ++q)
        if (q == t) {
          Hd[a * 6 + b] = 2.0 * k * k * s;
          Hd[b * 6 + a] = 2.0 * k * k * s;
        }
  }
}

// Jacobian rows J [n][6] (jacobian_row).
__global__ __launch_bounds__(256) void k_wrapped_jac(const double* __restrict__ pos, const double* __restrict__ ang,
                                                     long n, double* __restrict__ J) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) jacobian_row(pos + 3 * i, ang + 2 * i, J + 6 * i);
}

// ---------------------------------------------------------------------------------------------------------
// Dense wrapped search.  The wrapped cost is a sum of N periodic ridges, period 2 pi / (k |J_i|) along each target's
// J_i (0.0195 m/s in radial velocity at 77 GHz and dt = 0.1): a glassy landscape with millions of basins over the
// velocity box, which a coarse multi-start grid samples only in part.  Stage 1 runs a projected 2-D Gauss-Newton in
// (x0, x1) = (v_x, v_y) -- the coordinates the data term depends on for the reference's geometry (elevation 0 and
// p = r d make (w x p).d = 0 and d_z = 0: SURVEY §0 fact 8) -- from every point of a grid whose spacing is a fraction
// of the wrap period (a heuristic: the N ridge families cut cells smaller than the period, so not every basin is
// guaranteed to be entered; the contract checked is cost <= the reference DE, tests/test_gpu_wrapped.py, and the
// stage's latency at the reference's scale is measured there); x[2..5] are held at base (the regulariser's
// optimum for them).  Each block keeps its best start; the best nbest blocks seed stage 2, the full nv-D Gauss-Newton
// of k_wrapped_ms, together with the caller's extra starts.
// ---------------------------------------------------------------------------------------------------------
// Per-target stage-1 terms: (J_i0, J_i1, y_i - k sum_{a >= 2} J_ia base_a).
__global__ __launch_bounds__(256) void k_wrapped_prep2(const double* __restrict__ J, const double* __restrict__ y,
                                                       long n, double k, const double* __restrict__ base,
                                                       double* __restrict__ T) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double* Ji = J + 6 * i;
  double c = 0.0;
  for (int a = 2; a < 6; ++a) c += Ji[a] * base[a];
  T[3 * i] = Ji[0];
  T[3 * i + 1] = Ji[1];
  T[3 * i + 2] = y[i] - k * c;
}

struct Six {
  double v[6];
};
__global__ void k_fill6(double* __restrict__ dst, Six s) {
  if (threadIdx.x < 6) dst[threadIdx.x] = s.v[threadIdx.x];
}

struct Grid2 {
  long gx, gy;
  double x0, y0, hx, hy;  // start (ix, iy) = (x0 + (ix + 0.5) hx, y0 + (iy + 0.5) hy)
};

// The data cost on the stage-1 terms T at (v_x, v_y) = (v[0], v[1]); with GRAD also its gradient g[2].
template <bool GRAD>
RSL_DEV double data_cost2(const double* __restrict__ T, long n, double k, const double* v, double* g) {
  double c = 0.0, g0 = 0.0, g1 = 0.0;
  for (long i = 0; i < n; ++i) {
    const double j0 = T[3 * i], j1 = T[3 * i + 1];
    const double r = wrap_pi(T[3 * i + 2] - k * (j0 * v[0] + j1 * v[1]));
    c += r * r;
    if (GRAD) {
      g0 += j0 * r;
      g1 += j1 * r;
    }
  }
  if (GRAD) {
    g[0] = -2.0 * k * g0;
    g[1] = -2.0 * k * g1;
  }
  return c;
}

// One grid start per thread; block result = (cost, x0, x1, start index) of its best start.
__global__ __launch_bounds__(256) void k_wrapped_grid2(WrapProblem P, const double* __restrict__ T,
                                                       const double* __restrict__ Hd, const double* __restrict__ base,
                                                       Grid2 Gd, int iters, double* __restrict__ blk) {
  __shared__ double sc[256], sx[256], sy[256];
  __shared__ long si[256];
  const int t = threadIdx.x;
  const long s = (long)blockIdx.x * 256 + t;
  const long nstart = Gd.gx * Gd.gy;
  double f = INFINITY, x[6];
  for (int a = 0; a < 6; ++a) x[a] = base[a];
  if (s < nstart) {
    const long ix = s % Gd.gx, iy = s / Gd.gx;
    x[0] = fmin(fmax(Gd.x0 + ((double)ix + 0.5) * Gd.hx, P.lo[0]), P.hi[0]);
    x[1] = fmin(fmax(Gd.y0 + ((double)iy + 0.5) * Gd.hy, P.lo[1]), P.hi[1]);
    double g[2];
    f = data_cost2<true>(T, P.n, P.k, x, g) + reg_cost(P, x);
    const double h00 = Hd[0], h01 = Hd[1], h11 = Hd[7];
    const auto cost = [&](const double* xn) {  // at (xn[0], xn[1], x[2..5])
      const double xt[6] = {xn[0], xn[1], x[2], x[3], x[4], x[5]};
      return data_cost2<false>(T, P.n, P.k, xn, nullptr) + reg_cost(P, xt);
    };
    for (int it = 0; it < iters; ++it) {
      double gr[6], H[6][6];
      reg_grad_hess(P, x, gr, H);
      const double a = h00 + H[0][0], b = h01 + H[0][1], c = h11 + H[1][1];
      const double gt[2] = {g[0] + gr[0], g[1] + gr[1]};
      const double g0 = gt[0], g1 = gt[1];
      const unsigned fr = free_set(P, x, gt, 2);
      double d[2] = {0.0, 0.0};
      if (fr == 3u) {
        double det = a * c - b * b;
        if (!(det > 1e-300)) det = 1e-300;
        d[0] = -(c * g0 - b * g1) / det;
        d[1] = -(a * g1 - b * g0) / det;
      } else if (fr == 1u) {  // x1 held: the reduced Hessian is a
        d[0] = -g0 / (a > 1e-300 ? a : 1e-300);
      } else if (fr == 2u) {  // x0 held
        d[1] = -g1 / (c > 1e-300 ? c : 1e-300);
      }
      if (!backtrack<2>(P, x, d, f, cost)) break;
      data_cost2<true>(T, P.n, P.k, x, g);
    }
  }
  sx[t] = x[0];
  sy[t] = x[1];
  block_argmin<256>(f, s < nstart ? s : -1, sc, si);  // a start past the grid is no candidate; thread 0's is on it
  if (t == 0) {
    const long win = si[0] - (long)blockIdx.x * 256;  // the winning thread
    double* o = blk + 4 * (long)blockIdx.x;
    o[0] = sc[0];
    o[1] = sx[win];
    o[2] = sy[win];
    o[3] = (double)si[0];
  }
}

// The nbest lowest block results (cost, then start index), written as 6-D starts (x0, x1, base[2..5]) in front of
// the caller's extra starts; taken entries are marked +inf.  One block.
__global__ __launch_bounds__(1024) void k_wrapped_topk(double* __restrict__ blk, long nblk, int nbest,
                                                       const double* __restrict__ base, double* __restrict__ starts) {
  __shared__ double sc[1024];
  __shared__ long si[1024];
  const int t = threadIdx.x;
  for (int q = 0; q < nbest; ++q) {
    double bc = INFINITY;
    long bi = -1;  // the candidate's start index: the tie key, and 256 b + the winning thread of its block b
    for (long b = t; b < nblk; b += 1024) {
      const double c = blk[4 * b];
      const long idx = (long)blk[4 * b + 3];
      if (c < bc || (c == bc && bi >= 0 && idx < bi)) {
        bc = c;
        bi = idx;
      }
    }
    block_argmin<1024>(bc, bi, sc, si);
    if (t == 0) {
      const long b = si[0] >= 0 ? si[0] / 256 : -1;
      double* o = starts + 6 * q;
      o[0] = b >= 0 ? blk[4 * b + 1] : base[0];
      o[1] = b >= 0 ? blk[4 * b + 2] : base[1];
      for (int a = 2; a < 6; ++a) o[a] = base[a];
      if (b >= 0) blk[4 * b] = INFINITY;
    }
    __syncthreads();
  }
}

// The problem of one call into P, with its Jacobian J [6n] and data Hessian Hd [36] launched into the scratch sections
// given.
static hipError_t wrap_problem(hipStream_t st, const WrapArgs& a, double* J, double* Hd, WrapProblem& P) {
  P = {J, a.y, a.n, a.k, a.mode, a.w, a.vmax, a.wmax, a.prev, {}, {}, a.nv};
  for (int c = 0; c < 6; ++c) {
    P.lo[c] = a.lo[c];
    P.hi[c] = a.hi[c];
  }
  if (hipError_t e = launch(st, k_wrapped_jac, (a.n + 255) / 256, 256, 0, a.pos, a.ang, a.n, J)) return e;
  return launch(st, k_wrapped_hess, 1, 256, 0, J, a.n, a.k, Hd);
}

// The nv-D descent from nstart = gn^2 + nextra starts into res [8 nstart], and the best of them into out [8].
static hipError_t wrapped_descend(hipStream_t st, const WrapProblem& P, const double* Hd, int gn, const double* extra,
                                  long nextra, int iters, double* res, double* out) {
  const long nstart = (long)gn * gn + nextra;
  if (hipError_t e = launch(st, k_wrapped_ms, (nstart + 255) / 256, 256, 0, P, Hd, gn, extra, (int)nextra, iters, res))
    return e;
  return launch(st, k_wrapped_best, 1, 1024, 0, res, nstart, out);
}

hipError_t launch_wrapped_search(hipStream_t st, const WrapArgs& a, const double* base6, long gx, long gy, int nbest,
                                 double* scratch, double* out) {
  const long n = a.n, nstart = (long)nbest + a.nextra;
  const WrappedSearchScratch S(scratch, n, gx * gy, nstart);
  Six b6;
  for (int c = 0; c < 6; ++c) b6.v[c] = fmin(fmax(base6[c], a.lo[c]), a.hi[c]);
  hipError_t e = launch(st, k_fill6, 1, 64, 0, S.base, b6);  // by value: no pageable host copy
  if (!e && a.nextra > 0)
    e = hipMemcpyAsync(S.starts + 6L * nbest, a.extra, 6 * sizeof(double) * a.nextra, hipMemcpyDeviceToDevice, st);
  WrapProblem P;
  if (!e) e = wrap_problem(st, a, S.J, S.Hd, P);
  if (!e) e = launch(st, k_wrapped_prep2, (n + 255) / 256, 256, 0, S.J, a.y, n, a.k, S.base, S.T);
  const Grid2 Gd = {gx, gy, a.lo[0], a.lo[1], (a.hi[0] - a.lo[0]) / (double)gx, (a.hi[1] - a.lo[1]) / (double)gy};
  if (!e) e = launch(st, k_wrapped_grid2, S.nblk, 256, 0, P, S.T, S.Hd, S.base, Gd, a.iters, S.blk);
  if (!e) e = launch(st, k_wrapped_topk, 1, 1024, 0, S.blk, S.nblk, nbest, S.base, S.starts);
  if (e) return e;
  return wrapped_descend(st, P, S.Hd, 0, S.starts, nstart, a.iters, S.res, out);
}

hipError_t launch_wrapped_solve(hipStream_t st, const WrapArgs& a, int gn, double* scratch, double* out) {
  const WrappedSolveScratch S(scratch, a.n, (long)gn * gn + a.nextra);
  WrapProblem P;
  if (hipError_t e = wrap_problem(st, a, S.J, S.Hd, P)) return e;
  return wrapped_descend(st, P, S.Hd, gn, a.extra, a.nextra, a.iters, S.res, out);
}

}  // namespace rsl
