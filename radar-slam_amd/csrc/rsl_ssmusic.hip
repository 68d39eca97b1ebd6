// rsl_ssmusic.hip — spatially smoothed MUSIC for gfx950 (rsl_doa_smoothed, include/rsl.h): several directions of
// arrival per range-Doppler cell from one snapshot of a uniform linear array.
//
// Per cell: the unit-norm signature s (M antennas), the forward-backward smoothed covariance R (L x L Hermitian, rank
// > 1 from the K = M - L + 1 overlapping sub-arrays), its eigendecomposition by cyclic complex Jacobi in fp32, the
// model order k, the null spectrum den[g] = sum over the L - k noise eigenvectors of |v^H a_g|^2 on the G grid points,
// and the k deepest local minima of den.
//
// Mapping: 16 lanes per cell, 4 cells per wave, one wave per workgroup (so __syncthreads is one wave's barrier and
// every loop around it is uniform).  R, V and the rotation parameters live in LDS, indexed at run time there (LDS
// indexing costs nothing; a run-time indexed register array would go to scratch).  A Jacobi sweep is the L - 1 (L even)
// or L (L odd) rounds of a round-robin tournament; the floor(L / 2) disjoint pairs of a round rotate at once in three
// phases: (0) one lane per pair derives the rotation from R[p][p], R[q][q], R[p][q]; (A) R <- R J and V <- V J, one
// (pair, row, matrix) item per lane and step; (B) R <- J^H R, one (pair, column) item per lane, which also writes the
// rotated pair's exact results (diagonal a - t|c|, b + t|c|; R[p][q] = R[q][p] = 0), so off-diagonal elements keep
// shrinking quadratically below eps * ||R||; elements already below the stop rule's per-element share are skipped.
// One Newton-Schulz step then restores V's orthonormality (the rotations' accumulated rounding).  Every lane takes the
// L - k noise eigenvectors into registers (signal columns zeroed; every index static, the loops are unrolled through the template parameter L),
// scans a contiguous chunk of ceil(G / 16) grid points with a three-point sliding window (the two neighbours outside
// the chunk are evaluated again, by the same instruction sequence, hence bit-identical to their owner's values), keeps
// its L - 1 deepest local minima in a sorted register list, and the group merges the lists with 16-lane shuffles.
#include <climits>
#include <cmath>

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "../../include/rsl.h"
#include "rsl_common.h"
#include "rsl_doa_common.h"
#include "rsl_internal.h"

namespace rsl {

namespace {

constexpr int kSsLanes = 16;  // lanes per cell
constexpr int kSsCells = 4;   // cells per workgroup (one wave)

template <int L>
struct SsCell {
  float2 R[L][L];
  float2 V[L][L];       // V[i][c]: component i of eigenvector c; holds the forward covariance before the Jacobi
  float2 s[16];         // unit-norm signature
  float rot[4][8];      // per pair of the round: cs, sn, Re e, Im e (e = c / |c|), new R[p][p], new R[q][q], go
  float lam[L];         // eigenvalues, descending
  int rank[L];          // position of R's diagonal entry i in the descending order
};

RSL_DEV float group_sum(float v) {
  v += __shfl_xor(v, 8, kSsLanes);
  v += __shfl_xor(v, 4, kSsLanes);
  v += __shfl_xor(v, 2, kSsLanes);
  v += __shfl_xor(v, 1, kSsLanes);
  return v;
}

// pair t of round r of the round-robin tournament of NT players (NT even): player NT - 1 stays, the others rotate
template <int NT>
RSL_DEV void rr_pair(int t, int r, int& p, int& q) {
  int a, b;
  if (t == 0) {
    a = NT - 1;
    b = r;
  } else {
    a = (r + t) % (NT - 1);
    b = (r + (NT - 1) - t) % (NT - 1);
  }
  p = min(a, b);
  q = max(a, b);
}

}  // namespace

template <int L>
__global__ __launch_bounds__(64) void k_doa_smoothed(CellList cl, const float2* __restrict__ steer, int G, int nmax,
                                                     int num_sources, float rel, int* __restrict__ out_nsrc,
                                                     int* __restrict__ out_idx, float* __restrict__ out_den,
                                                     float* __restrict__ out_eig, float* __restrict__ out_spec) {
  constexpr int NT = L + (L & 1);  // tournament players (an odd L gets a bye)
  constexpr int NP = NT / 2;       // pairs per round
  constexpr int NM = L - 1;        // local minima kept per lane = the largest nmax
  __shared__ SsCell<L> cells[kSsCells];
  const long long n = cl.count();
  const int M = cl.A;
  const int lane = threadIdx.x & (kSsLanes - 1), grp = threadIdx.x / kSsLanes;
  SsCell<L>& sm = cells[grp];
  const int K = M - L + 1;
  const float fnan = __builtin_nanf("");

  for (long long base = (long long)blockIdx.x * kSsCells; base < n; base += (long long)gridDim.x * kSsCells) {
    const long long cell = base + grp;
    const bool live = cell < n;
    // 1. signature: one gather of the cell's M values, norm over the group
    float2 x = make_float2(0.f, 0.f);
    if (live && lane < M) x = cl.at(cell, lane);
    const float pw = group_sum(x.x * x.x + x.y * x.y);
    const bool ok = live && pw > 0.f;
    const float inv = ok ? 1.f / sqrtf(pw) : 0.f;
    __syncthreads();  // the previous iteration's readers of this cell's LDS are done
    sm.s[lane] = make_float2(x.x * inv, x.y * inv);
    __syncthreads();
    // 2. forward covariance (into V), upper triangle and its mirror: exactly Hermitian
    const float invK = 1.f / (float)K;
    for (int it = lane; it < L * L; it += kSsLanes) {
      const int p = it / L, q = it % L;
      if (p <= q) {
        float re = 0.f, im = 0.f;
        for (int k = 0; k < K; ++k) {
          const float2 a = sm.s[k + p], b = sm.s[k + q];
          re += a.x * b.x + a.y * b.y;
          im += a.y * b.x - a.x * b.y;
        }
        re *= invK;
        im = p == q ? 0.f : im * invK;
        sm.V[p][q] = make_float2(re, im);
        sm.V[q][p] = make_float2(re, -im);
      }
    }
    __syncthreads();
    //    forward-backward average, its Frobenius norm
    float fr2 = 0.f;
    for (int it = lane; it < L * L; it += kSsLanes) {
      const int p = it / L, q = it % L;
      const float2 f = sm.V[p][q], b = sm.V[L - 1 - p][L - 1 - q];
      const float2 v = make_float2(0.5f * (f.x + b.x), 0.5f * (f.y - b.y));
      sm.R[p][q] = v;
      fr2 += v.x * v.x + v.y * v.y;
    }
    fr2 = group_sum(fr2);
    const float stop2 = (RSL_SS_OFF_TOL * RSL_SS_OFF_TOL) * fr2;
    const float skip2 = stop2 * (1.f / (L * L));  // |R[p][q]|^2 up to here is left alone (far above the denormals)
    __syncthreads();
    for (int it = lane; it < L * L; it += kSsLanes) sm.V[it / L][it % L] = make_float2(it / L == it % L ? 1.f : 0.f, 0.f);
    __syncthreads();
    // 3. cyclic Jacobi, at most RSL_SS_MAX_SWEEPS sweeps; a cell below the stop rule no longer rotates
    for (int sweep = 0; sweep < RSL_SS_MAX_SWEEPS; ++sweep) {
      float off2 = 0.f;
      for (int it = lane; it < L * L; it += kSsLanes) {
        const float2 v = sm.R[it / L][it % L];
        if (it / L != it % L) off2 += v.x * v.x + v.y * v.y;
      }
      off2 = group_sum(off2);
      const bool active = ok && off2 > stop2;
      if (!__syncthreads_or(active)) break;
      for (int r = 0; r < NT - 1; ++r) {
        if (lane < NP) {  // phase 0
          int p, q;
          rr_pair<NT>(lane, r, p, q);
          float go = 0.f;
          if (active && q < L) {
            const float a = sm.R[p][p].x, b = sm.R[q][q].x;
            const float2 c = sm.R[p][q];
            const float m2 = c.x * c.x + c.y * c.y;
            if (m2 > skip2) {  // threshold Jacobi: L^2 elements below the threshold satisfy the stop rule
              const float mag = sqrtf(m2);
              const float tau = (b - a) / (2.f * mag);
              const float t = copysignf(1.f, tau) / (fabsf(tau) + sqrtf(1.f + tau * tau));
              const float cs = 1.f / sqrtf(1.f + t * t);
              sm.rot[lane][0] = cs;
              sm.rot[lane][1] = t * cs;
              sm.rot[lane][2] = c.x / mag;
              sm.rot[lane][3] = c.y / mag;
              sm.rot[lane][4] = a - t * mag;
              sm.rot[lane][5] = b + t * mag;
              go = 1.f;
            }
          }
          sm.rot[lane][6] = go;
        }
        __syncthreads();
        // phase A: columns p, q of R and V.  J[p][p] = cs, J[p][q] = sn, J[q][p] = -sn conj(e), J[q][q] = cs conj(e)
        for (int it = lane; it < 2 * NP * L; it += kSsLanes) {
          const int w = it / (NP * L), rem = it % (NP * L), t = rem / L, i = rem % L;
          if (sm.rot[t][6] != 0.f) {
            int p, q;
            rr_pair<NT>(t, r, p, q);
            const float cs = sm.rot[t][0], sn = sm.rot[t][1], er = sm.rot[t][2], ei = sm.rot[t][3];
            float2* row = w ? sm.V[i] : sm.R[i];
            const float2 xx = row[p], yy = row[q];
            const float2 ey = make_float2(yy.x * er + yy.y * ei, yy.y * er - yy.x * ei);  // y conj(e)
            row[p] = make_float2(cs * xx.x - sn * ey.x, cs * xx.y - sn * ey.y);
            row[q] = make_float2(sn * xx.x + cs * ey.x, sn * xx.y + cs * ey.y);
          }
        }
        __syncthreads();
        // phase B: rows p, q of R (J^H from the left); the pair's own 2 x 2 block is written exactly
        for (int it = lane; it < NP * L; it += kSsLanes) {
          const int t = it / L, j = it % L;
          if (sm.rot[t][6] != 0.f) {
            int p, q;
            rr_pair<NT>(t, r, p, q);
            const float cs = sm.rot[t][0], sn = sm.rot[t][1], er = sm.rot[t][2], ei = sm.rot[t][3];
            const float2 xx = sm.R[p][j], yy = sm.R[q][j];
            const float2 ey = make_float2(yy.x * er - yy.y * ei, yy.y * er + yy.x * ei);  // y e
            float2 xn = make_float2(cs * xx.x - sn * ey.x, cs * xx.y - sn * ey.y);
            float2 yn = make_float2(sn * xx.x + cs * ey.x, sn * xx.y + cs * ey.y);
            if (j == p) {
              xn = make_float2(sm.rot[t][4], 0.f);
              yn = make_float2(0.f, 0.f);
            } else if (j == q) {
              xn = make_float2(0.f, 0.f);
              yn = make_float2(sm.rot[t][5], 0.f);
            }
            sm.R[p][j] = xn;
            sm.R[q][j] = yn;
          }
        }
        __syncthreads();
      }
    }
    // 4. eigenvalues in descending order (ties: lower index first), model order
    if (lane < L) {
      const float li = sm.R[lane][lane].x;
      int rk = 0;
      for (int j = 0; j < L; ++j) {
        const float lj = sm.R[j][j].x;
        rk += (lj > li || (lj == li && j < lane)) ? 1 : 0;
      }
      sm.lam[rk] = li;
      sm.rank[lane] = rk;
    }
    __syncthreads();
    //    one Newton-Schulz step V <- V (3 I - V^H V) / 2: the rotations' rounding leaves V orthonormal to about
    //    sqrt(rotations) * 2^-24 only, which would scale den by as much; the step squares that defect
    for (int it = lane; it < L * L; it += kSsLanes) {
      const int c = it / L, d = it % L;
      float wr = 0.f, wi = 0.f;  // (V^H V)[c][d]
      for (int i = 0; i < L; ++i) {
        const float2 a = sm.V[i][c], b = sm.V[i][d];
        wr += a.x * b.x + a.y * b.y;
        wi += a.x * b.y - a.y * b.x;
      }
      sm.R[c][d] = make_float2((c == d ? 1.5f : 0.f) - 0.5f * wr, -0.5f * wi);
    }
    __syncthreads();
    constexpr int NI = (L * L + kSsLanes - 1) / kSsLanes;
    float2 vt[NI];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int it = lane + j * kSsLanes;
      float vr = 0.f, vi = 0.f;
      if (it < L * L) {
        const int i = it / L, c = it % L;
        for (int d = 0; d < L; ++d) {
          const float2 a = sm.V[i][d], b = sm.R[d][c];
          vr += a.x * b.x - a.y * b.y;
          vi += a.x * b.y + a.y * b.x;
        }
      }
      vt[j] = make_float2(vr, vi);
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const int it = lane + j * kSsLanes;
      if (it < L * L) sm.V[it / L][it % L] = vt[j];
    }
    __syncthreads();
    int k = 0;
    if (ok) {
      k = num_sources;
      if (k <= 0) {
        const float cut = rel * sm.lam[0];
        for (int j = 0; j < L; ++j) k += sm.lam[j] >= cut ? 1 : 0;
        k = min(max(k, 1), nmax);
      }
    }
    if (live) {
      if (lane == 0) out_nsrc[cell] = k;
      if (out_eig && lane < L) out_eig[cell * L + lane] = ok ? sm.lam[lane] : fnan;
    }
    // 5. null spectrum over this lane's chunk of the grid, local minima
    float2 vn[L][L];  // vn[c][i] = V[i][c] for the noise eigenvectors, 0 for the signal ones
#pragma unroll
    for (int c = 0; c < L; ++c) {
      const bool noise = sm.rank[c] >= k;
#pragma unroll
      for (int i = 0; i < L; ++i) vn[c][i] = noise ? sm.V[i][c] : make_float2(0.f, 0.f);
    }
    auto den_at = [&](int g) {
      float2 a[L];
#pragma unroll
      for (int i = 0; i < L; ++i) a[i] = steer[(size_t)g * L + i];
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < L; ++c) {
        float dr = 0.f, di = 0.f;  // v^H a
#pragma unroll
        for (int i = 0; i < L; ++i) {
          dr += vn[c][i].x * a[i].x + vn[c][i].y * a[i].y;
          di += vn[c][i].x * a[i].y - vn[c][i].y * a[i].x;
        }
        acc += dr * dr + di * di;
      }
      return acc;
    };
    float bd[NM];
    int bi[NM];
#pragma unroll
    for (int j = 0; j < NM; ++j) {
      bd[j] = INFINITY;
      bi[j] = INT_MAX;
    }
    const int ch = (G + kSsLanes - 1) / kSsLanes;
    const int g0 = min(lane * ch, G), g1 = ok ? min(g0 + ch, G) : g0;
    if (g0 < g1) {
      float prev = g0 > 0 ? den_at(g0 - 1) : 0.f;
      float cur = den_at(g0);
      for (int g = g0; g < g1; ++g) {
        const float next = g + 1 < G ? den_at(g + 1) : 0.f;
        const bool lo = g == 0 || cur < prev;
        const bool hi = g == G - 1 || (g == 0 ? cur < next : cur <= next);
        if (out_spec) out_spec[cell * G + g] = cur;
        if (lo && hi) {
          float d = cur;
          int gi = g;
#pragma unroll
          for (int j = 0; j < NM; ++j) {
            if (d < bd[j] || (d == bd[j] && gi < bi[j])) {
              const float td = bd[j];
              const int ti = bi[j];
              bd[j] = d;
              bi[j] = gi;
              d = td;
              gi = ti;
            }
          }
        }
        prev = cur;
        cur = next;
      }
    }
    if (live && !ok && out_spec)
      for (int g = lane; g < G; g += kSsLanes) out_spec[cell * G + g] = fnan;
    // 6. the group's k deepest minima in ascending den (ties: lower index), by L - 1 rounds of a 16-lane minimum
#pragma unroll
    for (int r = 0; r < NM; ++r) {
      float d = bd[0];
      int gi = bi[0];
#pragma unroll
      for (int m = kSsLanes / 2; m > 0; m >>= 1) {
        const float od = __shfl_xor(d, m, kSsLanes);
        const int oi = __shfl_xor(gi, m, kSsLanes);
        if (od < d || (od == d && oi < gi)) {
          d = od;
          gi = oi;
        }
      }
      if (gi != INT_MAX && bi[0] == gi) {  // the winner's owner drops it
#pragma unroll
        for (int j = 0; j + 1 < NM; ++j) {
          bd[j] = bd[j + 1];
          bi[j] = bi[j + 1];
        }
        bd[NM - 1] = INFINITY;
        bi[NM - 1] = INT_MAX;
      }
      if (live && lane == 0 && r < nmax) {
        const bool have = r < k && gi != INT_MAX;
        out_idx[cell * nmax + r] = have ? gi : -1;
        if (out_den) out_den[cell * nmax + r] = have ? d : fnan;
      }
    }
  }
}

hipError_t launch_doa_smoothed(hipStream_t st, CellList cl, const float2* steer, int G, int L, int nmax,
                               int num_sources, float rel, int* out_nsrc, int* out_idx, float* out_den, float* out_eig,
                               float* out_spec) {
  if (cl.n_host <= 0) return hipSuccess;
  // one wave of 4 cells per workgroup; a list whose count lives on the device is walked by at most 8192 workgroups
  long long blocks = (cl.n_host + kSsCells - 1) / kSsCells;
  if (blocks > 8192) blocks = 8192;
  return with_int<2, 3, 4, 5, 6, 7, 8>(L, [&](auto l) {
    return launch(st, k_doa_smoothed<decltype(l)::value>, blocks, 64, 0, cl, steer, G, nmax, num_sources, rel, out_nsrc,
                  out_idx, out_den, out_eig, out_spec);
  });
}

}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
