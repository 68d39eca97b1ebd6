// rsl_ramap.hip — range-azimuth maps for gfx950 (rsl_range_cov, rsl_range_azimuth, include/rsl.h): the multi-snapshot
// spatial covariance of every range bin (its Doppler bins are the snapshots) and the Bartlett / Capon power over an
// azimuth grid computed from it.
//
// k_range_cov: one wave per (frame, range bin).  With Z = [Re X; Im X] (2A real rows, one column per Doppler bin) the
// real Gram matrix G = Z Z^T holds the covariance: Re R[p][q] = G[p][q] + G[p+H][q+H], Im R[p][q] = G[p+H][q] -
// G[p][q+H] (H = half the tile: Re rows 0 .. H-1, Im rows H .. 2H-1).  G is one tile of the fp32 matrix pipe:
// v_mfma_f32_16x16x4_f32 for A <= 8, v_mfma_f32_32x32x2_f32 for A <= 16.  Lane l of a T x T tile supplies
// A[l % T][k = l / T] and B[k][l % T]; for a Gram matrix both are Z[l % T][k], so one register feeds both operands,
// and since the pipe computes a k-ordered fmaf chain whose products commute, G[i][j] and G[j][i] are the same bits:
// R is exactly Hermitian.  The sum over k is order-free, so the k <-> Doppler-bin assignment follows the loads: a
// lane reads two consecutive c64 (16 B) of its antenna's row, the Re lane feeds the two real parts to two MFMAs, the
// Im lane the two imaginary parts (both lanes read the same 16 B; the second is a cache hit).  That needs every row's
// window start on a 16-B boundary, i.e. an even C and an even first element; otherwise (odd C) or until then (odd
// start) and for the tail (fewer than 2 T' bins left, T' = 64 / T) a step reads one c64 per lane and out-of-window
// lanes supply zero.  Rows of absent antennas (A < H) supply zero without a load.  The tile goes through LDS (1 or 4
// KiB per wave) to pair G's four quadrants; A * A c64 are stored contiguously.
//
// k_range_azimuth: one wave per covariance row.  The row's quadratic-form matrix Q goes to LDS once: Q = R for
// Bartlett; for Capon Q = R_l^-1 by an fp32 Cholesky R_l = L L^H (one lane per matrix row, column by column), the
// triangular inverse T = L^-1 (one lane per column) and Q = T^H T (upper triangle and its mirror).  Then every lane
// takes grid points g = lane, lane + 64, ..: it loads a_g (A c64, zero-padded to the template's MA registers), forms
//   y = sum_p Q[p][p] |a_p|^2 + 2 Re sum_p conj(a_p) sum_{q > p} Q[p][q] a_q
// from LDS broadcasts of Q's upper triangle (2 A^2 + 2 A fma), stores along g (coalesced) and keeps its first maximum;
// a 64-lane reduction (ties to the lower index) gives the row's argmax.
#include <climits>
#include <cmath>

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "../../include/rsl.h"
#include "rsl_common.h"
#include "rsl_internal.h"

namespace rsl {

namespace {

typedef float floatx16 __attribute__((ext_vector_type(16)));

constexpr int kCovWaves = 4;  // (frame, range bin) rows per workgroup, one per wave

// One Gram tile G += z z^T on the fp32 matrix pipe: the lane's value is both the A and the B operand.
template <int T>
struct GramTile;
template <>
struct GramTile<16> {
  typedef floatx4 Acc;
  static RSL_DEV Acc mac(float z, Acc acc) { return __builtin_amdgcn_mfma_f32_16x16x4f32(z, z, acc, 0, 0, 0); }
  // C/D map: column lane % 16, row 4 (lane / 16) + reg
  static RSL_DEV void store(float* sm, int lane, Acc acc) {
    float* d = sm + 4 * (lane >> 4) * 16 + (lane & 15);
    d[0] = acc[0];
    d[16] = acc[1];
    d[32] = acc[2];
    d[48] = acc[3];
  }
};
template <>
struct GramTile<32> {
  typedef floatx16 Acc;
  static RSL_DEV Acc mac(float z, Acc acc) { return __builtin_amdgcn_mfma_f32_32x32x2f32(z, z, acc, 0, 0, 0); }
  // C/D map: column lane % 32, row (reg % 4) + 8 (reg / 4) + 4 (lane / 32)
  static RSL_DEV void store(float* sm, int lane, Acc acc) {
    float* d = sm + 4 * (lane >> 5) * 32 + (lane & 31);
#define RSL_RA_ST(r) d[((r & 3) + 8 * (r >> 2)) * 32] = acc[r]
    RSL_RA_ST(0); RSL_RA_ST(1); RSL_RA_ST(2); RSL_RA_ST(3); RSL_RA_ST(4); RSL_RA_ST(5); RSL_RA_ST(6); RSL_RA_ST(7);
    RSL_RA_ST(8); RSL_RA_ST(9); RSL_RA_ST(10); RSL_RA_ST(11); RSL_RA_ST(12); RSL_RA_ST(13); RSL_RA_ST(14);
    RSL_RA_ST(15);
#undef RSL_RA_ST
  }
};

}  // namespace

// rds c64 [F][A][S][C] -> cov c64 [F][S][A][A] over the Doppler window [c0, c1); rows = F * S; T = 16 (A <= 8) or 32.
// vec: every antenna row's element index ((f A + p) S + r) C is even and the base pointer is 16-B aligned (the
// launcher checks: C even), so that an even window start is a 16-B boundary in every row.
template <int T>
__global__ __launch_bounds__(64 * kCovWaves) void k_range_cov(const float2* __restrict__ rds, long long rows, int A,
                                                              int S, int C, int c0, int c1, int vec,
                                                              float2* __restrict__ cov) {
  constexpr int H = T / 2;    // Re rows 0 .. H-1, Im rows H .. T-1
  constexpr int KQ = 64 / T;  // k values per MFMA (4 or 2)
  __shared__ float tiles[kCovWaves][T * T];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * kCovWaves + wave;
  if (row >= rows) return;  // wave-uniform; no block-wide barrier below
  float* sm = tiles[wave];
  const long long f = row / S;
  const int r = (int)(row - f * S);
  const int i = lane % T, kq = lane / T;
  const int p = i % H;
  const bool im = i >= H;
  const bool have = p < A;
  // the lane's antenna row of this range bin; absent antennas keep a valid pointer that is never dereferenced
  const float2* src = rds + (((size_t)f * A + (have ? p : 0)) * S + r) * (size_t)C;
  typedef GramTile<T> Tile;
  typename Tile::Acc acc = {};
  // the lane's operand of a one-bin-per-lane step over [c, lim): bin c + kq, zero outside the window
  auto bin1 = [&](int c, int lim) {
    float z = 0.f;
    if (have && c + kq < lim) {
      const float2 v = src[c + kq];
      z = im ? v.y : v.x;
    }
    return z;
  };
  int c = c0;
  if (vec) {
    if (c & 1) {  // odd start: one bin alone
      acc = Tile::mac(bin1(c, c + 1), acc);
      c += 1;
    }
    constexpr int NV = 2 * KQ;  // bins per 16-B step
    constexpr int U = 4;        // steps whose loads are in flight together
    for (; c + U * NV <= c1; c += U * NV) {
      float4 v[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        v[u] = have ? *reinterpret_cast<const float4*>(src + c + u * NV + 2 * kq) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        acc = Tile::mac(im ? v[u].y : v[u].x, acc);
        acc = Tile::mac(im ? v[u].w : v[u].z, acc);
      }
    }
    for (; c + NV <= c1; c += NV) {
      const float4 v = have ? *reinterpret_cast<const float4*>(src + c + 2 * kq) : make_float4(0.f, 0.f, 0.f, 0.f);
      acc = Tile::mac(im ? v.y : v.x, acc);
      acc = Tile::mac(im ? v.w : v.z, acc);
    }
  }
  for (; c < c1; c += KQ) acc = Tile::mac(bin1(c, c1), acc);
  Tile::store(sm, lane, acc);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  const float inv = 1.f / (float)(c1 - c0);
  float2* dst = cov + (size_t)row * A * A;
  for (int it = lane; it < A * A; it += 64) {
    const int pp = it / A, qq = it - pp * A;
    const float re = sm[pp * T + qq] + sm[(pp + H) * T + qq + H];
    const float imv = sm[(pp + H) * T + qq] - sm[pp * T + qq + H];
    dst[it] = make_float2(re * inv, imv * inv);
  }
}

hipError_t launch_range_cov(hipStream_t st, const float2* rds, int F, int A, int S, int C, int c0, int c1,
                            float2* cov) {
  if (F <= 0 || S <= 0) return hipSuccess;
  const long long rows = (long long)F * S;
  const long long blocks = (rows + kCovWaves - 1) / kCovWaves;
  const int vec = C % 2 == 0 && (reinterpret_cast<size_t>(rds) & 15) == 0;
  return launch(st, A <= 8 ? k_range_cov<16> : k_range_cov<32>, blocks, 64 * kCovWaves, 0, rds, rows, A, S, C, c0, c1,
                vec, cov);
}

// cov c64 [n][A][A] -> map f32 [n][G], arg i32 [n] (nullable).  One wave per workgroup (so __syncthreads is one wave's
// barrier and every loop around it is uniform); MA = 8 (A <= 8) or 16 registers of a_g per lane.
template <int MA>
__global__ __launch_bounds__(64) void k_range_azimuth(const float2* __restrict__ cov, long long n, int A,
                                                      const float2* __restrict__ steer, int G, int capon, float loading,
                                                      float* __restrict__ map, int* __restrict__ arg) {
  __shared__ float2 Q[MA][MA];   // the quadratic form's matrix; rows and columns >= A are zero
  __shared__ float2 Lm[MA][MA];  // Capon: R_l, overwritten by its Cholesky factor (lower triangle)
  __shared__ float2 Tm[MA][MA];  // Capon: L^-1 (lower triangle)
  const int lane = threadIdx.x;
  const float scale = 1.f / ((float)A * (float)A);
  for (long long row = blockIdx.x; row < n; row += gridDim.x) {
    const float2* R = cov + (size_t)row * A * A;
    __syncthreads();  // the previous row's readers of Q are done
    // the Hermitian matrix its upper triangle and the diagonal's real part define
    for (int it = lane; it < MA * MA; it += 64) {
      const int pp = it / MA, qq = it % MA;
      float2 v = make_float2(0.f, 0.f);
      if (pp < A && qq < A) {
        if (pp < qq) {
          v = R[pp * A + qq];
        } else if (pp > qq) {
          const float2 w = R[qq * A + pp];
          v = make_float2(w.x, -w.y);
        } else {
          v = make_float2(R[pp * A + pp].x, 0.f);
        }
      }
      Q[pp][qq] = v;
    }
    __syncthreads();
    float t = 0.f;
    for (int pp = 0; pp < A; ++pp) t += Q[pp][pp].x;
    const bool ok = t > 0.f;  // uniform: every lane formed the same sum
    if (ok && capon) {
      const float load = loading * (t / (float)A);
      for (int it = lane; it < MA * MA; it += 64) {
        const int pp = it / MA, qq = it % MA;
        float2 v = Q[pp][qq];
        if (pp == qq && pp < A) v.x += load;
        Lm[pp][qq] = v;
      }
      __syncthreads();
      // Cholesky, left-looking: lane i owns row i; column j needs columns < j of rows i and j
      for (int j = 0; j < A; ++j) {
        if (lane >= j && lane < A) {
          float d = Lm[j][j].x;
          for (int k = 0; k < j; ++k) {
            const float2 a = Lm[j][k];
            d -= a.x * a.x + a.y * a.y;
          }
          const float ljj = sqrtf(d);
          float2 v;
          if (lane == j) {
            v = make_float2(ljj, 0.f);
          } else {
            float2 s = Lm[lane][j];
            for (int k = 0; k < j; ++k) {  // s -= L[i][k] conj(L[j][k])
              const float2 a = Lm[lane][k], b = Lm[j][k];
              s.x -= a.x * b.x + a.y * b.y;
              s.y -= a.y * b.x - a.x * b.y;
            }
            v = make_float2(s.x / ljj, s.y / ljj);
          }
          // one wave: every lane's reads of R_l[j][j] and of the columns < j above precede this store in program
          // order, and column j of another row is not read before the barrier
          Lm[lane][j] = v;
        }
        __syncthreads();
      }
      // T = L^-1, lane c owns column c: T[c][c] = 1 / L[c][c], T[i][c] = -(sum_{c <= k < i} L[i][k] T[k][c]) / L[i][i]
      if (lane < A) {
        const int cc = lane;
        Tm[cc][cc] = make_float2(1.f / Lm[cc][cc].x, 0.f);
        for (int ii = cc + 1; ii < A; ++ii) {
          float sr = 0.f, si = 0.f;
          for (int k = cc; k < ii; ++k) {
            const float2 a = Lm[ii][k], b = Tm[k][cc];
            sr += a.x * b.x - a.y * b.y;
            si += a.x * b.y + a.y * b.x;
          }
          const float d = Lm[ii][ii].x;
          Tm[ii][cc] = make_float2(-sr / d, -si / d);
        }
      }
      __syncthreads();
      // Q = T^H T: Q[p][q] = sum_{k >= q} conj(T[k][p]) T[k][q] for p <= q, and its mirror
      for (int it = lane; it < A * A; it += 64) {
        const int pp = it / A, qq = it - pp * A;
        if (pp <= qq) {
          float sr = 0.f, si = 0.f;
          for (int k = qq; k < A; ++k) {
            const float2 a = Tm[k][pp], b = Tm[k][qq];
            sr += a.x * b.x + a.y * b.y;
            si += a.x * b.y - a.y * b.x;
          }
          if (pp == qq) si = 0.f;
          Q[pp][qq] = make_float2(sr, si);
          Q[qq][pp] = make_float2(sr, -si);
        }
      }
      __syncthreads();
    }
    float best = -INFINITY;
    int bi = INT_MAX;
    float* out = map + (size_t)row * G;
    for (int g = lane; g < G; g += 64) {
      float val = 0.f;
      if (ok) {
        float2 a[MA];
#pragma unroll
        for (int q = 0; q < MA; ++q) a[q] = q < A ? steer[(size_t)g * A + q] : make_float2(0.f, 0.f);
        float y = 0.f;
#pragma unroll
        for (int pp = 0; pp < MA; ++pp) {
          if (pp < A) {  // uniform
            float wr = 0.f, wi = 0.f;
#pragma unroll
            for (int q = pp + 1; q < MA; ++q) {
              const float2 m = Q[pp][q];
              wr += m.x * a[q].x - m.y * a[q].y;
              wi += m.x * a[q].y + m.y * a[q].x;
            }
            const float off = a[pp].x * wr + a[pp].y * wi;  // Re conj(a_p) w
            y += Q[pp][pp].x * (a[pp].x * a[pp].x + a[pp].y * a[pp].y) + 2.f * off;
          }
        }
        val = capon ? 1.f / y : y * scale;
      }
      out[g] = val;
      if (val > best) {
        best = val;
        bi = g;
      }
    }
    if (arg) {
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        const float ob = __shfl_xor(best, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (ob > best || (ob == best && oi < bi)) {
          best = ob;
          bi = oi;
        }
      }
      if (lane == 0) arg[row] = (ok && bi != INT_MAX) ? bi : 0;
    }
  }
}

hipError_t launch_range_azimuth(hipStream_t st, const float2* cov, long long n, int A, const float2* steer, int G,
                                int capon, float loading, float* map, int* arg) {
  if (n <= 0) return hipSuccess;
  const long long blocks = n < 65536 ? n : 65536;  // one wave per row; more rows are walked with the grid's stride
  return launch(st, A <= 8 ? k_range_azimuth<8> : k_range_azimuth<16>, blocks, 64, 0, cov, n, A, steer, G, capon,
                loading, map, arg);
}

}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
