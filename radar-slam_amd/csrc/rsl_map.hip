// rsl_map.hip — the grid map for gfx950 (rsl_map_update, rsl_map_logodds; include/rsl.h is the specification): per-scan
// hit and free-space counts in world coordinates from the frames' point clouds and poses, and the clamped log-odds
// derived from the counts.
//
// k_map_update: one workgroup of 1024 threads per frame.  The (2 Rw + 1)^2 cells around the frame's origin cell are two
// bitmaps in dynamic LDS (hit, free; 2 x 47.9 KB at the default 0.25 m cell and 77 m, above 64 KiB: rsl::launch opts in).
//   1. every accepted point sets its cell's bit in the hit bitmap (LDS atomicOr);
//   2. a wave takes the words of the hit bitmap in turn and, for every set bit, casts the one ray of that cell: the
//      closed form of the integer line makes every step k independent, so the lanes stride k and set the free bits;
//   3. the window's rows inside the map are flushed: lanes take consecutive cells of a row, so a wave's global integer
//      atomicAdds (no return value) are contiguous; a free bit under a hit bit is dropped here (Free = rays \ hits);
//   4. the stats row is the number of bits flushed.
// The planes take integer adds only: every order of frames, launches and ranks gives the same bits.  All coordinate
// arithmetic is fp64 with contraction off (hipcc fuses by default): every product and sum is rounded once in the order
// the specification writes it, so the cells equal those of a numpy restatement bit for bit.
#pragma clang fp contract(off)
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "../../include/rsl.h"
#include "rsl_common.h"
#include "rsl_internal.h"
#include "rsl_launch.h"

namespace rsl {

namespace {

constexpr int kMapThreads = 1024;
constexpr int kMapWaves = kMapThreads / 64;
constexpr int kLogoddsThreads = 256;

}  // namespace

__global__ __launch_bounds__(kMapThreads) void k_map_update(MapProblem p, unsigned* __restrict__ hits,
                                                            unsigned* __restrict__ free_, int* __restrict__ stats) {
  extern __shared__ unsigned map_bits[];  // the hit bitmap, then (with free_) the free bitmap, nw words each
  __shared__ int cnt[3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long f = blockIdx.x;
  const int Rw = p.Rw, W = 2 * Rw + 1, nw = (W * W + 31) >> 5;
  unsigned* hb = map_bits;
  unsigned* fb = map_bits + nw;

  const double* ps = p.poses + f * 7;
  const double px = ps[0], py = ps[1], qw = ps[3], qx = ps[4], qy = ps[5], qz = ps[6];
  const double r00 = 1.0 - 2.0 * (qy * qy + qz * qz), r01 = 2.0 * (qx * qy - qw * qz);
  const double r10 = 2.0 * (qx * qy + qw * qz), r11 = 1.0 - 2.0 * (qx * qx + qz * qz);
  const double gx = (px - p.x0) * p.inv, gy = (py - p.y0) * p.inv;
  const double lim = 1073741824.0;  // 2^30: the origin cell and every cell of its window fit an int
  const bool ok = isfinite(px) && isfinite(py) && isfinite(r00) && isfinite(r01) && isfinite(r10) && isfinite(r11) &&
                  fabs(gx) < lim && fabs(gy) < lim;
  if (!ok) {  // uniform over the workgroup: nobody reaches a barrier
    if (t == 0 && stats) {
      int* s = stats + f * 4;
      s[0] = s[1] = s[2] = 0;
      s[3] = 1;
    }
    return;
  }
  const double oxd = floor(gx), oyd = floor(gy);
  const int ox = (int)oxd, oy = (int)oyd;

  for (int w = t; w < (free_ ? 2 * nw : nw); w += kMapThreads) map_bits[w] = 0u;
  if (t < 3) cnt[t] = 0;
  __syncthreads();

  // 1. hits
  long long b, e;
  cloud_frame(p.cloud, f, b, e);
  int acc = 0;
  for (long long i = b + t; i < e; i += kMapThreads) {
    const float pw = p.cloud.points[i * RSL_POINT_COLS + RSL_POINT_POWER_DB];  // first: one 12-byte load with x, y
    float xf, yf;
    if (!(cloud_point(p.cloud.points, p.cloud.weight, i, xf, yf) > 0.f)) continue;
    if ((double)pw < p.min_db) continue;
    const double x = (double)xf, y = (double)yf;
    const double r2 = x * x + y * y;
    if (!(p.rmin2 <= r2 && r2 <= p.rmax2)) continue;
    const double X = (r00 * x + r01 * y) + px, Y = (r10 * x + r11 * y) + py;
    const double hx = floor((X - p.x0) * p.inv), hy = floor((Y - p.y0) * p.inv);
    if (!(0.0 <= hx && hx < (double)p.nx && 0.0 <= hy && hy < (double)p.ny)) continue;
    const double ddx = hx - oxd, ddy = hy - oyd;  // exact: integers below 2^31
    if (!(fabs(ddx) <= (double)Rw && fabs(ddy) <= (double)Rw)) continue;
    const int bit = ((int)ddy + Rw) * W + ((int)ddx + Rw);
    atomicOr(&hb[bit >> 5], 1u << (bit & 31));
    ++acc;
  }
  __syncthreads();

  // 2. rays: one per set hit bit, from the origin cell up to, not including, the hit cell
  if (free_) {
    for (int w = wave; w < nw; w += kMapWaves) {
      unsigned m = __builtin_amdgcn_readfirstlane(hb[w]);
      while (m) {
        const int bit = w * 32 + __builtin_ctz(m);
        m &= m - 1;
        const int iy = bit / W, ix = bit - iy * W;
        const int ddx = ix - Rw, ddy = iy - Rw;
        const int dx = ddx < 0 ? -ddx : ddx, dy = ddy < 0 ? -ddy : ddy;
        const int sx = ddx >= 0 ? 1 : -1, sy = ddy >= 0 ? 1 : -1;
        const int L = dx > dy ? dx : dy;  // > 0 except for the origin cell itself
        const int lo = dx > dy ? dy : dx;   // the minor extent: the step is (2 k lo + L) div (2 L)
        const float rcp = 1.f / (float)(2 * L);
        for (int k = lane; k < L; k += 64) {
          // the quotient (below 2^9, the numerator below 2^19, exact in fp32) from the reciprocal, then made exact
          const int num = 2 * k * lo + L;
          int q = (int)((float)num * rcp);
          const int r = num - q * 2 * L;
          q += r >= 2 * L ? 1 : (r < 0 ? -1 : 0);
          const int cx = dx >= dy ? sx * k : sx * q, cy = dx >= dy ? sy * q : sy * k;
          const int cb = (cy + Rw) * W + (cx + Rw);
          atomicOr(&fb[cb >> 5], 1u << (cb & 31));
        }
      }
    }
    __syncthreads();
  }

  // 3. flush the window's cells inside the map: a wave per row, lanes on consecutive cells
  const long long wx0 = (long long)ox - Rw, wy0 = (long long)oy - Rw;  // the map cell of window cell (0, 0)
  const int ix_lo = wx0 < 0 ? (int)(-wx0 < W ? -wx0 : W) : 0, iy_lo = wy0 < 0 ? (int)(-wy0 < W ? -wy0 : W) : 0;
  const int ix_hi = (int)(p.nx - wx0 < W ? p.nx - wx0 : W), iy_hi = (int)(p.ny - wy0 < W ? p.ny - wy0 : W);
  int nh = 0, nf = 0;
  for (int iy = iy_lo + wave; iy < iy_hi; iy += kMapWaves) {
    const long long base = (wy0 + iy) * p.nx + wx0;  // base + ix: inside the row for ix_lo <= ix < ix_hi
    for (int ix = ix_lo + lane; ix < ix_hi; ix += 64) {
      const int bit = iy * W + ix;
      const unsigned h = (hb[bit >> 5] >> (bit & 31)) & 1u;
      if (h) {
        __hip_atomic_fetch_add(&hits[base + ix], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++nh;
      } else if (free_ && ((fb[bit >> 5] >> (bit & 31)) & 1u)) {
        __hip_atomic_fetch_add(&free_[base + ix], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ++nf;
      }
    }
  }

  // 4. stats
  if (stats) {
    if (acc) atomicAdd(&cnt[0], acc);
    if (nh) atomicAdd(&cnt[1], nh);
    if (nf) atomicAdd(&cnt[2], nf);
    __syncthreads();
    if (t < 4) stats[f * 4 + t] = t < 3 ? cnt[t] : 0;
  }
}

__global__ __launch_bounds__(kLogoddsThreads) void k_map_logodds(const unsigned* __restrict__ hits,
                                                                 const unsigned* __restrict__ free_, long long ncells,
                                                                 double l_occ, double l_free, double l_min, double l_max,
                                                                 float* __restrict__ out) {
  const long long step = (long long)gridDim.x * kLogoddsThreads;
  for (long long i = (long long)blockIdx.x * kLogoddsThreads + threadIdx.x; i < ncells; i += step) {
    const double occ = (double)hits[i] * l_occ;
    const double fr = free_ ? (double)free_[i] * l_free : 0.0;
    const double v = occ - fr;
    out[i] = (float)(v < l_min ? l_min : (v > l_max ? l_max : v));
  }
}

hipError_t launch_map_update(hipStream_t st, const MapProblem& p, unsigned* hits, unsigned* free_, int* stats) {
  const long long W = 2ll * p.Rw + 1, nw = (W * W + 31) / 32;
  return launch(st, k_map_update, p.cloud.F, kMapThreads, (size_t)nw * 4 * (free_ ? 2 : 1), p, hits, free_, stats);
}

hipError_t launch_map_logodds(hipStream_t st, const unsigned* hits, const unsigned* free_, long long ncells,
                              double l_occ, double l_free, double l_min, double l_max, float* out) {
  long long blocks = (ncells + kLogoddsThreads - 1) / kLogoddsThreads;
  const long long most = 8ll * cu_count();
  if (blocks > most) blocks = most;
  return launch(st, k_map_logodds, blocks, kLogoddsThreads, 0, hits, free_, ncells, l_occ, l_free, l_min, l_max, out);
}

}  // namespace rsl
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
