// rsl_oscfar.hip — 2-D ordered-statistic CFAR peak detection for gfx950 (rsl_detect_oscfar, include/rsl.h).
//
// The companion of k_detect_cfar (rsl_cfar.hip) with the same window, outputs and 3x3 rule, and the k-th smallest
// training cell in place of their mean.  Cell (i, j) of a (frame, antenna) power map p = |rds|^2 [S, C] is a peak iff
//   #{training cells q : alpha * q < p} >= k(i)      (<=> p > fl32(alpha * x_(k(i))): no sort, the count is exact and
//                                                      independent of the order in which the cells are visited)
//   and p >= every existing 3x3 neighbour (rsl_detect_common.h), i_lo <= i <= i_hi, p > thr_f,
// with k(i) = min(n(i), max(1, ceil(rank * n(i)))) in fp64, n(i) the training cells that exist for range row i.
//
// One workgroup walks a strip of R range rows of one map (cfar_strip, rsl_cfar_common.h, which also holds the window
// and the family's launcher), RB rows per step.  A ring PW of RB + 2 hh (hh = max(hr, 1)) fp32 power rows in LDS holds
// the whole window of every row it decides, each row with the wrapped Doppler halo on both ends; a row outside the map
// holds +inf, which is never below p, so range truncation needs no test in the count.  Per step, for the rows whose
// last window row has arrived:
//   1  gate: the cells that pass the 3x3 test, the range gate and the floor (about 1/9 of the cells in noise) are
//      compacted into an LDS list (ballot, one LDS atomic per 64-cell word);
//   2  count: one WAVE per candidate.  The lanes split the N training cells through a table of their ring offsets
//      (built once per workgroup, the guard box left out), 64 compares per pass, summed by ballot + popcount; a
//      candidate that reaches its row's k(i) sets its bit in the step's result words.  What a candidate needs besides
//      (ring slot, column, k) is wave-uniform and computed once per row in phase 1.  The count stops as soon as the
//      cells left cannot change the decision, which rejects a noise maximum after a little over half its window;
//   3  outputs of the step's rows from the result words and the ring (the RDS is read once).
// A wave per candidate keeps every lane busy whatever the candidate count (a step of 16 rows x 64 columns holds about
// 110 candidates, fewer than the workgroup has lanes), reads the ring in runs of 2 hd + 1 consecutive floats (no bank
// conflict inside a window row) and needs no divergent loop.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include <cmath>

#include "../../include/rsl.h"
#include "rsl_cfar_common.h"

namespace rsl {

namespace {

// LDS bytes of k_detect_oscfar with RB rows per step: the power ring (padded to 8 B), the result words, the
// candidate list, its count and the rows' ranks, the offset table
constexpr size_t oscfar_lds_bytes(int C, CfarWindow win, int RB) {
  const size_t NP = (size_t)RB + 2 * win.hh(), PS = (size_t)C + 2 * win.hd(), W = ((size_t)C + 63) / 64;
  const size_t box = (size_t)(2 * win.hr() + 1) * win.nfull();
  return 8 * ((NP * PS + 1) / 2) + 8 * RB * W + 4 * ((size_t)RB * C + 1 + RB) + 4 * box;
}
// Monotone in C, hr and hd, so every window that rsl_detect_oscfar admits fits at the launcher's smallest RB.
static_assert(oscfar_lds_bytes(RSL_CFAR_MAX_C, CfarWindow{0, 0, RSL_CFAR_MAX_HALF, RSL_CFAR_MAX_HALF}, 4) <=
                  kCfarLdsMax,
              "the largest OS-CFAR window must fit the LDS of a CU");

// A float of the power ring by its byte offset (the ring starts the workgroup's LDS).
RSL_DEV float ring_at(const float* PW, unsigned byte_off) {
  return *reinterpret_cast<const float*>(reinterpret_cast<const char*>(PW) + byte_off);
}

}  // namespace

// T: the map's element, float2 (c64 RDS, p = |z|^2) or float (a power map, rsl_detect_power): cell_power.
template <class T>
__global__ __launch_bounds__(256) void k_detect_oscfar(const T* __restrict__ rds, int S, int C, int W,
                                                       CfarWindow win, double rank, float alpha, float thr_f,
                                                       int i_lo, int i_hi, int R, int RB,
                                                       unsigned long long* __restrict__ mask,
                                                       int* __restrict__ row_count, float* __restrict__ dbmap,
                                                       float* __restrict__ pk_pow) {
  extern __shared__ unsigned long long os_lds[];
  const int gr = win.gr, tr = win.tr, td = win.td, hr = win.hr(), hd = win.hd(), hh = win.hh();
  const int NP = RB + 2 * hh, PS = C + 2 * hd;
  const int nfull = win.nfull(), nguard = win.nguard();
  const int box = (2 * hr + 1) * nfull, N = box - (2 * gr + 1) * nguard;  // full-window training cells
  float* PW = reinterpret_cast<float*>(os_lds);                  // [NP][PS] power rows (+inf: row outside the map)
  unsigned long long* RES = os_lds + ((size_t)NP * PS + 1) / 2;  // [RB][W] decisions of the step's rows
  int* CL = reinterpret_cast<int*>(RES + (size_t)RB * W);  // [RB * C] candidates: ring slot << 13 | step row << 9 | j
  int* NC = CL + (size_t)RB * C;                           // candidates of the step
  int* KR = NC + 1;                                        // [RB] k(i) of the step's rows
  unsigned* OFF = reinterpret_cast<unsigned*>(KR + RB);    // [N] ring byte offset 4 (di PS + dj) of a training cell

  const CfarStrip sp = cfar_strip(S, R);
  const size_t fa = sp.fa;
  const int Re = sp.Re;
  const int UL = Re + 2 * hh;  // rows the strip loads: u = 0 .. UL-1 is range row ibase + u
  const int ibase = sp.i0 - hh;
  const T* base = rds + fa * S * C;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const unsigned ringb = 4u * NP * PS;

  // offsets of the training cells from the window's first cell (row u - hr, column j - hd), row-major, guard box out:
  // cell t of the box lands at t minus the guard cells before it
  for (int t = threadIdx.x; t < box; t += 256) {
    const int di = t / nfull, dj = t - di * nfull;
    const int gi = di - tr, gj = dj - td;  // position inside the guard box where 0 <= gi <= 2 gr, 0 <= gj < nguard
    const bool row_in = gi >= 0 && gi <= 2 * gr;
    if (row_in && gj >= 0 && gj < nguard) continue;
    const int before = min(max(gi, 0), 2 * gr + 1) * nguard + (row_in ? min(max(gj, 0), nguard) : 0);
    OFF[t - before] = 4u * (di * PS + dj);
  }

  int done = hh;  // next row (u) to decide
  for (int uk = 0; uk < UL; uk += RB) {
    // powers of the step's rows
    power_rows_halo(PW, NP, PS, base, ibase, uk + wave, min(uk + RB, UL), S, C, hd, INFINITY);
    if (threadIdx.x == 0) *NC = 0;
    __syncthreads();
    const int loaded = min(uk + RB, UL);
    const int end = min(loaded - hh, hh + Re);
    if (end <= done) continue;  // the first window is not complete yet (workgroup-uniform)
    const int nb = end - done;  // <= RB rows, whose windows u - hh .. u + hh are all in the ring

    // 1: candidates
    for (int r = wave; r < nb; r += 4) {
      const int u = done + r, i = ibase + u, slot = u % NP;
      const float* up = PW + (size_t)((u - 1) % NP) * PS + hd;
      const float* mid = PW + (size_t)slot * PS + hd;
      const float* dn = PW + (size_t)((u + 1) % NP) * PS + hd;
      const bool gate = (i >= i_lo && i <= i_hi);
      if (lane == 0) {  // the row's rank
        const int n = win.cells(i, S);
        KR[r] = min(n, max(1, (int)ceil(rank * (double)n)));
      }
      for (int w = 0; w < W; ++w) {
        const int j = w * 64 + lane;
        bool cand = false;
        if (gate && j < C) {
          const float p = mid[j];
          cand = p >= window_max3(up, mid, dn, j, C, i > 0, i + 1 < S) && p > thr_f;
        }
        const unsigned long long b = __ballot(cand);
        if (lane == 0) RES[(size_t)r * W + w] = 0ull;
        if (b) {
          int at = 0;
          if (lane == 0) at = atomicAdd(NC, __popcll(b));
          at = __builtin_amdgcn_readfirstlane(at);
          if (cand) CL[at + lanes_below(b)] = (slot << 13) | (r << 9) | j;
        }
      }
    }
    __syncthreads();

    // 2: one wave per candidate counts the training cells below p / alpha
    const int ncand = *NC;
    for (int c = wave; c < ncand; c += 4) {
      const int e = __builtin_amdgcn_readfirstlane(CL[c]);
      const int j = e & 511, r = (e >> 9) & 15, slot = e >> 13;
      const float p = PW[slot * PS + hd + j];
      const int ws = slot - hr + (slot < hr ? NP : 0);  // ring slot of the window's first row, u - hr (u >= hh >= hr)
      const unsigned a0 = 4u * (ws * PS + j);           // ... and the byte offset of its first cell
      const unsigned* off = OFF + lane;
      const int k = __builtin_amdgcn_readfirstlane(KR[r]);
      // The count stops once the cells left cannot change the decision (below >= k, or below + the rest < k): in
      // noise a 3x3 maximum has about a third of its window below p / alpha and is rejected after the first trip.
      int below = 0, t0 = 0;
      for (; t0 + 256 <= N && below < k && below + (N - t0) >= k; t0 += 256) {  // four passes of 64 cells in flight
#pragma unroll
        for (int m = 0; m < 4; ++m) {
          const unsigned a = a0 + off[t0 + 64 * m];
          below += __popcll(__ballot(alpha * ring_at(PW, min(a, a - ringb)) < p));  // a < 2 ringb: at most one wrap
        }
      }
      for (; t0 < N && below < k && below + (N - t0) >= k; t0 += 64) {  // the tail: a lane past N does not count
        const int t = t0 + lane;
        const unsigned a = a0 + OFF[min(t, N - 1)];
        below += __popcll(__ballot(t < N && alpha * ring_at(PW, min(a, a - ringb)) < p));
      }
      if (lane == 0 && below >= k) atomicOr(&RES[(size_t)r * W + (j >> 6)], 1ull << (j & 63));
    }
    __syncthreads();

    // 3: outputs
    for (int r = wave; r < nb; r += 4) {
      const int u = done + r;
      const size_t orow = fa * S + (ibase + u);
      const float* mid = PW + (size_t)(u % NP) * PS + hd;
      int cnt = 0;
      for (int w = 0; w < W; ++w) {
        const int j = w * 64 + lane;
        const bool in = j < C;
        const float p = in ? mid[j] : 0.f;
        const bool pk = in && ((RES[(size_t)r * W + w] >> lane) & 1ull);
        detect_store_word(pk, p, in, orow, w, W, C, mask, dbmap, pk_pow, cnt);
      }
      detect_store_count(orow, cnt, row_count);
    }
    done = end;
    __syncthreads();  // the next step overwrites the oldest RB rows of the ring
  }
}

hipError_t launch_detect_oscfar(hipStream_t st, const float2* rds, int F, int A, int S, int C, CfarWindow win,
                                double rank, float alpha, const DetectArgs& d) {
  return launch_cfar_strips(st, k_detect_oscfar<float2>, oscfar_lds_bytes, rds, F, A, S, C, win, d, rank, alpha);
}

hipError_t launch_detect_oscfar(hipStream_t st, const float* power, int F, int S, int C, CfarWindow win, double rank,
                                float alpha, const DetectArgs& d) {
  return launch_cfar_strips(st, k_detect_oscfar<float>, oscfar_lds_bytes, power, F, 1, S, C, win, d, rank, alpha);
}

}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
