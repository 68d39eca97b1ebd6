// rsl_cfar.hip — 2-D cell-averaging CFAR peak detection for gfx950 (rsl_detect_cfar, include/rsl.h).
//
// A second detector next to k_detect (rsl_detect.hip), with the same outputs: per-antenna 64-bit ballot masks, row
// counts, the optional dB map and the row-compact peak powers, so offsets / emit and everything after run unchanged.
// Cell (i, j) of a (frame, antenna) power map p = |rds|^2 [S, C] is a peak iff
//   p * n(i) > alpha * sum   (sum over the training cells: |di| <= hr, |dj| <= hd without the guard box |di| <= gr,
//                             |dj| <= gd; Doppler wraps, range truncates, n(i) = the cells that exist)
//   and p >= every existing 3x3 neighbour (k_detect's rule, rsl_detect_common.h), i_lo <= i <= i_hi, p > thr_f.
//
// The training sum is formed by additions only (a cell 100 dB above its neighbours makes "box minus guard box" or a
// subtracting sliding window wrong by more than the whole noise sum): per row the side sum HS[j] (gd < |dj| <= hd) and
// the full sum HF[j] = HS[j] + centre sum (|dj| <= gd), then sum = HF over the rows gr < |di| <= hr plus HS over the
// rows |di| <= gr.  At most 33 * 33 - 1 = 1088 fp32 additions of non-negative terms: relative error < 1088 * 2^-24 =
// 6.5e-5.
//
// One workgroup walks a strip of R range rows of one map (the window, the strip walk and the launcher are the CFAR
// family's, rsl_cfar_common.h), RB rows per step, three phases per step:
//   A  load RB rows, power to a small LDS ring PW (RB + 2 rows, with the wrapped Doppler halo copied to both ends);
//   B  HS / HF of the new rows into LDS rings of NR = RB + hr + max(hr, 1) rows; the 3x3 local-maximum ballots of the
//      rows one behind into MX (64 bits per mask word);
//   C  the rows whose last training row has arrived: vertical sum from the rings, decision, ballots, outputs (the
//      cell's own power is re-read from the RDS, a row the same workgroup streamed hr + RB rows earlier).
// The RDS is read (R + 2 max(hr, 1)) / R times for the window (1.16 at R = 128, hr = 10) plus the re-read of phase C.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "../../include/rsl.h"
#include "rsl_cfar_common.h"

namespace rsl {

namespace {

// LDS bytes of k_detect_cfar with RB rows per step: HF + HS rings, the power ring, the local-maximum words
constexpr size_t cfar_lds_bytes(int C, CfarWindow win, int RB) {
  const size_t NR = (size_t)RB + win.hr() + win.hh(), NP = (size_t)RB + 2, W = ((size_t)C + 63) / 64;
  return 4 * (2 * NR * C + NP * ((size_t)C + 2 * win.hd())) + 8 * NR * W;
}
// Monotone in C, hr and hd, so every window that rsl_detect_cfar admits fits at the launcher's smallest RB.
static_assert(cfar_lds_bytes(RSL_CFAR_MAX_C, CfarWindow{0, 0, RSL_CFAR_MAX_HALF, RSL_CFAR_MAX_HALF}, 4) <= kCfarLdsMax,
              "the largest CA-CFAR window must fit the LDS of a CU");

}  // namespace

// T: the map's element, float2 (c64 RDS, p = |z|^2) or float (a power map, rsl_detect_power): cell_power.
template <class T>
__global__ __launch_bounds__(256) void k_detect_cfar(const T* __restrict__ rds, int S, int C, int W,
                                                     CfarWindow win, float alpha, float thr_f, int i_lo, int i_hi,
                                                     int R, int RB,
                                                     unsigned long long* __restrict__ mask,
                                                     int* __restrict__ row_count, float* __restrict__ dbmap,
                                                     float* __restrict__ pk_pow) {
  extern __shared__ float cf_lds[];
  const int gr = win.gr, gd = win.gd, hr = win.hr(), hd = win.hd(), hh = win.hh();
  const int NR = RB + hr + hh, NP = RB + 2, PS = C + 2 * hd;
  float* HF = cf_lds;               // [NR][C]  row sums over |dj| <= hd
  float* HS = HF + (size_t)NR * C;  // [NR][C]  row sums over gd < |dj| <= hd
  float* PW = HS + (size_t)NR * C;  // [NP][PS] power rows, hd wrapped cells on both sides (-1: row outside the map)
  unsigned long long* MX = reinterpret_cast<unsigned long long*>(PW + (size_t)NP * PS);  // [NR][W] 3x3 maxima

  const CfarStrip sp = cfar_strip(S, R);
  const size_t fa = sp.fa;
  const int i0 = sp.i0, Re = sp.Re;
  const int UL = Re + 2 * hh;  // rows the strip loads: u = 0 .. UL-1 is range row ibase + u
  const int ibase = i0 - hh;
  const T* base = rds + fa * S * C;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

  int done = hh;  // next row (u) to decide
  for (int uk = 0; uk < UL; uk += RB) {
    // A: powers of the step's rows
    power_rows_halo(PW, NP, PS, base, ibase, uk + wave, min(uk + RB, UL), S, C, hd, -1.f);
    __syncthreads();
    // B: row sums of the step's rows (rows of the map only)
    for (int r = wave; r < RB; r += 4) {
      const int u = uk + r;
      if (u >= UL) break;
      const int i = ibase + u;
      if (i < 0 || i >= S) continue;
      const float* pr = PW + (size_t)(u % NP) * PS + hd;
      float* hf = HF + (size_t)(u % NR) * C;
      float* hs = HS + (size_t)(u % NR) * C;
      for (int j = lane; j < C; j += 64) {
        float sl = 0.f, sr = 0.f;
        for (int k = gd + 1; k <= hd; ++k) {
          sl += pr[j - k];
          sr += pr[j + k];
        }
        float c = pr[j];
        for (int k = 1; k <= gd; ++k) c += pr[j - k] + pr[j + k];
        const float s = sl + sr;
        hs[j] = s;
        hf[j] = s + c;
      }
    }
    // B: 3x3 local maxima of the rows one behind the step (both neighbour rows are in the ring), output rows only
    for (int r = wave; r < RB; r += 4) {
      const int u = uk - 1 + r;
      if (u < hh || u >= hh + Re) continue;
      const float* up = PW + (size_t)((u - 1) % NP) * PS + hd;
      const float* mid = PW + (size_t)(u % NP) * PS + hd;
      const float* dn = PW + (size_t)((u + 1) % NP) * PS + hd;
      const int i = ibase + u;
      for (int w = 0; w < W; ++w) {
        const int j = w * 64 + lane;
        const bool pk = j < C && mid[j] >= window_max3(up, mid, dn, j, C, i > 0, i + 1 < S);
        const unsigned long long b = __ballot(pk);
        if (lane == 0) MX[(size_t)(u % NR) * W + w] = b;
      }
    }
    __syncthreads();
    // C: decide the rows whose window is complete
    const int loaded = min(uk + RB, UL);
    const int end = min(loaded - hh, hh + Re);
    for (int u = done + wave; u < end; u += 4) {
      const int i = ibase + u;
      const size_t orow = fa * S + i;
      const bool gate = (i >= i_lo && i <= i_hi);
      const float fn = (float)win.cells(i, S);  // n(i), exact in fp32 (<= 1088)
      const int dlo = -min(i, hr), dhi = min(S - 1 - i, hr);
      int cnt = 0;
      for (int w = 0; w < W; ++w) {
        const int j = w * 64 + lane;
        const unsigned long long mx = MX[(size_t)(u % NR) * W + w];
        const bool in = j < C;
        float p = 0.f;
        if (in && (dbmap || (gate && mx))) p = cell_power(base[(size_t)i * C + j]);
        bool pk = false;
        if (gate && mx && in) {  // gate, mx: wave-uniform
          float s = 0.f;
          int slot = (u + dlo) % NR;
          for (int di = dlo; di <= dhi; ++di) {
            const float* src = (di >= -gr && di <= gr) ? HS : HF;
            s += src[(size_t)slot * C + j];
            if (++slot == NR) slot = 0;
          }
          pk = ((mx >> lane) & 1ull) && (p * fn > alpha * s) && (p > thr_f);
        }
        detect_store_word(pk, p, in, orow, w, W, C, mask, dbmap, pk_pow, cnt);
      }
      detect_store_count(orow, cnt, row_count);
    }
    if (end > done) done = end;
  }
}

hipError_t launch_detect_cfar(hipStream_t st, const float2* rds, int F, int A, int S, int C, CfarWindow win,
                              float alpha, const DetectArgs& d) {
  return launch_cfar_strips(st, k_detect_cfar<float2>, cfar_lds_bytes, rds, F, A, S, C, win, d, alpha);
}

hipError_t launch_detect_cfar(hipStream_t st, const float* power, int F, int S, int C, CfarWindow win, float alpha,
                              const DetectArgs& d) {
  return launch_cfar_strips(st, k_detect_cfar<float>, cfar_lds_bytes, power, F, 1, S, C, win, d, alpha);
}

}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
