// rsl_doppler_detect.hip — K2 + K3 fused for gfx950: Doppler FFT, fftshift, RDS store and peak detection in one pass
// (dechirp.py:208-271), from c64 `work` rows (k_doppler_detect) or from the packed tiles of rsl_packed.h
// (k_doppler_detect_r128 / _r256 / _r64).  K1 and the plain Doppler FFT are in rsl_fft.hip; the detection rule is in
// rsl_detect_common.h.
// No packed-FP32 VALU in these kernels, as in rsl_fft.hip (the reason is given there).  The device pass
// only: the feature is unknown to the host target.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "rsl_common.h"
#include "rsl_detect_common.h"
#include "rsl_internal.h"
#include "rsl_packed.h"

namespace rsl {

constexpr int kR128Pitch = 128 + 7;      // k_doppler_detect_r128 tile row pitch (float2)
constexpr int kR128Skew = 1;             // ... and the upper halo row's extra offset
// The halo range bin below (side 0) or above (side 1) the KB-bin tile at k0, periodic in S ('reflect' is applied in the
// detect stage).
RSL_DEV int dd_halo_bin(int k0, int KB, int side, int S) {
  const int k = side ? k0 + KB : k0 - 1;
  return k < 0 ? k + S : (k >= S ? k - S : k);
}
// The ablation values the packed K2 kernels forward to dd_tile_compute_reg (6 and 7 act in their own prologue).
constexpr int dd_reg_dbg(int DBG) { return (DBG == 4 || DBG == 5 || DBG == 8 || DBG == 9) ? DBG : 0; }


// Tile body after the LDS fill (and its barrier): Doppler FFT, shifted RDS store, |X|^2 tile, 3x3 detection.
template <int C, int KB, int NT, int DBG>
RSL_DEV void dd_tile_compute(float2* buf, const float2* tws, int S, int k0, unsigned fa, float2* __restrict__ rds,
                             float thr_f, int i_lo, int i_hi, unsigned long long* __restrict__ mask,
                             int* __restrict__ row_count, float* __restrict__ dbmap, float* __restrict__ pk_pow) {
  constexpr int NR = KB + 2;
  constexpr int LD = lp_row(C) | 1;
  constexpr int W = (C + 63) / 64;
  constexpr int PER = (NR * C + NT - 1) / NT;
  const int tid = threadIdx.x;
  if constexpr (DBG != 1) fft_rows<C, NR, NT, LD>(buf, tws, tid);  // DBG 1: no FFT (ablation)
  const int hs = S / 2, hc = C / 2;
  int i0 = k0 + hs;  // shifted row of LDS row 1
  if (i0 >= S) i0 -= S;
  float2* dst = rds + ((size_t)fa * S + i0) * C;
  // one pass over the tile: shifted RDS stores (interior rows) and |X|^2 kept in registers
  float pr[PER];
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int idx = tid + q * NT;
    pr[q] = 0.f;
    if (idx < NR * C) {
      const int r = idx / C, j = idx - r * C;  // j: shifted doppler index
      int d = j - hc;                          // out[j] = X[(j - C//2) mod C]
      if (d < 0) d += C;
      const float2 z = buf[r * LD + lp(d)];
      if (DBG != 2 && r >= 1 && r <= KB) dst[(size_t)(r - 1) * C + j] = z;  // DBG 2: no RDS store
      pr[q] = cabs2(z);
    }
  }
  __syncthreads();
  float* pw = reinterpret_cast<float*>(buf);  // power tile [NR][C], shifted doppler order
#pragma unroll
  for (int q = 0; q < PER; ++q) {
    const int idx = tid + q * NT;
    if (idx < NR * C) pw[idx] = pr[q];
  }
  __syncthreads();
  const int lane = tid & 63, wave = tid >> 6;
  for (int kk = wave; kk < (DBG == 3 ? 0 : KB); kk += NT / 64) {  // DBG 3: no detection
    const int i = i0 + kk;
    const bool gate = (i >= i_lo && i <= i_hi);
    const bool has_up = i > 0, has_dn = i + 1 < S;
    const float* up = pw + kk * C;
    const float* mid = up + C;
    const float* dn = mid + C;
    const size_t row = (size_t)fa * S + i;
    int cnt = 0;
#pragma unroll
    for (int w = 0; w < W; ++w) {
      const int j = w * 64 + lane;
      const bool in = j < C;
      bool pk = false;
      float p = 0.f;
      if (in) {
        p = mid[j];
        const float m = window_max3(up, mid, dn, j, C, has_up, has_dn);  // before the tests: its loads go with p's
        pk = gate && (p > thr_f) && (p >= m);
      }
      detect_store_word(pk, p, in, row, w, W, C, mask, dbmap, pk_pow, cnt);
    }
    detect_store_count(row, cnt, row_count);
  }
}

// Register form of the tile body for C = 64 NCH and KB = 8 NRH with NCH * NRH waves: wave (ch, rh) owns Doppler
// columns 64 ch + lane and interior rows 8 rh + 1 .. 8 rh + 8.  Each lane reads its 10 LDS values once (8 rows +
// halo), stores the shifted RDS rows (coalesced), takes the vertical 3-max in registers and the horizontal one
// from neighbouring lanes (LDS only for the wave-edge columns), and ballots the peaks: no power tile in LDS and
// no 9-read window per cell.  Same decisions as the general body (max is separable: 3x3 max = max of the
// column-wise 3-max over j-1, j, j+1; 'reflect' edges repeat the in-window cell).
template <int C, int KB, int NT>
constexpr bool dd_reg_ok() {
  return C % 64 == 0 && KB % 8 == 0 && (C / 64) * (KB / 8) * 64 == NT && KB * (C / 64) <= 64;
}

// Stores: the shifted RDS rows are non-temporal 8-B stores (coalesced 512-B runs per wave and row; 16-B stores by a
// lane-pair DPP swap measured slower, 1.698 vs 1.677 ms per 1000 cfg2 frames); neighbour lanes and the peak-offset scan
// use DPP (wave_shr / wave_shl, row_shr / row_bcast: K2 3.52 vs 3.76 ms per 2000 cfg2 frames against ds_bpermute);
// the tile's compacted peak powers are staged in the dead LDS tile and stored block-wide (tools/pkb.sh).
// DBG (development builds only, ablations with wrong results): 4 no peak-power stores, 5 no mask / count stores,
// 8 no RDS stores, 9 RDS stores only (no detection).
// LD / PADC: the tile's row pitch and whether columns sit at padded positions lp(d) (the LDS Stockham FFT's layout) or
// at d (k_doppler_detect_r128).
// SKL: the last LDS row (NR - 1 = KB + 1, the upper halo row) starts SKL float2 after its pitch position (a bank skew of
// the caller's row writes; k_doppler_detect_r128).
// HSH: columns d >= C / 2 sit HSH float2 later in their row (k_doppler_detect_r256's bank shift).
template <int C, int KB, int NT, int DBG = 0, int LD = lp_row(C) | 1, bool PADC = true, int SKL = 0, int HSH = 0,
          bool UNI = false>
RSL_DEV void dd_tile_compute_reg(const float2* buf, float* xch, int S, int k0, unsigned fa, float2* __restrict__ rds,
                                 float thr_f, int i_lo, int i_hi, unsigned long long* __restrict__ mask,
                                 int* __restrict__ row_count, float* __restrict__ dbmap,
                                 float* __restrict__ pk_pow, int tid_in = -1) {
  constexpr int NCH = C / 64;
  // tid_in: a laundered thread index from a persistent caller (keeps per-thread addresses out of its tile loop)
  const int tid = tid_in >= 0 ? tid_in : (int)threadIdx.x, lane = tid & 63;
  // UNI: the wave and tile indices are declared wave-uniform (readfirstlane), so the row index i, the range gate and
  // the 'reflect' edge tests below are scalar instead of per-lane compares and selects: 884 -> 796 static VALU in
  // k_doppler_detect_r128, 2.616-2.621 vs 2.640-2.642 ms per 2000 cfg2 frames (one call, outputs identical); in
  // k_doppler_detect_r256 the same change measured slower (1.164 vs 1.144 ms per 100 configs[4] frames), so it is off
  const int wave = UNI ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
  const int ch = wave % NCH, rh = wave / NCH;
  const int j = ch * 64 + lane;  // shifted Doppler column: out[j] = X[(j - C//2) mod C]
  int d = j - C / 2;
  if (d < 0) d += C;
  if constexpr (UNI) {  // tile-uniform (the callers' tile math reaches here as vector values)
    fa = __builtin_amdgcn_readfirstlane(fa);
    k0 = __builtin_amdgcn_readfirstlane(k0);
  }
  int i0 = k0 + S / 2;  // shifted range row of LDS row 1
  if (i0 >= S) i0 -= S;
  const int rb = rh * 8;  // LDS rows rb .. rb + 9; interior rows rb + 1 .. rb + 8
  float p[10];
  const float2* col = buf + (PADC ? lp(d) : d + (d >= C / 2 ? HSH : 0));
  float2* dst = rds + ((size_t)fa * S + i0 + rb) * C + j;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const float2 z = col[(rb + r) * LD + ((SKL != 0 && r == 9 && rb + r == KB + 1) ? SKL : 0)];
    p[r] = cabs2(z);
    if (DBG != 8 && r >= 1 && r <= 8) st8<true>(dst + (size_t)(r - 1) * C, z);  // DBG 8: no RDS stores
  }
  if constexpr (DBG == 9) {  // DBG 9: RDS stores only, no detection
    if (p[0] == 1.2345e30f) mask[tid] = 0ull;
    return;
  }
  float vm[8];
  if (i0 + rb > 0 && i0 + rb + 8 < S) {  // no row of this wave at a shifted range edge (30 of 32 tiles at cfg2)
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) vm[rr] = fmaxf(fmaxf(p[rr], p[rr + 1]), p[rr + 2]);  // v_max3_f32
  } else {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int i = i0 + rb + rr;
      float m = p[rr + 1];
      if (i > 0) m = fmaxf(m, p[rr]);          // 'reflect' at the shifted range edges: no neighbour
      if (i + 1 < S) m = fmaxf(m, p[rr + 2]);
      vm[rr] = m;
    }
  }
  // wave-edge columns for the horizontal neighbours: xch[(rh * 8 + rr) * 2 NCH + 2 ch + {0: lane 0, 1: lane 63}]
  float* ex = xch + (rb + 0) * 2 * NCH;
  if (lane == 0 || lane == 63) {
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) ex[rr * 2 * NCH + 2 * ch + (lane == 63)] = vm[rr];
  }
  __syncthreads();
  unsigned long long* wb = reinterpret_cast<unsigned long long*>(xch + KB * 2 * NCH);  // [KB][NCH] ballots
  bool pkv[8];
  unsigned long long bal[8];  // this wave's ballot word of each of its rows (wave-uniform)
#pragma unroll
  for (int rr = 0; rr < 8; ++rr) {
    // neighbour lanes by DPP wavefront shifts (wave_shr:1 / wave_shl:1, one VALU op each) instead of ds_bpermute
    // round trips through the LDS unit; lanes 0 / 63 take their outside neighbour from the exchange words below
    float l = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(vm[rr]), 0x138, 0xF, 0xF, false));
    float r = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(vm[rr]), 0x130, 0xF, 0xF, false));
    if (lane == 0) l = ch > 0 ? ex[rr * 2 * NCH + 2 * (ch - 1) + 1] : vm[rr];
    if (lane == 63) r = ch + 1 < NCH ? ex[rr * 2 * NCH + 2 * (ch + 1)] : vm[rr];
    const float m = fmaxf(fmaxf(l, vm[rr]), r);
    const int i = i0 + rb + rr;
    const float pc = p[rr + 1];
    const bool pk = (i >= i_lo && i <= i_hi) && (pc > thr_f) && (pc >= m);
    pkv[rr] = pk;
    const unsigned long long b = __ballot(pk);
    bal[rr] = b;
    if (lane == 0) wb[(rb + rr) * NCH + ch] = b;
    if (dbmap) dbmap[((size_t)fa * S + i) * C + j] = 10.f * log10f(pc + 1e-12f);
  }
  __syncthreads();
  // peak powers compact over the tile's KB rows (one contiguous run from the tile's first row slot): an exclusive
  // scan of the tile's KB * NCH <= 64 ballot-word popcounts (one word per lane) gives every word's offset; each row
  // reads its word's offset with one v_readlane (the word index is wave-uniform) and ranks its lanes in its ballot
  const unsigned long long myw = lane < KB * NCH ? wb[lane] : 0ull;
  const int cw = __popcll(myw);
  const int incl = wave_incl_scan(cw);
  const int excl = incl - cw;
  float* tile_pk = pk_pow ? pk_pow + ((size_t)fa * S + i0) * C : nullptr;
  {
    // stage the tile's compacted peak powers in the (now dead) LDS tile, then one block-wide contiguous store of the
    // whole run instead of 8 partial-line stores per wave
    float* stg = reinterpret_cast<float*>(const_cast<float2*>(buf));
    const int total = __builtin_amdgcn_readlane(incl, 63);
#pragma unroll
    for (int rr = 0; rr < 8; ++rr) {
      const int off = __builtin_amdgcn_readlane(excl, (rb + rr) * NCH + ch);
      if (pkv[rr]) stg[off + lanes_below(bal[rr])] = p[rr + 1];
    }
    __syncthreads();
    if (DBG != 4 && tile_pk)
      for (int k = tid; k < total; k += NT) tile_pk[k] = stg[k];
  }
  // the tile's mask words and row counts from the ballots in LDS, one coalesced store each (the tile's shifted rows
  // i0 .. i0 + KB - 1 are contiguous), instead of single-lane stores per row and wave
  if (DBG != 5) {  // DBG 5: no mask / count stores (ablation)
    const size_t row0 = (size_t)fa * S + i0;
    if (tid < KB * NCH) mask[row0 * NCH + tid] = wb[tid];
    if (tid < KB) {
      int cnt = 0;
#pragma unroll
      for (int c = 0; c < NCH; ++c) cnt += __popcll(wb[tid * NCH + c]);
      row_count[row0 + tid] = cnt;
    }
  }
}

// ---------------------------------------------------------------------------------------------
// K2+K3 fused: Doppler FFT, fftshift, RDS store AND peak detection (dechirp.py:208-271) in one pass.
// The block FFTs KB interior range bins plus one halo bin on each side (KB+2 rows), writes the KB shifted
// RDS rows, overwrites the LDS tile with |X|^2, and runs the 3x3 'reflect' local-max test, threshold and
// range gate on the interior rows.  Halo rows are neighbours in shifted range space except across the
// shifted edges i = 0 / S-1, where 'reflect' means "no neighbour".  Saves k_detect's full RDS re-read.
// Requires S % KB == 0 and (S/2) % KB == 0 (each block's shifted rows contiguous).
// ---------------------------------------------------------------------------------------------
template <int C, int KB, int NT, int DBG = 0>
__global__ __launch_bounds__(NT) void k_doppler_detect(const float2* __restrict__ work, int S,
                                                       const float2* __restrict__ tw, float2* __restrict__ rds,
                                                       float thr_f, int i_lo, int i_hi,
                                                       unsigned long long* __restrict__ mask,
                                                       int* __restrict__ row_count, float* __restrict__ dbmap,
                                                       float* __restrict__ pk_pow) {
  constexpr int NR = KB + 2;
  constexpr int LD = lp_row(C) | 1;  // odd: conflict-free transposed (column) writes
  constexpr int PER = (NR * C + NT - 1) / NT;
  extern __shared__ float2 sm[];
  float2* tws = sm;
  float2* buf = sm + C;
  const int tid = threadIdx.x;
  const unsigned nkb = (unsigned)(S / KB);
  // XCD-grouped tile order: neighbouring tiles (which share halo cache lines) meet in one L2
  const unsigned tile = (unsigned)xcd_tile(blockIdx.x, gridDim.x);
  const int kb = (int)(tile % nkb);
  const unsigned fa = tile / nkb;
  const int k0 = kb * KB;
  const float2* src = work + (size_t)fa * C * S;
  // all of the thread's loads in flight before the first LDS write (a rolled loop waits on each load in turn);
  // the twiddles first, so their LDS copy waits only on them
  constexpr int TWP = (C + NT - 1) / NT;
  float2 twv[TWP];
#pragma unroll
  for (int q = 0; q < TWP; ++q)
    if (C % NT == 0 || tid + q * NT < C) twv[q] = tw[tid + q * NT];
  // structured map: thread = (interior range bin ri, chirp slot cs), chirps cs + CS q at a constant stride
  // (one address add per load, 128-B aligned row segments), then the two halo rows spread over all threads
  constexpr int CS = NT / KB;
  constexpr bool STRUCT = (NT % KB == 0) && (C % (NT / KB) == 0) && ((NT / KB) % 8 == 0) && (C / (NT / KB) <= 16);
  if constexpr (STRUCT) {
    constexpr int PI = C / CS, PH = (2 * C + NT - 1) / NT;
    const int ri = tid % KB, cs = tid / KB;
    float2 ld[PI + PH];
    const float2* p = src + (unsigned)(cs * S + k0 + ri);
#pragma unroll
    for (int q = 0; q < PI; ++q) ld[q] = DBG == 6 ? make_float2((float)tid, (float)q) : p[(unsigned)(q * CS * S)];
    int kl = k0 - 1, kh = k0 + KB;  // halo range bins (periodic: reflect is applied in the detect stage)
    if (kl < 0) kl += S;
    if (kh >= S) kh -= S;
#pragma unroll
    for (int h = 0; h < PH; ++h) {
      const int e = tid + h * NT;
      if ((2 * C) % NT == 0 || e < 2 * C) {
        const int side = e / C, c = e - side * C;
        ld[PI + h] = DBG == 6 ? make_float2((float)c, (float)h) : src[(unsigned)(c * S + (side ? kh : kl))];
      }
    }
#pragma unroll
    for (int q = 0; q < TWP; ++q)
      if (C % NT == 0 || tid + q * NT < C) tws[tid + q * NT] = twv[q];
    float2* row = buf + (ri + 1) * LD + lp(cs);
#pragma unroll
    for (int q = 0; q < PI; ++q) row[lp(q * CS)] = ld[q];
#pragma unroll
    for (int h = 0; h < PH; ++h) {
      const int e = tid + h * NT;
      if ((2 * C) % NT == 0 || e < 2 * C) {
        const int side = e / C, c = e - side * C;
        buf[(side ? NR - 1 : 0) * LD + lp(c)] = ld[PI + h];
      }
    }
  } else {
    float2 ld[PER];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int idx = tid + q * NT;
      if ((NR * C) % NT == 0 || idx < NR * C) {
        const int c = idx / NR, r = idx - c * NR;
        int k = k0 - 1 + r;  // unshifted range bin of LDS row r
        k = k < 0 ? k + S : (k >= S ? k - S : k);
        ld[q] = src[(unsigned)(c * S + k)];
      }
    }
#pragma unroll
    for (int q = 0; q < TWP; ++q)
      if (C % NT == 0 || tid + q * NT < C) tws[tid + q * NT] = twv[q];
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int idx = tid + q * NT;
      if ((NR * C) % NT == 0 || idx < NR * C) {
        const int c = idx / NR, r = idx - c * NR;
        buf[r * LD + lp(c)] = ld[q];
      }
    }
  }
  __syncthreads();
  if constexpr (DBG == 7) {  // loads and LDS staging only
    if (buf[tid].x == 1.2345e30f) rds[tid] = buf[tid];
    return;
  }
  if constexpr ((DBG == 0 || DBG >= 4) && dd_reg_ok<C, KB, NT>()) {
    fft_rows<C, NR, NT, LD>(buf, tws, tid);
    dd_tile_compute_reg<C, KB, NT, DBG>(buf, reinterpret_cast<float*>(buf + NR * LD), S, k0, fa, rds, thr_f, i_lo, i_hi,
                                   mask, row_count, dbmap, pk_pow);
  } else {
    dd_tile_compute<C, KB, NT, DBG>(buf, tws, S, k0, fa, rds, thr_f, i_lo, i_hi, mask, row_count, dbmap, pk_pow);
  }
}

// K2 + K3 for C = 128 with packed `work` (the cfg2 shape): the Doppler FFT as 8 x 16 in registers.  K1 stores chirp
// class c (chirps c + 16 r, r < 8) as one packed tile after the first radix-8 step, Y'_c[k1] = W128^(c k1) DFT8_r
// x[c + 16 r] (k_range_fft_r512), so thread (bin b, class c) = (tid % 16, tid / 16) loads the 8 values of its bin
// (3 x 16 B) and
//   exchange: Y' -> xi[c][k1][b] (interior bins, 128 float2 per class) and, from threads 0-31, the two halo bins'
//   values -> xh[c][k1][side] (17 float2 per class);
//   stage 2: thread t < 128 = (k1 = t / 16, b = t % 16) reads xi[c][k1][b], threads 128-143 = (k1, side) read
//   xh[c][k1][side], for c < 16 (consecutive per instruction); X[k1 + 8 k2] = DFT16_c (registers), written to tile row
//   b2 (b + 1, or the halo rows 0 / 17) at the unshifted Doppler position;
// then the register-form detection (dd_tile_compute_reg) as in k_doppler_detect.  X[k1 + 8 k2] = sum_c W128^(c k1)
// W16^(c k2) sum_r x[c + 16 r] W8^(r k1): the 128-point DFT exactly.  Against the LDS Stockham form (staging + two
// stage passes) a third less LDS traffic.  DBG (development builds only): 6 no work loads, 7 loads only.
// LDS banks (MI355X_MICROARCH §LDS; ds_write_b64: 16-lane groups, bank = dword mod 32; ds_read_b64: 32-lane groups,
// dword mod 64): every exchange and stage-2 access is conflict-free.  The tile rows are C + 7 float2 apart (7 b2 mod 16
// distinct over the 16 interior rows of a k1 group) and the upper halo row sits 1 float2 later (the halo group's rows
// 0 and 17 then fill banks 0-15 and 16-31).  Round 4's map (stage-2 thread t = 18 k1 + b2, rows C + 1 apart, halo
// rows inside the exchange) put (k1, 17) and (k1 + 1, 0) on one bank in 7 of the 9 write groups: 112 conflict
// cycles per tile, 28.7 M per 1000 cfg2 frames, the r4n counter's 29.2 M.
template <int DBG = 0>
__global__ __launch_bounds__(256) void k_doppler_detect_r128(const float2* __restrict__ work, float2* __restrict__ rds,
                                                             float thr_f, int i_lo, int i_hi,
                                                             unsigned long long* __restrict__ mask,
                                                             int* __restrict__ row_count, float* __restrict__ dbmap,
                                                             float* __restrict__ pk_pow) {
  // S = 512 wherever this kernel runs (work_packed_supported): the tile index math folds to shifts and masks instead of
  // a runtime 32-bit division (≈ 200 SALU per wave before)
  constexpr int KB = 16, C = 128, S = 512, NT = 16 * KB, NR = KB + 2, NCB = 16;
  constexpr int LD = kR128Pitch, SKL = kR128Skew;
  constexpr int XPI = 8 * KB, XPH = 17;  // exchange float2 per class: interior [k1][b], halo [k1][side] + 1 pad
  static_assert(NCB * (XPI + XPH) <= NR * LD, "exchange buffer must fit in the tile buffer");
  extern __shared__ float2 sm[];
  float2* buf = sm;
  float2* xi = buf;               // exchange, then the tile rows (aliased: a barrier separates the last read from the
  float2* xh = buf + NCB * XPI;   // first write)
  const int tid = threadIdx.x;
  constexpr unsigned nkb = (unsigned)(S / KB);
  const unsigned tile = (unsigned)__builtin_amdgcn_readfirstlane((int)xcd_tile(blockIdx.x, gridDim.x));
  const int b = tid % KB, cls = tid / KB;
  const bool halo = tid < 2 * NCB;  // threads 0-31: (side, class) = (tid / 16, tid % 16)
  const int hside = tid >> 4, hcls = tid & 15;
  const int k0 = (int)(tile % nkb) * KB;
  const unsigned fa = tile / nkb;
  const size_t tile0 = (size_t)fa * NCB;
  // every load issued before the first LDS write
  uint4 wi[3], wh[3];
  pk_load_unit<S, DBG>(work, tile0, k0 + b, cls, wi);
  if (halo) pk_load_unit<S, DBG>(work, tile0, dd_halo_bin(k0, KB, hside, S), hcls, wh);
  if constexpr (DBG == 7) {
    if (__uint_as_float(wi[0].x ^ wh[1].y) == 1.2345e30f) rds[tid] = make_float2((float)wi[1].z, 0.f);
    return;
  }
  // one unit (K1 stored Y'_c[k1] = W128^(c k1) DFT8_r already): decode, write its 8 values (k1 = 0..7) at stride st
  auto stage1 = [&](const uint4(&w)[3], float2* dst, int st) {
    float f[16];
    pk_unpack16(w, f);
#pragma unroll
    for (int k = 0; k < 8; ++k) dst[k * st] = make_float2(f[2 * k], f[2 * k + 1]);
  };
  stage1(wi, xi + cls * XPI + b, KB);
  if (halo) stage1(wh, xh + hcls * XPH + hside, 2);
  __syncthreads();
  // stage 2: DFT16 over the classes
  const bool s2 = tid < 8 * NR;
  const bool hs = tid >= 8 * KB;  // threads 128-143: the halo rows
  const int k1 = hs ? (tid - 8 * KB) >> 1 : tid / KB;
  const int b2 = hs ? ((tid & 1) ? NR - 1 : 0) : (tid % KB) + 1;
  float2 x[16];
  if (s2) {
    const float2* src = hs ? xh + 2 * k1 + (tid & 1) : xi + tid;
    const int cs = hs ? XPH : XPI;
#pragma unroll
    for (int c = 0; c < 16; ++c) x[c] = src[c * cs];
    Dft<16>::run(x);
  }
  __syncthreads();  // exchange reads done: the tile rows alias it
  if (s2) {
    float2* row = buf + b2 * LD + (b2 == NR - 1 ? SKL : 0);
#pragma unroll
    for (int k2 = 0; k2 < 16; ++k2) row[k1 + 8 * k2] = x[k2];
  }
  __syncthreads();
  dd_tile_compute_reg<C, KB, NT, dd_reg_dbg(DBG), LD, false, SKL, 0, true>(
      buf, reinterpret_cast<float*>(buf + NR * LD), S, k0, fa, rds, thr_f, i_lo, i_hi, mask, row_count, dbmap, pk_pow);
}

// K2 + K3 for C = 256, S = 1024 with packed `work` (the configs[4] shape; K1 = k_range_fft_r1024): the Doppler FFT
// as 8 x 32.  K1 stored chirp class c (chirps c + 32 r, r < 8) after the radix-8 step, Y'_c[k1] = W256^(c k1) DFT8_r,
// so thread (bin b, class c) = (tid % 16, tid / 16) loads its bin's unit (3 x 16 B) and
//   exchange: Y' -> xi[c][(16 k1 + b) ^ 16 (c & 1)] (interior bins) and, from threads 0-63, the halo bins' values
//   -> xh[c][(2 k1 + side) ^ (c & 15)];
//   stage 2: lane (k1, b2, h) takes the classes c = 2 i + h: E or O = DFT16_i (registers), then the lane pair (h = 0, 1)
//   forms X[k1 + 8 k'] = E + W32^k' O and X[k1 + 8 (k' + 16)] = E - W32^k' O by one DPP swap (as K1's radix-2 step at
//   S = 512); 256 lanes for the 16 interior bins, 32 for the two halo bins;
//   tile rows: X -> row b2 at the unshifted Doppler position d, columns d >= 128 one float2 later (HSH = 1) and the
//   upper halo row 1 float2 later (SKL): every exchange and row access is bank-conflict-free except the halo rows';
// then the register-form detection (dd_tile_compute_reg, 16 rows x 4 column waves).  X[k1 + 8 k2] = sum_c W256^(c k1)
// W32^(c k2) sum_r x[c + 32 r] W8^(r k1): the 256-point DFT exactly.  16 bins x 256 chirps on 512 threads, 37 KiB of
// LDS: 4 workgroups (32 waves) per CU.  DBG (development builds only): 6 no work loads, 7 loads only.
constexpr int kR256Pitch = 258;  // tile row pitch (float2): 256 columns + the HSH shift + 1 (516 b2 = 4 b2 mod 32 dwords)
// upper halo row: 6 float2 later, i.e. at 8 mod 16 positions (2 + 6) from row 0, so that each 16-lane group of the
// halo wave's row writes (k1 of one parity x both sides x both h) covers 16 distinct bank pairs (skew 1 with k1 = u / 4:
// 2- to 3-way on all 16 writes, ~76 of the 7.8 M conflict cycles per tile of 100 configs[4] frames, gpurun_out/r5aa_ddctr5)
constexpr int kR256Skew = 6;
constexpr int kR256Gap = 8;  // float2 between the tile rows (+ the skew's overhang) and the detection exchange words
template <int DBG = 0>
__global__ __launch_bounds__(512) void k_doppler_detect_r256(const float2* __restrict__ work, float2* __restrict__ rds,
                                                             float thr_f, int i_lo, int i_hi,
                                                             unsigned long long* __restrict__ mask,
                                                             int* __restrict__ row_count, float* __restrict__ dbmap,
                                                             float* __restrict__ pk_pow) {
  constexpr int KB = 16, C = 256, S = 1024, NT = 512, NR = KB + 2, NCB = 32;
  constexpr int LD = kR256Pitch, SKL = kR256Skew, HSH = 1;
  constexpr int XPI = 8 * KB, XPH = 16;  // exchange float2 per class: interior [k1][b] (swizzled), halo [k1][side]
  static_assert(NCB * (XPI + XPH) <= NR * LD, "exchange buffer must fit in the tile buffer");
  extern __shared__ float2 sm[];
  float2* buf = sm;
  float2* xi = buf;
  float2* xh = buf + NCB * XPI;
  const int tid = threadIdx.x;
  constexpr unsigned nkb = (unsigned)(S / KB);
  const unsigned tile = (unsigned)xcd_tile(blockIdx.x, gridDim.x);
  const int b = tid % KB, cls = tid / KB;
  const bool halo = tid < 2 * NCB;  // threads 0-63: (side, class) = (tid / 32, tid % 32)
  const int hside = tid >> 5, hcls = tid & 31;
  const int k0 = (int)(tile % nkb) * KB;
  const unsigned fa = tile / nkb;
  const size_t tile0 = (size_t)fa * NCB;
  uint4 wi[3], wh[3] = {};
  pk_load_unit<S, DBG>(work, tile0, k0 + b, cls, wi);
  if (halo) pk_load_unit<S, DBG>(work, tile0, dd_halo_bin(k0, KB, hside, S), hcls, wh);
  if constexpr (DBG == 7) {
    if (__uint_as_float(wi[0].x ^ wh[1].y) == 1.2345e30f) rds[tid] = make_float2((float)wi[1].z, 0.f);
    return;
  }
  {
    float f[16];
    pk_unpack16(wi, f);
    float2* d = xi + cls * XPI;
    const int sw = 16 * (cls & 1);
#pragma unroll
    for (int k = 0; k < 8; ++k) d[(16 * k + b) ^ sw] = make_float2(f[2 * k], f[2 * k + 1]);
  }
  if (halo) {
    float f[16];
    pk_unpack16(wh, f);
    float2* d = xh + hcls * XPH;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[(2 * k + hside) ^ (hcls & 15)] = make_float2(f[2 * k], f[2 * k + 1]);
  }
  __syncthreads();
  // stage 2: DFT32 over the classes as two DFT16 (c = 2 i + h) and one radix-2 step across the lane pair
  const bool s2 = tid < 8 * KB * 2 + 32;
  const bool hs = tid >= 8 * KB * 2;  // threads 256-287: the halo rows
  const int u = tid - 8 * KB * 2;
  const int hh = tid & 1;
  const int k1 = hs ? 2 * ((u >> 2) & 3) + ((u >> 4) & 1) : (tid >> 5);  // halo: one k1 parity per 16-lane group
  const int side = (u >> 1) & 1;
  const int bi = (tid >> 1) & 15;
  const int b2 = hs ? (side ? NR - 1 : 0) : bi + 1;
  float2 x[16];  // defined on the stage-2 lanes only: every use below is under s2
  if (s2) {
    // hs is wave-uniform (waves 0-3: interior lanes only; wave 4: halo lanes 0-31, lanes 32-63 idle): a scalar branch,
    // so that each path's 16 reads are one base address plus immediate offsets instead of both address forms and a
    // select per read
    if (__builtin_amdgcn_readfirstlane((int)hs)) {
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int c = 2 * i + hh;
        x[i] = xh[c * XPH + ((2 * k1 + side) ^ (c & 15))];
      }
    } else {
      const float2* xb = xi + hh * XPI + ((16 * k1 + bi) ^ (16 * hh));
#pragma unroll
      for (int i = 0; i < 16; ++i) x[i] = xb[2 * i * XPI];
    }
    Dft<16>::run(x);
  }
  __syncthreads();  // exchange reads done: the tile rows alias it (each output is written as it forms)
  // the radix-2 step under s2 as a whole: waves 5-7 hold no stage-2 lane and skip it (they issued its ~175 VALU for
  // nothing before); the lane pairs (h = 0, 1) of the DPP swap are both inside or both outside s2
  if (s2) {
    const float sg = hh ? -1.f : 1.f;
    float2* rw = buf + b2 * LD + (b2 == NR - 1 ? SKL : 0) + k1 + (C / 2 + HSH) * hh;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float2 uu = hh ? cmul(x[k], w32(k)) : x[k];
      float2 r;
      r.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(uu.x), 0xB1, 0xF, 0xF, true));
      r.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(uu.y), 0xB1, 0xF, 0xF, true));
      rw[8 * k] = make_float2(fmaf(sg, uu.x, r.x), fmaf(sg, uu.y, r.y));
    }
  }
  __syncthreads();
  dd_tile_compute_reg<C, KB, NT, dd_reg_dbg(DBG), LD, false, SKL, HSH>(
      buf, reinterpret_cast<float*>(buf + NR * LD + kR256Gap), S, k0, fa, rds, thr_f, i_lo, i_hi, mask, row_count, dbmap, pk_pow);
}

// K2 + K3 for C = 64, S = 256 with packed `work` (the cfg1 shape; K1 = k_range_fft_r256): the Doppler FFT as 8 x 8.
// K1 stored chirp class c (chirps c + 8 r, r < 8) after the radix-8 step, Y'_c[k1] = W64^(c k1) DFT8_r, so thread
// (bin b, class c) = (tid % 32, tid / 32) loads its bin's unit (3 x 16 B) and decodes it into xi[c][k1][b] (every 16th
// thread a halo unit into xh[c][k1][side]); lane (k1, b) then takes X[k1 + 8 k2] = DFT8_c (registers) for its interior
// bin and threads 0-15 the halo bins' transforms, each written to its tile row (rows C + 1 apart: conflict-free); the
// register-form detection (one column wave x 4 row quarters) follows.  32 bins x 64 chirps on 256 threads, 18 KiB LDS.
template <int DBG = 0>
__global__ __launch_bounds__(256) void k_doppler_detect_r64(const float2* __restrict__ work, float2* __restrict__ rds,
                                                            float thr_f, int i_lo, int i_hi,
                                                            unsigned long long* __restrict__ mask,
                                                            int* __restrict__ row_count, float* __restrict__ dbmap,
                                                            float* __restrict__ pk_pow) {
  constexpr int KB = 32, C = 64, S = 256, NT = 256, NR = KB + 2, NCB = 8;
  constexpr int LD = C + 1;
  constexpr int XPI = 8 * KB, XPH = 16;  // exchange float2 per class: interior [k1][b], halo [k1][side]
  static_assert(NCB * (XPI + XPH) <= NR * LD, "exchange buffer must fit in the tile buffer");
  extern __shared__ float2 sm[];
  float2* buf = sm;
  float2* xi = buf;
  float2* xh = buf + NCB * XPI;
  const int tid = threadIdx.x;
  constexpr unsigned nkb = (unsigned)(S / KB);
  const unsigned tile = (unsigned)xcd_tile(blockIdx.x, gridDim.x);
  const int b = tid % KB, cls = tid / KB;
  const bool halo = (tid & 15) == 0;  // 16 halo units, one per 16 threads: (side, class) = (h / 8, h % 8), h = tid / 16
  const int hside = tid >> 7, hcls = (tid >> 4) & 7;
  const int k0 = (int)(tile % nkb) * KB;
  const unsigned fa = tile / nkb;
  const size_t tile0 = (size_t)fa * NCB;
  uint4 wi[3], wh[3] = {};
  pk_load_unit<S, DBG>(work, tile0, k0 + b, cls, wi);
  if (halo) pk_load_unit<S, DBG>(work, tile0, dd_halo_bin(k0, KB, hside, S), hcls, wh);
  {
    float f[16];
    pk_unpack16(wi, f);
    float2* d = xi + cls * XPI + b;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k * KB] = make_float2(f[2 * k], f[2 * k + 1]);
  }
  if (halo) {
    float f[16];
    pk_unpack16(wh, f);
    float2* d = xh + hcls * XPH + hside;
#pragma unroll
    for (int k = 0; k < 8; ++k) d[2 * k] = make_float2(f[2 * k], f[2 * k + 1]);
  }
  __syncthreads();
  // stage 2: DFT8 over the classes; lane (k1, b) = (tid / 32, tid % 32) for the interior bins, threads 0-15 also
  // (k1, side) = (tid / 2, tid % 2) for the halo bins
  const int k1 = tid / KB;
  float2 x[8], y[8] = {};
#pragma unroll
  for (int c = 0; c < 8; ++c) x[c] = xi[c * XPI + k1 * KB + b];
  Dft<8>::run(x);
  const bool hs = tid < 16;
  const int hk1 = tid >> 1, hsd = tid & 1;
  if (hs) {
#pragma unroll
    for (int c = 0; c < 8; ++c) y[c] = xh[c * XPH + 2 * hk1 + hsd];
    Dft<8>::run(y);
  }
  __syncthreads();  // exchange reads done: the tile rows alias it
  {
    float2* rw = buf + (b + 1) * LD + k1;
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) rw[8 * k2] = x[k2];
  }
  if (hs) {
    float2* rw = buf + (hsd ? NR - 1 : 0) * LD + hk1;
#pragma unroll
    for (int k2 = 0; k2 < 8; ++k2) rw[8 * k2] = y[k2];
  }
  __syncthreads();
  dd_tile_compute_reg<C, KB, NT, dd_reg_dbg(DBG), LD, false>(
      buf, reinterpret_cast<float*>(buf + NR * LD), S, k0, fa, rds, thr_f, i_lo, i_hi, mask, row_count, dbmap, pk_pow);
}

// The K2 half of the packed shapes (work_packed_supported), by C (S = 4 C; the K1 half is PackedK1 in rsl_fft.hip): tiles
// of KB range bins on NT2 threads, their rows in kRows2 bytes of dynamic LDS.  k2() gives the kernel: the product one
// or, in development builds, the ablation variant that RSL_DD_DBG names (results are wrong).
using K2Fn = void (*)(const float2*, float2*, float, int, int, unsigned long long*, int*, float*, float*);
template <int C>
struct PackedK2;
// cfg2: 16 range bins per tile (2.59 ms per 2000 cfg2 frames against 2.67 for 32 on 512 threads, and 3.10 for two
// tiles per workgroup; round 3); the upper halo row is skewed inside its pitch: with the detection exchange area
// 19,952 B of LDS, 8 workgroups per CU
template <>
struct PackedK2<128> {
  static constexpr int KB = 16, NT2 = 256;
  static constexpr size_t kRows2 = sizeof(float2) * (KB + 2) * kR128Pitch;
  static K2Fn k2() {
#ifdef RSL_DEV_KNOBS
    switch (dev_knob("RSL_DD_DBG")) {
      case 4: return k_doppler_detect_r128<4>;
      case 5: return k_doppler_detect_r128<5>;
      case 6: return k_doppler_detect_r128<6>;
      case 7: return k_doppler_detect_r128<7>;
      case 8: return k_doppler_detect_r128<8>;
      case 9: return k_doppler_detect_r128<9>;
    }
#endif
    return k_doppler_detect_r128<>;
  }
};
// configs[4]
template <>
struct PackedK2<256> {
  static constexpr int KB = 16, NT2 = 512;
  static constexpr size_t kRows2 = sizeof(float2) * ((KB + 2) * kR256Pitch + kR256Gap);
  static K2Fn k2() {
#ifdef RSL_DEV_KNOBS
    switch (dev_knob("RSL_DD_DBG")) {
      case 6: return k_doppler_detect_r256<6>;
      case 7: return k_doppler_detect_r256<7>;
      case 8: return k_doppler_detect_r256<8>;
    }
#endif
    return k_doppler_detect_r256<>;
  }
};
// cfg1
template <>
struct PackedK2<64> {
  static constexpr int KB = 32, NT2 = 256;
  static constexpr size_t kRows2 = sizeof(float2) * (KB + 2) * (64 + 1);
  static K2Fn k2() {
#ifdef RSL_DEV_KNOBS
    switch (dev_knob("RSL_DD_DBG")) {
      case 6: return k_doppler_detect_r64<6>;
      case 8: return k_doppler_detect_r64<8>;
    }
#endif
    return k_doppler_detect_r64<>;
  }
};

// K2 + K3 on packed work: one workgroup per tile of KB range bins.
template <int C>
static hipError_t launch_k2d_packed(hipStream_t st, const float2* work, int F, int A, int S, float2* rds,
                                    const DetectArgs& d, int* pk_group) {
  using P = PackedK2<C>;
  static_assert(dd_reg_ok<C, P::KB, P::NT2>(), "register tile body shape");
  if (S != 4 * C) return hipErrorInvalidValue;  // the kernel's tile math is compiled for its S
  const long ntile = (long)F * A * (S / P::KB);
  // the tile rows + the register body's exchange area (edge columns and ballots: 16 B per row per 64 columns)
  const size_t lds = P::kRows2 + (size_t)P::KB * (C / 64) * 16;
  const K2Fn kern = P::k2();
  *pk_group = P::KB;  // tile-compact peak powers (dd_tile_compute_reg)
  return launch(st, kern, ntile, P::NT2, lds, work, rds, threshold_as_float(d.thr_p), d.i_lo, d.i_hi, d.mask,
                d.row_count, d.dbmap, d.pk_pow);
}

template <int C, int KB>
static hipError_t launch_k2d_kb(hipStream_t st, const float2* work, int F, int A, int S, const float2* tw,
                                float2* rds, const DetectArgs& d, int* pk_group) {
  constexpr int NT = 256;
  const long ntile = (long)F * A * (S / KB);
  // padded LDS rows (plain rows measured slower: 2.14 vs 1.98 ms per 1000 cfg2 frames) + the register body's exchange
  // area (edge columns and ballots: 16 B per row per 64 columns)
  const size_t lds = sizeof(float2) * (C + (size_t)(KB + 2) * (lp_row(C) | 1)) + (size_t)KB * (C / 64) * 16;
  // One tile per workgroup, 256 threads.  Measured and not kept: a persistent variant with a register prefetch of the
  // next tile (5.0-5.25 vs 3.85 ms per 2000 cfg2 frames), a 320-thread block (2.72 vs 2.48 ms per 1000 frames).
  auto kern = k_doppler_detect<C, KB, NT>;
#ifdef RSL_DEV_KNOBS
  // ablation variants (development builds only; results are wrong); any other value keeps the product kernel
  (void)with_int<1, 2, 3, 4, 5, 6, 7>(dev_knob("RSL_DD_DBG"), [&](auto v) {
    kern = k_doppler_detect<C, KB, NT, decltype(v)::value>;
    return hipSuccess;
  });
#endif
  // tile-compact peak powers from the register tile body (KB rows per group), row-compact from the general body
  *pk_group = dd_reg_ok<C, KB, NT>() ? KB : 1;
  return launch(st, kern, ntile, NT, lds, work, S, tw, rds, threshold_as_float(d.thr_p), d.i_lo, d.i_hi, d.mask,
                d.row_count, d.dbmap, d.pk_pow);
}

// range bins per Doppler/detect tile: ~20 KiB tiles (KB 16 at C = 128: 2.42 ms vs KB 32: 3.23 ms per 1000 cfg2
// frames; more resident workgroups hide the per-tile load -> FFT -> store phases), rows_for(C) where that does not
// tile S / 2
static int dd_kb(int C, int S) {
  int kb = 2048 / C < 1 ? 1 : 2048 / C;
  if (kb > rows_for(C) || (S / 2) % kb != 0 || S % kb != 0) kb = rows_for(C);
  return kb;
}

template <int C>
static hipError_t launch_k2d(hipStream_t st, const float2* work, int F, int A, int S, const float2* tw, float2* rds,
                             const DetectArgs& d, int* pk_group, bool packed) {
  if constexpr (C == 64 || C == 128 || C == 256) {
    if (packed) return launch_k2d_packed<C>(st, work, F, A, S, rds, d, pk_group);
  }
  constexpr int K0 = rows_for(C);
  constexpr int K1 = (2048 / C) < 1 ? 1 : (2048 / C) > K0 ? K0 : (2048 / C);
  if (dd_kb(C, S) == K1)
    return launch_k2d_kb<C, K1>(st, work, F, A, S, tw, rds, d, pk_group);
  return launch_k2d_kb<C, K0>(st, work, F, A, S, tw, rds, d, pk_group);
}

// Packed `work` between K1 and K2 (pk_pack16): the K1 tile holds one bin pair per thread and the K2 tile one (bin,
// chirp class) per thread, at the three shapes with register-form kernels: S = 512, C = 128 (k_range_fft_r512,
// k_doppler_detect_r128), S = 1024, C = 256 (k_range_fft_r1024, k_doppler_detect_r256) and S = 256, C = 64
// (k_range_fft_r256, k_doppler_detect_r64).  Development builds:
// RSL_WORK_C64=1 keeps c64 rows (A/B).
bool work_packed_supported(int C, int S) {
  if (dev_knob("RSL_WORK_C64") != 0) return false;
  return ((S == 512 && C == 128) || (S == 1024 && C == 256) || (S == 256 && C == 64)) &&
         doppler_detect_supported(C, S);
}

bool doppler_detect_supported(int C, int S) {
  if (!fft_supported(C) || (C & (C - 1)) != 0 || C < 8 || C > 1024 || (S & 1)) return false;  // LDS <= 64 KiB
  const int KB = dd_kb(C, S);
  return S % KB == 0 && (S / 2) % KB == 0;
}

hipError_t launch_doppler_detect(hipStream_t st, const float2* work, int F, int A, int C, int S, const float2* tw_C,
                                 float2* rds, const DetectArgs& det, int* pk_group, bool packed) {
  *pk_group = 1;
  if (!doppler_detect_supported(C, S)) return hipErrorInvalidValue;
  if (F <= 0 || A <= 0) return hipSuccess;
  switch (C) {
#define CASE(n) \
  case n:       \
    return launch_k2d<n>(st, work, F, A, S, tw_C, rds, det, pk_group, packed);
    CASE(8) CASE(16) CASE(32) CASE(64) CASE(128) CASE(256) CASE(512) CASE(1024)
#undef CASE
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
