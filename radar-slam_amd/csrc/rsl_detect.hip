// rsl_detect.hip — K3 peak detection and order-preserving compaction for gfx950.
//
// Replaces SignalPreprocessor.extract_range_doppler_peaks (reference src/radar_signal/dechirp.py:215-278):
//   db = 10 log10(|rds|^2 + 1e-12); peak = (maximum_filter(db, 3, mode='reflect') == db) & (db > thr)
//   & (min_range <= range_m[i] <= max_range); peaks listed antenna -> range -> doppler (np.where order).
// The 3x3 test runs on fp32 power p (log10 is monotone); 'reflect' boundary duplicates the edge cell,
// so out-of-range neighbours simply do not take part (rsl_detect_common.h).  The threshold 10^(thr/10) - 1e-12 and the
// range gate, an index interval, are precomputed in fp64.
// Per-antenna 64-bit ballots give one mask word per 64 Doppler cells; a per-frame scan then turns
// row counts into entry offsets (antenna-major) and union-cell offsets (range-major), and the emit
// kernel writes both lists in reference order without any sort.
// Two emit paths (emit_compact_supported, rsl_internal.h, chooses):
//   compact (k_emit_cells + k_emit_entries, launch_emit_compact): from the masks, the union mask and the peak powers,
//     power_db = 10 log10f of the stored fp32 peak power; where W = ceil(C / 64) is a power of two <= 64, the union
//     mask is given, and peak_pow is given or no power_db is wanted.  The chain runs this one.
//   general (k_emit, launch_emit_rows): one wave per range row, power_db rounded from a double-precision log10 of the
//     RDS power; every other case: W not a power of two or above 64, no union mask, or power_db wanted without
//     peak_pow.  The last is the drop-in extract_range_doppler_peaks, whose power_db bits depend on it.
#include "rsl_common.h"
#include "rsl_detect_common.h"
#include "rsl_internal.h"

namespace rsl {

constexpr int kDetRows = 16;  // shifted range rows per workgroup (fewer at large C: detect_rows)

// The largest float t <= thr: for a float p, (double)p > thr  <=>  p > t.
float threshold_as_float(double thr) {
  float t = (float)thr;
  if ((double)t > thr) t = nextafterf(t, -INFINITY);
  return t;
}

// T: the map's element, float2 (c64 RDS, p = |z|^2) or float (a power map, rsl_detect_power): cell_power.
// rows: the workgroup's shifted range rows (detect_rows); the decisions do not depend on it.
template <class T>
__global__ __launch_bounds__(256) void k_detect(const T* __restrict__ rds, int S, int C, int W, int rows, float thr_f,
                                                int i_lo, int i_hi, unsigned long long* __restrict__ mask,
                                                int* __restrict__ row_count, float* __restrict__ dbmap,
                                                float* __restrict__ pk_pow) {
  extern __shared__ float pw[];  // (rows + 2) x C power values
  const int nib = (S + rows - 1) / rows;
  const int ib = blockIdx.x % nib;
  const long fa = blockIdx.x / nib;
  const int i0 = ib * rows;
  const int nrows = min(rows, S - i0);
  const T* base = rds + (size_t)fa * S * C;
  for (int idx = threadIdx.x; idx < (nrows + 2) * C; idx += 256) {
    const int r = idx / C, j = idx - r * C;
    const int i = i0 - 1 + r;
    pw[idx] = (i >= 0 && i < S) ? cell_power(base[(size_t)i * C + j]) : -1.f;  // outside the map: never read
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = wave; r < nrows; r += 4) {
    const int i = i0 + r;
    const bool gate = (i >= i_lo && i <= i_hi);
    const float* up = pw + r * C;
    const float* mid = up + C;
    const float* dn = mid + C;
    const size_t row = (size_t)fa * S + i;
    int cnt = 0;
    for (int w = 0; w < W; ++w) {
      const int j = w * 64 + lane;
      const bool in = j < C;
      float p = 0.f;
      bool pk = false;
      if (in) {
        p = mid[j];
        const float m = window_max3(up, mid, dn, j, C, i > 0, i + 1 < S);  // before the tests: its loads go with p's
        pk = gate && (p > thr_f) && (p >= m);
      }
      detect_store_word(pk, p, in, row, w, W, C, mask, dbmap, pk_pow, cnt);
    }
    detect_store_count(row, cnt, row_count);
  }
}

// Exclusive scan of one value per thread over an NT-thread block (a wave scan + one LDS round over the NT / 64 wave
// sums in lds); *total = the block's sum.  A caller that scans again through the same lds puts a barrier in between.
// Every thread of the block must call it.
template <class T, int NT>
RSL_DEV T block_exscan(T v, T* lds, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T inc;
  if constexpr (sizeof(T) == 4) {
    inc = wave_incl_scan(v);  // DPP
  } else {
    inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const T u = __shfl_up(inc, d);
      if (lane >= d) inc += u;
    }
  }
  if (lane == 63) lds[w] = inc;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NT / 64; ++k) {
    const T x = lds[k];
    if (k < w) base += x;
    tot += x;
  }
  *total = tot;
  return base + inc - v;
}

// Exclusive scan of n ints (global) into out (global) by one NT-thread block; returns total.
template <int NT>
__device__ long long block_scan_global(const int* in, int* out, int n, long long* lds) {
  const int t = threadIdx.x;
  const int per = (n + NT - 1) / NT;
  const int b = t * per, e = min(n, b + per);
  long long total;
  if (per % 4 == 0 && n % per == 0 && ((reinterpret_cast<size_t>(in) | reinterpret_cast<size_t>(out)) & 15) == 0) {
    // whole 16-B runs per thread (e.g. the A * S = 4096 row counts of a cfg2 frame: 4 int4 per thread, each thread's
    // 64-B segment read and written by 16-B accesses instead of 16 lane-strided 4-B ones)
    const int4* in4 = reinterpret_cast<const int4*>(in);
    int4* out4 = reinterpret_cast<int4*>(out);
    const int q0 = b >> 2, nq = (e - b) >> 2;
    int4 v[8];
    long long s = 0;
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q < nq) {
        v[q] = in4[q0 + q];
        s += (long long)v[q].x + v[q].y + v[q].z + v[q].w;
      }
    for (int q = 8; q < nq; ++q) {  // long runs (per > 32): a second pass over the rest
      const int4 x = in4[q0 + q];
      s += (long long)x.x + x.y + x.z + x.w;
    }
    long long run = block_exscan<long long, NT>(s, lds, &total);
    auto put = [&](int q, const int4& x) {
      int4 o;
      o.x = (int)run; run += x.x;
      o.y = (int)run; run += x.y;
      o.z = (int)run; run += x.z;
      o.w = (int)run; run += x.w;
      out4[q0 + q] = o;
    };
#pragma unroll
    for (int q = 0; q < 8; ++q)
      if (q < nq) put(q, v[q]);
    for (int q = 8; q < nq; ++q) put(q, in4[q0 + q]);
    return total;
  }
  long long s = 0;
  for (int k = b; k < e; ++k) s += in[k];
  long long run = block_exscan<long long, NT>(s, lds, &total);
  for (int k = b; k < e; ++k) {
    const int v = in[k];
    out[k] = (int)run;
    run += v;
  }
  return total;
}

// One block per frame: entry offsets over (antenna, range) rows and union-cell offsets over range rows.  NT = 256:
// small blocks get CU slots between the long-lived DoA blocks of the other batch in the pipelined chain (a 1024-thread
// block waits for a whole CU to drain).
template <int NT>
__global__ __launch_bounds__(NT) void k_offsets(const unsigned long long* __restrict__ mask,
                                                const int* __restrict__ row_count, int A, int S, int W,
                                                int* __restrict__ entry_row_off, int* __restrict__ cell_row_off,
                                                int* __restrict__ cell_row_cnt, long long* __restrict__ frame_counts,
                                                unsigned long long* __restrict__ umask) {
  __shared__ long long lds[NT / 64];
  const long f = blockIdx.x;
  const long long te = block_scan_global<NT>(row_count + f * A * S, entry_row_off + f * A * S, A * S, lds);
  const unsigned long long* mf = mask + (size_t)f * A * S * W;
  if (W == 2) {  // C = 65..128 (cfg2): a row's two words as one 16-B load / store
    const ulonglong2* mf2 = reinterpret_cast<const ulonglong2*>(mf);
    ulonglong2* um2 = umask ? reinterpret_cast<ulonglong2*>(umask + (size_t)f * S * 2) : nullptr;
    for (int i = threadIdx.x; i < S; i += NT) {
      ulonglong2 u = make_ulonglong2(0ull, 0ull);
#pragma unroll 8
      for (int a = 0; a < A; ++a) {
        const ulonglong2 x = mf2[(size_t)a * S + i];
        u.x |= x.x;
        u.y |= x.y;
      }
      if (um2) um2[i] = u;
      cell_row_cnt[f * S + i] = __popcll(u.x) + __popcll(u.y);
    }
  } else
  for (int i = threadIdx.x; i < S; i += NT) {
    int c = 0;
    for (int w = 0; w < W; ++w) {
      unsigned long long u = 0;
      for (int a = 0; a < A; ++a) u |= mf[((size_t)a * S + i) * W + w];
      c += __popcll(u);
      if (umask) umask[((size_t)f * S + i) * W + w] = u;
    }
    cell_row_cnt[f * S + i] = c;
  }
  __syncthreads();
  const long long tc = block_scan_global<NT>(cell_row_cnt + f * S, cell_row_off + f * S, S, lds);
  if (threadIdx.x == 0) {
    frame_counts[2 * f] = te;
    frame_counts[2 * f + 1] = tc;
  }
}

// One block: exclusive scan over frames -> entry_base[F+1], cell_base[F+1].
template <int NT>
__global__ __launch_bounds__(NT) void k_frame_scan(const long long* __restrict__ frame_counts, int F,
                                                   long long* __restrict__ entry_base,
                                                   long long* __restrict__ cell_base) {
  __shared__ long long lds[NT / 64];
  const int t = threadIdx.x;
  const int per = (F + NT - 1) / NT;
  const int b = t * per, e = min(F, b + per);
  long long se = 0, sc = 0;
  for (int k = b; k < e; ++k) {
    se += frame_counts[2 * k];
    sc += frame_counts[2 * k + 1];
  }
  long long tot_e, tot_c;
  long long re = block_exscan<long long, NT>(se, lds, &tot_e);
  __syncthreads();  // lds is reused
  long long rc = block_exscan<long long, NT>(sc, lds, &tot_c);
  for (int k = b; k < e; ++k) {
    entry_base[k] = re;
    cell_base[k] = rc;
    re += frame_counts[2 * k];
    rc += frame_counts[2 * k + 1];
  }
  if (t == 0) {
    entry_base[F] = tot_e;
    cell_base[F] = tot_c;
  }
}

// One wave per (frame, range row): lane j of word w owns Doppler cell 64 w + j.  Ranks inside a word are
// popcounts of the lower lanes' bits, so every entry/cell index is computed without serial loops and the
// per-entry stores and RDS reads (power_db) are coalesced across the wave.
__global__ __launch_bounds__(256) void k_emit(const float2* __restrict__ rds, const unsigned long long* __restrict__ mask,
                                              int F, int A, int S, int C, int W,
                                              const int* __restrict__ entry_row_off, const int* __restrict__ cell_row_off,
                                              const long long* __restrict__ entry_base,
                                              const long long* __restrict__ cell_base, long long entry_cap,
                                              long long cell_cap, unsigned* __restrict__ e_coord,
                                              int* __restrict__ e_cell, float* __restrict__ e_pdb,
                                              int* __restrict__ c_frame,
                                              int* __restrict__ c_rc, unsigned* __restrict__ c_amask) {
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);  // f * S + i
  if (row >= (long)F * S) return;
  const int lane = threadIdx.x & 63;
  const long f = row / S;
  const int i = (int)(row - f * S);
  const unsigned long long* mf = mask + (size_t)f * A * S * W;
  const float2* rf = rds + (size_t)f * A * S * C;
  long long cnext = cell_base[f] + cell_row_off[row];
  const long long e0 = entry_base[f];
  for (int w = 0; w < W; ++w) {
    unsigned long long u = 0;
    for (int a = 0; a < A; ++a) u |= mf[((size_t)a * S + i) * W + w];
    if (u == 0) continue;  // wave-uniform
    const int j = w * 64 + lane;
    const bool has = (u >> lane) & 1ull;
    const long long c = cnext + lanes_below(u);
    unsigned am = 0;
    for (int a = 0; a < A; ++a) {
      const unsigned long long m = mf[((size_t)a * S + i) * W + w];
      if (!m) continue;  // wave-uniform
      const bool hb = (m >> lane) & 1ull;
      if (hb) {
        am |= 1u << a;
        const unsigned long long* mrow = mf + ((size_t)a * S + i) * W;
        long long e = e0 + entry_row_off[(size_t)f * A * S + (size_t)a * S + i] + lanes_below(m);
        for (int ww = 0; ww < w; ++ww) e += __popcll(mrow[ww]);
        if (e < entry_cap) {
          e_coord[e] = ((unsigned)a << 26) | ((unsigned)i << 13) | (unsigned)j;
          e_cell[e] = (int)c;
          if (e_pdb) {
            const float p = cabs2(rf[((size_t)a * S + i) * C + j]);
            e_pdb[e] = (float)(10.0 * log10((double)p + 1e-12));
          }
        }
      }
    }
    if (has && c < cell_cap) {
      c_frame[c] = (int)f;
      c_rc[c] = i * C + j;
      c_amask[c] = am;
    }
    cnext += __popcll(u);
  }
}

// Stream compaction of the peak bit masks into the entry list: 256 consecutive mask words per block produce one
// contiguous run of entries.  Phase 1: per-word popcounts, a block scan, and one packed (word, bit) code per item in
// LDS.  Phase 2: item k of the block is written by lane k % 256, so every store instruction is coalesced
// (consecutive lanes -> consecutive addresses); scattered 4-byte stores from a per-word set-bit loop would cost
// one memory request per lane.  Entries follow dechirp.py:257 (np.where order: antenna -> range -> doppler).
// power_db comes from the detector's compacted peak powers (pk_group rows per group, 1 = row-compact; no RDS
// re-read), 10 log10 in fp32 (the powers are fp32).  A block with more than kEmitCap items runs phases 1-2 in rounds of
// kEmitCap.
constexpr int kEmitCap = 2048;
constexpr int kEmitU = 4;  // phase-2 items per lane per trip

// Registers capped for 8 waves per SIMD (44 VGPRs, no spill; 14 KiB of LDS).  The cells are k_emit_cells' work: this
// kernel holds no antenna masks, neither in LDS nor in registers.
// (Non-temporal entry stores were measured slower: 0.53 vs 0.48 ms per 1000 cfg2 frames.)
template <int W>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8))) void k_emit_entries(
    const unsigned long long* __restrict__ mask, const unsigned long long* __restrict__ umask,
    const float* __restrict__ pk_pow, int pk_group, long long F, int A, int S, int C,
    const int* __restrict__ entry_row_off, const int* __restrict__ cell_row_off,
    const long long* __restrict__ entry_base, const long long* __restrict__ cell_base, long long entry_cap,
    unsigned* __restrict__ e_coord, int* __restrict__ e_cell, float* __restrict__ e_pdb) {
  static_assert(64 % W == 0, "a mask row must lie within one wave");
  __shared__ unsigned pk[kEmitCap];  // item code: (word << 6) | bit
  __shared__ int wsum[4];
  __shared__ int s_cw[256], s_fi[256];
  __shared__ long long s_pkb[256];  // peak_pow index of the word's item 0 minus its block rank
  __shared__ unsigned long long s_u[256];
  __shared__ long long s_first;
  const int t = threadIdx.x, lane = t & 63;
  const long long nw = F * A * S * W;
  const long long gw0 = (long long)blockIdx.x * 256;  // row-aligned
  const bool valid = gw0 + t < nw;
  const long long gw = valid ? gw0 + t : gw0;  // past-the-end words alias the block's first word (then m = 0)
  // word -> (row, w), row = (f*A + a)*S + i  (divisions once per word)
  const long long row = gw / W;
  const int w = (int)(gw - row * W);
  const long long q = row / S;  // f*A + a
  const int i = (int)(row - q * S);
  const long long f = q / A;
  const int a = (int)(q - f * A);
  // every global load of the word is issued here, independent of its value (one memory round trip)
  unsigned long long m = mask[gw];
  long long fst = 0;  // thread 0: the block's first item index (the block starts a row: no earlier words)
  if (t == 0) fst = entry_base[f] + entry_row_off[row];
  int gof = 0;  // peaks of the earlier rows of the row's peak_pow group
  const int ig = i - i % pk_group;
  if (ig != i) gof = entry_row_off[row] - entry_row_off[row - (i - ig)];
  const unsigned long long* urow = umask + ((size_t)f * S + i) * W;
  const unsigned long long u = urow[w];  // the union word of (f, i, w)
  const long long cwb = cell_base[f] + cell_row_off[f * S + i];
  int cwo = 0;
#pragma unroll
  for (int ww = 0; ww < W; ++ww)
    if (ww < w) cwo += __popcll(urow[ww]);
  if (!valid) m = 0;
  const int cnt = __popcll(m);
  int total;
  const int loc = block_exscan<int, 256>(cnt, wsum, &total);
  // peaks of the earlier words of this row (the row's words are lanes lane-w .. lane of this wave)
  const int r0 = loc - __shfl(loc, lane - w);
  if (t == 0) s_first = fst;
  s_cw[t] = (int)(cwb + cwo);
  s_u[t] = u;
  s_fi[t] = (a << 16) | i;
  // the row's group starts at row - i % pk_group; item k of the block reads peak_pow[s_pkb + base + k] (divisions once
  // per word instead of 64-bit divisions per item)
  s_pkb[t] = (row - i % pk_group) * (long long)C + (r0 + gof) - loc;
  // rounds of kEmitCap items (one round unless the block is dense)
  for (int base = 0; base < total; base += kEmitCap) {
    // phase 1: packed (word, bit) codes of this round's items, in LDS
    if (loc < base + kEmitCap && loc + cnt > base) {
      unsigned long long mm = m;
      int o = loc;
      while (mm && o < base + kEmitCap) {
        const int b = __ffsll((long long)mm) - 1;
        mm &= mm - 1;
        if (o >= base) pk[o - base] = ((unsigned)t << 6) | (unsigned)b;
        ++o;
      }
    }
    __syncthreads();
    const long long first = s_first + base;
    const int nk = total - base < kEmitCap ? total - base : kEmitCap;
    // phase 2: coalesced stores, lane k % 256 writes item k; kEmitU items per trip with their peak-power
    // gathers issued first (a rolled loop waits on each gather in turn)
    for (int k0 = t; k0 < nk; k0 += 256 * kEmitU) {
      float pw[kEmitU];
#pragma unroll
      for (int uu = 0; uu < kEmitU; ++uu) {
        const int k = k0 + 256 * uu;
        pw[uu] = 0.f;
        if (k < nk && e_pdb) {
          pw[uu] = pk_pow[s_pkb[pk[k] >> 6] + base + k];
        }
      }
#pragma unroll
      for (int uu = 0; uu < kEmitU; ++uu) {
        const int k = k0 + 256 * uu;
        const long long e = first + k;
        if (k < nk && e < entry_cap) {
          const unsigned code = pk[k];
          const int tt = (int)(code >> 6), b = (int)(code & 63);
          const int ww = (int)((gw0 + tt) % W);
          const int ai = s_fi[tt];
          e_coord[e] = ((unsigned)(ai >> 16) << 26) | ((unsigned)(ai & 0xffff) << 13) | (unsigned)(ww * 64 + b);
          e_cell[e] = s_cw[tt] + __popcll(s_u[tt] & ((1ull << b) - 1ull));
          if (e_pdb) e_pdb[e] = 10.0f * log10f(pw[uu] + 1e-12f);  // dechirp.py:235-236
        }
      }
    }
    __syncthreads();  // pk reused by the next round
  }
}

// Cell-list compaction (union masks, ~54 % dense at cfg2; cells are range-major unions over antennas): 4 threads per
// mask word (16-bit slices), 64 words per block, so every block's items (at most 4096) are expanded in one round and no
// thread walks more than 16 set bits.  Each frame has its own nbf = ceil(S * W / 64) blocks, the last one partly filled
// where 64 does not divide S * W: a block lies in one frame and starts a row (64 % W == 0), so it writes one contiguous
// run of cells from cell_base[f] + the row's offset, and every index below is a 32-bit word index within the frame.
constexpr int kCellWords = 64;
constexpr int kCellCap = kCellWords * 64;

template <int W, int MAXA>
__global__ __launch_bounds__(256) void k_emit_cells(const unsigned long long* __restrict__ mask,
                                                    const unsigned long long* __restrict__ umask, int nbf, int A,
                                                    int S, int C, const int* __restrict__ cell_row_off,
                                                    const long long* __restrict__ cell_base, long long cell_cap,
                                                    int* __restrict__ c_frame, int* __restrict__ c_rc,
                                                    unsigned* __restrict__ c_amask) {
  static_assert(kCellWords % W == 0, "a block must start a row");
  // item code (thread << 4) | bit within the thread's 16-bit slice (12 bits); for MAXA <= 16 the cell's antenna mask
  // is packed above it (16 KiB of LDS instead of 32: 5 workgroups per CU instead of 4)
  constexpr bool PACK = MAXA <= 16;
  __shared__ unsigned pk[kCellCap];
  __shared__ unsigned pam[PACK ? 1 : kCellCap];
  __shared__ int wsum[4];
  __shared__ long long s_first;
  const int t = threadIdx.x;
  const int f = (int)(blockIdx.x / (unsigned)nbf);
  const int lw0 = (int)(blockIdx.x - (unsigned)f * (unsigned)nbf) * kCellWords;  // the block's first word in the frame
  const int wl = t >> 2, sl = t & 3;
  const bool valid = lw0 + wl < S * W;
  const int lw = valid ? lw0 + wl : lw0;  // past-the-end words load the block's first word and contribute no bits
  const int i = lw / W, w = lw % W;
  unsigned long long m = valid ? umask[(size_t)f * S * W + lw] : 0ull;
  unsigned long long ma[MAXA];
#pragma unroll
  for (int aa = 0; aa < MAXA; ++aa) ma[aa] = aa < A ? mask[(((size_t)f * A + aa) * S + i) * W + w] : 0ull;
  if (t == 0) s_first = cell_base[f] + cell_row_off[(size_t)f * S + i];
  const unsigned sm16 = (unsigned)(m >> (16 * sl)) & 0xffffu;
  unsigned sa[MAXA];  // this thread's 16-bit slice of every antenna's word: 32-bit bit extracts per cell below
#pragma unroll
  for (int aa = 0; aa < MAXA; ++aa) sa[aa] = (unsigned)(ma[aa] >> (16 * sl)) & 0xffffu;
  int total;
  const int loc = block_exscan<int, 256>((int)__popc(sm16), wsum, &total);
  {
    unsigned mm = sm16;
    int o = loc;
    while (mm) {
      const int b = __ffs(mm) - 1;
      mm &= mm - 1;
      unsigned am = 0;
#pragma unroll
      for (int aa = 0; aa < MAXA; ++aa) am |= ((sa[aa] >> b) & 1u) << aa;
      if constexpr (PACK) {
        pk[o] = ((unsigned)t << 4) | (unsigned)b | (am << 12);
      } else {
        pk[o] = ((unsigned)t << 4) | (unsigned)b;
        pam[o] = am;
      }
      ++o;
    }
  }
  __syncthreads();
  const long long first = s_first;
  for (int k = t; k < total; k += 256) {
    const long long e = first + k;
    if (e < cell_cap) {
      const unsigned code = pk[k];
      const int tt = (int)((code >> 4) & 0xffu);
      const int lw2 = lw0 + (tt >> 2);
      c_frame[e] = f;
      c_rc[e] = (lw2 / W) * C + (lw2 % W) * 64 + 16 * (tt & 3) + (int)(code & 15);
      c_amask[e] = PACK ? code >> 12 : pam[k];
    }
  }
}

bool emit_compact_supported(int C, bool union_mask, bool peak_pow, bool want_pdb) {
  const int W = (C + 63) / 64;
  return union_mask && (peak_pow || !want_pdb) && (W & (W - 1)) == 0 && W <= 64;
}

hipError_t launch_emit_compact(hipStream_t st, const unsigned long long* mask, const unsigned long long* umask,
                               const float* pk_pow, int pk_group, int F, int A, int S, int C, const PeakOffsets& off,
                               const PeakLists& out) {
  if (F <= 0) return hipSuccess;
  if (A > 32) return hipErrorInvalidValue;
  const int W = (C + 63) / 64;
  const int nbf = (S * W + kCellWords - 1) / kCellWords;
  const long long nbe = ((long long)F * A * S * W + 255) / 256;
  return with_int<1, 2, 4, 8, 16, 32, 64>(W, [&](auto w) {
    constexpr int WW = decltype(w)::value;
    const auto cells = A <= 8 ? k_emit_cells<WW, 8> : A <= 16 ? k_emit_cells<WW, 16> : k_emit_cells<WW, 32>;
    if (hipError_t e = launch(st, cells, (long long)F * nbf, 256, 0, mask, umask, nbf, A, S, C, off.cell_row_off,
                              off.cell_base, out.cell_cap, out.c_frame, out.c_rc, out.c_amask))
      return e;
    return launch(st, k_emit_entries<WW>, nbe, 256, 0, mask, umask, pk_pow, pk_group, (long long)F, A, S, C,
                  off.entry_row_off, off.cell_row_off, off.entry_base, off.cell_base, out.entry_cap, out.e_coord,
                  out.e_cell, out.e_pdb);
  });
}

// Rows per k_detect workgroup: kDetRows where its (rows + 2) x C power tile fits 64 KiB of LDS (C <= 910), else the
// largest of 8 / 4 / 2 that does (C <= 4096, every length the FFTs produce); 0 where none does.
int detect_rows(int C) {
  for (int r = kDetRows; r >= 2; r /= 2)
    if (sizeof(float) * (r + 2) * (size_t)C <= 64 * 1024) return r;
  return 0;
}

template <class T>
static hipError_t launch_detect_maps(hipStream_t st, const T* maps, int F, int A, int S, int C, const DetectArgs& d) {
  if (F <= 0 || A <= 0 || S <= 0 || C <= 0) return hipSuccess;
  const int W = (C + 63) / 64;
  const int rows = detect_rows(C);
  if (!rows) return hipErrorInvalidValue;
  const long nblk = (long)F * A * ((S + rows - 1) / rows);
  const size_t lds = sizeof(float) * (rows + 2) * (size_t)C;
  return launch(st, k_detect<T>, nblk, 256, lds, maps, S, C, W, rows, threshold_as_float(d.thr_p), d.i_lo, d.i_hi,
                d.mask, d.row_count, d.dbmap, d.pk_pow);
}

hipError_t launch_detect(hipStream_t st, const float2* rds, int F, int A, int S, int C, const DetectArgs& d) {
  return launch_detect_maps(st, rds, F, A, S, C, d);
}

hipError_t launch_detect(hipStream_t st, const float* power, int F, int S, int C, const DetectArgs& d) {
  return launch_detect_maps(st, power, F, 1, S, C, d);
}

hipError_t launch_offsets(hipStream_t st, const unsigned long long* mask, const int* row_count, int F, int A, int S,
                          int C, int* entry_row_off, int* cell_row_off, int* cell_row_cnt, long long* entry_base,
                          long long* cell_base, long long* frame_counts, unsigned long long* umask) {
  if (F <= 0) return hipSuccess;
  const int W = (C + 63) / 64;
  // 256-thread blocks: 1024-thread ones waited for a whole CU to drain behind the other batch's DoA blocks
  if (hipError_t e = launch(st, k_offsets<256>, F, 256, 0, mask, row_count, A, S, W, entry_row_off, cell_row_off,
                            cell_row_cnt, frame_counts, umask))
    return e;
  return launch(st, k_frame_scan<256>, 1, 256, 0, frame_counts, F, entry_base, cell_base);
}

hipError_t launch_emit_rows(hipStream_t st, const float2* rds, const unsigned long long* mask, int F, int A, int S,
                            int C, const PeakOffsets& off, const PeakLists& out) {
  if (F <= 0) return hipSuccess;
  const int W = (C + 63) / 64;
  const long rows = (long)F * S;
  return launch(st, k_emit, (rows + 3) / 4, 256, 0, rds, mask, F, A, S, C, W, off.entry_row_off, off.cell_row_off,
                off.entry_base, off.cell_base, out.entry_cap, out.cell_cap, out.e_coord, out.e_cell, out.e_pdb,
                out.c_frame, out.c_rc, out.c_amask);
}

}  // namespace rsl
