// rsl_fft.hip — K1 (dechirp*window + range FFT + DC) and K2 (Doppler FFT + fftshift) for gfx950.  K2 fused with the
// detection (K2 + K3) is in rsl_doppler_detect.hip; the packed `work` format between the two in rsl_packed.h.
//
// Replaces SignalPreprocessor.generate_range_doppler_spectrum (reference src/radar_signal/dechirp.py:168-213):
//   per chirp  y = x * conj(ref) * w ; y -= mean(y)      (dechirp.py:156-164)
//   rds = fftshift(fft2(y^T, axes=(1,2)), axes=(1,2))     (dechirp.py:193-211)
// DC removal is folded into the range FFT: FFT(y - mean y)[k] = FFT(y)[k] for k != 0 and 0 for k = 0,
// so the kernel zeroes range bin 0 instead of reducing a mean (exact in real arithmetic).
// conj(ref)*w is precomputed on the host in fp64 (the chirp phase reaches 2.5e7 rad) and passed as a c64 table.
#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <unordered_map>

// No packed-FP32 VALU (v_pk_add / v_pk_mul / v_pk_fma_f32) in the FFT kernels: both recorded pipelined-mode wrong
// results (round 3 in K2, round 4 in K1) sit in a packed-FP32 instruction whose source register pair the
// very next packed instruction overwrites, and the round-4 values fit, on all 16 lanes of the pass to fp32 rounding,
// that instruction reading its source AFTER the next one wrote it (tools/transient_fit.py).  Scalar fp32 ops compute
// the same roundings (fma for fma, mul for mul), so the outputs are bit-identical.  The device pass only: the feature
// is unknown to the host target.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif
#include "rsl_common.h"
#include "rsl_internal.h"
#include "rsl_packed.h"

namespace rsl {

constexpr int kThreads = 256;

// K1 work queues (RSL_RF_DYN): per (handle, stream), 8 per-XCD dequeue heads and 8 exit counters, each on its own
// 128-B line ([2][8][32] unsigned, 2 KiB of device memory allocated on the handle's device and zeroed on the stream's
// first K1 launch through that handle).  The last workgroup of an XCD to leave resets its pair, so the queue is clean
// for the stream's next launch; launches on one stream run in order, so no two K1 launches in flight ever share a
// queue.  The set lives in the handle (rsl_context::rfq) and rsl_destroy frees it: handles share no mutable state
// (rsl.h).  Round 5 kept one process-global map keyed by the stream handle alone, so two devices' null streams (both
// handle 0, what torch reports for a default stream) shared one queue on the first device.
constexpr size_t kRfQueueBytes = 2 * 8 * 32 * sizeof(unsigned);

struct RfQueues {
  int device = 0;
  std::mutex mu;
  std::unordered_map<hipStream_t, unsigned*> q;  // a destroyed stream's address may come back on this handle's device:
};                                               // its queue is clean between launches, so reuse is safe

RfQueues* rf_queues_new(int device) {
  RfQueues* s = new RfQueues();
  s->device = device;
  return s;
}

void rf_queues_free(RfQueues* s) {
  if (!s) return;
  int cur = 0;
  (void)hipGetDevice(&cur);
  (void)hipSetDevice(s->device);
  for (auto& kv : s->q) (void)hipFree(kv.second);  // hipFree waits for the device: no K1 still reads the queue
  (void)hipSetDevice(cur);
  delete s;
}

// The queue of stream `st` in the set, allocated at its first use.  hipErrorStreamCaptureUnsupported when that first
// use is inside a graph capture (hipMalloc is not capturable: run one uncaptured K1 launch on the stream first, and
// never replay one captured K1 concurrently on two streams, which would share the captured queue); hipErrorInvalidDevice
// when the stream belongs to another device than the handle.
static hipError_t rf_queue(RfQueues* s, hipStream_t st, unsigned** out) {
  *out = nullptr;
  if (!s) return hipErrorInvalidValue;
  std::lock_guard<std::mutex> lock(s->mu);
  auto it = s->q.find(st);
  if (it != s->q.end()) {
    *out = it->second;
    return hipSuccess;
  }
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone)
    return hipErrorStreamCaptureUnsupported;
  hipDevice_t sd = 0;
  if (st && hipStreamGetDevice(st, &sd) == hipSuccess && (int)sd != s->device) return hipErrorInvalidDevice;
  unsigned* q = nullptr;
  hipError_t e = hipMalloc(&q, kRfQueueBytes);
  if (e != hipSuccess) return e;
  e = hipMemsetAsync(q, 0, kRfQueueBytes, st);  // ordered before the stream's first K1
  if (e != hipSuccess) {
    (void)hipFree(q);
    return e;
  }
  s->q.emplace(st, q);
  *out = q;
  return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// K1: range FFT.  One workgroup = CB consecutive chirp rows of one (frame, antenna).
// Rows are contiguous S-sample vectors: loads/stores are fully coalesced 16-B accesses.
// ---------------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(kThreads) void k_range_fft(const float2* __restrict__ cube, int Ct, int c0, int C,
                                                         const float2* __restrict__ table,
                                                         const float2* __restrict__ tw, int dc,
                                                         float2* __restrict__ work) {
  constexpr int CB = rows_for(S);
  constexpr int LD = lp_row(S);
  extern __shared__ float2 sm[];
  float2* tws = sm;
  float2* buf = sm + S;
  const int tid = threadIdx.x;
  const int ncb = (C + CB - 1) / CB;
  const int cb = blockIdx.x % ncb;
  const long fa = blockIdx.x / ncb;  // frame * A + antenna
  const int cbeg = cb * CB;
  const int nrows = min(CB, C - cbeg);
  for (int k = tid; k < S; k += kThreads) tws[k] = tw[k];
  const float2* src = cube + ((size_t)fa * Ct + c0 + cbeg) * S;
  if constexpr (S % 2 == 0) {
    const float4* src4 = reinterpret_cast<const float4*>(src);
    const float4* tab4 = reinterpret_cast<const float4*>(table);
    for (int idx = tid; idx < CB * S / 2; idx += kThreads) {
      const int r = idx / (S / 2), s2 = idx - r * (S / 2);
      float2 lo = make_float2(0.f, 0.f), hi = lo;
      if (r < nrows) {
        const float4 x = src4[(size_t)r * (S / 2) + s2];
        const float4 t = tab4[s2];
        lo = cmul(make_float2(x.x, x.y), make_float2(t.x, t.y));
        hi = cmul(make_float2(x.z, x.w), make_float2(t.z, t.w));
      }
      buf[r * LD + lp(2 * s2)] = lo;
      buf[r * LD + lp(2 * s2 + 1)] = hi;
    }
  } else {
    for (int idx = tid; idx < CB * S; idx += kThreads) {
      const int r = idx / S, s = idx - r * S;
      buf[r * LD + lp(s)] = (r < nrows) ? cmul(src[(size_t)r * S + s], table[s]) : make_float2(0.f, 0.f);
    }
  }
  __syncthreads();
  fft_rows<S, CB, kThreads, LD>(buf, tws, tid);
  if (dc) {
    if (tid < CB) buf[tid * LD] = make_float2(0.f, 0.f);
    __syncthreads();
  }
  float2* dst = work + ((size_t)fa * C + cbeg) * S;
  if constexpr (S % 2 == 0) {
    float4* dst4 = reinterpret_cast<float4*>(dst);
    for (int idx = tid; idx < nrows * S / 2; idx += kThreads) {
      const int r = idx / (S / 2), s2 = idx - r * (S / 2);
      const float2 lo = buf[r * LD + lp(2 * s2)], hi = buf[r * LD + lp(2 * s2 + 1)];
      dst4[idx] = make_float4(lo.x, lo.y, hi.x, hi.y);
    }
  } else {
    for (int idx = tid; idx < nrows * S; idx += kThreads) {
      const int r = idx / S, s = idx - r * S;
      dst[idx] = buf[r * LD + lp(s)];
    }
  }
}

// The tile walk of the persistent K1 kernels.  DYN: workgroup b serves XCD x = b % 8 (dispatch order) and walks that
// XCD's tile range [lo, hi) with its gx workgroups: the first two tiles are static (lo + b / 8, then + gx), every later
// one comes from the XCD's dequeue head (rfq: kRfQueueBytes above), claimed one tile ahead (the atomic returns during a
// whole tile), so workgroups that start late (CUs held by a concurrent kernel) take fewer tiles (tools/dyn.sh: K1 alone
// 1.499 vs 1.667 ms per 1000 cfg2 frames for the static walk, outputs bit-identical).  A tile's body calls claim() at
// its top and publish(claim) before its last barrier, which hands tile lo + 2 gx + claim over through the LDS word
// *nn: written before that barrier, read after it, rewritten only after the next body's first barrier.  Every body
// call claims once and every tile below hi is consumed once, so an XCD's claims are 0 .. hi - lo - 1 and the largest
// index the walk forms is hi + 2 gx - 1 (k1_tiles_fit).  The XCD's last workgroup to leave (every dequeue of a leaver
// has returned) resets the head and the exit counter for the stream's next launch.  Without DYN (grids of fewer than 8
// workgroups) the walk is static over [0, ntile) with stride gridDim.x.
// run() drives load(nx, t) (tile t's global loads into the registers nx) and body(nx, t, tn) (tile t from nx, refilling
// nx with tile tn while it computes; a body narrows t / tn itself where it wants them scalar).
template <bool DYN>
struct TileWalk {
  long lo, hi, gx;
  unsigned* head;  // this XCD's dequeue head (the exit counter: + 256)
  long* nn;        // the hand-off word (LDS, the kernel's)
  RSL_DEV TileWalk(long ntile, unsigned* rfq, long* nn_) : nn(nn_) {
    const int xcd = blockIdx.x & 7;
    gx = ((long)gridDim.x - xcd + 7) / 8;
    lo = DYN ? xcd * ntile / 8 : 0;
    hi = DYN ? (xcd + 1) * ntile / 8 : ntile;
    head = rfq + xcd * 32;
  }
  RSL_DEV unsigned claim() const {
    unsigned c = 0;
    if (DYN && threadIdx.x == 0) c = atomicAdd(head, 1u);
    return c;
  }
  RSL_DEV void publish(unsigned c) const {
    if (DYN && threadIdx.x == 0) *nn = lo + 2 * gx + (long)c;
  }
  template <class T, int N, class Load, class Body>
  RSL_DEV void run(Load&& load, Body&& body) const {
    T nx[N];
    if constexpr (DYN) {
      long t = lo + (blockIdx.x >> 3), tn = t + gx;
      if (t < hi) load(nx, t);
      while (t < hi) {
        body(nx, t, tn);
        t = tn;
        tn = *nn;
      }
      if (threadIdx.x == 0 && atomicAdd(head + 8 * 32, 1u) == (unsigned)gx - 1u) {
        atomicExch(head, 0u);
        atomicExch(head + 8 * 32, 0u);
      }
    } else {
      const long G = gridDim.x;
      long t = blockIdx.x;
      if (t < hi) load(nx, t);
      for (; t < hi; t += G) body(nx, t, t + G);
    }
  }
};

// Persistent K1: the grid holds only resident workgroups; each loops over (frame, antenna, chirp-block) tiles
// and issues the next tile's 16-B global loads into registers before running the current tile's LDS FFT, so
// HBM latency overlaps the FFT instead of stalling every tile's load phase.  Requires even S with
// CB * S / 2 a multiple of the block size (every power-of-two S >= 16).  Cube loads and `work` stores are
// non-temporal (`nt`: both streamed once per batch; tools/cp_ab.py: 1.48-1.57 vs 1.57-1.64 ms per 1000 cfg2 frames).
// The tiles come from a TileWalk: DYN on grids that span the 8 XCDs, static on grids of fewer than 8 workgroups.
// DBG (development builds only; ablations with wrong results): 1 no FFT, 2 no cube loads (constant tiles), 3 loads and
// LDS staging only (no FFT, no stores).
template <int S, int CB, bool DYN, int DBG = 0>
__global__ __launch_bounds__(kThreads) void k_range_fft_p(const float2* __restrict__ cube, int Ct, int c0, int C,
                                                           long ntile, const float2* __restrict__ table,
                                                           const float2* __restrict__ tw, int dc,
                                                           float2* __restrict__ work, unsigned* __restrict__ rfq) {
  constexpr int LD = lp_row(S);
  constexpr int H = S / 2;                 // float4 (2 complex) per row
  constexpr int PF = CB * H / kThreads;    // float4 per thread per tile
  static_assert((CB * H) % kThreads == 0, "tile must split evenly over the block");
  extern __shared__ float2 sm[];
  float2* tws = sm;
  float2* buf = sm + lp_row(S);
  const int tid = threadIdx.x;
  const int ncb = (C + CB - 1) / CB;
  for (int k = tid; k < S; k += kThreads) tws[lp(k)] = tw[k];
  const float4* tab4 = reinterpret_cast<const float4*>(table);
  // the thread's table entries (one float4 when the block spans whole rows: every q hits the same samples)
  constexpr int NTAB = (kThreads % H == 0) ? 1 : PF;
  float4 tab[NTAB];
#pragma unroll
  for (int q = 0; q < NTAB; ++q) tab[q] = tab4[(tid + q * kThreads) % H];
  auto load = [&](float4(&nx)[PF], long t) {
    const int cb = (int)(t % ncb);
    const long fa = t / ncb;
    const int nrows = min(CB, C - cb * CB);
    const float4* src4 = reinterpret_cast<const float4*>(cube + ((size_t)fa * Ct + c0 + cb * CB) * S);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int idx = tid + q * kThreads;
      const int r = idx / H;
      // unconditional (clamped) load, rows past nrows zeroed at consumption (a select on the loaded value here
      // would wait for it)
      if constexpr (DBG == 2)
        nx[q] = make_float4((float)tid, (float)q, (float)r, 1.f);
      else
        nx[q] = ld16<true>(src4 + (r < nrows ? idx : 0));
    }
  };
  __shared__ long s_nn;
  const TileWalk<DYN> walk(ntile, rfq, &s_nn);
  // one tile: stage nx (x conj(ref) w) in LDS, refill nx with tile tn, FFT, DC bin, store
  auto body = [&](float4(&nx)[PF], long t, long tn) {
    const unsigned claim = walk.claim();
    const int cb = (int)(t % ncb);
    const long fa = t / ncb;
    const int nrows = min(CB, C - cb * CB);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int idx = tid + q * kThreads;
      const int r = idx / H, s2 = idx - r * H;
      float4 x = nx[q];
      const float4 tb = tab[NTAB == 1 ? 0 : q];
      if (r >= nrows) x = make_float4(0.f, 0.f, 0.f, 0.f);
      buf[r * LD + lp(2 * s2)] = cmul(make_float2(x.x, x.y), make_float2(tb.x, tb.y));
      buf[r * LD + lp(2 * s2 + 1)] = cmul(make_float2(x.z, x.w), make_float2(tb.z, tb.w));
    }
    __syncthreads();
    if (tn < walk.hi) load(nx, tn);  // in flight during the FFT below
    if constexpr (DBG == 3) {  // loads only: keep the staged tile live, skip the FFT and the stores
      if (buf[tid * 2].x == 1.2345e30f) work[tid] = buf[tid * 2];
      walk.publish(claim);
      __syncthreads();
      return;
    }
    if constexpr (DBG != 1) fft_rows<S, CB, kThreads, LD, true>(buf, tws, tid);
    if (dc) {
      if (tid < CB) buf[tid * LD] = make_float2(0.f, 0.f);
      __syncthreads();
    }
    float4* dst4 = reinterpret_cast<float4*>(work + ((size_t)fa * C + cb * CB) * S);
#pragma unroll
    for (int q = 0; q < PF; ++q) {
      const int idx = tid + q * kThreads;
      const int r = idx / H, s2 = idx - r * H;
      if (r < nrows) {
        const float2 lo2 = buf[r * LD + lp(2 * s2)], hi2 = buf[r * LD + lp(2 * s2 + 1)];
        st16<true>(dst4 + idx, make_float4(lo2.x, lo2.y, hi2.x, hi2.y));
      }
    }
    walk.publish(claim);
    __syncthreads();  // buf is rewritten by the next tile
  };
  walk.template run<float4, PF>(load, body);
}

// ---------------------------------------------------------------------------------------------
// K1 for S = 512 with packed `work` (the cfg2 shape): the range FFT as 16 x 32 in registers instead of three radix-8
// Stockham passes through LDS.  The LDS FFT was LDS-bound (SQ_LDS_IDX_ACTIVE ~70 % of the kernel's cycles, 21 % of wave
// time waiting on LDS issue, 42 % extra bank-conflict cycles): staging + 3 stage writes + 3 stage reads + the output
// read.  Here a tile (8 chirp rows of one (frame, antenna)) takes two LDS exchanges, both conflict-free:
//   a tile is chirp class c of one (frame, antenna): the 8 chirps c + 16 q (q < 8; C = 128, c < 16), so that the
//   Doppler transform's radix-8 step over q (and its W128^(c k1) twiddle) runs here, in registers, at the packed
//   store; K2 (k_doppler_detect_r128) does the 16-point step over the classes;
//   x[n], n = j + 32 m (j < 32, m < 16), thread t = (row q = t / 32, j = t % 32) loads x[j + 32 m] of chirp c + 16 q
//   (8-B loads, two 256-B runs per wave instruction) and multiplies by conj(ref) w;
//   stage 1: V[j][k1] = DFT16_m x[j + 32 m]  (registers), times W512^(j k1) (LDS table, 17-float2 pitch per j);
//   exchange: V' -> xbuf[row][k1][j] (pitch 34: the stage-2 reads of 32 lanes hit 64 distinct banks);
//   stage 2: thread t = (row, k1 = (t / 2) % 16, h = t % 2) takes j = 2 i + h: E or O = DFT16_i (registers); lane
//   pairs swap halves by DPP and form X[k1 + 16 k2] = E + W32^k2 O, X[k1 + 16 (k2 + 16)] = E - W32^k2 O;
//   output: X -> obuf[row][b + 8 (b / 256)] (the b >= 256 half shifted by 8: conflict-free writes), then thread p
//   reads bins 2p, 2p + 1 of the 8 rows (16-B reads), takes W128^(c k1) DFT8_q of each and stores them packed.
// X[k1 + 16 k2'] = sum_j W512^(j k1) W32^(j k2') sum_m x[j + 32 m] W16^(m k1): the 512-point DFT exactly.
// DBG (development builds only; wrong results): 2 no cube loads, 3 loads only.
constexpr int kR512Pitch = 34;             // xbuf pitch per (row, k1): 32 j + 2 pad
constexpr int kR512Obuf = 520;             // obuf row pitch (512 bins + 8 shift)
constexpr int kR512TwPitch = 17;           // ldtw pitch per j
template <int DBG = 0, bool NTW = true>
__global__ __launch_bounds__(kThreads) void k_range_fft_r512(const float2* __restrict__ cube, int Ct, int c0,
                                                              long ntile, const float2* __restrict__ table,
                                                              const float2* __restrict__ tw, int dc,
                                                              float2* __restrict__ work, unsigned* __restrict__ rfq) {
  constexpr int S = 512, CB = 8;
  __shared__ float2 ldtab[S];
  __shared__ float2 ldtw[32 * kR512TwPitch];
  __shared__ float2 xbuf[CB * 16 * kR512Pitch];  // stage exchange; aliased by the output buffer
  static_assert(CB * kR512Obuf <= CB * 16 * kR512Pitch, "output buffer must fit in the exchange buffer");
  float2* obuf = xbuf;
  const int tid = threadIdx.x;
  const int row = tid >> 5, j = tid & 31;
  const int k1b = (tid >> 1) & 15, h = tid & 1;
  constexpr int ncb = 128 / CB;  // C = 128 wherever this kernel runs (work_packed_supported): tile index math by shifts
  for (int k = tid; k < S; k += kThreads) ldtab[k] = table[k];
  for (int k = tid; k < 32 * 16; k += kThreads) {
    const int jj = k >> 4, kk = k & 15;
    ldtw[jj * kR512TwPitch + kk] = tw[jj * kk];  // W512^(j k1), j k1 <= 465
  }
  auto load = [&](float2(&nx)[16], long t) {
    t = (long)__builtin_amdgcn_readfirstlane((int)t);  // the tile index is workgroup-uniform (below 2^31: k1_tiles_fit)
    const int cb = (int)(t % ncb);
    const long fa = t / ncb;
    const float2* src = cube + ((size_t)fa * Ct + c0 + cb + 16 * row) * S + j;  // chirp class cb, row q = row
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      if constexpr (DBG == 2)
        nx[m] = make_float2((float)tid, (float)m);
      else
        nx[m] = ld8<true>(src + 32 * m);
    }
  };
  __shared__ long s_nn;
  const TileWalk<true> walk(ntile, rfq, &s_nn);
  __syncthreads();
  auto body = [&](float2(&nx)[16], long t, long tn) {
    // workgroup-uniform tile indices (read from LDS or derived from blockIdx; below 2^31: k1_tiles_fit): scalar, so the
    // tile's address arithmetic runs on the SALU
    t = (long)__builtin_amdgcn_readfirstlane((int)t);
    tn = (long)__builtin_amdgcn_readfirstlane((int)tn);
    const unsigned claim = walk.claim();
    const int cb = (int)(t % ncb);
    const long fa = t / ncb;
    float2 v[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = cmul(nx[m], ldtab[j + 32 * m]);
    // in flight during this tile's transforms and stores; unconditional (past the range: this tile again, an L2 hit
    // once per workgroup), which spares a copy of the 32 loaded registers per tile
    load(nx, tn < walk.hi ? tn : t);
    if constexpr (DBG == 3) {
      if (v[0].x == 1.2345e30f) work[tid] = v[1];
      walk.publish(claim);
      __syncthreads();
      return;
    }
    // stage 1: DFT16 over m, twiddle W512^(j k1)
    Dft<16>::run(v);
#pragma unroll
    for (int k = 1; k < 16; ++k) v[k] = cmul(v[k], ldtw[j * kR512TwPitch + k]);
    float2* xw = xbuf + row * 16 * kR512Pitch + j;
#pragma unroll
    for (int k = 0; k < 16; ++k) xw[k * kR512Pitch] = v[k];
    __syncthreads();
    // stage 2: DFT16 over i of V'[2 i + h][k1], then the radix-2 combine across the lane pair (h = 0, 1)
    const float2* xr = xbuf + (row * 16 + k1b) * kR512Pitch + h;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = xr[2 * i];
    Dft<16>::run(v);
    // lane h = 0 holds E[k], lane h = 1 holds O[k]: u = E[k] or W32^k O[k], swapped with the partner lane by DPP;
    // bin k1 + 16 k = E + W O on h = 0 (u + recv), bin k1 + 16 (k + 16) = E - W O on h = 1 (recv - u): one packed
    // fma with a per-lane sign (+1 / -1) instead of selecting operands and both sums
    float2 xo[16];
    const rsl_f2v sgn = h ? (rsl_f2v){-1.f, -1.f} : (rsl_f2v){1.f, 1.f};
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      const float2 u = h ? cmul(v[k], w32(k)) : v[k];
      float2 recv;
      recv.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(u.x), 0xB1, 0xF, 0xF, true));
      recv.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(u.y), 0xB1, 0xF, 0xF, true));
      xo[k] = cf(__builtin_elementwise_fma(sgn, cv(u), cv(recv)));
    }
    if (dc && k1b == 0 && h == 0) xo[0] = make_float2(0.f, 0.f);  // DC removal = zero range bin 0
    __syncthreads();  // xbuf reads done: obuf aliases it
    float2* ow = obuf + row * kR512Obuf + k1b + 264 * h;  // bin k1 + 16 k + 256 h at position bin + 8 h
#pragma unroll
    for (int k = 0; k < 16; ++k) ow[16 * k] = xo[k];
    __syncthreads();
    // thread tid holds bins 2 tid, 2 tid + 1 of the 8 rows (chirps cb + 16 q); the b >= 256 half sits 8 later
    k1_packed_store<S, NTW>(obuf, kR512Obuf, 2 * tid + (tid >= 128 ? 8 : 0), cb, tw, work, (size_t)fa * ncb + cb, tid);
    walk.publish(claim);
    __syncthreads();  // obuf is read above; the next tile's exchange writes overwrite it
  };
  walk.template run<float2, 16>(load, body);
}

// ---------------------------------------------------------------------------------------------
// K1 for S = 1024 with packed `work` (the configs[4] shape: C = 256): k_range_fft_r512's design at
// twice the length, on 512 threads.  A tile is chirp class c of one (frame, antenna), the 8 chirps c + 32 q (q < 8,
// c < 32), so that the radix-8 step of the 256-point Doppler transform over q, with its W256^(c k1) twiddle, runs here
// and K2 (k_doppler_detect_r256) does the 32-point step over the classes.  One wave per chirp row:
//   x[n], n = j + 64 m (j < 64, m < 16): lane j of wave q loads x[j + 64 m] (8-B loads, 512-B runs), x conj(ref) w
//   (the dechirp table is read through L1: in LDS it would not leave room for two workgroups per CU);
//   stage 1: V[j][k1] = DFT16_m, times W1024^(j k1) (LDS, 16 per j, XOR-swizzled: k1 ^ ((j >> 1) & 15));
//   exchange: V -> xbuf[q][k1][j ^ 4 k1] (the stage-2 reads of 32 lanes then hit 64 distinct banks, the writes 32);
//   stage 2: lane (k1 = lane / 4, h = lane % 4) takes j = 4 i + h: F_h = DFT16_i, u_h = W64^(h k') F_h[k'], and the
//   radix-4 step over h across the lane quad by two DPP swaps (h ^ 2, then h ^ 1 after the W4 twiddle), after which
//   lane h holds Y[k' + 16 s], s = (h >> 1) | 2 (h & 1): bin k1 + 16 k' + 256 s;
//   output: -> obuf[q][bin ^ 4 s] (conflict-free 16-lane writes), then thread p reads bins 2p, 2p + 1 of the 8 rows
//   (16-B reads), takes W256^(c k1) DFT8_q and stores both bins packed (pk_pack16; planes of 512 pairs x 16 B).
// LDS: xbuf 64 KiB (aliased by obuf) + twiddles 8 KiB: two workgroups (16 waves) per CU.
constexpr int kR1kThreads = 512;
// W1024^(j k) in ldtw.  Swizzle (j / 2) ^ (j / 32): the stage-1 reads (lane j, one k) hit 64 distinct banks per 32-lane
// group, and the stage-2 reads of rows j = 16 h (h = lane % 4: swizzles 0, 8, 1, 9) do too; with (j / 2) alone rows
// 0 / 32 and 16 / 48 shared banks (2-way on 15 reads per tile and wave: most of the 17.2 M conflict cycles per 100
// configs[4] frames, gpurun_out/r5aa_ddctr5)
RSL_DEV int r1k_tw(int j, int k) { return j * 16 + (k ^ (((j >> 1) ^ (j >> 5)) & 15)); }

template <int DBG = 0>
__global__ __launch_bounds__(kR1kThreads) __attribute__((amdgpu_waves_per_eu(4))) void k_range_fft_r1024(const float2* __restrict__ cube, int Ct,
                                                                  int c0, long ntile,
                                                                  const float2* __restrict__ table,
                                                                  const float2* __restrict__ tw, int dc,
                                                                  float2* __restrict__ work, unsigned* __restrict__ rfq) {
  constexpr int S = 1024, NT = kR1kThreads, ncb = 32;  // C = 256 wherever this kernel runs (work_packed_supported)
  __shared__ float2 ldtab[S];
  __shared__ float2 ldtw[64 * 16];
  __shared__ float2 xbuf[8 * S];  // stage exchange; aliased by the output buffer
  // 80 KiB exactly (two workgroups per CU): the tile hand-off word lives in a twiddle slot no lane reads (k1 = 0 of j = 0)
  long* s_nn = reinterpret_cast<long*>(&ldtw[r1k_tw(0, 0)]);
  float2* obuf = xbuf;
  const int tid = threadIdx.x;
  for (int k = tid; k < S; k += NT) ldtab[k] = table[k];
  for (int k = tid; k < 64 * 16; k += NT) {
    const int jj = k >> 4, kk = k & 15;
    if (kk) ldtw[r1k_tw(jj, kk)] = tw[jj * kk];  // W1024^(j k1), j k1 <= 945 (k1 = 0: never read)
  }
  auto load = [&](float2(&nx)[16], long t) {
    t = (long)__builtin_amdgcn_readfirstlane((int)t);  // the tile index is workgroup-uniform (below 2^31: k1_tiles_fit)
    int lt = tid;
    asm volatile("" : "+v"(lt));
    const int row = __builtin_amdgcn_readfirstlane(lt >> 6), j = lt & 63;  // one wave per chirp row: row is scalar
    const int cb = (int)(t % ncb);
    const long fa = t / ncb;
    const float2* src = cube + ((size_t)fa * Ct + c0 + cb + 32 * row) * S + j;  // chirp class cb, row q = row
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      if constexpr (DBG == 2)
        nx[m] = make_float2((float)tid, (float)m);
      else
        nx[m] = ld8<true>(src + 64 * m);
    }
  };
  const TileWalk<true> walk(ntile, rfq, s_nn);
  __syncthreads();
  auto body = [&](float2(&nx)[16], long t, long tn) {
    // workgroup-uniform tile indices (read from LDS or derived from blockIdx; below 2^31: k1_tiles_fit): scalar, so the
    // tile's address arithmetic runs on the SALU
    t = (long)__builtin_amdgcn_readfirstlane((int)t);
    tn = (long)__builtin_amdgcn_readfirstlane((int)tn);
    const unsigned claim = walk.claim();
    const int cb = (int)(t % ncb);
    const long fa = t / ncb;
    // the thread index laundered per tile: otherwise the compiler hoists the tile-invariant table and twiddle reads
    // out of the tile loop (92 registers live across it: 256 VGPRs with spills)
    int lt = tid;
    asm volatile("" : "+v"(lt));
    const int row = __builtin_amdgcn_readfirstlane(lt >> 6), j = lt & 63;  // one wave per chirp row: row is scalar
    const int k1b = (lt >> 2) & 15, h = lt & 3;
    const int s_out = (h >> 1) | ((h & 1) << 1);  // the radix-4 output index lane h ends with
    float2 v[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = cmul(nx[m], ldtab[j + 64 * m]);
    load(nx, tn < walk.hi ? tn : t);  // in flight during this tile's transforms and stores
    if constexpr (DBG == 3) {
      if (v[0].x == 1.2345e30f) work[tid] = v[1];
      walk.publish(claim);
      __syncthreads();
      return;
    }
    // stage 1: DFT16 over m, twiddle W1024^(j k1)
    Dft<16>::run(v);
#pragma unroll
    for (int k = 1; k < 16; ++k) v[k] = cmul(v[k], ldtw[r1k_tw(j, k)]);
    float2* xw = xbuf + row * S;
#pragma unroll
    for (int k = 0; k < 16; ++k) xw[k * 64 + (j ^ ((4 * k) & 63))] = v[k];
    __syncthreads();
    // stage 2: DFT16 over i of V[4 i + h][k1], then the radix-4 step over h across the lane quad
    const float2* xr = xbuf + row * S + k1b * 64;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = xr[4 * (i ^ k1b) + h];
    Dft<16>::run(v);
    const float sg1 = (h & 2) ? -1.f : 1.f, sg2 = (h & 1) ? -1.f : 1.f;
    __syncthreads();  // xbuf reads done: obuf aliases it (the radix-4 step below writes each output as it forms)
    // bin k1 + 16 k + 256 s at (bin ^ 4 s) = ((k1 ^ 4 s) + 256 s) + 16 k: one base, constant offsets
    float2* ow = obuf + row * S + ((k1b ^ (4 * s_out)) + 256 * s_out);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
      float2 u = v[k];
      // W64^(h k) = W1024^(16 h k); unconditional (lanes h = 0 multiply by W^0 = 1: exact up to the sign of a zero)
      if (k > 0) u = cmul(u, ldtw[r1k_tw(16 * h, k)]);
      // h ^ 2: a = u_h0 +- u_(h0 + 2) (lanes with h & 2 hold the difference)
      float2 r;
      r.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(u.x), 0x4E, 0xF, 0xF, true));
      r.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(u.y), 0x4E, 0xF, 0xF, true));
      float2 a = make_float2(fmaf(sg1, u.x, r.x), fmaf(sg1, u.y, r.y));
      // lanes h0 = 1 take W4^(s0) = (-i)^(h >> 1) before the h ^ 1 swap
      if ((h & 1) && (h & 2)) a = make_float2(a.y, -a.x);
      r.x = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(a.x), 0xB1, 0xF, 0xF, true));
      r.y = __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(a.y), 0xB1, 0xF, 0xF, true));
      float2 xo = make_float2(fmaf(sg2, a.x, r.x), fmaf(sg2, a.y, r.y));
      if (k == 0 && dc && k1b == 0 && h == 0) xo = make_float2(0.f, 0.f);  // DC removal = zero range bin 0
      ow[16 * k] = xo;
    }
    __syncthreads();
    // thread lt holds bins 2 lt, 2 lt + 1 of the 8 rows (chirps cb + 32 q), at the output swizzle's position
    k1_packed_store<S, true>(obuf, S, (2 * lt) ^ (4 * ((lt >> 7) & 3)), cb, tw, work, (size_t)fa * ncb + cb, lt);
    walk.publish(claim);
    __syncthreads();  // obuf is read above; the next tile's exchange writes overwrite it
  };
  walk.template run<float2, 16>(load, body);
}

// ---------------------------------------------------------------------------------------------
// K1 for S = 256 with packed `work` (the cfg1 / configs[0] shape: C = 64): the same chirp-class tiles on
// 128 threads.  A tile is chirp class c of one (frame, antenna), the 8 chirps c + 8 q (q < 8, c < 8); K2
// (k_doppler_detect_r64) does the 8-point step over the classes.  16 lanes per chirp row:
//   x[n], n = j + 16 m (j, m < 16): lane j of row q loads x[j + 16 m] (8-B loads, 128-B runs), x conj(ref) w;
//   stage 1: V[j][k1] = DFT16_m, times W256^(j k1) (LDS, XOR-swizzled);
//   exchange: V -> xbuf[q][k1][j ^ k1 ^ (q & 1)] (both rows of a 32-lane read group cover the 64 banks once);
//   stage 2: lane (q, k1) takes the 16 j: X[k1 + 16 k2] = DFT16_j, no cross-lane step;
//   output: -> obuf[q][bin] (aliasing xbuf), then thread p reads bins 2p, 2p + 1 of the 8 rows (16-B reads), takes
//   W64^(c k1) DFT8_q and stores both bins packed (planes of 128 pairs x 16 B).
// LDS 20 KiB: 8 workgroups (16 waves) per CU.
constexpr int kR256Threads = 128;
RSL_DEV int r256_tw(int j, int k) { return j * 16 + (k ^ j); }  // W256^(j k) in ldtw

template <int DBG = 0>
__global__ __launch_bounds__(kR256Threads) void k_range_fft_r256(const float2* __restrict__ cube, int Ct, int c0,
                                                                 long ntile, const float2* __restrict__ table,
                                                                 const float2* __restrict__ tw, int dc,
                                                                 float2* __restrict__ work, unsigned* __restrict__ rfq) {
  constexpr int S = 256, NT = kR256Threads, ncb = 8;  // C = 64 wherever this kernel runs (work_packed_supported)
  __shared__ float2 ldtab[S];
  __shared__ float2 ldtw[16 * 16];
  __shared__ float2 xbuf[8 * S];  // stage exchange; aliased by the output buffer
  __shared__ long s_nn;
  float2* obuf = xbuf;
  const int tid = threadIdx.x;
  for (int k = tid; k < S; k += NT) ldtab[k] = table[k];
  for (int k = tid; k < 16 * 16; k += NT) {
    const int jj = k >> 4, kk = k & 15;
    ldtw[r256_tw(jj, kk)] = tw[jj * kk];  // W256^(j k1), j k1 <= 225
  }
  auto load = [&](float2(&nx)[16], long t) {
    t = (long)__builtin_amdgcn_readfirstlane((int)t);  // the tile index is workgroup-uniform (below 2^31: k1_tiles_fit)
    int lt = tid;
    asm volatile("" : "+v"(lt));
    const int row = lt >> 4, j = lt & 15;
    const int cb = (int)(t % ncb);
    const long fa = t / ncb;
    const float2* src = cube + ((size_t)fa * Ct + c0 + cb + 8 * row) * S + j;  // chirp class cb, row q = row
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      if constexpr (DBG == 2)
        nx[m] = make_float2((float)tid, (float)m);
      else
        nx[m] = ld8<true>(src + 16 * m);
    }
  };
  const TileWalk<true> walk(ntile, rfq, &s_nn);
  __syncthreads();
  auto body = [&](float2(&nx)[16], long t, long tn) {
    // workgroup-uniform tile indices (read from LDS or derived from blockIdx; below 2^31: k1_tiles_fit): scalar, so the
    // tile's address arithmetic runs on the SALU
    t = (long)__builtin_amdgcn_readfirstlane((int)t);
    tn = (long)__builtin_amdgcn_readfirstlane((int)tn);
    const unsigned claim = walk.claim();
    const int cb = (int)(t % ncb);
    const long fa = t / ncb;
    int lt = tid;  // laundered per tile: keeps the tile-invariant table reads inside the tile loop
    asm volatile("" : "+v"(lt));
    const int row = lt >> 4, j = lt & 15, k1 = lt & 15;
    float2 v[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) v[m] = cmul(nx[m], ldtab[j + 16 * m]);
    load(nx, tn < walk.hi ? tn : t);  // in flight during this tile's transforms and stores
    Dft<16>::run(v);
#pragma unroll
    for (int k = 1; k < 16; ++k) v[k] = cmul(v[k], ldtw[r256_tw(j, k)]);
    float2* xw = xbuf + row * S;
    const int rsw = j ^ (row & 1);
#pragma unroll
    for (int k = 0; k < 16; ++k) xw[k * 16 + (rsw ^ k)] = v[k];
    __syncthreads();
    const float2* xr = xbuf + row * S + k1 * 16;
    const int rk = k1 ^ (row & 1);
#pragma unroll
    for (int jj = 0; jj < 16; ++jj) v[jj] = xr[jj ^ rk];
    Dft<16>::run(v);
    if (dc && k1 == 0) v[0] = make_float2(0.f, 0.f);  // DC removal = zero range bin 0
    __syncthreads();  // xbuf reads done: obuf aliases it
    float2* ow = obuf + row * S + k1;
#pragma unroll
    for (int k = 0; k < 16; ++k) ow[16 * k] = v[k];
    __syncthreads();
    // thread lt holds bins 2 lt, 2 lt + 1 of the 8 rows (chirps cb + 8 q)
    k1_packed_store<S, true>(obuf, S, 2 * lt, cb, tw, work, (size_t)fa * ncb + cb, lt);
    walk.publish(claim);
    __syncthreads();  // obuf is read above; the next tile's exchange writes overwrite it
  };
  walk.template run<float2, 16>(load, body);
}

// ---------------------------------------------------------------------------------------------
// K2: Doppler FFT.  One workgroup = KB consecutive (unshifted) range bins of one (frame, antenna):
// reads C segments of KB contiguous complex values (KB*8 bytes each), transposes into LDS rows of
// C points (odd stride C+1: conflict-free column writes), FFTs, and writes each shifted range row of
// the RDS [A, S, C] contiguously with the Doppler fftshift folded into the store index.
// ---------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kThreads) void k_doppler_fft(const float2* __restrict__ work, int S,
                                                           const float2* __restrict__ tw, float2* __restrict__ rds) {
  constexpr int KB = rows_for(C);
  constexpr int LD = lp_row(C) | 1;  // odd: conflict-free transposed (column) writes
  extern __shared__ float2 sm[];
  float2* tws = sm;
  float2* buf = sm + C;
  const int tid = threadIdx.x;
  const int nkb = (S + KB - 1) / KB;
  const int kb = blockIdx.x % nkb;
  const long fa = blockIdx.x / nkb;
  const int k0 = kb * KB;
  const int nk = min(KB, S - k0);
  for (int k = tid; k < C; k += kThreads) tws[k] = tw[k];
  const float2* src = work + (size_t)fa * C * S + k0;
  for (int idx = tid; idx < C * KB; idx += kThreads) {
    const int c = idx / KB, kk = idx - c * KB;
    buf[kk * LD + lp(c)] = (kk < nk) ? src[(size_t)c * S + kk] : make_float2(0.f, 0.f);
  }
  __syncthreads();
  fft_rows<C, KB, kThreads, LD>(buf, tws, tid);
  float2* dst = rds + (size_t)fa * S * C;
  const int hs = S / 2, hc = C / 2;
  for (int idx = tid; idx < nk * C; idx += kThreads) {
    const int kk = idx / C, j = idx - kk * C;
    const int k = k0 + kk;
    int i = k + hs;
    if (i >= S) i -= S;
    int d = j - hc;  // out[j] = X[(j - C//2) mod C]
    if (d < 0) d += C;
    dst[(size_t)i * C + j] = buf[kk * LD + lp(d)];
  }
}

// An integer knob of the development build (make dev): 0 when unset, and always 0 in the product build.
int dev_knob(const char* name) {
#ifdef RSL_DEV_KNOBS
  if (const char* e = getenv(name)) return atoi(e);
#endif
  (void)name;
  return 0;
}

// The K1 half of the packed shapes (work_packed_supported), by C = S / 4 (the K2 half: PackedK2, rsl_doppler_detect.hip):
// tiles of one chirp class (8 chirps, C / 8 classes per (frame, antenna)) on NT1 threads with static LDS only.  k1(): the
// product kernel or, in development builds, the ablation variant that RSL_RF_DBG names (results are wrong) and, at
// C = 128, the `work` stores without the nt hint of RSL_WORK_TEMPORAL=1 (MALL study).
using K1Fn = void (*)(const float2*, int, int, long, const float2*, const float2*, int, float2*, unsigned*);
template <int C>
struct PackedK1;
template <>
struct PackedK1<128> {  // cfg2
  static constexpr int NT1 = kThreads;
  static K1Fn k1() {
#ifdef RSL_DEV_KNOBS
    switch (dev_knob("RSL_RF_DBG")) {
      case 2: return k_range_fft_r512<2>;
      case 3: return k_range_fft_r512<3>;
    }
    if (dev_knob("RSL_WORK_TEMPORAL") == 1) return k_range_fft_r512<0, false>;
#endif
    return k_range_fft_r512<>;
  }
};
template <>
struct PackedK1<256> {  // configs[4]
  static constexpr int NT1 = kR1kThreads;
  static K1Fn k1() {
#ifdef RSL_DEV_KNOBS
    switch (dev_knob("RSL_RF_DBG")) {
      case 2: return k_range_fft_r1024<2>;
      case 3: return k_range_fft_r1024<3>;
    }
#endif
    return k_range_fft_r1024<>;
  }
};
template <>
struct PackedK1<64> {  // cfg1
  static constexpr int NT1 = kR256Threads;
  static K1Fn k1() {
#ifdef RSL_DEV_KNOBS
    if (dev_knob("RSL_RF_DBG") == 2) return k_range_fft_r256<2>;
#endif
    return k_range_fft_r256<>;
  }
};

// K1's grid, that of a persistent kernel: the resident workgroups (at most 8 per CU), at most ntile.  wg_knob:
// RSL_K1_WG_PER_CU (development builds) caps them per CU (room for the other stream).
template <class K>
static long k1_grid(K kern, size_t lds, long ntile, int nt, bool wg_knob = true) {
  const int ncu = cu_count();
  long nblk = (long)std::min(occupancy(kern, nt, lds), 8) * ncu;
  nblk = nblk < ntile ? nblk : (ntile > 0 ? ntile : 1);
  if (const int per_cu = wg_knob ? dev_knob("RSL_K1_WG_PER_CU") : 0) {
    const long cap = (long)per_cu * ncu;
    if (cap >= 8 && cap < nblk) nblk = cap;
  }
  return nblk;
}

// The register-form K1 bodies narrow the walk's tile indices to 32 bits (readfirstlane), the hand-off they read back
// included.  The largest index a TileWalk forms is a published hand-off, lo + 2 gx + claim <= hi + 2 gx - 1 (an XCD's
// claims stay below hi - lo), where hi <= ntile and gx <= ceil(nblk / 8): ntile + 2 ceil(nblk / 8) - 1 must be below
// 2^31.  (ntile < 2^31 alone let a hand-off past the range wrap negative, pass `tn < hi` and be walked.)  Every K1
// launcher holds to it, k_range_fft_p's 64-bit walk too.
static bool k1_tiles_fit(long ntile, long nblk) { return ntile + 2 * ((nblk + 7) / 8) - 1 < (1L << 31); }

// K1 on packed work: one tile per (frame, antenna, chirp class).  ntile >= 8 and every CU holds a workgroup, so the
// grid always spans the 8 XCDs that the per-XCD dequeue needs (no static-walk instance); a grid that does not is an
// error.
template <int S>
static hipError_t launch_k1_packed(hipStream_t st, const float2* cube, int F, int A, int Ct, int c0, int C,
                                   const float2* table, const float2* tw, int dc, float2* work, RfQueues* qs) {
  using P = PackedK1<S / 4>;
  if (C != S / 4) return hipErrorInvalidValue;  // its chirp-class tiles are compiled for this C
  const long ntile = (long)F * A * (C / 8);
  const K1Fn kern = P::k1();
  // RSL_K1_WG_PER_CU (k1_grid) acts on the S = 512 kernel only, as before the launchers were merged
  const long nblk = k1_grid(kern, 0, ntile, P::NT1, S == 512);
  if (nblk < 8 || !k1_tiles_fit(ntile, nblk)) return hipErrorInvalidValue;
  unsigned* rfq = nullptr;
  if (hipError_t qe = rf_queue(qs, st, &rfq)) return qe;
  return launch(st, kern, nblk, P::NT1, 0, cube, Ct, c0, ntile, table, tw, dc, work, rfq);
}

template <int S>
static hipError_t launch_k1(hipStream_t st, const float2* cube, int F, int A, int Ct, int c0, int C,
                            const float2* table, const float2* tw, int dc, float2* work, bool packed, RfQueues* qs) {
  if constexpr (S == 256 || S == 512 || S == 1024) {
    if (packed) return launch_k1_packed<S>(st, cube, F, A, Ct, c0, C, table, tw, dc, work, qs);
  }
  constexpr int CB = rows_for(S);
  if constexpr (S % 2 == 0 && (CB * (S / 2)) % kThreads == 0) {
    // 8 chirp rows per tile at S = 512: 16 rows (78 KiB LDS) is faster alone (1.53 vs 1.63 ms per 1000 cfg2 frames)
    // but leaves no LDS for the previous batch's DoA blocks in the pipelined chain (153 k vs 171 k frames/s)
    const long ntile = (long)F * A * ((C + CB - 1) / CB);
    const size_t lds = sizeof(float2) * (lp_row(S) + (size_t)CB * lp_row(S));
    auto kern = k_range_fft_p<S, CB, true>;
#ifdef RSL_DEV_KNOBS
    switch (dev_knob("RSL_RF_DBG")) {  // ablation (development builds only; results are wrong)
      case 1: kern = k_range_fft_p<S, CB, true, 1>; break;
      case 2: kern = k_range_fft_p<S, CB, true, 2>; break;
      case 3: kern = k_range_fft_p<S, CB, true, 3>; break;
    }
#endif
    const long nblk = k1_grid(kern, lds, ntile, kThreads);
    if (!k1_tiles_fit(ntile, nblk)) return hipErrorInvalidValue;
    unsigned* rfq = nullptr;
    if (nblk >= 8) {  // the per-XCD dequeue needs a workgroup on every XCD
      if (hipError_t qe = rf_queue(qs, st, &rfq)) return qe;
    } else {
      kern = k_range_fft_p<S, CB, false>;  // fewer than 8 workgroups: a tiny batch
    }
    return launch(st, kern, nblk, kThreads, lds, cube, Ct, c0, C, ntile, table, tw, dc, work, rfq);
  }
  const long nblk = (long)F * A * ((C + CB - 1) / CB);
  const size_t lds = sizeof(float2) * (S + (size_t)CB * lp_row(S));
  return launch(st, k_range_fft<S>, nblk, kThreads, lds, cube, Ct, c0, C, table, tw, dc, work);
}

template <int C>
static hipError_t launch_k2(hipStream_t st, const float2* work, int F, int A, int S, const float2* tw,
                            float2* rds) {
  constexpr int KB = rows_for(C);
  const long nblk = (long)F * A * ((S + KB - 1) / KB);
  const size_t lds = sizeof(float2) * (C + (size_t)KB * (lp_row(C) | 1));
  return launch(st, k_doppler_fft<C>, nblk, kThreads, lds, work, S, tw, rds);
}

// ---------------------------------------------------------------------------------------------
// Any-length fallback (sizes whose prime factors are not all in {2,3,5,7}, e.g. a chirp_subset of 59
// chirps): direct DFT from LDS with the fp64-accurate twiddle table, O(N) per output point.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_range_dft(const float2* __restrict__ cube, int Ct, int c0, int C, int S,
                                                        const float2* __restrict__ table,
                                                        const float2* __restrict__ tw, int dc,
                                                        float2* __restrict__ work) {
  extern __shared__ float2 sm[];
  float2* tws = sm;
  float2* row = sm + S;
  const long r = blockIdx.x;  // (f*A + a)*C + c
  const long fa = r / C;
  const int c = (int)(r - fa * C);
  const float2* src = cube + ((size_t)fa * Ct + c0 + c) * S;
  for (int k = threadIdx.x; k < S; k += kThreads) {
    tws[k] = tw[k];
    row[k] = cmul(src[k], table[k]);
  }
  __syncthreads();
  float2* dst = work + (size_t)r * S;
  for (int k = threadIdx.x; k < S; k += kThreads) {
    float2 acc = make_float2(0.f, 0.f);
    int idx = 0;
    for (int n = 0; n < S; ++n) {
      acc = cadd(acc, cmul(row[n], tws[idx]));
      idx += k;
      if (idx >= S) idx -= S;
    }
    dst[k] = (dc && k == 0) ? make_float2(0.f, 0.f) : acc;
  }
}

__global__ __launch_bounds__(kThreads) void k_doppler_dft(const float2* __restrict__ work, int C, int S,
                                                          const float2* __restrict__ tw, float2* __restrict__ rds) {
  extern __shared__ float2 sm[];
  float2* tws = sm;
  float2* col = sm + C;
  const long r = blockIdx.x;  // (f*A + a)*S + k
  const long fa = r / S;
  const int k = (int)(r - fa * S);
  const float2* src = work + (size_t)fa * C * S + k;
  for (int c = threadIdx.x; c < C; c += kThreads) {
    tws[c] = tw[c];
    col[c] = src[(size_t)c * S];
  }
  __syncthreads();
  int i = k + S / 2;
  if (i >= S) i -= S;
  float2* dst = rds + ((size_t)fa * S + i) * C;
  for (int j = threadIdx.x; j < C; j += kThreads) {
    int d = j - C / 2;
    if (d < 0) d += C;
    float2 acc = make_float2(0.f, 0.f);
    int idx = 0;
    for (int n = 0; n < C; ++n) {
      acc = cadd(acc, cmul(col[n], tws[idx]));
      idx += d;
      if (idx >= C) idx -= C;
    }
    dst[j] = acc;
  }
}

hipError_t launch_range_dft(hipStream_t st, const float2* cube, int F, int A, int Ct, int c0, int C, int S,
                            const float2* table, const float2* tw, int dc, float2* work) {
  const long nblk = (long)F * A * C;
  return launch(st, k_range_dft, nblk, kThreads, sizeof(float2) * 2 * (size_t)S, cube, Ct, c0, C, S, table, tw, dc,
                work);
}

hipError_t launch_doppler_dft(hipStream_t st, const float2* work, int F, int A, int C, int S, const float2* tw,
                              float2* rds) {
  const long nblk = (long)F * A * S;
  return launch(st, k_doppler_dft, nblk, kThreads, sizeof(float2) * 2 * (size_t)C, work, C, S, tw, rds);
}

hipError_t launch_range_fft(hipStream_t st, const float2* cube, int F, int A, int Ct, int chirp0, int C, int S,
                            const float2* table, const float2* tw_S, int dc, float2* work, RfQueues* queues,
                            bool packed) {
  if (F <= 0 || A <= 0 || C <= 0) return hipSuccess;
  switch (S) {
#define CASE(n) \
  case n:       \
    return launch_k1<n>(st, cube, F, A, Ct, chirp0, C, table, tw_S, dc, work, packed, queues);
    RSL_FFT_SIZES(CASE)
#undef CASE
    default:
      if (S > 4096) return hipErrorInvalidValue;
      return launch_range_dft(st, cube, F, A, Ct, chirp0, C, S, table, tw_S, dc, work);
  }
}

hipError_t launch_doppler_fft(hipStream_t st, const float2* work, int F, int A, int C, int S, const float2* tw_C,
                              float2* rds) {
  if (F <= 0 || A <= 0 || S <= 0) return hipSuccess;
  switch (C) {
#define CASE(n) \
  case n:       \
    return launch_k2<n>(st, work, F, A, S, tw_C, rds);
    RSL_FFT_SIZES(CASE)
#undef CASE
    default:
      if (C > 4096) return hipErrorInvalidValue;
      return launch_doppler_dft(st, work, F, A, C, S, tw_C, rds);
  }
}


}  // namespace rsl

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
