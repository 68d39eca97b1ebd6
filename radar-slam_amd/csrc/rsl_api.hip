// rsl_api.hip — C-ABI layer of librsl.so (see include/rsl.h).  No kernels here: argument checks,
// per-size twiddle tables, launch + optional hipEvent timing on the handle's stream.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rsl.h"
#include "rsl_cfar_common.h"
#include "rsl_common.h"
#include "rsl_doa_common.h"
#include "rsl_internal.h"

struct rsl_context {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  std::map<int, float2*> tw;  // N -> device table exp(-2 pi i k / N)
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev[RSL_K_COUNT];
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  double ms[RSL_K_COUNT] = {0};
  long long cnt[RSL_K_COUNT] = {0};
  // per-launch [start, end] in ms after the reference event t0 (recorded by rsl_timing_reset on the handle's stream):
  // the live timeline of the launches since the reset, every stream's launches on one device clock
  hipEvent_t t0 = nullptr;
  std::vector<std::pair<double, double>> span[RSL_K_COUNT];
  rsl::RfQueues* rfq = nullptr;  // K1 tile queues, one per stream this handle launched K1 on (freed by rsl_destroy)
};

namespace {

int fail(rsl_context* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}

int hip_check(rsl_context* h, hipError_t e, const char* what) {
  if (e == hipSuccess) return RSL_OK;
  return fail(h, RSL_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

struct Scope {
  rsl_context* h;
  int kid;
  hipEvent_t a = nullptr, b = nullptr;
  Scope(rsl_context* h_, int kid_) : h(h_), kid(kid_) {
    hipSetDevice(h->device);
    if (h->timing) {
      if (!h->ev_pool.empty()) {
        a = h->ev_pool.back().first;
        b = h->ev_pool.back().second;
        h->ev_pool.pop_back();
      } else {
        hipEventCreate(&a);
        hipEventCreate(&b);
      }
      hipEventRecord(a, h->stream);
    }
  }
  ~Scope() {
    if (a) {
      hipEventRecord(b, h->stream);
      h->ev[kid].push_back({a, b});
    }
  }
};

float2* twiddles(rsl_context* h, int n) {
  auto it = h->tw.find(n);
  if (it != h->tw.end()) return it->second;
  std::vector<float2> t(n);
  for (int k = 0; k < n; ++k) {
    const double ang = -2.0 * M_PI * (double)k / (double)n;
    t[k] = make_float2((float)std::cos(ang), (float)std::sin(ang));
  }
  float2* d = nullptr;
  if (hipMalloc(&d, sizeof(float2) * n) != hipSuccess) return nullptr;
  if (hipMemcpy(d, t.data(), sizeof(float2) * n, hipMemcpyHostToDevice) != hipSuccess) {
    hipFree(d);
    return nullptr;
  }
  h->tw[n] = d;
  return d;
}

// Folds the recorded launch events into the per-kernel totals and spans.  t0 is recorded on the stream bound at the
// reset, which need not be the stream of a given launch: it is waited for once, and a span whose elapsed-time query
// fails is dropped (never recorded as a silent (0, 0)); a failed duration query drops the launch from the totals.
void collect(rsl_context* h) {
  const bool t0_ok = h->t0 && hipEventSynchronize(h->t0) == hipSuccess;
  for (int k = 0; k < RSL_K_COUNT; ++k) {
    for (auto& p : h->ev[k]) {
      hipEventSynchronize(p.second);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, p.first, p.second) == hipSuccess) {
        h->ms[k] += ms;
        h->cnt[k] += 1;
      }
      if (t0_ok) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, h->t0, p.first) == hipSuccess &&
            hipEventElapsedTime(&b, h->t0, p.second) == hipSuccess)
          h->span[k].push_back({a, b});
      }
      h->ev_pool.push_back(p);
    }
    h->ev[k].clear();
  }
}

// The cell list of a DoA entry point from its untyped arguments.
rsl::CellList cell_list(const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                        const void* ncell_dev, long long ncell) {
  return {(const float2*)rds, A, S, C, (const int*)c_frame, (const int*)c_rc, (const long long*)ncell_dev, ncell};
}

// The point cloud of a registration or map entry point from its untyped arguments (rsl_cloud.h).
rsl::CloudView cloud_view(const void* points, const void* seg, long long n, int F, const void* weight) {
  return {(const float*)points, (const long long*)seg, n, F, (const float*)weight};
}

// The sections of a steering table that rsl_steer_table_build(G, M) wrote (rsl_doa_common.h SteerLayout).
struct SteerView {
  rsl::SteerLayout lay;
  const float* f32;
  const float* toep;
  const double* t64;
};

SteerView steer_view(const void* tab, int G, int M) {
  const rsl::SteerLayout lay = rsl::steer_layout(G, M);
  const float* t = (const float*)tab;
  return {lay, t, t + lay.f32_floats, reinterpret_cast<const double*>(t + lay.t64_offset)};
}

}  // namespace

extern "C" {

int rsl_version(void) { return RSL_VERSION; }

// 1: radix-{2,3,4,5,7,8} Stockham FFT in LDS; 2: any other length up to 4096 (direct DFT fallback); 0: no.
int rsl_fft_supported(int n) {
  switch (n) {
#define CASE(n) case n:
    RSL_FFT_SIZES(CASE)
#undef CASE
      return 1;
    default:
      return (n >= 1 && n <= 4096) ? 2 : 0;
  }
}

int rsl_create(rsl_handle* out, int device) {
  if (!out) return RSL_ERR_INVALID;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return RSL_ERR_HIP;
  rsl_context* h = new rsl_context();
  h->device = device;
  h->rfq = rsl::rf_queues_new(device);
  *out = h;
  return RSL_OK;
}

int rsl_destroy(rsl_handle h) {
  if (!h) return RSL_OK;
  hipSetDevice(h->device);
  for (auto& kv : h->tw) hipFree(kv.second);
  for (int k = 0; k < RSL_K_COUNT; ++k)
    for (auto& p : h->ev[k]) {
      hipEventDestroy(p.first);
      hipEventDestroy(p.second);
    }
  for (auto& p : h->ev_pool) {
    hipEventDestroy(p.first);
    hipEventDestroy(p.second);
  }
  if (h->t0) hipEventDestroy(h->t0);
  rsl::rf_queues_free(h->rfq);
  delete h;
  return RSL_OK;
}

const char* rsl_last_error(rsl_handle h) { return h ? h->err.c_str() : "null handle"; }

int rsl_set_stream(rsl_handle h, void* s) {
  if (!h) return RSL_ERR_INVALID;
  h->stream = reinterpret_cast<hipStream_t>(s);
  return RSL_OK;
}

int rsl_sync(rsl_handle h) {
  if (!h) return RSL_ERR_INVALID;
  hipSetDevice(h->device);
  return hip_check(h, hipStreamSynchronize(h->stream), "hipStreamSynchronize");
}

int rsl_timing_enable(rsl_handle h, int on) {
  if (!h) return RSL_ERR_INVALID;
  h->timing = on != 0;
  return RSL_OK;
}

int rsl_timing_reset(rsl_handle h) {
  if (!h) return RSL_ERR_INVALID;
  collect(h);
  for (int k = 0; k < RSL_K_COUNT; ++k) {
    h->ms[k] = 0;
    h->cnt[k] = 0;
    h->span[k].clear();
  }
  hipSetDevice(h->device);
  if (!h->t0) hipEventCreate(&h->t0);
  hipEventRecord(h->t0, h->stream);
  return RSL_OK;
}

int rsl_timing_spans(rsl_handle h, int kid, int max, double* start_ms, double* end_ms) {
  if (!h || kid < 0 || kid >= RSL_K_COUNT || max < 0) return -1;
  collect(h);
  const int n = (int)h->span[kid].size();
  for (int i = 0; i < n && i < max; ++i) {
    if (start_ms) start_ms[i] = h->span[kid][i].first;
    if (end_ms) end_ms[i] = h->span[kid][i].second;
  }
  return n;
}

int rsl_timing_read(rsl_handle h, int kid, double* total_ms, long long* launches) {
  if (!h || kid < 0 || kid >= RSL_K_COUNT) return RSL_ERR_INVALID;
  collect(h);
  if (total_ms) *total_ms = h->ms[kid];
  if (launches) *launches = h->cnt[kid];
  return RSL_OK;
}

int rsl_rds(rsl_handle h, const void* cube, int F, int A, int C_total, int chirp0, int C, int S, const void* table,
            int dc_removal, void* work, void* rds) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || A <= 0 || S <= 0 || C <= 0 || chirp0 < 0 || chirp0 + C > C_total)
    return fail(h, RSL_ERR_INVALID, "rsl_rds: bad shape");
  if (F == 0) return RSL_OK;  // empty batch: the (zero-size) buffers may be null
  if (!cube || !table || !work || !rds) return fail(h, RSL_ERR_INVALID, "rsl_rds: null pointer");
  if (!rsl_fft_supported(S) || !rsl_fft_supported(C))
    return fail(h, RSL_ERR_UNSUPPORTED, "rsl_rds: FFT size not supported (S=" + std::to_string(S) +
                                            ", C=" + std::to_string(C) + ")");
  hipSetDevice(h->device);
  float2* tS = twiddles(h, S);
  float2* tC = twiddles(h, C);
  if (!tS || !tC) return fail(h, RSL_ERR_HIP, "twiddle table allocation failed");
  bool sup = true;
  hipError_t e;
  {
    Scope sc(h, RSL_K_RANGE_FFT);
    e = rsl::launch_range_fft(h->stream, (const float2*)cube, F, A, C_total, chirp0, C, S, (const float2*)table, tS,
                              dc_removal, (float2*)work, &sup, h->rfq);
  }
  if (int r = hip_check(h, e, "range_fft")) return r;
  {
    Scope sc(h, RSL_K_DOPPLER_FFT);
    e = rsl::launch_doppler_fft(h->stream, (const float2*)work, F, A, C, S, tC, (float2*)rds, &sup);
  }
  return hip_check(h, e, "doppler_fft");
}

// What a detector entry point hands its launcher, from the untyped arguments of the C ABI.
static rsl::DetectArgs detect_args(double thr_power, int i_lo, int i_hi, void* mask, void* row_count, void* db_map,
                                   void* peak_pow) {
  return {thr_power, i_lo, i_hi, (unsigned long long*)mask, (int*)row_count, (float*)db_map, (float*)peak_pow};
}

int rsl_rds_detect(rsl_handle h, const void* cube, int F, int A, int C_total, int chirp0, int C, int S,
                   const void* table, int dc_removal, void* work, void* rds, double thr_power, int i_lo, int i_hi,
                   void* mask, void* row_count, void* db_map, void* peak_pow, int* peak_pow_group) {
  if (!h) return RSL_ERR_INVALID;
  if (peak_pow_group) *peak_pow_group = 1;
  if (F < 0 || A <= 0 || S <= 0 || C <= 0 || chirp0 < 0 || chirp0 + C > C_total)
    return fail(h, RSL_ERR_INVALID, "rsl_rds_detect: bad shape");
  if (F == 0) return RSL_OK;  // empty batch: the (zero-size) buffers may be null
  if (!mask || !row_count) return fail(h, RSL_ERR_INVALID, "rsl_rds_detect: null pointer");
  if (!rsl::doppler_detect_supported(C, S)) {  // unfused: a7 then a8
    if (int r = rsl_rds(h, cube, F, A, C_total, chirp0, C, S, table, dc_removal, work, rds)) return r;
    return rsl_detect(h, rds, F, A, S, C, thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow);
  }
  if (!cube || !table || !work || !rds) return fail(h, RSL_ERR_INVALID, "rsl_rds_detect: null pointer");
  if (!rsl_fft_supported(S)) return fail(h, RSL_ERR_UNSUPPORTED, "rsl_rds_detect: FFT size not supported");
  hipSetDevice(h->device);
  float2* tS = twiddles(h, S);
  float2* tC = twiddles(h, C);
  if (!tS || !tC) return fail(h, RSL_ERR_HIP, "twiddle table allocation failed");
  bool sup = true;
  int group = 1;
  hipError_t e;
  // packed range spectra between K1 and K2 (6 B per value, each bin's exponent inside its 48-B unit; the tiles fill
  // the first 3/4 of the c64-sized work buffer the caller provides)
  const bool packed = rsl::work_packed_supported(C, S);
  {
    Scope sc(h, RSL_K_RANGE_FFT);
    e = rsl::launch_range_fft(h->stream, (const float2*)cube, F, A, C_total, chirp0, C, S, (const float2*)table, tS,
                              dc_removal, (float2*)work, &sup, h->rfq, packed);
  }
  if (int r = hip_check(h, e, "range_fft")) return r;
  {
    Scope sc(h, RSL_K_DOPPLER_FFT);
    const rsl::DetectArgs det = detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow);
    e = rsl::launch_doppler_detect(h->stream, (const float2*)work, F, A, C, S, tC, (float2*)rds, det, &sup, &group,
                                   packed);
  }
  if (peak_pow_group) *peak_pow_group = group;
  return hip_check(h, e, "doppler_detect");
}

int rsl_detect(rsl_handle h, const void* rds, int F, int A, int S, int C, double thr_power, int i_lo, int i_hi,
               void* mask, void* row_count, void* db_map, void* peak_pow) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || A <= 0 || S <= 0 || C <= 0) return fail(h, RSL_ERR_INVALID, "rsl_detect: bad shape");
  if (F == 0) return RSL_OK;
  if (!rds || !mask || !row_count) return fail(h, RSL_ERR_INVALID, "rsl_detect: null pointer");
  if (!rsl::detect_rows(C)) return fail(h, RSL_ERR_UNSUPPORTED, "rsl_detect: C too large");
  Scope sc(h, RSL_K_DETECT);
  const rsl::DetectArgs det = detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow);
  return hip_check(h, rsl::launch_detect(h->stream, (const float2*)rds, F, A, S, C, det), "detect");
}

// rsl_detect_cfar (rank null) and rsl_detect_oscfar (its rank), and rsl_detect_power's two CFAR rules (power: `maps`
// holds F fp32 power maps and A is 1): the checks in the order the header lists them, `fn` naming the entry point in the
// error text, then the launch.  No LDS check: every window within the limits fits at every C <= RSL_CFAR_MAX_C, which
// rsl_cfar.hip and rsl_oscfar.hip assert at compile time.
static int detect_cfar_family(rsl_handle h, const std::string& fn, const void* maps, bool power, int F, int A, int S,
                              int C, rsl::CfarWindow win, const double* rank, double alpha,
                              const rsl::DetectArgs& det) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || A <= 0 || S <= 0 || C <= 0 || S > 8192) return fail(h, RSL_ERR_INVALID, fn + ": bad shape");
  if (win.gr < 0 || win.gd < 0 || win.tr < 0 || win.td < 0 || win.tr + win.td < 1)
    return fail(h, RSL_ERR_INVALID, fn + ": bad window (half-sizes >= 0, at least one training cell)");
  if (win.hr() > RSL_CFAR_MAX_HALF || win.hd() > RSL_CFAR_MAX_HALF)
    return fail(h, RSL_ERR_INVALID, fn + ": window half-size above RSL_CFAR_MAX_HALF");
  if (win.nfull() > C || 2 * win.hr() + 1 > S) return fail(h, RSL_ERR_INVALID, fn + ": window larger than the map");
  if (!(alpha > 0) || !std::isfinite(alpha)) return fail(h, RSL_ERR_INVALID, fn + ": alpha must be finite, > 0");
  if (C > RSL_CFAR_MAX_C) return fail(h, RSL_ERR_UNSUPPORTED, fn + ": C above RSL_CFAR_MAX_C");
  if (rank && !(*rank > 0 && *rank <= 1)) return fail(h, RSL_ERR_INVALID, fn + ": rank must lie in (0, 1]");
  if (F == 0) return RSL_OK;
  if (!maps || !det.mask || !det.row_count) return fail(h, RSL_ERR_INVALID, fn + ": null pointer");
  Scope sc(h, RSL_K_DETECT);
  const float2* z = (const float2*)maps;
  const float* p = (const float*)maps;
  const float af = (float)alpha;
  if (rank)
    return hip_check(h,
                     power ? rsl::launch_detect_oscfar(h->stream, p, F, S, C, win, *rank, af, det)
                           : rsl::launch_detect_oscfar(h->stream, z, F, A, S, C, win, *rank, af, det),
                     "detect_oscfar");
  return hip_check(h,
                   power ? rsl::launch_detect_cfar(h->stream, p, F, S, C, win, af, det)
                         : rsl::launch_detect_cfar(h->stream, z, F, A, S, C, win, af, det),
                   "detect_cfar");
}

int rsl_detect_cfar(rsl_handle h, const void* rds, int F, int A, int S, int C, int guard_r, int guard_d, int train_r,
                    int train_d, double alpha, double thr_power, int i_lo, int i_hi, void* mask, void* row_count,
                    void* db_map, void* peak_pow) {
  return detect_cfar_family(h, "rsl_detect_cfar", rds, false, F, A, S, C, {guard_r, guard_d, train_r, train_d},
                            nullptr, alpha, detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow));
}

int rsl_detect_oscfar(rsl_handle h, const void* rds, int F, int A, int S, int C, int guard_r, int guard_d,
                      int train_r, int train_d, double rank, double alpha, double thr_power, int i_lo, int i_hi,
                      void* mask, void* row_count, void* db_map, void* peak_pow) {
  // the factor is checked as the float the kernel multiplies by
  return detect_cfar_family(h, "rsl_detect_oscfar", rds, false, F, A, S, C, {guard_r, guard_d, train_r, train_d},
                            &rank, (float)alpha,
                            detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow));
}

int rsl_power_integrate(rsl_handle h, const void* rds, int F, int A, int S, int C, void* power) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || A <= 0 || S <= 0 || C <= 0) return fail(h, RSL_ERR_INVALID, "rsl_power_integrate: bad shape");
  if (A > 32) return fail(h, RSL_ERR_INVALID, "rsl_power_integrate: more than 32 antennas");
  if (F == 0) return RSL_OK;
  if (!rds || !power) return fail(h, RSL_ERR_INVALID, "rsl_power_integrate: null pointer");
  Scope sc(h, RSL_K_DETECT);
  return hip_check(h, rsl::launch_power_integrate(h->stream, (const float2*)rds, F, A, S, C, (float*)power),
                   "power_integrate");
}

int rsl_detect_power(rsl_handle h, const void* power, int F, int S, int C, int rule, int guard_r, int guard_d,
                     int train_r, int train_d, double rank, double alpha, double thr_power, int i_lo, int i_hi,
                     void* mask, void* row_count, void* db_map, void* peak_pow) {
  if (!h) return RSL_ERR_INVALID;
  const rsl::DetectArgs det = detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow);
  const rsl::CfarWindow win = {guard_r, guard_d, train_r, train_d};
  switch (rule) {
    case RSL_RULE_THRESHOLD: {  // rsl_detect's checks; window, rank and alpha are not looked at
      if (F < 0 || S <= 0 || C <= 0) return fail(h, RSL_ERR_INVALID, "rsl_detect_power: bad shape");
      if (F == 0) return RSL_OK;
      if (!power || !mask || !row_count) return fail(h, RSL_ERR_INVALID, "rsl_detect_power: null pointer");
      if (!rsl::detect_rows(C)) return fail(h, RSL_ERR_UNSUPPORTED, "rsl_detect_power: C too large");
      Scope sc(h, RSL_K_DETECT);
      return hip_check(h, rsl::launch_detect(h->stream, (const float*)power, F, S, C, det), "detect");
    }
    case RSL_RULE_CA:
      return detect_cfar_family(h, "rsl_detect_power", power, true, F, 1, S, C, win, nullptr, alpha, det);
    case RSL_RULE_OS:
      return detect_cfar_family(h, "rsl_detect_power", power, true, F, 1, S, C, win, &rank, (float)alpha, det);
    default:
      return fail(h, RSL_ERR_INVALID, "rsl_detect_power: unknown rule");
  }
}

int rsl_peak_offsets(rsl_handle h, const void* mask, const void* row_count, int F, int A, int S, int C,
                     void* entry_row_off, void* cell_row_off, void* scratch, void* entry_base, void* cell_base,
                     void* frame_counts, void* union_mask) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || A <= 0 || S <= 0 || C <= 0 || A > 32) return fail(h, RSL_ERR_INVALID, "rsl_peak_offsets: bad shape");
  if (!entry_base || !cell_base) return fail(h, RSL_ERR_INVALID, "rsl_peak_offsets: null pointer");
  if (F > 0 && (!mask || !row_count || !entry_row_off || !cell_row_off || !scratch || !frame_counts))
    return fail(h, RSL_ERR_INVALID, "rsl_peak_offsets: null pointer");
  if (F == 0) {
    hipSetDevice(h->device);
    long long z = 0;
    hipMemcpyAsync(entry_base, &z, 8, hipMemcpyHostToDevice, h->stream);
    hipMemcpyAsync(cell_base, &z, 8, hipMemcpyHostToDevice, h->stream);
    return hip_check(h, hipStreamSynchronize(h->stream), "offsets(F=0)");
  }
  Scope sc(h, RSL_K_OFFSETS);
  return hip_check(h,
                   rsl::launch_offsets(h->stream, (const unsigned long long*)mask, (const int*)row_count, F, A, S, C,
                                       (int*)entry_row_off, (int*)cell_row_off, (int*)scratch,
                                       (long long*)entry_base, (long long*)cell_base, (long long*)frame_counts,
                                       (unsigned long long*)union_mask),
                   "offsets");
}

int rsl_peak_emit(rsl_handle h, const void* rds, const void* mask, const void* union_mask, const void* peak_pow,
                  int peak_pow_group, int F, int A, int S, int C, const void* entry_row_off, const void* cell_row_off, const void* entry_base,
                  const void* cell_base, long long entry_cap, long long cell_cap, void* e_coord, void* e_cell,
                  void* e_pdb, void* c_frame, void* c_rc, void* c_amask) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || A <= 0 || A > 32 || S <= 0 || C <= 0 || S > 8192 || C > 8192)
    return fail(h, RSL_ERR_INVALID, "rsl_peak_emit: bad shape");
  if (F == 0) return RSL_OK;
  if (!mask || !entry_row_off || !cell_row_off || !entry_base || !cell_base)
    return fail(h, RSL_ERR_INVALID, "rsl_peak_emit: null pointer");
  if ((entry_cap > 0 && (!e_coord || !e_cell)) || (cell_cap > 0 && (!c_frame || !c_rc || !c_amask)))
    return fail(h, RSL_ERR_INVALID, "rsl_peak_emit: null output");
  if (peak_pow && (peak_pow_group < 1 || S % peak_pow_group != 0))
    return fail(h, RSL_ERR_INVALID, "rsl_peak_emit: peak_pow_group must divide S");
  Scope sc(h, RSL_K_EMIT);
  if (rsl::emit_compact_supported(C, union_mask, peak_pow, e_pdb))
    return hip_check(h,
                     rsl::launch_emit_compact(h->stream, (const unsigned long long*)mask,
                                              (const unsigned long long*)union_mask, (const float*)peak_pow,
                                              peak_pow_group, F, A, S, C, (const int*)entry_row_off,
                                              (const int*)cell_row_off, (const long long*)entry_base,
                                              (const long long*)cell_base, entry_cap, cell_cap, (unsigned*)e_coord,
                                              (int*)e_cell, (float*)e_pdb, (int*)c_frame, (int*)c_rc,
                                              (unsigned*)c_amask),
                     "emit2");
  if (!rds) return fail(h, RSL_ERR_INVALID, "rsl_peak_emit: rds needed without union_mask / peak_pow");
  return hip_check(h,
                   rsl::launch_emit_rows(h->stream, (const float2*)rds, (const unsigned long long*)mask, F, A, S, C,
                                         (const int*)entry_row_off, (const int*)cell_row_off,
                                         (const long long*)entry_base, (const long long*)cell_base, entry_cap,
                                         cell_cap, (unsigned*)e_coord, (int*)e_cell, (float*)e_pdb, (int*)c_frame,
                                         (int*)c_rc, (unsigned*)c_amask),
                   "emit");
}

long long rsl_steer_table_floats(int G, int M) {
  if (G <= 0 || M <= 0) return 0;
  return rsl::steer_layout(G, M).total_floats;
}

int rsl_steer_table_build(const double* steer, int G, int M, float* out, int* ntiles_out, int* flags_out) {
  if (!steer || !out || G <= 0 || M <= 0 || M > 16) return RSL_ERR_INVALID;
  const rsl::SteerLayout lay = rsl::steer_layout(G, M);
  const int KS = lay.ks, KSG = lay.ksg, ntiles = lay.ntiles16;
  for (int t = 0; t < ntiles; ++t)
    for (int sg = 0; sg < KSG; ++sg)
      for (int lane = 0; lane < 64; ++lane)
        for (int e = 0; e < 4; ++e) {
          const int s = 4 * sg + e;
          const int i = lane & 15, qq = lane >> 4;
          const int k = 4 * s + qq;
          const int g = 8 * t + (i >> 1), part = i & 1;
          double v = 0.0;
          if (s < KS && g < G && k < 2 * M) {
            const int m = k < M ? k : k - M;
            const double ar = steer[((size_t)g * M + m) * 2], ai = steer[((size_t)g * M + m) * 2 + 1];
            if (part == 0) v = k < M ? ar : ai;
            else v = k < M ? -ai : ar;
          }
          out[(((size_t)t * KSG + sg) * 64 + lane) * 4 + e] = (float)v;
        }
  if (ntiles_out) *ntiles_out = ntiles;
  const int uni = rsl::toep_table_build(steer, G, M, reinterpret_cast<uint16_t*>(out + lay.f32_floats));
  if (flags_out) *flags_out = (uni && lay.toep_fits) ? RSL_STEER_TOEPLITZ : 0;
  double* tT = reinterpret_cast<double*>(out + lay.t64_offset);
  for (int m = 0; m < M; ++m)
    for (int g = 0; g < G; ++g) {
      tT[((size_t)m * G + g) * 2] = steer[((size_t)g * M + m) * 2];
      tT[((size_t)m * G + g) * 2 + 1] = steer[((size_t)g * M + m) * 2 + 1];
    }
  return RSL_OK;
}

int rsl_doa(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
            const void* ncell_dev, long long ncell, const void* steer_tab, const void* steer_c128, int G, int method,
            void* out_idx, void* out_gmax, void* out_spec) {
  if (!h) return RSL_ERR_INVALID;
  if (A <= 0 || A > 16 || S <= 0 || C <= 0 || G <= 0) return fail(h, RSL_ERR_INVALID, "rsl_doa: bad shape");
  if (!rds || !c_frame || !c_rc || !steer_tab || !out_idx) return fail(h, RSL_ERR_INVALID, "rsl_doa: null pointer");
  const int base_method = method & 0xff;
  const bool toep = (method & RSL_DOA_TOEPLITZ) != 0;
  if (base_method != RSL_METHOD_MUSIC && base_method != RSL_METHOD_BEAMFORMING)
    return fail(h, RSL_ERR_INVALID, "rsl_doa: unknown method");
  const bool music = base_method == RSL_METHOD_MUSIC;
  (void)steer_c128;  // the exact re-scan reads the fp64 copy inside steer_tab (rsl_steer_table_build)
  const SteerView tab = steer_view(steer_tab, G, A);
  const rsl::CellList cl = cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell);
  if (!ncell_dev && ncell <= 0) return RSL_OK;
  Scope sc(h, RSL_K_DOA_SCAN);
  // the Toeplitz f16-MFMA scan: argmax only, or with the whole spectrum in the cell-blocked layout (no gmax there)
  const bool toep_spec = out_spec && (method & RSL_DOA_SPEC_BLOCKED) && !out_gmax;
  if (toep && (!out_spec || toep_spec) && tab.lay.toep_fits)
    return hip_check(h,
                     rsl::launch_doa_toep(h->stream, cl, tab.toep, G, music, tab.t64, (int*)out_idx, (float*)out_gmax,
                                          0.0, nullptr, nullptr, toep_spec ? (float*)out_spec : nullptr),
                     "doa_toep");
  const long long spec_ld = (method & RSL_DOA_SPEC_BLOCKED) ? -1 : (method & RSL_DOA_SPEC_GMAJOR) ? ncell : 0;
  if (int r = hip_check(h,
                        rsl::launch_doa_scan(h->stream, cl, tab.f32, G, music, (int*)out_idx, (float*)out_gmax,
                                             (float*)out_spec, spec_ld),
                        "doa_scan"))
    return r;
  // the cells the f32 scan marked ambiguous: exact fp64 argmax (rsl_doa_toep.hip k_doa_fixup)
  return hip_check(h, rsl::launch_doa_fixup(h->stream, cl, G, music, tab.t64, (int*)out_idx, (float*)out_gmax),
                   "doa_fixup");
}

int rsl_doa_extras(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                   const void* ncell_dev, long long ncell, const void* steer_tab, const void* steer_c128, int G,
                   int method, double esprit_scale, void* out_idx, void* out_gmax, void* esprit_deg, void* phase) {
  if (!h) return RSL_ERR_INVALID;
  if (A < 2 || A > 16 || S <= 0 || C <= 0 || G <= 0) return fail(h, RSL_ERR_INVALID, "rsl_doa_extras: bad shape");
  if (!rds || !c_frame || !c_rc || !steer_tab || !out_idx)
    return fail(h, RSL_ERR_INVALID, "rsl_doa_extras: null pointer");
  if (method != RSL_METHOD_MUSIC && method != RSL_METHOD_BEAMFORMING)
    return fail(h, RSL_ERR_INVALID, "rsl_doa_extras: unknown method");
  const bool music = method == RSL_METHOD_MUSIC;
  (void)steer_c128;  // the exact re-scan reads the fp64 copy inside steer_tab (rsl_steer_table_build)
  const SteerView tab = steer_view(steer_tab, G, A);
  if (!tab.lay.toep_fits)
    return fail(h, RSL_ERR_UNSUPPORTED, "rsl_doa_extras: grid too large for the Toeplitz path (use rsl_doa)");
  if (!ncell_dev && ncell <= 0) return RSL_OK;
  Scope sc(h, RSL_K_DOA_SCAN);
  return hip_check(h,
                   rsl::launch_doa_toep(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell), tab.toep,
                                        G, music, tab.t64, (int*)out_idx, (float*)out_gmax, esprit_scale,
                                        (double*)esprit_deg, (double*)phase),
                   "doa_extras");
}

int rsl_doa_smoothed(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                     const void* ncell_dev, long long ncell, const void* steer_sub_c64, int G, int L, int nmax,
                     int num_sources, double rel, void* out_nsrc, void* out_idx, void* out_den, void* out_eig,
                     void* out_spec) {
  if (!h) return RSL_ERR_INVALID;
  if (A < 3 || A > 16 || S <= 0 || C <= 0) return fail(h, RSL_ERR_INVALID, "rsl_doa_smoothed: bad shape (3 <= A <= 16)");
  if (L < 2 || L > A || L > RSL_SS_MAX_L)
    return fail(h, RSL_ERR_INVALID, "rsl_doa_smoothed: sub-array length outside [2, min(A, RSL_SS_MAX_L)]");
  if (nmax < 1 || nmax > L - 1) return fail(h, RSL_ERR_INVALID, "rsl_doa_smoothed: nmax outside [1, L - 1]");
  if (num_sources < 0 || num_sources > nmax)
    return fail(h, RSL_ERR_INVALID, "rsl_doa_smoothed: num_sources outside [0, nmax]");
  if (!(rel > 0.0 && rel < 1.0)) return fail(h, RSL_ERR_INVALID, "rsl_doa_smoothed: rel outside (0, 1)");
  if (G < 3) return fail(h, RSL_ERR_INVALID, "rsl_doa_smoothed: G < 3");
  if (!rds || !c_frame || !c_rc || !steer_sub_c64 || !out_nsrc || !out_idx)
    return fail(h, RSL_ERR_INVALID, "rsl_doa_smoothed: null pointer");
  if (ncell <= 0) return RSL_OK;  // ncell is the launch bound (capacity) when ncell_dev is given
  Scope sc(h, RSL_K_DOA_SCAN);
  return hip_check(h,
                   rsl::launch_doa_smoothed(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell),
                                            (const float2*)steer_sub_c64, G, L, nmax, num_sources, (float)rel,
                                            (int*)out_nsrc, (int*)out_idx, (float*)out_den, (float*)out_eig,
                                            (float*)out_spec),
                   "doa_smoothed");
}

int rsl_range_cov(rsl_handle h, const void* rds, int F, int A, int S, int C, int c0, int c1, void* cov) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || S <= 0 || C <= 0) return fail(h, RSL_ERR_INVALID, "rsl_range_cov: bad shape");
  if (A < 2 || A > RSL_RA_MAX_A) return fail(h, RSL_ERR_INVALID, "rsl_range_cov: antennas outside [2, RSL_RA_MAX_A]");
  if (c0 < 0 || c0 >= c1 || c1 > C) return fail(h, RSL_ERR_INVALID, "rsl_range_cov: window needs 0 <= c0 < c1 <= C");
  if (F == 0) return RSL_OK;
  if (!rds || !cov) return fail(h, RSL_ERR_INVALID, "rsl_range_cov: null pointer");
  Scope sc(h, RSL_K_DOA_SCAN);
  return hip_check(h, rsl::launch_range_cov(h->stream, (const float2*)rds, F, A, S, C, c0, c1, (float2*)cov),
                   "range_cov");
}

int rsl_range_azimuth(rsl_handle h, const void* cov, long long n, int A, const void* steer_c64, int G, int method,
                      double loading, void* map, void* arg) {
  if (!h) return RSL_ERR_INVALID;
  if (n < 0) return fail(h, RSL_ERR_INVALID, "rsl_range_azimuth: n < 0");
  if (method != RSL_RA_BARTLETT && method != RSL_RA_CAPON)
    return fail(h, RSL_ERR_INVALID, "rsl_range_azimuth: method must be RSL_RA_BARTLETT or RSL_RA_CAPON");
  if (A < 2 || A > RSL_RA_MAX_A)
    return fail(h, RSL_ERR_INVALID, "rsl_range_azimuth: antennas outside [2, RSL_RA_MAX_A]");
  if (G < 1) return fail(h, RSL_ERR_INVALID, "rsl_range_azimuth: G < 1");
  if (!(loading >= RSL_RA_MIN_LOADING && loading <= 1.0))
    return fail(h, RSL_ERR_INVALID, "rsl_range_azimuth: loading outside [RSL_RA_MIN_LOADING, 1]");
  if (n == 0) return RSL_OK;
  if (!cov || !steer_c64 || !map) return fail(h, RSL_ERR_INVALID, "rsl_range_azimuth: null pointer");
  Scope sc(h, RSL_K_DOA_SCAN);
  return hip_check(h,
                   rsl::launch_range_azimuth(h->stream, (const float2*)cov, n, A, (const float2*)steer_c64, G,
                                             method == RSL_RA_CAPON, (float)loading, (float*)map, (int*)arg),
                   "range_azimuth");
}

int rsl_cell_extras(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                    const void* ncell_dev, long long ncell, double esprit_scale, const void* gidx,
                    const void* az_table, void* sig_out, void* esprit_deg, void* phase, void* az_out) {
  if (!h) return RSL_ERR_INVALID;
  if (A <= 0 || A > 32 || S <= 0 || C <= 0) return fail(h, RSL_ERR_INVALID, "rsl_cell_extras: bad shape");
  if (A < 2) return fail(h, RSL_ERR_INVALID, "rsl_cell_extras: needs at least 2 antennas");  // phase reads s0 and s1
  if (!rds || !c_frame || !c_rc) return fail(h, RSL_ERR_INVALID, "rsl_cell_extras: null pointer");
  if (az_out && (!gidx || !az_table)) return fail(h, RSL_ERR_INVALID, "rsl_cell_extras: az_out needs gidx+table");
  if (ncell <= 0) return RSL_OK;  // ncell is the launch bound (capacity) when ncell_dev is given
  Scope sc(h, RSL_K_CELL_EXTRAS);
  return hip_check(h,
                   rsl::launch_cell_extras(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell),
                                           esprit_scale, (const int*)gidx, (const double*)az_table, (float2*)sig_out,
                                           (double*)esprit_deg, (double*)phase, (double*)az_out),
                   "cell_extras");
}

int rsl_cell_refine(rsl_handle h, const void* rds, const void* power, int A, int S, int C, const void* c_frame,
                    const void* c_rc, const void* ncell_dev, long long ncell, const void* gidx, const void* az_table,
                    const void* steer_c64, int G, int range_mode, int doppler_mode, const double* axes4,
                    void* out_points, void* out_az) {
  if (!h) return RSL_ERR_INVALID;
  if (A < 2 || A > 32) return fail(h, RSL_ERR_INVALID, "rsl_cell_refine: antennas outside [2, 32]");
  if (S <= 0 || C <= 0 || G <= 0) return fail(h, RSL_ERR_INVALID, "rsl_cell_refine: bad shape");
  for (int mode : {range_mode, doppler_mode})
    if (mode < RSL_REFINE_NONE || mode > RSL_REFINE_HANN)
      return fail(h, RSL_ERR_INVALID, "rsl_cell_refine: unknown RSL_REFINE_* mode");
  if (axes4 && !(std::isfinite(axes4[1]) && std::isfinite(axes4[3])))
    return fail(h, RSL_ERR_INVALID, "rsl_cell_refine: an axis step is not finite");
  if (!out_points && !out_az) return fail(h, RSL_ERR_INVALID, "rsl_cell_refine: both outputs null");
  if (reinterpret_cast<size_t>(out_points) & 15)
    return fail(h, RSL_ERR_INVALID, "rsl_cell_refine: out_points is not 16-byte aligned");
  if (ncell <= 0) return RSL_OK;  // ncell is the launch bound (capacity) when ncell_dev is given
  if (!rds || !c_frame || !c_rc || !gidx || !az_table || !steer_c64 || !axes4)
    return fail(h, RSL_ERR_INVALID, "rsl_cell_refine: null pointer");
  Scope sc(h, RSL_K_CELL_EXTRAS);
  return hip_check(h,
                   rsl::launch_cell_refine(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell),
                                           (const float*)power, (const int*)gidx, (const double*)az_table,
                                           (const float2*)steer_c64, G, range_mode, doppler_mode, axes4,
                                           (float*)out_points, (double*)out_az),
                   "cell_refine");
}

int rsl_confidence(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                   long long n, const void* gidx, const void* steer_c128, const void* steer_phase, void* conf) {
  if (!h) return RSL_ERR_INVALID;
  if (A <= 0 || A > 32 || S <= 0 || C <= 0) return fail(h, RSL_ERR_INVALID, "rsl_confidence: bad shape");
  if (!rds || !c_frame || !c_rc || !gidx || !steer_c128 || !steer_phase || !conf)
    return fail(h, RSL_ERR_INVALID, "rsl_confidence: null pointer");
  Scope sc(h, RSL_K_CONFIDENCE);
  return hip_check(h,
                   rsl::launch_confidence(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, nullptr, n),
                                          (const int*)gidx, (const double*)steer_c128, (const double*)steer_phase,
                                          (double*)conf),
                   "confidence");
}

// The checks rsl_velocity, rsl_velocity_robust and rsl_velocity_consensus (fn) share, in one order: the counts; the
// entry point's own scalars (own: the message of the first that fails, else null); the ridge; an empty batch (RSL_OK
// with p->F = 0: nothing to launch); the pointers; the grid table; the box.  Fills *p with the typed problem.
static int velocity_problem(rsl_handle h, const char* fn, const char* own, const void* az, const void* gidx,
                            const void* az_table, int G, const void* y, const void* amask, const void* seg, long long n,
                            int F, double k, double ridge, const double* bounds4, const void* out, rsl::VelProblem* p) {
  *p = {};
  if (!h) return RSL_ERR_INVALID;
  auto bad = [&](const char* what) { return fail(h, RSL_ERR_INVALID, std::string(fn) + ": " + what); };
  if (F < 0 || n < 0) return bad("bad argument");
  if (own) return bad(own);
  if (!(ridge >= 0)) return bad("ridge must be >= 0");
  if (F == 0) return RSL_OK;
  if ((!az && !gidx) || !y || !seg || !bounds4 || !out) return bad("null pointer");
  if (gidx && (!az_table || G <= 0 || G > 2048)) return bad("bad grid table");
  if (!(bounds4[0] <= bounds4[1]) || !(bounds4[2] <= bounds4[3])) return bad("bad bounds");
  *p = {(const double*)az, (const int*)gidx, (const double*)az_table, G, (const double*)y, (const unsigned*)amask,
        (const long long*)seg, n, F, k, ridge, bounds4[0], bounds4[1], bounds4[2], bounds4[3]};
  return RSL_OK;
}

int rsl_velocity(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G, const void* y,
                 const void* amask, const void* seg, long long n, int F, double k, double ridge, const double* bounds4,
                 void* out, void* resid, void* pred) {
  rsl::VelProblem p;
  const int rc = velocity_problem(h, "rsl_velocity", nullptr, az, gidx, az_table, G, y, amask, seg, n, F, k, ridge,
                                  bounds4, out, &p);
  if (rc || p.F == 0) return rc;
  Scope sc(h, RSL_K_VELOCITY);
  return hip_check(h, rsl::launch_velocity(h->stream, p, (double*)out, (double*)resid, (double*)pred), "velocity");
}

int rsl_velocity_robust(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G, const void* y,
                        const void* amask, const void* seg, long long n, int F, double k, double ridge,
                        const double* bounds4, int loss, double c, double scale, int iters, double tol, void* out,
                        void* weight, void* resid) {
  const char* own = (loss != RSL_LOSS_HUBER && loss != RSL_LOSS_TUKEY) ? "loss must be RSL_LOSS_HUBER or RSL_LOSS_TUKEY"
                    : (!(c > 0) || !std::isfinite(c))                  ? "c must be finite, > 0"
                    : (std::isnan(scale) || (std::isinf(scale) && scale > 0))
                        ? "scale must be finite (<= 0: estimated)"
                    : (iters < 1 || iters > 1000) ? "iters outside 1..1000"
                    : !(tol >= 0)                 ? "tol must be >= 0"
                                                  : nullptr;
  rsl::VelProblem p;
  const int rc = velocity_problem(h, "rsl_velocity_robust", own, az, gidx, az_table, G, y, amask, seg, n, F, k, ridge,
                                  bounds4, out, &p);
  if (rc || p.F == 0) return rc;
  Scope sc(h, RSL_K_VELOCITY);
  return hip_check(h,
                   rsl::launch_velocity_robust(h->stream, p, loss, c, scale, iters, tol, (double*)out, (float*)weight,
                                               (double*)resid),
                   "velocity_robust");
}

int rsl_velocity_consensus(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G, const void* y,
                           const void* amask, const void* seg, long long n, int F, double k, double ridge,
                           const double* bounds4, double c, double scale, int hyps, double min_det, int refine,
                           unsigned long long seed, long long frame0, void* out, void* weight, void* resid) {
  const char* own = (!(c > 0) || !std::isfinite(c))           ? "c must be finite, > 0"
                    : (!(scale > 0) || !std::isfinite(scale)) ? "scale must be finite, > 0"
                    : (hyps < 1 || hyps > RSL_CONSENSUS_MAX_H) ? "hyps outside 1..RSL_CONSENSUS_MAX_H"
                    : (!(min_det > 0) || !(min_det <= 1))     ? "min_det outside (0, 1]"
                    : (refine < 0 || refine > 100)            ? "refine outside 0..100"
                    : frame0 < 0                              ? "frame0 must be >= 0"
                                                              : nullptr;
  rsl::VelProblem p;
  const int rc = velocity_problem(h, "rsl_velocity_consensus", own, az, gidx, az_table, G, y, amask, seg, n, F, k,
                                  ridge, bounds4, out, &p);
  if (rc || p.F == 0) return rc;
  Scope sc(h, RSL_K_VELOCITY);
  return hip_check(h,
                   rsl::launch_velocity_consensus(h->stream, p, c, scale, hyps, min_det, refine, seed, frame0,
                                                  (double*)out, (float*)weight, (double*)resid),
                   "velocity_consensus");
}

int rsl_scan_register(rsl_handle h, const void* points, const void* seg, int F, long long n, const void* weight,
                      const void* rc, int C, const double* axes4, const void* prev_points, const void* prev_weight,
                      const void* prev_rc, long long prev_n, const void* prev_n_dev, const void* init, double h_fine,
                      double h_coarse, double dtheta, int K, int iters, double shrink, double tol, double w_min,
                      double dt, void* out, void* omega) {
  if (!h) return RSL_ERR_INVALID;
  auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
  const bool cull = rc || prev_rc;
  const char* why = !(pos(h_fine) && pos(h_coarse) && pos(dtheta) && pos(dt))
                        ? "h, h_coarse, dtheta and dt must be finite, > 0"
                    : !(std::isfinite(w_min) && w_min >= 0.0)                ? "w_min must be finite, >= 0"
                    : std::isnan(tol)                                        ? "tol is NaN"
                    : h_coarse < h_fine                                      ? "h_coarse < h"
                    : (K < 0 || K > RSL_REG_MAX_K)                           ? "K outside 0..RSL_REG_MAX_K"
                    : (iters < 0 || iters > RSL_REG_MAX_ITERS)               ? "iters outside 0..RSL_REG_MAX_ITERS"
                    : !(shrink > 0.0 && shrink <= 1.0)                       ? "shrink outside (0, 1]"
                    : (F < 0 || n < 0 || prev_n < 0)                         ? "negative count"
                    : (cull && (!axes4 || C <= 0 || !pos(axes4[1]) || !std::isfinite(axes4[0])))
                        ? "rc needs C > 0 and axes4 with a finite r0 and a finite r_step > 0"
                    : (F > 0 && (!points || !seg || !out)) ? "null points, seg or out"
                                                           : nullptr;
  if (why) {
    const std::string msg = std::string("rsl_scan_register: ") + why;
    return fail(h, RSL_ERR_INVALID, msg.c_str());
  }
  if (F == 0) return RSL_OK;
  const rsl::RegProblem p{cloud_view(points, seg, n, F, weight), (const int*)rc, cull ? C : 1,
                          cull ? axes4[0] : 0.0, cull ? 1.0 / axes4[1] : 0.0,
                          (const float*)prev_points, prev_points ? (const float*)prev_weight : nullptr,
                          prev_points ? (const int*)prev_rc : nullptr, prev_points ? prev_n : 0,
                          prev_points ? (const long long*)prev_n_dev : nullptr, (const double*)init, h_fine, h_coarse,
                          dtheta, K, iters, shrink, tol, w_min, dt};
  Scope sc(h, RSL_K_AUX);
  return hip_check(h, rsl::launch_scan_register(h->stream, p, (double*)out, (double*)omega), "scan_register");
}

int rsl_map_update(rsl_handle h, const void* points, const void* seg, int F, long long n, const void* weight,
                   const void* poses, const double* grid4, int nx, int ny, double r_min, double r_max, double min_db,
                   void* hits, void* free_, void* stats) {
  if (!h) return RSL_ERR_INVALID;
  const bool grid_ok = grid4 && std::isfinite(grid4[0]) && std::isfinite(grid4[1]) && std::isfinite(grid4[2]) &&
                       grid4[2] > 0.0;
  const char* why = (F < 0 || n < 0)                                      ? "negative count"
                    : (F > 0 && (!points || !seg || !poses || !grid4 || !hits)) ? "null points, seg, poses, grid4 or hits"
                    : (grid4 && !grid_ok)                                 ? "x0, y0 and cell must be finite, cell > 0"
                    : !(r_min >= 0.0)                                     ? "r_min must be >= 0"
                    : !(std::isfinite(r_max) && r_max >= r_min)           ? "r_max must be finite, >= r_min"
                    : (std::isnan(min_db) || min_db == INFINITY)          ? "min_db is NaN or +inf"
                    : (nx <= 0 || ny <= 0 || (long long)nx * ny >= (1ll << 31)) ? "nx, ny must be > 0, nx ny < 2^31"
                                                                          : nullptr;
  if (why) {
    const std::string msg = std::string("rsl_map_update: ") + why;
    return fail(h, RSL_ERR_INVALID, msg.c_str());
  }
  if (!grid4) return RSL_OK;  // only with F = 0
  const double inv = 1.0 / grid4[2], rw = std::ceil(r_max * inv) + 1.0;
  if (!(rw <= (double)RSL_MAP_MAX_RW))
    return fail(h, RSL_ERR_UNSUPPORTED, "rsl_map_update: ceil(r_max / cell) + 1 above RSL_MAP_MAX_RW");
  if (F == 0) return RSL_OK;
  const rsl::MapProblem p{cloud_view(points, seg, n, F, weight), (const double*)poses, grid4[0], grid4[1], inv, nx, ny,
                          (int)rw, r_min * r_min, r_max * r_max, min_db};
  Scope sc(h, RSL_K_AUX);
  return hip_check(h, rsl::launch_map_update(h->stream, p, (unsigned*)hits, (unsigned*)free_, (int*)stats),
                   "map_update");
}

int rsl_map_logodds(rsl_handle h, const void* hits, const void* free_, long long ncells, double l_occ, double l_free,
                    double l_min, double l_max, void* out) {
  if (!h) return RSL_ERR_INVALID;
  if (!(std::isfinite(l_occ) && std::isfinite(l_free) && std::isfinite(l_min) && std::isfinite(l_max)))
    return fail(h, RSL_ERR_INVALID, "rsl_map_logodds: l_occ, l_free, l_min and l_max must be finite");
  if (l_min > l_max) return fail(h, RSL_ERR_INVALID, "rsl_map_logodds: l_min > l_max");
  if (ncells < 0 || (ncells > 0 && (!hits || !out)))
    return fail(h, RSL_ERR_INVALID, "rsl_map_logodds: negative count, or null hits or out");
  if (ncells == 0) return RSL_OK;
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_map_logodds(h->stream, (const unsigned*)hits, (const unsigned*)free_, ncells, l_occ,
                                           l_free, l_min, l_max, (float*)out),
                   "map_logodds");
}

int rsl_preprocess_rows(rsl_handle h, const void* in, long long rows, int S, const void* table, int dc, void* out) {
  if (!h) return RSL_ERR_INVALID;
  if (rows < 0 || S <= 0 || !in || !table || !out) return fail(h, RSL_ERR_INVALID, "rsl_preprocess_rows: bad argument");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h, rsl::launch_preprocess_rows(h->stream, (const float2*)in, rows, S, (const float2*)table, dc,
                                                  (float2*)out),
                   "preprocess_rows");
}

int rsl_phase_model(rsl_handle h, const void* pos, const void* ang, long long n, const void* x, double k,
                    const void* y, int wrap, double ridge, void* pred, void* resid, void* cost) {
  if (!h) return RSL_ERR_INVALID;
  if (n < 0 || !pos || !ang || !x) return fail(h, RSL_ERR_INVALID, "rsl_phase_model: bad argument");
  if ((resid || cost) && !y) return fail(h, RSL_ERR_INVALID, "rsl_phase_model: residual/cost need y");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h, rsl::launch_phase_model(h->stream, (const double*)pos, (const double*)ang, n, (const double*)x,
                                              k, (const double*)y, wrap, ridge, (double*)pred, (double*)resid,
                                              (double*)cost),
                   "phase_model");
}

int rsl_bvls(rsl_handle h, const void* pos, const void* ang, long long n, const void* y, double k, int nv,
             double ridge, const void* lo, const void* hi, void* out) {
  if (!h) return RSL_ERR_INVALID;
  if (n < 0 || (nv != 3 && nv != 6) || !pos || !ang || !y || !lo || !hi || !out || ridge < 0)
    return fail(h, RSL_ERR_INVALID, "rsl_bvls: bad argument");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h, rsl::launch_bvls(h->stream, (const double*)pos, (const double*)ang, n, (const double*)y, k, nv,
                                       ridge, (const double*)lo, (const double*)hi, (double*)out),
                   "bvls");
}

int rsl_associate(rsl_handle h, const void* cur_xy, int nc, const void* prev_xy, int np, double thr, void* scratch,
                  void* match, void* dist) {
  if (!h) return RSL_ERR_INVALID;
  if (nc < 0 || np < 0 || !(thr >= 0)) return fail(h, RSL_ERR_INVALID, "rsl_associate: bad argument");
  if (nc > 0 && (!cur_xy || !match || !dist || (np > 0 && (!prev_xy || !scratch))))
    return fail(h, RSL_ERR_INVALID, "rsl_associate: null pointer");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_associate(h->stream, (const double*)cur_xy, nc, (const double*)prev_xy, np, thr,
                                         (unsigned*)scratch, (int*)match, (double*)dist),
                   "associate");
}

int rsl_peak_topk(rsl_handle h, const void* entry_base, long long entry_cap, int ncube, const void* e_coord,
                  const void* e_pdb, double thr_db, int kmax, int C, void* sel_entry, void* sel_frame, void* sel_rc,
                  void* sel_n) {
  if (!h) return RSL_ERR_INVALID;
  if (ncube < 0 || entry_cap < 0 || C <= 0 || C > 8192) return fail(h, RSL_ERR_INVALID, "rsl_peak_topk: bad argument");
  if (kmax < 1 || kmax > 256) return fail(h, RSL_ERR_UNSUPPORTED, "rsl_peak_topk: kmax must be 1..256");
  if (ncube == 0) return RSL_OK;
  if (!entry_base || !sel_entry || !sel_frame || !sel_rc || !sel_n || (entry_cap > 0 && (!e_coord || !e_pdb)))
    return fail(h, RSL_ERR_INVALID, "rsl_peak_topk: null pointer");
  Scope sc(h, RSL_K_AUX);
  // the reference compares float64 power_db > thr_db; the entries' power_db is f32, so compare against the largest
  // float <= thr_db (identical decisions for every f32 value)
  return hip_check(h,
                   rsl::launch_topk_entries(h->stream, (const long long*)entry_base, entry_cap, ncube,
                                            (const unsigned*)e_coord, (const float*)e_pdb,
                                            rsl::threshold_as_float(thr_db), kmax, C, (int*)sel_entry,
                                            (int*)sel_frame, (int*)sel_rc, (int*)sel_n),
                   "peak_topk");
}

int rsl_associate_nearest(rsl_handle h, const void* range_m, const void* az_rad, const void* s0, const void* off,
                          int nframes, long long ntargets, double thr, void* match, void* dist, void* phase) {
  if (!h) return RSL_ERR_INVALID;
  if (nframes < 0 || ntargets < 0 || !(thr >= 0)) return fail(h, RSL_ERR_INVALID, "rsl_associate_nearest: bad argument");
  if (nframes == 0 || ntargets == 0) return RSL_OK;
  if (!range_m || !az_rad || !s0 || !off || !match || !dist || !phase)
    return fail(h, RSL_ERR_INVALID, "rsl_associate_nearest: null pointer");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_associate_nearest(h->stream, (const double*)range_m, (const double*)az_rad,
                                                 (const double2*)s0, (const long long*)off, nframes, ntargets, thr,
                                                 (int*)match, (double*)dist, (double*)phase),
                   "associate_nearest");
}

// The checks rsl_wrapped_solve and rsl_wrapped_search (fn) share, in their order: the arguments (own_bad: the entry
// point's own conditions), the pointers (own_null: one of the entry point's own is null), the box, then the scratch
// size (need: the entry point's *_scratch_bytes).
static int wrapped_check(rsl_handle h, const std::string& fn, const rsl::WrapArgs& a, bool own_bad, bool own_null,
                         const void* scratch, long long scratch_bytes, long long need, const void* out) {
  if (!h) return RSL_ERR_INVALID;
  if (a.n < 1 || (a.nv != 3 && a.nv != 6) || (a.mode != 0 && a.mode != 1) || own_bad || a.nextra < 0 || a.iters < 0)
    return fail(h, RSL_ERR_INVALID, fn + ": bad argument");
  if (!a.pos || !a.ang || !a.y || !a.lo || !a.hi || own_null || !scratch || !out || (a.nextra > 0 && !a.extra))
    return fail(h, RSL_ERR_INVALID, fn + ": null pointer");
  for (int c = 0; c < 6; ++c)
    if (!(a.lo[c] <= a.hi[c])) return fail(h, RSL_ERR_INVALID, fn + ": bad bounds");
  if (scratch_bytes < need) return fail(h, RSL_ERR_INVALID, fn + ": scratch too small");
  return RSL_OK;
}

long long rsl_wrapped_scratch_bytes(long long n, int grid_n, int nextra) {
  if (n < 0 || grid_n < 0 || nextra < 0) return -1;
  return 8LL * rsl::WrappedSolveScratch(nullptr, n, (long long)grid_n * grid_n + nextra).total;
}

int rsl_wrapped_solve(rsl_handle h, const void* pos, const void* ang, long long n, const void* y, double k, int mode,
                      double w, double vmax, double wmax, const void* prev, const double* lo6, const double* hi6,
                      int nv, int grid_n, const void* extra, int nextra, int iters, void* scratch,
                      long long scratch_bytes, void* out) {
  const rsl::WrapArgs a = {(const double*)pos, (const double*)ang, n, (const double*)y, k, mode, w, vmax, wmax,
                           (const double*)prev, lo6, hi6, nv, (const double*)extra, nextra, iters};
  const bool own_bad = grid_n < 0 || grid_n * (long long)grid_n + nextra < 1;
  if (const int rc = wrapped_check(h, "rsl_wrapped_solve", a, own_bad, false, scratch, scratch_bytes,
                                   rsl_wrapped_scratch_bytes(n, grid_n, nextra), out))
    return rc;
  Scope sc(h, RSL_K_VELOCITY);
  return hip_check(h, rsl::launch_wrapped_solve(h->stream, a, grid_n, (double*)scratch, (double*)out),
                   "wrapped_solve");
}

// stage-1 grid of rsl_wrapped_search: ceil(width / spacing) points per axis, at least 1, at most 2^15 (so the grid
// has < 2^30 starts)
static void search_grid(const double* lo6, const double* hi6, double spacing, long long* gx, long long* gy) {
  auto pts = [&](double w) {
    double g = spacing > 0 ? ceil(w / spacing) : 1.0;
    if (!(g >= 1.0)) g = 1.0;
    if (g > 32768.0) g = 32768.0;
    return (long long)g;
  };
  *gx = pts(hi6[0] - lo6[0]);
  *gy = pts(hi6[1] - lo6[1]);
}

long long rsl_wrapped_search_scratch_bytes(long long n, const double* lo6, const double* hi6, double spacing,
                                           int nbest, int nextra) {
  if (n < 0 || !lo6 || !hi6 || nbest < 1 || nextra < 0) return -1;
  long long gx, gy;
  search_grid(lo6, hi6, spacing, &gx, &gy);
  return 8LL * rsl::WrappedSearchScratch(nullptr, n, gx * gy, (long long)nbest + nextra).total;
}

int rsl_wrapped_search(rsl_handle h, const void* pos, const void* ang, long long n, const void* y, double k, int mode,
                       double w, double vmax, double wmax, const void* prev, const double* lo6, const double* hi6,
                       int nv, const double* base6, double spacing, int nbest, const void* extra, int nextra, int iters,
                       void* scratch, long long scratch_bytes, void* out) {
  const rsl::WrapArgs a = {(const double*)pos, (const double*)ang, n, (const double*)y, k, mode, w, vmax, wmax,
                           (const double*)prev, lo6, hi6, nv, (const double*)extra, nextra, iters};
  const bool own_bad = !(spacing > 0) || nbest < 1 || nbest > 1024;
  if (const int rc = wrapped_check(h, "rsl_wrapped_search", a, own_bad, !base6, scratch, scratch_bytes,
                                   rsl_wrapped_search_scratch_bytes(n, lo6, hi6, spacing, nbest, nextra), out))
    return rc;
  long long gx, gy;
  search_grid(lo6, hi6, spacing, &gx, &gy);
  Scope sc(h, RSL_K_VELOCITY);
  return hip_check(h, rsl::launch_wrapped_search(h->stream, a, base6, gx, gy, nbest, (double*)scratch, (double*)out),
                   "wrapped_search");
}

int rsl_traj_scan(rsl_handle h, const void* vel, int vstride, int nv, const void* omega, int ostride,
                  const void* timestamps, double dt, long long F, int method, void* pos, void* quat, void* summary) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || nv < 0 || nv > 3 || vstride < nv || (omega && ostride < 3) || (method != 0 && method != 1))
    return fail(h, RSL_ERR_INVALID, "rsl_traj_scan: bad argument");
  if (F > 0 && (!vel || !pos || !quat)) return fail(h, RSL_ERR_INVALID, "rsl_traj_scan: null pointer");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_traj_scan(h->stream, (const double*)vel, vstride, nv, (const double*)omega, ostride,
                                         (const double*)timestamps, dt, F, method, (double*)pos, (double*)quat,
                                         (double*)summary),
                   "traj_scan");
}

int rsl_traj_apply(rsl_handle h, void* pos, void* quat, long long F, const void* base) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || (F > 0 && (!pos || !quat || !base))) return fail(h, RSL_ERR_INVALID, "rsl_traj_apply: bad argument");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h, rsl::launch_traj_apply(h->stream, (double*)pos, (double*)quat, F, (const double*)base),
                   "traj_apply");
}

int rsl_traj_smooth(rsl_handle h, const void* x, long long F, int ncol, int size, void* out) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || ncol < 1 || size < 1 || (F > 0 && (!x || !out)))
    return fail(h, RSL_ERR_INVALID, "rsl_traj_smooth: bad argument");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h, rsl::launch_traj_smooth(h->stream, (const double*)x, F, ncol, size, (double*)out),
                   "traj_smooth");
}

int rsl_traj_stitch(rsl_handle h, const void* summaries, int R, int rank, double dt, int method, void* state,
                    void* base) {
  if (!h) return RSL_ERR_INVALID;
  if (R < 1 || rank < 0 || rank >= R || (method != 0 && method != 1) || !summaries || !state || !base)
    return fail(h, RSL_ERR_INVALID, "rsl_traj_stitch: bad argument");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_traj_stitch(h->stream, (const double*)summaries, R, rank, dt, method, (double*)state,
                                           (double*)base),
                   "traj_stitch");
}

int rsl_synth_pattern(rsl_handle h, const void* scatterers, int n, int A, int S, double fc, double bandwidth,
                      double chirp_duration, double antenna_spacing, void* pattern) {
  if (!h) return RSL_ERR_INVALID;
  if (n < 0 || A <= 0 || S <= 0 || !(fc > 0) || !(chirp_duration > 0))
    return fail(h, RSL_ERR_INVALID, "rsl_synth_pattern: bad arguments");
  if (!pattern || (n > 0 && !scatterers)) return fail(h, RSL_ERR_INVALID, "rsl_synth_pattern: null pointer");
  const double d = antenna_spacing > 0 ? antenna_spacing : 0.5 * 3e8 / fc;
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_synth_pattern(h->stream, (const double*)scatterers, n, A, S, fc, bandwidth,
                                             chirp_duration, d, (double2*)pattern),
                   "synth_pattern");
}

int rsl_synth_cube(rsl_handle h, const void* pattern, int F, int A, int C, int S, double noise_power,
                   unsigned long long seed, long long frame0, void* cube) {
  if (!h) return RSL_ERR_INVALID;
  if (F < 0 || A <= 0 || C <= 0 || S <= 0 || frame0 < 0 || !(noise_power >= 0))
    return fail(h, RSL_ERR_INVALID, "rsl_synth_cube: bad arguments");
  if (S % 2) return fail(h, RSL_ERR_UNSUPPORTED, "rsl_synth_cube: S must be even");
  if (!pattern || !cube) return fail(h, RSL_ERR_INVALID, "rsl_synth_cube: null pointer");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_synth_cube(h->stream, (const double2*)pattern, F, A, C, S, noise_power, seed, frame0,
                                          (float2*)cube),
                   "synth_cube");
}

long long rsl_pose_error_scratch_bytes(long long n, int nlen) {
  if (n < 0 || nlen < 0) return -1;
  return 8 * rsl::pose_error_scratch_doubles(n, nlen);
}

int rsl_pose_align(rsl_handle h, const void* est, const void* gt, long long n, void* scratch, void* align,
                   void* aligned, void* ape_err, void* ape_stats) {
  if (!h) return RSL_ERR_INVALID;
  if (n < 1) return fail(h, RSL_ERR_INVALID, "rsl_pose_align: need at least one pose");
  if (!est || !gt || !scratch || !align || !aligned || !ape_err)
    return fail(h, RSL_ERR_INVALID, "rsl_pose_align: null pointer");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_pose_align(h->stream, (const double*)est, (const double*)gt, n, (double*)scratch,
                                          (double*)align, (double*)aligned, (double*)ape_err, (double*)ape_stats),
                   "pose_align");
}

int rsl_pose_rte(rsl_handle h, const void* aligned, const void* gt, long long n, const void* lengths, int nlen,
                 void* scratch, void* err, void* counts, void* stats) {
  if (!h) return RSL_ERR_INVALID;
  if (n < 1 || nlen < 0 || nlen > 1024) return fail(h, RSL_ERR_INVALID, "rsl_pose_rte: bad arguments");
  if (nlen == 0) return RSL_OK;
  if (!aligned || !gt || !lengths || !scratch || !err || !counts || !stats)
    return fail(h, RSL_ERR_INVALID, "rsl_pose_rte: null pointer");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_pose_rte(h->stream, (const double*)aligned, (const double*)gt, n,
                                        (const double*)lengths, nlen, (double*)scratch, (double*)err,
                                        (unsigned long long*)counts, (double*)stats),
                   "pose_rte");
}

int rsl_music_subspace(rsl_handle h, const void* sigs, long long n, int M, int num_sources, const void* steer_c128,
                       int G, void* spec) {
  if (!h) return RSL_ERR_INVALID;
  if (n < 0 || M < 1 || M > 16 || G < 1) return fail(h, RSL_ERR_INVALID, "rsl_music_subspace: bad shape");
  if (n == 0) return RSL_OK;
  if (!sigs || !steer_c128 || !spec) return fail(h, RSL_ERR_INVALID, "rsl_music_subspace: null pointer");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_music_subspace(h->stream, (const double*)sigs, n, M, num_sources,
                                              (const double*)steer_c128, G, (double*)spec),
                   "music_subspace");
}

int rsl_esprit_subspace(rsl_handle h, const void* sigs, long long n, int M, int num_sources, double esprit_scale,
                        void* deg) {
  if (!h) return RSL_ERR_INVALID;
  if (n < 0 || M < 1 || M > 16) return fail(h, RSL_ERR_INVALID, "rsl_esprit_subspace: bad shape");
  if (n == 0) return RSL_OK;
  if (!sigs || !deg) return fail(h, RSL_ERR_INVALID, "rsl_esprit_subspace: null pointer");
  Scope sc(h, RSL_K_AUX);
  return hip_check(h,
                   rsl::launch_esprit_subspace(h->stream, (const double*)sigs, n, M, num_sources, esprit_scale,
                                               (double*)deg),
                   "esprit_subspace");
}

}  // extern "C"
