// rsl_api.hip — C-ABI layer of librsl.so (see include/rsl.h).  No kernels here.  Every launching entry point is three
// steps in one order: its argument checks on one `Check` (first refusal kept, the entry point's name put in front of the
// text, a null handle the first refusal of all), with its empty-batch return where the header puts it among them; the
// typed view of its untyped arguments (cell_list, cloud_view, detect_args, peak_offsets, peak_lists, steer_view); and
// `enter`, the one frame a launch runs in: the handle's device made current and checked, the optional hipEvent timing
// scope on the handle's stream, the launcher, its hipError_t mapped to the status.  Also here: the handle, the per-size
// twiddle tables, and the host-side steering table.
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

// The argument check of one entry point, built from (h, "rsl_x").  It keeps the first refusal, puts the entry point's
// name in front of its text and holds the status; a null handle is refused before anything else (RSL_ERR_INVALID,
// nothing stored).  Every test returns whether the call now stands refused, so the checks of an entry point chain with
// || in the order in which they are to win, and none is evaluated after the first that fails:
//   if (chk.invalid(F < 0, "bad shape") || chk.unsupported(C > 4096, "C too large")) return chk.status;
struct Check {
  rsl_context* h;
  const char* fn;
  int status;
  Check(rsl_context* h_, const char* fn_) : h(h_), fn(fn_), status(h_ ? RSL_OK : RSL_ERR_INVALID) {}
  bool refuse(int code, bool cond, const char* what) {
    if (!status && cond) status = fail(h, code, std::string(fn) + ": " + what);
    return status != RSL_OK;
  }
  bool invalid(bool cond, const char* what) { return refuse(RSL_ERR_INVALID, cond, what); }
  bool unsupported(bool cond, const char* what) { return refuse(RSL_ERR_UNSUPPORTED, cond, what); }
};

int set_device(rsl_context* h) { return hip_check(h, hipSetDevice(h->device), "hipSetDevice"); }

// The frame of a launch, after the checks and the empty-batch return of its entry point (so a refused or empty call
// records no event), in this order: the handle's device is made current, and where that fails the call is RSL_ERR_HIP
// and nothing launches; with timing on, an event pair opens on the handle's stream (one that cannot be created or
// recorded is given up: the launch then runs untimed); steps() launches and returns the status; the pair closes and
// goes to collect() under the kernel id.  The caller's current device is not put back.
template <class Steps>
int scoped(rsl_context* h, int kid, Steps&& steps) {
  if (int r = set_device(h)) return r;
  std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
  bool timed = false;
  if (h->timing) {
    if (!h->ev_pool.empty()) {
      ev = h->ev_pool.back();
      h->ev_pool.pop_back();
    } else if (hipEventCreate(&ev.first) != hipSuccess || hipEventCreate(&ev.second) != hipSuccess) {
      if (ev.first) hipEventDestroy(ev.first);
      ev.first = nullptr;
    }
    timed = ev.first && hipEventRecord(ev.first, h->stream) == hipSuccess;
    if (ev.first && !timed) h->ev_pool.push_back(ev);
  }
  const int r = steps();
  if (timed) {
    hipEventRecord(ev.second, h->stream);  // where this fails, collect() drops the launch from totals and spans
    h->ev[kid].push_back(ev);
  }
  return r;
}

// The frame around one launcher call: `what` names it in the text of an RSL_ERR_HIP.
template <class Launch>
int enter(rsl_context* h, int kid, const char* what, Launch&& launch) {
  return scoped(h, kid, [&] { return hip_check(h, launch(), what); });
}

// The table of size n on the current device (the caller has made the handle's device current), built at first use.
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

// What a detector entry point hands its launcher, from the untyped arguments of the C ABI.
rsl::DetectArgs detect_args(double thr_power, int i_lo, int i_hi, void* mask, void* row_count, void* db_map,
                            void* peak_pow) {
  return {thr_power, i_lo, i_hi, (unsigned long long*)mask, (int*)row_count, (float*)db_map, (float*)peak_pow};
}

// What rsl_peak_emit reads of rsl_peak_offsets' results, and the lists it writes, from its untyped arguments.
rsl::PeakOffsets peak_offsets(const void* entry_row_off, const void* cell_row_off, const void* entry_base,
                              const void* cell_base) {
  return {(const int*)entry_row_off, (const int*)cell_row_off, (const long long*)entry_base,
          (const long long*)cell_base};
}

rsl::PeakLists peak_lists(long long entry_cap, long long cell_cap, void* e_coord, void* e_cell, void* e_pdb,
                          void* c_frame, void* c_rc, void* c_amask) {
  return {entry_cap, cell_cap, (unsigned*)e_coord, (int*)e_cell, (float*)e_pdb, (int*)c_frame, (int*)c_rc,
          (unsigned*)c_amask};
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

// What rsl_rds and rsl_rds_detect share: the cube, its shape rule, and K1.
struct RangeStage {
  const void* cube;
  int F, A, C_total, chirp0, C, S;
  const void* table;
  int dc_removal;
  void* work;
  bool bad_shape() const { return F < 0 || A <= 0 || S <= 0 || C <= 0 || chirp0 < 0 || chirp0 + C > C_total; }
  // The twiddle tables of both stages on the handle's device (*tC: the one K2 takes), then K1 in its frame.  packed:
  // range spectra of 6 B per value between K1 and K2 (each bin's exponent inside its 48-B unit; the tiles fill the
  // first 3/4 of the c64-sized work buffer the caller provides).
  int launch(rsl_context* h, bool packed, float2** tC) const {
    if (int r = set_device(h)) return r;
    float2* tS = twiddles(h, S);
    *tC = twiddles(h, C);
    if (!tS || !*tC) return fail(h, RSL_ERR_HIP, "twiddle table allocation failed");
    return enter(h, RSL_K_RANGE_FFT, "range_fft", [&] {
      return rsl::launch_range_fft(h->stream, (const float2*)cube, F, A, C_total, chirp0, C, S, (const float2*)table,
                                   tS, dc_removal, (float2*)work, h->rfq, packed);
    });
  }
};

// rsl_detect_cfar (rank null) and rsl_detect_oscfar (its rank), and rsl_detect_power's two CFAR rules (power: `maps`
// holds F fp32 power maps and A is 1): the checks in the order the header lists them, on the entry point's `chk`, then
// the launch.  No LDS check: every window within the limits fits at every C <= RSL_CFAR_MAX_C, which rsl_cfar.hip and
// rsl_oscfar.hip assert at compile time.
int detect_cfar_family(Check& chk, const void* maps, bool power, int F, int A, int S, int C, rsl::CfarWindow win,
                       const double* rank, double alpha, const rsl::DetectArgs& det) {
  if (chk.invalid(F < 0 || A <= 0 || S <= 0 || C <= 0 || S > 8192, "bad shape") ||
      chk.invalid(win.gr < 0 || win.gd < 0 || win.tr < 0 || win.td < 0 || win.tr + win.td < 1,
                  "bad window (half-sizes >= 0, at least one training cell)") ||
      chk.invalid(win.hr() > RSL_CFAR_MAX_HALF || win.hd() > RSL_CFAR_MAX_HALF,
                  "window half-size above RSL_CFAR_MAX_HALF") ||
      chk.invalid(win.nfull() > C || 2 * win.hr() + 1 > S, "window larger than the map") ||
      chk.invalid(!(alpha > 0) || !std::isfinite(alpha), "alpha must be finite, > 0") ||
      chk.unsupported(C > RSL_CFAR_MAX_C, "C above RSL_CFAR_MAX_C") ||
      chk.invalid(rank && !(*rank > 0 && *rank <= 1), "rank must lie in (0, 1]"))
    return chk.status;
  if (F == 0) return RSL_OK;
  if (chk.invalid(!maps || !det.mask || !det.row_count, "null pointer")) return chk.status;
  rsl_context* h = chk.h;
  const float2* z = (const float2*)maps;
  const float* p = (const float*)maps;
  const float af = (float)alpha;
  if (rank)
    return enter(h, RSL_K_DETECT, "detect_oscfar", [&] {
      return power ? rsl::launch_detect_oscfar(h->stream, p, F, S, C, win, *rank, af, det)
                   : rsl::launch_detect_oscfar(h->stream, z, F, A, S, C, win, *rank, af, det);
    });
  return enter(h, RSL_K_DETECT, "detect_cfar", [&] {
    return power ? rsl::launch_detect_cfar(h->stream, p, F, S, C, win, af, det)
                 : rsl::launch_detect_cfar(h->stream, z, F, A, S, C, win, af, det);
  });
}

// The checks rsl_velocity, rsl_velocity_robust and rsl_velocity_consensus share, on the entry point's `chk`, in one
// order: the counts; the entry point's own scalars (own(): its checks on chk, whether one refused); the ridge; an empty
// batch (RSL_OK with p->F = 0: nothing to launch); the pointers; the grid table; the box.  Fills *p with the typed
// problem.
template <class Own>
int velocity_problem(Check& chk, Own&& own, const void* az, const void* gidx, const void* az_table, int G,
                     const void* y, const void* amask, const void* seg, long long n, int F, double k, double ridge,
                     const double* bounds4, const void* out, rsl::VelProblem* p) {
  *p = {};
  if (chk.invalid(F < 0 || n < 0, "bad argument") || own() || chk.invalid(!(ridge >= 0), "ridge must be >= 0"))
    return chk.status;
  if (F == 0) return RSL_OK;
  if (chk.invalid((!az && !gidx) || !y || !seg || !bounds4 || !out, "null pointer") ||
      chk.invalid(gidx && (!az_table || G <= 0 || G > 2048), "bad grid table") ||
      chk.invalid(!(bounds4[0] <= bounds4[1]) || !(bounds4[2] <= bounds4[3]), "bad bounds"))
    return chk.status;
  *p = {(const double*)az, (const int*)gidx, (const double*)az_table, G, (const double*)y, (const unsigned*)amask,
        (const long long*)seg, n, F, k, ridge, bounds4[0], bounds4[1], bounds4[2], bounds4[3]};
  return RSL_OK;
}

// The checks rsl_wrapped_solve and rsl_wrapped_search share, on the entry point's `chk`, in their order: the arguments
// (own_bad: the entry point's own conditions), the pointers (own_null: one of the entry point's own is null), the box,
// then the scratch size (need: the entry point's *_scratch_bytes).
int wrapped_check(Check& chk, const rsl::WrapArgs& a, bool own_bad, bool own_null, const void* scratch,
                  long long scratch_bytes, long long need, const void* out) {
  auto bad_box = [&] {
    for (int c = 0; c < 6; ++c)
      if (!(a.lo[c] <= a.hi[c])) return true;
    return false;
  };
  if (chk.invalid(a.n < 1 || (a.nv != 3 && a.nv != 6) || (a.mode != 0 && a.mode != 1) || own_bad || a.nextra < 0 ||
                      a.iters < 0,
                  "bad argument") ||
      chk.invalid(!a.pos || !a.ang || !a.y || !a.lo || !a.hi || own_null || !scratch || !out ||
                      (a.nextra > 0 && !a.extra),
                  "null pointer") ||
      chk.invalid(bad_box(), "bad bounds") || chk.invalid(scratch_bytes < need, "scratch too small"))
    return chk.status;
  return RSL_OK;
}

// stage-1 grid of rsl_wrapped_search: ceil(width / spacing) points per axis, at least 1, at most 2^15 (so the grid
// has < 2^30 starts)
void search_grid(const double* lo6, const double* hi6, double spacing, long long* gx, long long* gy) {
  auto pts = [&](double w) {
    double g = spacing > 0 ? ceil(w / spacing) : 1.0;
    if (!(g >= 1.0)) g = 1.0;
    if (g > 32768.0) g = 32768.0;
    return (long long)g;
  };
  *gx = pts(hi6[0] - lo6[0]);
  *gy = pts(hi6[1] - lo6[1]);
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
  if (int r = set_device(h)) return r;
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
  Check chk(h, "rsl_rds");
  const RangeStage k1{cube, F, A, C_total, chirp0, C, S, table, dc_removal, work};
  if (chk.invalid(k1.bad_shape(), "bad shape")) return chk.status;
  if (F == 0) return RSL_OK;  // empty batch: the (zero-size) buffers may be null
  if (chk.invalid(!cube || !table || !work || !rds, "null pointer")) return chk.status;
  if (!rsl_fft_supported(S) || !rsl_fft_supported(C)) {  // the one text that carries values
    const std::string sizes = "FFT size not supported (S=" + std::to_string(S) + ", C=" + std::to_string(C) + ")";
    chk.unsupported(true, sizes.c_str());
    return chk.status;
  }
  float2* tC;
  if (int r = k1.launch(h, false, &tC)) return r;
  return enter(h, RSL_K_DOPPLER_FFT, "doppler_fft", [&] {
    return rsl::launch_doppler_fft(h->stream, (const float2*)work, F, A, C, S, tC, (float2*)rds);
  });
}

int rsl_rds_detect(rsl_handle h, const void* cube, int F, int A, int C_total, int chirp0, int C, int S,
                   const void* table, int dc_removal, void* work, void* rds, double thr_power, int i_lo, int i_hi,
                   void* mask, void* row_count, void* db_map, void* peak_pow, int* peak_pow_group) {
  Check chk(h, "rsl_rds_detect");
  if (chk.status) return chk.status;  // a null handle: nothing is written
  if (peak_pow_group) *peak_pow_group = 1;
  const RangeStage k1{cube, F, A, C_total, chirp0, C, S, table, dc_removal, work};
  if (chk.invalid(k1.bad_shape(), "bad shape")) return chk.status;
  if (F == 0) return RSL_OK;  // empty batch: the (zero-size) buffers may be null
  if (chk.invalid(!mask || !row_count, "null pointer")) return chk.status;
  if (!rsl::doppler_detect_supported(C, S)) {  // unfused: a7 then a8, each under its own name
    if (int r = rsl_rds(h, cube, F, A, C_total, chirp0, C, S, table, dc_removal, work, rds)) return r;
    return rsl_detect(h, rds, F, A, S, C, thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow);
  }
  if (chk.invalid(!cube || !table || !work || !rds, "null pointer") ||
      chk.unsupported(!rsl_fft_supported(S), "FFT size not supported"))
    return chk.status;
  const bool packed = rsl::work_packed_supported(C, S);
  float2* tC;
  if (int r = k1.launch(h, packed, &tC)) return r;
  int group = 1;
  const int r = enter(h, RSL_K_DOPPLER_FFT, "doppler_detect", [&] {
    return rsl::launch_doppler_detect(h->stream, (const float2*)work, F, A, C, S, tC, (float2*)rds,
                                      detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow), &group,
                                      packed);
  });
  if (peak_pow_group) *peak_pow_group = group;
  return r;
}

int rsl_detect(rsl_handle h, const void* rds, int F, int A, int S, int C, double thr_power, int i_lo, int i_hi,
               void* mask, void* row_count, void* db_map, void* peak_pow) {
  Check chk(h, "rsl_detect");
  if (chk.invalid(F < 0 || A <= 0 || S <= 0 || C <= 0, "bad shape")) return chk.status;
  if (F == 0) return RSL_OK;
  if (chk.invalid(!rds || !mask || !row_count, "null pointer") ||
      chk.unsupported(!rsl::detect_rows(C), "C too large"))
    return chk.status;
  return enter(h, RSL_K_DETECT, "detect", [&] {
    return rsl::launch_detect(h->stream, (const float2*)rds, F, A, S, C,
                              detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow));
  });
}

int rsl_detect_cfar(rsl_handle h, const void* rds, int F, int A, int S, int C, int guard_r, int guard_d, int train_r,
                    int train_d, double alpha, double thr_power, int i_lo, int i_hi, void* mask, void* row_count,
                    void* db_map, void* peak_pow) {
  Check chk(h, "rsl_detect_cfar");
  return detect_cfar_family(chk, rds, false, F, A, S, C, {guard_r, guard_d, train_r, train_d}, nullptr, alpha,
                            detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow));
}

int rsl_detect_oscfar(rsl_handle h, const void* rds, int F, int A, int S, int C, int guard_r, int guard_d,
                      int train_r, int train_d, double rank, double alpha, double thr_power, int i_lo, int i_hi,
                      void* mask, void* row_count, void* db_map, void* peak_pow) {
  Check chk(h, "rsl_detect_oscfar");
  // the factor is checked as the float the kernel multiplies by
  return detect_cfar_family(chk, rds, false, F, A, S, C, {guard_r, guard_d, train_r, train_d}, &rank, (float)alpha,
                            detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow));
}

int rsl_power_integrate(rsl_handle h, const void* rds, int F, int A, int S, int C, void* power) {
  Check chk(h, "rsl_power_integrate");
  if (chk.invalid(F < 0 || A <= 0 || S <= 0 || C <= 0, "bad shape") ||
      chk.invalid(A > 32, "more than 32 antennas"))
    return chk.status;
  if (F == 0) return RSL_OK;
  if (chk.invalid(!rds || !power, "null pointer")) return chk.status;
  return enter(h, RSL_K_DETECT, "power_integrate", [&] {
    return rsl::launch_power_integrate(h->stream, (const float2*)rds, F, A, S, C, (float*)power);
  });
}

int rsl_detect_power(rsl_handle h, const void* power, int F, int S, int C, int rule, int guard_r, int guard_d,
                     int train_r, int train_d, double rank, double alpha, double thr_power, int i_lo, int i_hi,
                     void* mask, void* row_count, void* db_map, void* peak_pow) {
  Check chk(h, "rsl_detect_power");
  const rsl::DetectArgs det = detect_args(thr_power, i_lo, i_hi, mask, row_count, db_map, peak_pow);
  const rsl::CfarWindow win = {guard_r, guard_d, train_r, train_d};
  switch (rule) {
    case RSL_RULE_THRESHOLD:  // rsl_detect's checks; window, rank and alpha are not looked at
      if (chk.invalid(F < 0 || S <= 0 || C <= 0, "bad shape")) return chk.status;
      if (F == 0) return RSL_OK;
      if (chk.invalid(!power || !mask || !row_count, "null pointer") ||
          chk.unsupported(!rsl::detect_rows(C), "C too large"))
        return chk.status;
      return enter(h, RSL_K_DETECT, "detect",
                   [&] { return rsl::launch_detect(h->stream, (const float*)power, F, S, C, det); });
    case RSL_RULE_CA:
      return detect_cfar_family(chk, power, true, F, 1, S, C, win, nullptr, alpha, det);
    case RSL_RULE_OS:
      return detect_cfar_family(chk, power, true, F, 1, S, C, win, &rank, (float)alpha, det);
    default:
      chk.invalid(true, "unknown rule");
      return chk.status;
  }
}

int rsl_peak_offsets(rsl_handle h, const void* mask, const void* row_count, int F, int A, int S, int C,
                     void* entry_row_off, void* cell_row_off, void* scratch, void* entry_base, void* cell_base,
                     void* frame_counts, void* union_mask) {
  Check chk(h, "rsl_peak_offsets");
  if (chk.invalid(F < 0 || A <= 0 || S <= 0 || C <= 0 || A > 32, "bad shape") ||
      chk.invalid(!entry_base || !cell_base, "null pointer") ||
      chk.invalid(F > 0 && (!mask || !row_count || !entry_row_off || !cell_row_off || !scratch || !frame_counts),
                  "null pointer"))
    return chk.status;
  if (F == 0) {
    if (int r = set_device(h)) return r;
    long long z = 0;
    hipMemcpyAsync(entry_base, &z, 8, hipMemcpyHostToDevice, h->stream);
    hipMemcpyAsync(cell_base, &z, 8, hipMemcpyHostToDevice, h->stream);
    return hip_check(h, hipStreamSynchronize(h->stream), "offsets(F=0)");
  }
  return enter(h, RSL_K_OFFSETS, "offsets", [&] {
    return rsl::launch_offsets(h->stream, (const unsigned long long*)mask, (const int*)row_count, F, A, S, C,
                               (int*)entry_row_off, (int*)cell_row_off, (int*)scratch, (long long*)entry_base,
                               (long long*)cell_base, (long long*)frame_counts, (unsigned long long*)union_mask);
  });
}

int rsl_peak_emit(rsl_handle h, const void* rds, const void* mask, const void* union_mask, const void* peak_pow,
                  int peak_pow_group, int F, int A, int S, int C, const void* entry_row_off, const void* cell_row_off, const void* entry_base,
                  const void* cell_base, long long entry_cap, long long cell_cap, void* e_coord, void* e_cell,
                  void* e_pdb, void* c_frame, void* c_rc, void* c_amask) {
  Check chk(h, "rsl_peak_emit");
  if (chk.invalid(F < 0 || A <= 0 || A > 32 || S <= 0 || C <= 0 || S > 8192 || C > 8192, "bad shape"))
    return chk.status;
  if (F == 0) return RSL_OK;
  const bool compact = rsl::emit_compact_supported(C, union_mask, peak_pow, e_pdb);
  if (chk.invalid(!mask || !entry_row_off || !cell_row_off || !entry_base || !cell_base, "null pointer") ||
      chk.invalid((entry_cap > 0 && (!e_coord || !e_cell)) || (cell_cap > 0 && (!c_frame || !c_rc || !c_amask)),
                  "null output") ||
      chk.invalid(peak_pow && (peak_pow_group < 1 || S % peak_pow_group != 0), "peak_pow_group must divide S") ||
      chk.invalid(!compact && !rds, "rds needed without union_mask / peak_pow"))
    return chk.status;
  const rsl::PeakOffsets off = peak_offsets(entry_row_off, cell_row_off, entry_base, cell_base);
  const rsl::PeakLists out = peak_lists(entry_cap, cell_cap, e_coord, e_cell, e_pdb, c_frame, c_rc, c_amask);
  if (compact)
    return enter(h, RSL_K_EMIT, "emit2", [&] {
      return rsl::launch_emit_compact(h->stream, (const unsigned long long*)mask,
                                      (const unsigned long long*)union_mask, (const float*)peak_pow, peak_pow_group,
                                      F, A, S, C, off, out);
    });
  return enter(h, RSL_K_EMIT, "emit", [&] {
    return rsl::launch_emit_rows(h->stream, (const float2*)rds, (const unsigned long long*)mask, F, A, S, C, off, out);
  });
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
  Check chk(h, "rsl_doa");
  const int base_method = method & 0xff;
  if (chk.invalid(A <= 0 || A > 16 || S <= 0 || C <= 0 || G <= 0, "bad shape") ||
      chk.invalid(!rds || !c_frame || !c_rc || !steer_tab || !out_idx, "null pointer") ||
      chk.invalid(base_method != RSL_METHOD_MUSIC && base_method != RSL_METHOD_BEAMFORMING, "unknown method"))
    return chk.status;
  const bool toep = (method & RSL_DOA_TOEPLITZ) != 0;
  const bool music = base_method == RSL_METHOD_MUSIC;
  (void)steer_c128;  // the exact re-scan reads the fp64 copy inside steer_tab (rsl_steer_table_build)
  const SteerView tab = steer_view(steer_tab, G, A);
  const rsl::CellList cl = cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell);
  if (!ncell_dev && ncell <= 0) return RSL_OK;
  // one scope for the scan and its fixup, ending at the first step that fails
  return scoped(h, RSL_K_DOA_SCAN, [&] {
    // the Toeplitz f16-MFMA scan: argmax only, or with the whole spectrum in the cell-blocked layout (no gmax there)
    const bool toep_spec = out_spec && (method & RSL_DOA_SPEC_BLOCKED) && !out_gmax;
    if (toep && (!out_spec || toep_spec) && tab.lay.toep_fits)
      return hip_check(h,
                       rsl::launch_doa_toep(h->stream, cl, tab.toep, G, music, tab.t64, (int*)out_idx,
                                            (float*)out_gmax, 0.0, nullptr, nullptr,
                                            toep_spec ? (float*)out_spec : nullptr),
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
  });
}

int rsl_doa_extras(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                   const void* ncell_dev, long long ncell, const void* steer_tab, const void* steer_c128, int G,
                   int method, double esprit_scale, void* out_idx, void* out_gmax, void* esprit_deg, void* phase) {
  Check chk(h, "rsl_doa_extras");
  if (chk.invalid(A < 2 || A > 16 || S <= 0 || C <= 0 || G <= 0, "bad shape") ||
      chk.invalid(!rds || !c_frame || !c_rc || !steer_tab || !out_idx, "null pointer") ||
      chk.invalid(method != RSL_METHOD_MUSIC && method != RSL_METHOD_BEAMFORMING, "unknown method"))
    return chk.status;
  const bool music = method == RSL_METHOD_MUSIC;
  (void)steer_c128;  // the exact re-scan reads the fp64 copy inside steer_tab (rsl_steer_table_build)
  const SteerView tab = steer_view(steer_tab, G, A);
  if (chk.unsupported(!tab.lay.toep_fits, "grid too large for the Toeplitz path (use rsl_doa)")) return chk.status;
  if (!ncell_dev && ncell <= 0) return RSL_OK;
  return enter(h, RSL_K_DOA_SCAN, "doa_extras", [&] {
    return rsl::launch_doa_toep(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell), tab.toep, G,
                                music, tab.t64, (int*)out_idx, (float*)out_gmax, esprit_scale, (double*)esprit_deg,
                                (double*)phase);
  });
}

int rsl_doa_smoothed(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                     const void* ncell_dev, long long ncell, const void* steer_sub_c64, int G, int L, int nmax,
                     int num_sources, double rel, void* out_nsrc, void* out_idx, void* out_den, void* out_eig,
                     void* out_spec) {
  Check chk(h, "rsl_doa_smoothed");
  if (chk.invalid(A < 3 || A > 16 || S <= 0 || C <= 0, "bad shape (3 <= A <= 16)") ||
      chk.invalid(L < 2 || L > A || L > RSL_SS_MAX_L, "sub-array length outside [2, min(A, RSL_SS_MAX_L)]") ||
      chk.invalid(nmax < 1 || nmax > L - 1, "nmax outside [1, L - 1]") ||
      chk.invalid(num_sources < 0 || num_sources > nmax, "num_sources outside [0, nmax]") ||
      chk.invalid(!(rel > 0.0 && rel < 1.0), "rel outside (0, 1)") || chk.invalid(G < 3, "G < 3") ||
      chk.invalid(!rds || !c_frame || !c_rc || !steer_sub_c64 || !out_nsrc || !out_idx, "null pointer"))
    return chk.status;
  if (ncell <= 0) return RSL_OK;  // ncell is the launch bound (capacity) when ncell_dev is given
  return enter(h, RSL_K_DOA_SCAN, "doa_smoothed", [&] {
    return rsl::launch_doa_smoothed(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell),
                                    (const float2*)steer_sub_c64, G, L, nmax, num_sources, (float)rel, (int*)out_nsrc,
                                    (int*)out_idx, (float*)out_den, (float*)out_eig, (float*)out_spec);
  });
}

int rsl_range_cov(rsl_handle h, const void* rds, int F, int A, int S, int C, int c0, int c1, void* cov) {
  Check chk(h, "rsl_range_cov");
  if (chk.invalid(F < 0 || S <= 0 || C <= 0, "bad shape") ||
      chk.invalid(A < 2 || A > RSL_RA_MAX_A, "antennas outside [2, RSL_RA_MAX_A]") ||
      chk.invalid(c0 < 0 || c0 >= c1 || c1 > C, "window needs 0 <= c0 < c1 <= C"))
    return chk.status;
  if (F == 0) return RSL_OK;
  if (chk.invalid(!rds || !cov, "null pointer")) return chk.status;
  return enter(h, RSL_K_DOA_SCAN, "range_cov", [&] {
    return rsl::launch_range_cov(h->stream, (const float2*)rds, F, A, S, C, c0, c1, (float2*)cov);
  });
}

int rsl_range_azimuth(rsl_handle h, const void* cov, long long n, int A, const void* steer_c64, int G, int method,
                      double loading, void* map, void* arg) {
  Check chk(h, "rsl_range_azimuth");
  if (chk.invalid(n < 0, "n < 0") ||
      chk.invalid(method != RSL_RA_BARTLETT && method != RSL_RA_CAPON,
                  "method must be RSL_RA_BARTLETT or RSL_RA_CAPON") ||
      chk.invalid(A < 2 || A > RSL_RA_MAX_A, "antennas outside [2, RSL_RA_MAX_A]") || chk.invalid(G < 1, "G < 1") ||
      chk.invalid(!(loading >= RSL_RA_MIN_LOADING && loading <= 1.0), "loading outside [RSL_RA_MIN_LOADING, 1]"))
    return chk.status;
  if (n == 0) return RSL_OK;
  if (chk.invalid(!cov || !steer_c64 || !map, "null pointer")) return chk.status;
  return enter(h, RSL_K_DOA_SCAN, "range_azimuth", [&] {
    return rsl::launch_range_azimuth(h->stream, (const float2*)cov, n, A, (const float2*)steer_c64, G,
                                     method == RSL_RA_CAPON, (float)loading, (float*)map, (int*)arg);
  });
}

int rsl_cell_extras(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                    const void* ncell_dev, long long ncell, double esprit_scale, const void* gidx,
                    const void* az_table, void* sig_out, void* esprit_deg, void* phase, void* az_out) {
  Check chk(h, "rsl_cell_extras");
  if (chk.invalid(A <= 0 || A > 32 || S <= 0 || C <= 0, "bad shape") ||
      chk.invalid(A < 2, "needs at least 2 antennas") ||  // phase reads s0 and s1
      chk.invalid(!rds || !c_frame || !c_rc, "null pointer") ||
      chk.invalid(az_out && (!gidx || !az_table), "az_out needs gidx+table"))
    return chk.status;
  if (ncell <= 0) return RSL_OK;  // ncell is the launch bound (capacity) when ncell_dev is given
  return enter(h, RSL_K_CELL_EXTRAS, "cell_extras", [&] {
    return rsl::launch_cell_extras(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell), esprit_scale,
                                   (const int*)gidx, (const double*)az_table, (float2*)sig_out, (double*)esprit_deg,
                                   (double*)phase, (double*)az_out);
  });
}

int rsl_cell_refine(rsl_handle h, const void* rds, const void* power, int A, int S, int C, const void* c_frame,
                    const void* c_rc, const void* ncell_dev, long long ncell, const void* gidx, const void* az_table,
                    const void* steer_c64, int G, int range_mode, int doppler_mode, const double* axes4,
                    void* out_points, void* out_az) {
  Check chk(h, "rsl_cell_refine");
  auto unknown = [](int mode) { return mode < RSL_REFINE_NONE || mode > RSL_REFINE_HANN; };
  if (chk.invalid(A < 2 || A > 32, "antennas outside [2, 32]") ||
      chk.invalid(S <= 0 || C <= 0 || G <= 0, "bad shape") ||
      chk.invalid(unknown(range_mode) || unknown(doppler_mode), "unknown RSL_REFINE_* mode") ||
      chk.invalid(axes4 && !(std::isfinite(axes4[1]) && std::isfinite(axes4[3])), "an axis step is not finite") ||
      chk.invalid(!out_points && !out_az, "both outputs null") ||
      chk.invalid((reinterpret_cast<size_t>(out_points) & 15) != 0, "out_points is not 16-byte aligned"))
    return chk.status;
  if (ncell <= 0) return RSL_OK;  // ncell is the launch bound (capacity) when ncell_dev is given
  if (chk.invalid(!rds || !c_frame || !c_rc || !gidx || !az_table || !steer_c64 || !axes4, "null pointer"))
    return chk.status;
  return enter(h, RSL_K_CELL_EXTRAS, "cell_refine", [&] {
    return rsl::launch_cell_refine(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, ncell_dev, ncell),
                                   (const float*)power, (const int*)gidx, (const double*)az_table,
                                   (const float2*)steer_c64, G, range_mode, doppler_mode, axes4, (float*)out_points,
                                   (double*)out_az);
  });
}

int rsl_confidence(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                   long long n, const void* gidx, const void* steer_c128, const void* steer_phase, void* conf) {
  Check chk(h, "rsl_confidence");
  if (chk.invalid(A <= 0 || A > 32 || S <= 0 || C <= 0, "bad shape") ||
      chk.invalid(!rds || !c_frame || !c_rc || !gidx || !steer_c128 || !steer_phase || !conf, "null pointer"))
    return chk.status;
  return enter(h, RSL_K_CONFIDENCE, "confidence", [&] {
    return rsl::launch_confidence(h->stream, cell_list(rds, A, S, C, c_frame, c_rc, nullptr, n), (const int*)gidx,
                                  (const double*)steer_c128, (const double*)steer_phase, (double*)conf);
  });
}

int rsl_velocity(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G, const void* y,
                 const void* amask, const void* seg, long long n, int F, double k, double ridge, const double* bounds4,
                 void* out, void* resid, void* pred) {
  Check chk(h, "rsl_velocity");
  rsl::VelProblem p;
  const int rc = velocity_problem(chk, [] { return false; }, az, gidx, az_table, G, y, amask, seg, n, F, k, ridge,
                                  bounds4, out, &p);
  if (rc || p.F == 0) return rc;
  return enter(h, RSL_K_VELOCITY, "velocity", [&] {
    return rsl::launch_velocity(h->stream, p, (double*)out, (double*)resid, (double*)pred);
  });
}

int rsl_velocity_robust(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G, const void* y,
                        const void* amask, const void* seg, long long n, int F, double k, double ridge,
                        const double* bounds4, int loss, double c, double scale, int iters, double tol, void* out,
                        void* weight, void* resid) {
  Check chk(h, "rsl_velocity_robust");
  auto own = [&] {
    return chk.invalid(loss != RSL_LOSS_HUBER && loss != RSL_LOSS_TUKEY,
                       "loss must be RSL_LOSS_HUBER or RSL_LOSS_TUKEY") ||
           chk.invalid(!(c > 0) || !std::isfinite(c), "c must be finite, > 0") ||
           chk.invalid(std::isnan(scale) || (std::isinf(scale) && scale > 0),
                       "scale must be finite (<= 0: estimated)") ||
           chk.invalid(iters < 1 || iters > 1000, "iters outside 1..1000") ||
           chk.invalid(!(tol >= 0), "tol must be >= 0");
  };
  rsl::VelProblem p;
  const int rc = velocity_problem(chk, own, az, gidx, az_table, G, y, amask, seg, n, F, k, ridge, bounds4, out, &p);
  if (rc || p.F == 0) return rc;
  return enter(h, RSL_K_VELOCITY, "velocity_robust", [&] {
    return rsl::launch_velocity_robust(h->stream, p, loss, c, scale, iters, tol, (double*)out, (float*)weight,
                                       (double*)resid);
  });
}

int rsl_velocity_consensus(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G, const void* y,
                           const void* amask, const void* seg, long long n, int F, double k, double ridge,
                           const double* bounds4, double c, double scale, int hyps, double min_det, int refine,
                           unsigned long long seed, long long frame0, void* out, void* weight, void* resid) {
  Check chk(h, "rsl_velocity_consensus");
  auto own = [&] {
    return chk.invalid(!(c > 0) || !std::isfinite(c), "c must be finite, > 0") ||
           chk.invalid(!(scale > 0) || !std::isfinite(scale), "scale must be finite, > 0") ||
           chk.invalid(hyps < 1 || hyps > RSL_CONSENSUS_MAX_H, "hyps outside 1..RSL_CONSENSUS_MAX_H") ||
           chk.invalid(!(min_det > 0) || !(min_det <= 1), "min_det outside (0, 1]") ||
           chk.invalid(refine < 0 || refine > 100, "refine outside 0..100") ||
           chk.invalid(frame0 < 0, "frame0 must be >= 0");
  };
  rsl::VelProblem p;
  const int rc = velocity_problem(chk, own, az, gidx, az_table, G, y, amask, seg, n, F, k, ridge, bounds4, out, &p);
  if (rc || p.F == 0) return rc;
  return enter(h, RSL_K_VELOCITY, "velocity_consensus", [&] {
    return rsl::launch_velocity_consensus(h->stream, p, c, scale, hyps, min_det, refine, seed, frame0, (double*)out,
                                          (float*)weight, (double*)resid);
  });
}

int rsl_scan_register(rsl_handle h, const void* points, const void* seg, int F, long long n, const void* weight,
                      const void* rc, int C, const double* axes4, const void* prev_points, const void* prev_weight,
                      const void* prev_rc, long long prev_n, const void* prev_n_dev, const void* init, double h_fine,
                      double h_coarse, double dtheta, int K, int iters, double shrink, double tol, double w_min,
                      double dt, void* out, void* omega) {
  Check chk(h, "rsl_scan_register");
  auto pos = [](double v) { return std::isfinite(v) && v > 0.0; };
  const bool cull = rc || prev_rc;
  if (chk.invalid(!(pos(h_fine) && pos(h_coarse) && pos(dtheta) && pos(dt)),
                  "h, h_coarse, dtheta and dt must be finite, > 0") ||
      chk.invalid(!(std::isfinite(w_min) && w_min >= 0.0), "w_min must be finite, >= 0") ||
      chk.invalid(std::isnan(tol), "tol is NaN") || chk.invalid(h_coarse < h_fine, "h_coarse < h") ||
      chk.invalid(K < 0 || K > RSL_REG_MAX_K, "K outside 0..RSL_REG_MAX_K") ||
      chk.invalid(iters < 0 || iters > RSL_REG_MAX_ITERS, "iters outside 0..RSL_REG_MAX_ITERS") ||
      chk.invalid(!(shrink > 0.0 && shrink <= 1.0), "shrink outside (0, 1]") ||
      chk.invalid(F < 0 || n < 0 || prev_n < 0, "negative count") ||
      chk.invalid(cull && (!axes4 || C <= 0 || !pos(axes4[1]) || !std::isfinite(axes4[0])),
                  "rc needs C > 0 and axes4 with a finite r0 and a finite r_step > 0") ||
      chk.invalid(F > 0 && (!points || !seg || !out), "null points, seg or out"))
    return chk.status;
  if (F == 0) return RSL_OK;
  const rsl::RegProblem p{cloud_view(points, seg, n, F, weight), (const int*)rc, cull ? C : 1,
                          cull ? axes4[0] : 0.0, cull ? 1.0 / axes4[1] : 0.0,
                          (const float*)prev_points, prev_points ? (const float*)prev_weight : nullptr,
                          prev_points ? (const int*)prev_rc : nullptr, prev_points ? prev_n : 0,
                          prev_points ? (const long long*)prev_n_dev : nullptr, (const double*)init, h_fine, h_coarse,
                          dtheta, K, iters, shrink, tol, w_min, dt};
  return enter(h, RSL_K_AUX, "scan_register",
               [&] { return rsl::launch_scan_register(h->stream, p, (double*)out, (double*)omega); });
}

int rsl_map_update(rsl_handle h, const void* points, const void* seg, int F, long long n, const void* weight,
                   const void* poses, const double* grid4, int nx, int ny, double r_min, double r_max, double min_db,
                   void* hits, void* free_, void* stats) {
  Check chk(h, "rsl_map_update");
  const bool grid_ok = grid4 && std::isfinite(grid4[0]) && std::isfinite(grid4[1]) && std::isfinite(grid4[2]) &&
                       grid4[2] > 0.0;
  if (chk.invalid(F < 0 || n < 0, "negative count") ||
      chk.invalid(F > 0 && (!points || !seg || !poses || !grid4 || !hits), "null points, seg, poses, grid4 or hits") ||
      chk.invalid(grid4 && !grid_ok, "x0, y0 and cell must be finite, cell > 0") ||
      chk.invalid(!(r_min >= 0.0), "r_min must be >= 0") ||
      chk.invalid(!(std::isfinite(r_max) && r_max >= r_min), "r_max must be finite, >= r_min") ||
      chk.invalid(std::isnan(min_db) || min_db == INFINITY, "min_db is NaN or +inf") ||
      chk.invalid(nx <= 0 || ny <= 0 || (long long)nx * ny >= (1ll << 31), "nx, ny must be > 0, nx ny < 2^31"))
    return chk.status;
  if (!grid4) return RSL_OK;  // only with F = 0
  const double inv = 1.0 / grid4[2], rw = std::ceil(r_max * inv) + 1.0;
  if (chk.unsupported(!(rw <= (double)RSL_MAP_MAX_RW), "ceil(r_max / cell) + 1 above RSL_MAP_MAX_RW"))
    return chk.status;
  if (F == 0) return RSL_OK;
  const rsl::MapProblem p{cloud_view(points, seg, n, F, weight), (const double*)poses, grid4[0], grid4[1], inv, nx, ny,
                          (int)rw, r_min * r_min, r_max * r_max, min_db};
  return enter(h, RSL_K_AUX, "map_update", [&] {
    return rsl::launch_map_update(h->stream, p, (unsigned*)hits, (unsigned*)free_, (int*)stats);
  });
}

int rsl_map_logodds(rsl_handle h, const void* hits, const void* free_, long long ncells, double l_occ, double l_free,
                    double l_min, double l_max, void* out) {
  Check chk(h, "rsl_map_logodds");
  if (chk.invalid(!(std::isfinite(l_occ) && std::isfinite(l_free) && std::isfinite(l_min) && std::isfinite(l_max)),
                  "l_occ, l_free, l_min and l_max must be finite") ||
      chk.invalid(l_min > l_max, "l_min > l_max") ||
      chk.invalid(ncells < 0 || (ncells > 0 && (!hits || !out)), "negative count, or null hits or out"))
    return chk.status;
  if (ncells == 0) return RSL_OK;
  return enter(h, RSL_K_AUX, "map_logodds", [&] {
    return rsl::launch_map_logodds(h->stream, (const unsigned*)hits, (const unsigned*)free_, ncells, l_occ, l_free,
                                   l_min, l_max, (float*)out);
  });
}

int rsl_preprocess_rows(rsl_handle h, const void* in, long long rows, int S, const void* table, int dc, void* out) {
  Check chk(h, "rsl_preprocess_rows");
  if (chk.invalid(rows < 0 || S <= 0 || !in || !table || !out, "bad argument")) return chk.status;
  return enter(h, RSL_K_AUX, "preprocess_rows", [&] {
    return rsl::launch_preprocess_rows(h->stream, (const float2*)in, rows, S, (const float2*)table, dc, (float2*)out);
  });
}

int rsl_phase_model(rsl_handle h, const void* pos, const void* ang, long long n, const void* x, double k,
                    const void* y, int wrap, double ridge, void* pred, void* resid, void* cost) {
  Check chk(h, "rsl_phase_model");
  if (chk.invalid(n < 0 || !pos || !ang || !x, "bad argument") ||
      chk.invalid((resid || cost) && !y, "residual/cost need y"))
    return chk.status;
  return enter(h, RSL_K_AUX, "phase_model", [&] {
    return rsl::launch_phase_model(h->stream, (const double*)pos, (const double*)ang, n, (const double*)x, k,
                                   (const double*)y, wrap, ridge, (double*)pred, (double*)resid, (double*)cost);
  });
}

int rsl_bvls(rsl_handle h, const void* pos, const void* ang, long long n, const void* y, double k, int nv,
             double ridge, const void* lo, const void* hi, void* out) {
  Check chk(h, "rsl_bvls");
  if (chk.invalid(n < 0 || (nv != 3 && nv != 6) || !pos || !ang || !y || !lo || !hi || !out || ridge < 0,
                  "bad argument"))
    return chk.status;
  return enter(h, RSL_K_AUX, "bvls", [&] {
    return rsl::launch_bvls(h->stream, (const double*)pos, (const double*)ang, n, (const double*)y, k, nv, ridge,
                            (const double*)lo, (const double*)hi, (double*)out);
  });
}

int rsl_associate(rsl_handle h, const void* cur_xy, int nc, const void* prev_xy, int np, double thr, void* scratch,
                  void* match, void* dist) {
  Check chk(h, "rsl_associate");
  if (chk.invalid(nc < 0 || np < 0 || !(thr >= 0), "bad argument") ||
      chk.invalid(nc > 0 && (!cur_xy || !match || !dist || (np > 0 && (!prev_xy || !scratch))), "null pointer"))
    return chk.status;
  return enter(h, RSL_K_AUX, "associate", [&] {
    return rsl::launch_associate(h->stream, (const double*)cur_xy, nc, (const double*)prev_xy, np, thr,
                                 (unsigned*)scratch, (int*)match, (double*)dist);
  });
}

int rsl_peak_topk(rsl_handle h, const void* entry_base, long long entry_cap, int ncube, const void* e_coord,
                  const void* e_pdb, double thr_db, int kmax, int C, void* sel_entry, void* sel_frame, void* sel_rc,
                  void* sel_n) {
  Check chk(h, "rsl_peak_topk");
  if (chk.invalid(ncube < 0 || entry_cap < 0 || C <= 0 || C > 8192, "bad argument") ||
      chk.unsupported(kmax < 1 || kmax > 256, "kmax must be 1..256"))
    return chk.status;
  if (ncube == 0) return RSL_OK;
  if (chk.invalid(!entry_base || !sel_entry || !sel_frame || !sel_rc || !sel_n ||
                      (entry_cap > 0 && (!e_coord || !e_pdb)),
                  "null pointer"))
    return chk.status;
  // the reference compares float64 power_db > thr_db; the entries' power_db is f32, so compare against the largest
  // float <= thr_db (identical decisions for every f32 value)
  return enter(h, RSL_K_AUX, "peak_topk", [&] {
    return rsl::launch_topk_entries(h->stream, (const long long*)entry_base, entry_cap, ncube,
                                    (const unsigned*)e_coord, (const float*)e_pdb, rsl::threshold_as_float(thr_db),
                                    kmax, C, (int*)sel_entry, (int*)sel_frame, (int*)sel_rc, (int*)sel_n);
  });
}

int rsl_associate_nearest(rsl_handle h, const void* range_m, const void* az_rad, const void* s0, const void* off,
                          int nframes, long long ntargets, double thr, void* match, void* dist, void* phase) {
  Check chk(h, "rsl_associate_nearest");
  if (chk.invalid(nframes < 0 || ntargets < 0 || !(thr >= 0), "bad argument")) return chk.status;
  if (nframes == 0 || ntargets == 0) return RSL_OK;
  if (chk.invalid(!range_m || !az_rad || !s0 || !off || !match || !dist || !phase, "null pointer")) return chk.status;
  return enter(h, RSL_K_AUX, "associate_nearest", [&] {
    return rsl::launch_associate_nearest(h->stream, (const double*)range_m, (const double*)az_rad, (const double2*)s0,
                                         (const long long*)off, nframes, ntargets, thr, (int*)match, (double*)dist,
                                         (double*)phase);
  });
}

long long rsl_wrapped_scratch_bytes(long long n, int grid_n, int nextra) {
  if (n < 0 || grid_n < 0 || nextra < 0) return -1;
  return 8LL * rsl::WrappedSolveScratch(nullptr, n, (long long)grid_n * grid_n + nextra).total;
}

int rsl_wrapped_solve(rsl_handle h, const void* pos, const void* ang, long long n, const void* y, double k, int mode,
                      double w, double vmax, double wmax, const void* prev, const double* lo6, const double* hi6,
                      int nv, int grid_n, const void* extra, int nextra, int iters, void* scratch,
                      long long scratch_bytes, void* out) {
  Check chk(h, "rsl_wrapped_solve");
  const rsl::WrapArgs a = {(const double*)pos, (const double*)ang, n, (const double*)y, k, mode, w, vmax, wmax,
                           (const double*)prev, lo6, hi6, nv, (const double*)extra, nextra, iters};
  const bool own_bad = grid_n < 0 || grid_n * (long long)grid_n + nextra < 1;
  if (const int rc = wrapped_check(chk, a, own_bad, false, scratch, scratch_bytes,
                                   rsl_wrapped_scratch_bytes(n, grid_n, nextra), out))
    return rc;
  return enter(h, RSL_K_VELOCITY, "wrapped_solve", [&] {
    return rsl::launch_wrapped_solve(h->stream, a, grid_n, (double*)scratch, (double*)out);
  });
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
  Check chk(h, "rsl_wrapped_search");
  const rsl::WrapArgs a = {(const double*)pos, (const double*)ang, n, (const double*)y, k, mode, w, vmax, wmax,
                           (const double*)prev, lo6, hi6, nv, (const double*)extra, nextra, iters};
  const bool own_bad = !(spacing > 0) || nbest < 1 || nbest > 1024;
  if (const int rc = wrapped_check(chk, a, own_bad, !base6, scratch, scratch_bytes,
                                   rsl_wrapped_search_scratch_bytes(n, lo6, hi6, spacing, nbest, nextra), out))
    return rc;
  long long gx, gy;
  search_grid(lo6, hi6, spacing, &gx, &gy);
  return enter(h, RSL_K_VELOCITY, "wrapped_search", [&] {
    return rsl::launch_wrapped_search(h->stream, a, base6, gx, gy, nbest, (double*)scratch, (double*)out);
  });
}

int rsl_traj_scan(rsl_handle h, const void* vel, int vstride, int nv, const void* omega, int ostride,
                  const void* timestamps, double dt, long long F, int method, void* pos, void* quat, void* summary) {
  Check chk(h, "rsl_traj_scan");
  if (chk.invalid(F < 0 || nv < 0 || nv > 3 || vstride < nv || (omega && ostride < 3) || (method != 0 && method != 1),
                  "bad argument") ||
      chk.invalid(F > 0 && (!vel || !pos || !quat), "null pointer"))
    return chk.status;
  return enter(h, RSL_K_AUX, "traj_scan", [&] {
    return rsl::launch_traj_scan(h->stream, (const double*)vel, vstride, nv, (const double*)omega, ostride,
                                 (const double*)timestamps, dt, F, method, (double*)pos, (double*)quat,
                                 (double*)summary);
  });
}

int rsl_traj_apply(rsl_handle h, void* pos, void* quat, long long F, const void* base) {
  Check chk(h, "rsl_traj_apply");
  if (chk.invalid(F < 0 || (F > 0 && (!pos || !quat || !base)), "bad argument")) return chk.status;
  return enter(h, RSL_K_AUX, "traj_apply", [&] {
    return rsl::launch_traj_apply(h->stream, (double*)pos, (double*)quat, F, (const double*)base);
  });
}

int rsl_traj_smooth(rsl_handle h, const void* x, long long F, int ncol, int size, void* out) {
  Check chk(h, "rsl_traj_smooth");
  if (chk.invalid(F < 0 || ncol < 1 || size < 1 || (F > 0 && (!x || !out)), "bad argument")) return chk.status;
  return enter(h, RSL_K_AUX, "traj_smooth", [&] {
    return rsl::launch_traj_smooth(h->stream, (const double*)x, F, ncol, size, (double*)out);
  });
}

int rsl_traj_stitch(rsl_handle h, const void* summaries, int R, int rank, double dt, int method, void* state,
                    void* base) {
  Check chk(h, "rsl_traj_stitch");
  if (chk.invalid(R < 1 || rank < 0 || rank >= R || (method != 0 && method != 1) || !summaries || !state || !base,
                  "bad argument"))
    return chk.status;
  return enter(h, RSL_K_AUX, "traj_stitch", [&] {
    return rsl::launch_traj_stitch(h->stream, (const double*)summaries, R, rank, dt, method, (double*)state,
                                   (double*)base);
  });
}

int rsl_synth_pattern(rsl_handle h, const void* scatterers, int n, int A, int S, double fc, double bandwidth,
                      double chirp_duration, double antenna_spacing, void* pattern) {
  Check chk(h, "rsl_synth_pattern");
  if (chk.invalid(n < 0 || A <= 0 || S <= 0 || !(fc > 0) || !(chirp_duration > 0), "bad arguments") ||
      chk.invalid(!pattern || (n > 0 && !scatterers), "null pointer"))
    return chk.status;
  const double d = antenna_spacing > 0 ? antenna_spacing : 0.5 * 3e8 / fc;
  return enter(h, RSL_K_AUX, "synth_pattern", [&] {
    return rsl::launch_synth_pattern(h->stream, (const double*)scatterers, n, A, S, fc, bandwidth, chirp_duration, d,
                                     (double2*)pattern);
  });
}

int rsl_synth_cube(rsl_handle h, const void* pattern, int F, int A, int C, int S, double noise_power,
                   unsigned long long seed, long long frame0, void* cube) {
  Check chk(h, "rsl_synth_cube");
  if (chk.invalid(F < 0 || A <= 0 || C <= 0 || S <= 0 || frame0 < 0 || !(noise_power >= 0), "bad arguments") ||
      chk.unsupported(S % 2, "S must be even") || chk.invalid(!pattern || !cube, "null pointer"))
    return chk.status;
  return enter(h, RSL_K_AUX, "synth_cube", [&] {
    return rsl::launch_synth_cube(h->stream, (const double2*)pattern, F, A, C, S, noise_power, seed, frame0,
                                  (float2*)cube);
  });
}

long long rsl_pose_error_scratch_bytes(long long n, int nlen) {
  if (n < 0 || nlen < 0) return -1;
  return 8 * rsl::pose_error_scratch_doubles(n, nlen);
}

int rsl_pose_align(rsl_handle h, const void* est, const void* gt, long long n, void* scratch, void* align,
                   void* aligned, void* ape_err, void* ape_stats) {
  Check chk(h, "rsl_pose_align");
  if (chk.invalid(n < 1, "need at least one pose") ||
      chk.invalid(!est || !gt || !scratch || !align || !aligned || !ape_err, "null pointer"))
    return chk.status;
  return enter(h, RSL_K_AUX, "pose_align", [&] {
    return rsl::launch_pose_align(h->stream, (const double*)est, (const double*)gt, n, (double*)scratch,
                                  (double*)align, (double*)aligned, (double*)ape_err, (double*)ape_stats);
  });
}

int rsl_pose_rte(rsl_handle h, const void* aligned, const void* gt, long long n, const void* lengths, int nlen,
                 void* scratch, void* err, void* counts, void* stats) {
  Check chk(h, "rsl_pose_rte");
  if (chk.invalid(n < 1 || nlen < 0 || nlen > 1024, "bad arguments")) return chk.status;
  if (nlen == 0) return RSL_OK;
  if (chk.invalid(!aligned || !gt || !lengths || !scratch || !err || !counts || !stats, "null pointer"))
    return chk.status;
  return enter(h, RSL_K_AUX, "pose_rte", [&] {
    return rsl::launch_pose_rte(h->stream, (const double*)aligned, (const double*)gt, n, (const double*)lengths, nlen,
                                (double*)scratch, (double*)err, (unsigned long long*)counts, (double*)stats);
  });
}

int rsl_music_subspace(rsl_handle h, const void* sigs, long long n, int M, int num_sources, const void* steer_c128,
                       int G, void* spec) {
  Check chk(h, "rsl_music_subspace");
  if (chk.invalid(n < 0 || M < 1 || M > 16 || G < 1, "bad shape")) return chk.status;
  if (n == 0) return RSL_OK;
  if (chk.invalid(!sigs || !steer_c128 || !spec, "null pointer")) return chk.status;
  return enter(h, RSL_K_AUX, "music_subspace", [&] {
    return rsl::launch_music_subspace(h->stream, (const double*)sigs, n, M, num_sources, (const double*)steer_c128, G,
                                      (double*)spec);
  });
}

int rsl_esprit_subspace(rsl_handle h, const void* sigs, long long n, int M, int num_sources, double esprit_scale,
                        void* deg) {
  Check chk(h, "rsl_esprit_subspace");
  if (chk.invalid(n < 0 || M < 1 || M > 16, "bad shape")) return chk.status;
  if (n == 0) return RSL_OK;
  if (chk.invalid(!sigs || !deg, "null pointer")) return chk.status;
  return enter(h, RSL_K_AUX, "esprit_subspace", [&] {
    return rsl::launch_esprit_subspace(h->stream, (const double*)sigs, n, M, num_sources, esprit_scale, (double*)deg);
  });
}

}  // extern "C"
