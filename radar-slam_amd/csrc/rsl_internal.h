// rsl_internal.h — launcher declarations shared between the kernel files and the C-ABI layer.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rsl_cloud.h"   // CloudView, the point cloud of the registration and map problems
#include "rsl_launch.h"  // what every launcher launches with

namespace rsl {

// Cell count of a capacity-sized list: the device count (written by the emit stage) clamped to the list capacity,
// so an overflowing batch reads and writes only the slots that exist (the host sees the overflow in the count).
__device__ __forceinline__ long long list_count(const long long* dev, long long cap) {
  if (!dev) return cap;
  const long long n = *dev;
  return n < cap ? n : cap;
}

struct CellList;  // rsl_doa_common.h

// The lengths with a Stockham FFT in LDS (every other length up to 4096 takes the direct DFT): the size switches of
// launch_range_fft / launch_doppler_fft and rsl_fft_supported.
#define RSL_FFT_SIZES(X) \
  X(8) X(16) X(32) X(64) X(128) X(256) X(512) X(1024) X(2048) X(4096) X(25) X(50) X(100) X(200) X(400) X(800) X(1600)

// K1 tile queues of one handle (rsl_fft.hip): one 2 KiB queue per stream the handle launches K1 on, allocated on the
// handle's device at that stream's first K1 launch, freed by rf_queues_free (rsl_destroy).
struct RfQueues;
RfQueues* rf_queues_new(int device);
void rf_queues_free(RfQueues* s);
// An integer knob of the development build (make dev), by its environment name: 0 when unset, and always 0 in the
// product build.
int dev_knob(const char* name);
// A size that launch_range_fft, launch_doppler_fft or launch_doppler_detect cannot serve is hipErrorInvalidValue.  The
// C ABI never lets such a call through: rsl_fft_supported and doppler_detect_supported decide beforehand (rsl_api.hip).
// K1: dechirp * window (table), range FFT (S points), DC bin zeroing.
// cube c64 [F, A, Ct, S] (chirps chirp0 .. chirp0+C-1 used) -> work c64 [F, A, C, S]
hipError_t launch_range_fft(hipStream_t st, const float2* cube, int F, int A, int Ct, int chirp0, int C, int S,
                            const float2* table, const float2* tw_S, int dc, float2* work, RfQueues* queues,
                            bool packed = false);
// K2: Doppler FFT (C points) + fftshift on both axes, transposed store.
// work c64 [F, A, C, S] -> rds c64 [F, A, S, C]
hipError_t launch_doppler_fft(hipStream_t st, const float2* work, int F, int A, int C, int S, const float2* tw_C,
                              float2* rds);

// K2+K3 fused (Doppler FFT + fftshift + RDS store + detection); supported when C is a power of two and the
// block's KB range bins tile both halves of S.
bool doppler_detect_supported(int C, int S);
float threshold_as_float(double thr);  // largest float t <= thr
// What a detector is asked and where it answers, as the launcher layers hand it down (host side only: the kernels take
// the members as separate `__restrict__` arguments).  thr_p: power threshold (the kernels compare against its
// threshold_as_float); i_lo..i_hi: range gate; mask u64 [F, A, S, W], row_count [F, A, S], optional dbmap, pk_pow.
struct DetectArgs {
  double thr_p;
  int i_lo, i_hi;
  unsigned long long* mask;
  int* row_count;
  float* dbmap;
  float* pk_pow;
};
// *pk_group: the rows per group of the compacted peak powers (1 = row-compact).
hipError_t launch_doppler_detect(hipStream_t st, const float2* work, int F, int A, int C, int S, const float2* tw_C,
                                 float2* rds, const DetectArgs& det, int* pk_group, bool packed = false);
// packed (both launches): `work` holds packed rows (rsl_packed.h: 6 B per value in 24 KiB tiles, each bin's int8
// exponent inside its 48-B unit) -- only where work_packed_supported(C, S).
bool work_packed_supported(int C, int S);
// K3: 3x3 local max (reflect), threshold, range gate -> per-antenna bit masks + row counts.  detect_rows(C): the range
// rows per workgroup at C Doppler cells, 0 where C is too large for the kernel's LDS tile (C > 4096).
int detect_rows(int C);
hipError_t launch_detect(hipStream_t st, const float2* rds, int F, int A, int S, int C, const DetectArgs& det);
// K3 alternatives, the CFAR family (CfarWindow and the launcher both share: rsl_cfar_common.h).  Every window within
// RSL_CFAR_MAX_HALF fits the CU's LDS at every C <= RSL_CFAR_MAX_C: each kernel file asserts it at compile time.
// rsl_cfar.hip: 2-D cell-averaging CFAR (guard and training half-sizes of the window; Doppler wraps, range truncates)
// + 3x3 local max + range gate + power floor -> the same outputs as launch_detect, peak_pow row-compact.
struct CfarWindow;
hipError_t launch_detect_cfar(hipStream_t st, const float2* rds, int F, int A, int S, int C, CfarWindow win,
                              float alpha, const DetectArgs& det);
// rsl_oscfar.hip: 2-D ordered-statistic CFAR on the same window and with the same outputs: the rank-th fraction of the
// training cells (k(i) = min(n(i), max(1, ceil(rank n(i))))) in place of their mean.
hipError_t launch_detect_oscfar(hipStream_t st, const float2* rds, int F, int A, int S, int C, CfarWindow win,
                                double rank, float alpha, const DetectArgs& det);
// rsl_nci.hip: non-coherent integration, rds c64 [F, A, S, C] -> power f32 [F, S, C], the fp32 sum over the antennas
// in antenna order.
hipError_t launch_power_integrate(hipStream_t st, const float2* rds, int F, int A, int S, int C, float* power);
// The three detectors on F fp32 power maps [F, S, C] in place of the F * A c64 maps (rsl_detect_power): the same
// kernels with the element type float (cell_power, rsl_detect_common.h), outputs as with A = 1.
hipError_t launch_detect(hipStream_t st, const float* power, int F, int S, int C, const DetectArgs& det);
hipError_t launch_detect_cfar(hipStream_t st, const float* power, int F, int S, int C, CfarWindow win, float alpha,
                              const DetectArgs& det);
hipError_t launch_detect_oscfar(hipStream_t st, const float* power, int F, int S, int C, CfarWindow win, double rank,
                                float alpha, const DetectArgs& det);
// Per-frame offsets of peak entries (antenna-major) and union cells (range-major).
hipError_t launch_offsets(hipStream_t st, const unsigned long long* mask, const int* row_count, int F, int A, int S,
                          int C, int* entry_row_off, int* cell_row_off, int* cell_row_cnt, long long* entry_base,
                          long long* cell_base, long long* frame_counts, unsigned long long* umask);
// Emit compacted entries and cells in reference order, by one of two paths (rsl_detect.hip's header says what each
// computes).  The compact path serves a call with the union mask, with peak powers unless no power_db is wanted, and
// with a power-of-two count W = ceil(C / 64) <= 64 of mask words per row; the general path serves every other call.
bool emit_compact_supported(int C, bool union_mask, bool peak_pow, bool want_pdb);
// What both emit paths read of rsl_peak_offsets' results and where they write the lists, typed by peak_offsets and
// peak_lists (rsl_api.hip).  Host side only, like DetectArgs: the kernels take the members as separate `__restrict__`
// arguments.  The caps are the lists' capacities in entries and cells; e_pdb is optional.
struct PeakOffsets {
  const int* entry_row_off;
  const int* cell_row_off;
  const long long* entry_base;
  const long long* cell_base;
};
struct PeakLists {
  long long entry_cap, cell_cap;
  unsigned* e_coord;
  int* e_cell;
  float* e_pdb;
  int* c_frame;
  int* c_rc;
  unsigned* c_amask;
};
// General path: one wave per range row, power_db from the RDS.
hipError_t launch_emit_rows(hipStream_t st, const float2* rds, const unsigned long long* mask, int F, int A, int S,
                            int C, const PeakOffsets& off, const PeakLists& out);
// Compact path, only where emit_compact_supported: block compactions of the masks and the union masks, power_db from
// the group-compact peak powers (pk_group rows per group, 1 = row-compact); no RDS read.
hipError_t launch_emit_compact(hipStream_t st, const unsigned long long* mask, const unsigned long long* umask,
                               const float* pk_pow, int pk_group, int F, int A, int S, int C, const PeakOffsets& off,
                               const PeakLists& out);
// K4..K7, the direction-of-arrival stage.  CellList (the cells of a call) and steer_layout (the sections of the
// steering table) are in rsl_doa_common.h.
// K5: steering scan on MFMA (f32 16x16x4), argmax; optional spectrum (spec_ld 0: cell-major [n][G], > 0: grid-major
// with that leading dimension, < 0: cell-blocked [ceil(n / 32)][G][32]).  steer_tab: section (1) of the table.
hipError_t launch_doa_scan(hipStream_t st, CellList cl, const float* steer_tab, int G, int music, int* out_idx,
                           float* out_gmax, float* out_spec, long long spec_ld);
// Exact fp64 re-scan of the cells a DoA scan marked ambiguous (out_idx < 0), rsl_doa_toep.hip k_doa_fixup.
hipError_t launch_doa_fixup(hipStream_t st, CellList cl, int G, int music, const double* steerT, int* out_idx,
                            float* out_gmax);
// K5 fast path: Toeplitz-form argmax on f16 MFMA with hi/lo split (rsl_doa_toep.hip), followed by its fixup.
// toep_tab: section (2) of the table, where steer_layout(G, A).toep_fits.
hipError_t launch_doa_toep(hipStream_t st, CellList cl, const void* toep_tab, int G, int music, const double* steerT,
                           int* out_idx, float* out_gmax, double esprit_scale, double* out_esprit, double* out_phase,
                           float* out_spec = nullptr);
// K5 alternative (rsl_ssmusic.hip): forward-backward spatially smoothed MUSIC, up to nmax angles per cell (the
// estimator is specified at rsl_doa_smoothed in include/rsl.h).  steer c64 [G][L]; 2 <= L <= RSL_SS_MAX_L.
hipError_t launch_doa_smoothed(hipStream_t st, CellList cl, const float2* steer, int G, int L, int nmax,
                               int num_sources, float rel, int* out_nsrc, int* out_idx, float* out_den, float* out_eig,
                               float* out_spec);
// Range-azimuth maps (rsl_ramap.hip; the contracts are rsl_range_cov's and rsl_range_azimuth's in rsl.h): the
// covariance of every range bin over the Doppler window [c0, c1) as one fp32 MFMA Gram tile, rds c64 [F, A, S, C] ->
// cov c64 [F, S, A, A] (2 <= A <= 16), and the Bartlett (capon = 0) / Capon power of n covariances over the grid of
// steer c64 [G][A] -> map f32 [n, G], arg i32 [n] (nullable).
hipError_t launch_range_cov(hipStream_t st, const float2* rds, int F, int A, int S, int C, int c0, int c1,
                            float2* cov);
hipError_t launch_range_azimuth(hipStream_t st, const float2* cov, long long n, int A, const float2* steer, int G,
                                int capon, float loading, float* map, int* arg);
// Host: builds the Toeplitz operand table; returns 1 if the steering matrix is a uniform linear array.
int toep_table_build(const double* steer_c128, int G, int M, uint16_t* out);
// K4/K6: normalised signature, ESPRIT closed form (fp64), spatial phase, azimuth lookup.
hipError_t launch_cell_extras(hipStream_t st, CellList cl, double esprit_scale, const int* gidx,
                              const double* az_table, float2* sig_out, double* esprit_deg, double* phase,
                              double* az_out);
// Point cloud (rsl_refine.hip; the contract is rsl_cell_refine's in rsl.h): sub-bin range / Doppler offsets from the
// five powers around each cell (power f32 [*, S, C], or null: formed from the RDS), azimuth at the parabola vertex of
// the beamforming values around gidx over steer c64 [G][A] -> out_points, the rows of rsl_cloud.h (16-B aligned), out_az f64 [n].
hipError_t launch_cell_refine(hipStream_t st, CellList cl, const float* power, const int* gidx, const double* az_table,
                              const float2* steer, int G, int range_mode, int doppler_mode, const double* axes4,
                              float* out_points, double* out_az);
// K7: robust confidence for (cell, grid index) pairs (fp64).
hipError_t launch_confidence(hipStream_t st, CellList cl, const int* gidx, const double* steer_c128,
                             const double* steer_phase, double* conf_out);
// The problem the three velocity solvers share (rsl_velocity's inputs in include/rsl.h), checked and typed by
// velocity_problem (rsl_api.hip); the box is bounds4 unpacked.  Host side only, like DetectArgs: the kernels take the
// members as separate `__restrict__` arguments (a member loses it, and they store weight / resid between loads of y).
struct VelProblem {
  const double* az;
  const int* gidx;
  const double* az_table;
  int G;
  const double* y;
  const unsigned* amask;
  const long long* seg;
  long long n;
  int F;
  double k, ridge, lx, hx, ly, hy;
};
// K8: batched bounded / ridge least squares velocity solve, one segment per frame.
hipError_t launch_velocity(hipStream_t st, const VelProblem& p, double* out, double* resid, double* pred);
// K8 alternative (rsl_vel_robust.hip): Huber / Tukey IRLS from the LS start, fixed or median-estimated scale.
hipError_t launch_velocity_robust(hipStream_t st, const VelProblem& p, int loss, double c, double scale, int iters,
                                  double tol, double* out, float* weight, double* resid);
// K8c: consensus (RANSAC) velocity solve (rsl_vel_consensus.hip); the contract is rsl_velocity_consensus's in rsl.h.
hipError_t launch_velocity_consensus(hipStream_t st, const VelProblem& p, double c, double scale, int hyps,
                                     double min_det, int refine, unsigned long long seed, long long frame0, double* out,
                                     float* weight, double* resid);

// Scan registration (rsl_register.hip; the contract is rsl_scan_register's in rsl.h), checked and typed by
// rsl_scan_register (rsl_api.hip).  Passed to the kernel by value.  inv_step = 1 / axes4[1], 0 without axes.
struct RegProblem {
  CloudView cloud;
  const int* rc;
  int C;
  double r0, inv_step;
  const float* prev_points;
  const float* prev_weight;
  const int* prev_rc;
  long long prev_n;
  const long long* prev_n_dev;
  const double* init;
  double h, h_coarse, dtheta;
  int K, iters;
  double shrink, tol, w_min, dt;
};
hipError_t launch_scan_register(hipStream_t st, const RegProblem& p, double* out, double* omega);

// Grid map (rsl_map.hip; the contract is rsl_map_update's in rsl.h), checked and typed by rsl_map_update (rsl_api.hip).
// Passed to the kernel by value.  inv = 1 / cell, Rw = (int)ceil(r_max inv) + 1, rmin2 / rmax2 the squared range gate.
struct MapProblem {
  CloudView cloud;
  const double* poses;
  double x0, y0, inv;
  int nx, ny, Rw;
  double rmin2, rmax2, min_db;
};
hipError_t launch_map_update(hipStream_t st, const MapProblem& p, unsigned* hits, unsigned* free_, int* stats);
hipError_t launch_map_logodds(hipStream_t st, const unsigned* hits, const unsigned* free_, long long ncells,
                              double l_occ, double l_free, double l_min, double l_max, float* out);

// K9: greedy association and wrapped-phase multi-start solve (rsl_wrap.hip).
// configs[3] pattern (rsl_scene.hip): per-cube top-k peak selection and the analyser's nearest association.
hipError_t launch_topk_entries(hipStream_t st, const long long* entry_base, long long entry_cap, int ncube,
                               const unsigned* e_coord, const float* e_pdb, float thr_db, int kmax, int C,
                               int* sel_entry, int* sel_frame, int* sel_rc, int* sel_n);
hipError_t launch_associate_nearest(hipStream_t st, const double* range_m, const double* az_rad, const double2* s0,
                                    const long long* off, int nframes, long long ntargets, double thr, int* match,
                                    double* dist, double* phase);
hipError_t launch_associate(hipStream_t st, const double* cur, int nc, const double* prev, int np, double thr,
                            unsigned* used_scratch, int* match, double* dist);
// The arguments rsl_wrapped_solve and rsl_wrapped_search share (include/rsl.h).
struct WrapArgs {
  const double *pos, *ang;
  long n;
  const double* y;
  double k;
  int mode;
  double w, vmax, wmax;
  const double *prev, *lo, *hi;
  int nv;
  const double* extra;
  int nextra, iters;
};
// The scratch buffers of the two wrapped launchers, in doubles.  Each section's size is stated once, in the order of
// the layout: the launcher carves its pointers with the struct, rsl_wrapped_scratch_bytes and
// rsl_wrapped_search_scratch_bytes take `total` of one built on a null buffer (whose pointers stay null).
struct ScratchCarver {
  double* buf;
  long used;
  double* take(long doubles) {
    double* p = buf ? buf + used : nullptr;
    used += doubles;
    return p;
  }
};
struct WrappedSolveScratch {
  double *J, *Hd, *res;  // J [6n] | Hd [36] | per-start results [8 nstart], nstart = grid_n^2 + nextra
  long total;
  WrappedSolveScratch(double* buf, long n, long nstart) {
    ScratchCarver c{buf, 0};
    J = c.take(6 * n);
    Hd = c.take(36);
    res = c.take(8 * nstart);
    total = c.used;
  }
};
struct WrappedSearchScratch {
  // J [6n] | Hd [36] | stage-1 terms T [3n] | base [6] | block results [4 nblk], one block per 256 stage-1 starts |
  // stage-2 starts [6 nstart] | per-start results [8 nstart], nstart = nbest + nextra
  double *J, *Hd, *T, *base, *blk, *starts, *res;
  long nblk, total;
  WrappedSearchScratch(double* buf, long n, long nstart1, long nstart) : nblk((nstart1 + 255) / 256) {
    ScratchCarver c{buf, 0};
    J = c.take(6 * n);
    Hd = c.take(36);
    T = c.take(3 * n);
    base = c.take(6);
    blk = c.take(4 * nblk);
    starts = c.take(6 * nstart);
    res = c.take(8 * nstart);
    total = c.used;
  }
};
hipError_t launch_wrapped_search(hipStream_t st, const WrapArgs& a, const double* base6, long gx, long gy, int nbest,
                                 double* scratch, double* out);
hipError_t launch_wrapped_solve(hipStream_t st, const WrapArgs& a, int gn, double* scratch, double* out);

// Trajectory scans (rsl_traj.hip).
hipError_t launch_traj_scan(hipStream_t st, const double* vel, int vstride, int nv, const double* om, int ostride,
                            const double* ts, double dt, long F, int method, double* pos, double* quat,
                            double* summary);
hipError_t launch_traj_apply(hipStream_t st, double* pos, double* quat, long F, const double* base);
hipError_t launch_traj_stitch(hipStream_t st, const double* summ, int R, int rank, double dt, int method,
                              double* state, double* base);
hipError_t launch_traj_smooth(hipStream_t st, const double* x, long F, int ncol, int size, double* out);
// MUSIC / ESPRIT with num_sources != 1 (rsl_subspace.hip), fp64, per-call drop-in paths.
hipError_t launch_music_subspace(hipStream_t st, const double* sigs, long n, int M, int K, const double* steer,
                                 int G, double* spec);
hipError_t launch_esprit_subspace(hipStream_t st, const double* sigs, long n, int M, int K, double esprit_scale,
                                  double* deg);
// Pose-error evaluation (rsl_eval.hip): Umeyama + quaternion-mean alignment, APE errors / statistics, RTE.
long long pose_error_scratch_doubles(long long n, int nlen);
hipError_t launch_pose_align(hipStream_t st, const double* est, const double* gt, long n, double* scratch,
                             double* align, double* aligned, double* ape_err, double* ape_stats);
hipError_t launch_pose_rte(hipStream_t st, const double* aligned, const double* gt, long n, const double* len,
                           int nlen, double* scratch, double* err, unsigned long long* cnt, double* stats);

hipError_t launch_preprocess_rows(hipStream_t st, const float2* in, long rows, int S, const float2* table, int dc,
                                  float2* out);
hipError_t launch_phase_model(hipStream_t st, const double* pos, const double* ang, long n, const double* x, double k,
                              const double* y, int wrap, double ridge, double* pred, double* resid, double* cost);
hipError_t launch_bvls(hipStream_t st, const double* pos, const double* ang, long n, const double* y, double k, int nv,
                       double ridge, const double* lo, const double* hi, double* out);
// Synthetic cube generator (simulate_raw.py:102-221): fp64 [A, S] pattern, then pattern + Philox noise.
hipError_t launch_synth_pattern(hipStream_t st, const double* sc, int n, int A, int S, double fc, double bandwidth,
                                double Tc, double d, double2* pattern);
hipError_t launch_synth_cube(hipStream_t st, const double2* pattern, int F, int A, int C, int S, double noise_power,
                             unsigned long long seed, long long frame0, float2* cube);

}  // namespace rsl
