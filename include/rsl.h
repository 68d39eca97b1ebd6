/* rsl.h — C ABI of the MI355X-native radar signal chain (librsl.so, gfx950 / CDNA4).
 *
 * Drop-in boundary for the per-frame chain of zaidcontractor/radar-slam (snapshot 2025-11-21).
 * The reference is pure Python with no FFI; its boundary is the Python class surface listed per
 * entry point below (file:line in the reference tree).  The Python host layer
 * radar-slam_amd/src/... keeps those module paths and signatures and binds these symbols with
 * ctypes (radar-slam_amd/rsl/_lib.py; binding stubs for other hosts: INTEGRATION.md).
 *
 * Conventions
 *   - every pointer named dev_* / void* data argument is DEVICE memory (hipMalloc / torch tensor);
 *     complex values are interleaved float32 (c64) unless the name says c128 / f64;
 *   - all launches are asynchronous on the handle's stream (rsl_set_stream); rsl_sync waits;
 *   - return 0 (RSL_OK) or an RSL_ERR_* code; rsl_last_error(h) describes the last failure;
 *   - a handle belongs to one device and may launch on any of that device's streams (rsl_set_stream); one thread
 *     drives a handle at a time; handles share no mutable state (the K1 tile queues are per handle and stream,
 *     allocated on the handle's device at a stream's first K1 launch, freed by rsl_destroy);
 *   - graph capture: K1's first launch on a stream allocates that stream's queue, which capture forbids (RSL_ERR_HIP,
 *     "operation not permitted when stream is capturing"): launch once uncaptured first, and never replay one captured
 *     K1 on two streams concurrently (the replays would share the captured queue);
 *   - F = 0 (an empty batch) is valid: nothing is launched (rsl_peak_offsets zeroes the two bases), and
 *     buffers sized by F may be null;
 *   - a problem that needs more workgroups than a grid holds (2^31 - 1) is refused (RSL_ERR_HIP, "invalid argument"),
 *     never cut down to the part that fits: that launch does not run, nor any after it in the same call;
 *   - capacity-sized lists (entries, cells) never overflow in memory: items past the capacity are dropped,
 *     the bases keep the true counts, and the list consumers stop at the capacity.
 */
#ifndef RSL_H
#define RSL_H

#ifdef __cplusplus
extern "C" {
#endif

#define RSL_OK 0
#define RSL_ERR_INVALID 1     /* bad argument (shape, null pointer)        -> Python ValueError   */
#define RSL_ERR_UNSUPPORTED 2 /* FFT size / antenna count not implemented  -> Python ValueError   */
#define RSL_ERR_HIP 3         /* HIP runtime error                          -> Python RuntimeError */

#define RSL_METHOD_BEAMFORMING 0
#define RSL_METHOD_MUSIC 1
/* rsl_doa method flag: use the Toeplitz f16-MFMA argmax path (requires RSL_STEER_TOEPLITZ from the table build) */
#define RSL_DOA_TOEPLITZ 0x100
/* rsl_doa method flag: out_spec is grid-major f32 [G][ncell] (leading dimension = the list capacity ncell) instead of
 * cell-major [n][G]; the batched spectrum path (coalesced stores) */
#define RSL_DOA_SPEC_GMAJOR 0x200
/* rsl_doa method flag: out_spec is cell-blocked f32 [ceil(ncell / 32)][G][32] (cell c, grid point g at
 * ((c / 32) G + g) 32 + c % 32): every store is a contiguous run; the batched chain's spectrum layout */
#define RSL_DOA_SPEC_BLOCKED 0x400
/* rsl_steer_table_build flags */
#define RSL_STEER_TOEPLITZ 1

/* kernel ids for rsl_timing_read */
#define RSL_K_RANGE_FFT 0
#define RSL_K_DOPPLER_FFT 1
#define RSL_K_DETECT 2
#define RSL_K_OFFSETS 3
#define RSL_K_EMIT 4
#define RSL_K_DOA_SCAN 5
#define RSL_K_CELL_EXTRAS 6
#define RSL_K_CONFIDENCE 7
#define RSL_K_VELOCITY 8
#define RSL_K_AUX 9
#define RSL_K_COUNT 10

typedef struct rsl_context* rsl_handle;

/* ABI version returned by rsl_version().
 *   1  rounds 1-4;
 *   2  rsl_rds_detect_chunked removed; rsl_steer_table_floats grew by the 4GM-float fp64 transposed section
 *      (steer_t64_offset) that rsl_doa / rsl_doa_extras now read: tables built or sized by a v1 library must be
 *      rebuilt; K1 tile queues are per handle and stream (freed by rsl_destroy). */
#define RSL_VERSION 2
int rsl_version(void);
int rsl_create(rsl_handle* out, int device);
int rsl_destroy(rsl_handle h);
const char* rsl_last_error(rsl_handle h);
int rsl_set_stream(rsl_handle h, void* hip_stream); /* NULL = null stream */
int rsl_sync(rsl_handle h);
/* 1 = radix-{2,3,4,5,7,8} LDS FFT, 2 = direct-DFT fallback (any n <= 4096), 0 = unsupported */
int rsl_fft_supported(int n);

/* Per-kernel device time (hipEvents recorded on the handle's stream around every launch). */
int rsl_timing_enable(rsl_handle h, int on);
int rsl_timing_reset(rsl_handle h);
int rsl_timing_read(rsl_handle h, int kernel_id, double* total_ms, long long* launches);
/* The launches of one kernel id since the last rsl_timing_reset: [start, end] of each, in ms after an event that the
 * reset recorded on the handle's stream (one device clock for every stream the handle ran on), in launch order.
 * Writes min(n, max) pairs (nullable arrays) and returns n, the launch count (-1 on a bad argument). */
int rsl_timing_spans(rsl_handle h, int kernel_id, int max, double* start_ms, double* end_ms);

/* a7  SignalPreprocessor.generate_range_doppler_spectrum  (dechirp.py:168-213, incl. process_chirp
 *     :143-166, dechirp_signal :122-141, apply_window :85-108, remove_dc :110-120, chirp_subset :183-187).
 *     cube c64 [F, A, C_total, S]; chirps chirp0 .. chirp0+C-1 are used;
 *     table c64 [S] = conj(reference_chirp) * window, built on the host in fp64 (dechirp.py:74-83);
 *     dc_removal != 0 zeroes range bin 0 (== subtracting the complex mean before the FFT);
 *     work c64 [F, A, C, S] scratch; rds c64 [F, A, S, C], fftshift on both axes. */
int rsl_rds(rsl_handle h, const void* cube, int F, int A, int C_total, int chirp0, int C, int S,
            const void* table, int dc_removal, void* work, void* rds);

/* a8  SignalPreprocessor.extract_range_doppler_peaks  (dechirp.py:215-278).
 *     thr_power = 10^(threshold_db/10) - 1e-12 (a cell passes when (double)|rds|^2 > thr_power);
 *     range gate i_lo <= range_bin <= i_hi (from linspace(0, rr*S, S) on the host);
 *     mask u64 [F, A, S, W], W = ceil(C/64) (bit j%64 of word j/64 = peak at doppler j);
 *     row_count i32 [F, A, S];  db_map f32 [F, A, S, C] (nullable) = 10 log10(|rds|^2 + 1e-12);
 *     peak_pow f32 [F, A, S, C] (nullable): row-compact |rds|^2 of the peaks, slot = rank within the row.
 *     RSL_ERR_UNSUPPORTED: C > 4096 (every length rsl_rds produces is supported). */
int rsl_detect(rsl_handle h, const void* rds, int F, int A, int S, int C, double thr_power, int i_lo, int i_hi,
               void* mask, void* row_count, void* db_map, void* peak_pow);

/* CA-CFAR detector: an alternative to rsl_detect's fixed threshold with the same outputs (mask, row_count, db_map,
 *     peak_pow row-compact, group 1), so rsl_peak_offsets / rsl_peak_emit and everything after run unchanged.
 *     2-D cell averaging on the fp32 power p = |rds|^2 of every (frame, antenna) map [S, C].  With half-sizes
 *     guard (guard_r, guard_d) and training (train_r, train_d) in range and Doppler, hr = guard_r + train_r and
 *     hd = guard_d + train_d, the training cells of cell (i, j) are the offsets |di| <= hr, |dj| <= hd without the
 *     guard box |di| <= guard_r, |dj| <= guard_d (which holds the cell under test).  The Doppler axis wraps (column
 *     (j + dj) mod C); the range axis truncates (rows outside [0, S) are skipped), so the mean divides by the number
 *     n(i) of training cells that exist; no window reads another antenna's or frame's map.
 *     Cell (i, j) is a peak iff  p > alpha * sum / n(i)  (strict: an all-zero map has no peak),  p >= every existing
 *     3x3 neighbour (rsl_detect's rule and boundary),  i_lo <= i <= i_hi,  and  (double)p > thr_power (a negative
 *     thr_power disables the floor).  alpha multiplies the training MEAN (for a false-alarm rate Pfa in exponential
 *     noise: alpha = N (Pfa^(-1/N) - 1), N the full-window count).  The sum is formed by fp32 additions of
 *     training-cell powers only (relative error < 7e-5).
 *     RSL_ERR_INVALID: a negative half-size, train_r + train_d < 1, hr or hd > RSL_CFAR_MAX_HALF, 2 hd + 1 > C,
 *     2 hr + 1 > S, alpha <= 0 or not finite, S > 8192.  RSL_ERR_UNSUPPORTED: C > RSL_CFAR_MAX_C.
 *     F = 0 is valid and launches nothing.  Timed under RSL_K_DETECT. */
#define RSL_CFAR_MAX_HALF 16
#define RSL_CFAR_MAX_C 512
int rsl_detect_cfar(rsl_handle h, const void* rds, int F, int A, int S, int C, int guard_r, int guard_d, int train_r,
                    int train_d, double alpha, double thr_power, int i_lo, int i_hi, void* mask, void* row_count,
                    void* db_map, void* peak_pow);

/* OS-CFAR detector (ordered statistic, Rohling 1983): rsl_detect_cfar with the k-th smallest training cell in place
 *     of the training mean, so that a second reflector inside the window does not raise the noise estimate.  There is
 *     no reference counterpart: this comment is the specification.
 *     Training cells: exactly those of rsl_detect_cfar (offsets |di| <= hr, |dj| <= hd without the guard box; Doppler
 *     wraps, range truncates; no window reads another antenna's or frame's map); n(i) is the number of training cells
 *     that exist for range row i.
 *     Rank: k(i) = min(n(i), max(1, ceil(rank * n(i)))), evaluated in fp64, rank in (0, 1].  Truncated edge rows keep
 *     the same fraction; rank = 1 is the window maximum, a tiny rank the minimum.
 *     Decision: with p = |rds|^2 in fp32 and alpha_f = (float)alpha, cell (i, j) is a peak iff
 *       the number of existing training cells q with alpha_f * q < p (one fp32 multiply) is >= k(i)  -- fp32
 *       multiplication by a positive constant is monotone, so this is p > fl32(alpha_f * x_(k(i))), x_(k) the k-th
 *       smallest training power; strict: an all-zero map has no peak,
 *       p >= every existing 3x3 neighbour (rsl_detect's rule and boundary),  i_lo <= i <= i_hi,  and
 *       (double)p > thr_power (a negative thr_power disables the floor).
 *     The count is exact and independent of the order in which the cells are visited.
 *     Factor: alpha multiplies the order statistic, not a mean.  For a square-law detector in exponential noise with
 *     N training cells and rank k:  Pfa = prod_{m=0}^{k-1} (N - m) / (N - m + alpha)  (N = 16, k = 12, Pfa 1e-6:
 *     alpha = 20.95); the host inverts it with N the full-window count.
 *     Outputs, F = 0 and timing (RSL_K_DETECT) as rsl_detect_cfar; peak_pow row-compact, group 1.
 *     RSL_ERR_INVALID: every case of rsl_detect_cfar; rank not in (0, 1] or NaN; (float)alpha not finite and > 0.
 *     RSL_ERR_UNSUPPORTED: C > RSL_CFAR_MAX_C.  Every window up to RSL_CFAR_MAX_HALF is supported at every
 *     C <= RSL_CFAR_MAX_C. */
int rsl_detect_oscfar(rsl_handle h, const void* rds, int F, int A, int S, int C, int guard_r, int guard_d,
                      int train_r, int train_d, double rank, double alpha, double thr_power, int i_lo, int i_hi,
                      void* mask, void* row_count, void* db_map, void* peak_pow);

/* Non-coherent integration: the antenna-summed power map, the input of rsl_detect_power and an output in its own
 *     right (the integrated range-Doppler map).  There is no reference counterpart: this comment is the specification.
 *     rds c64 [F, A, S, C] -> power f32 [F, S, C]:
 *       P[f, i, j] = ((p_0 + p_1) + p_2) + ... + p_{A-1}   in fp32,
 *     where p_a is the fp32 power of rds[f, a, i, j] exactly as the detectors form it (fmaf(re, re, im * im)).  The
 *     antenna order is fixed, so the result is deterministic; its relative error against the exact sum is at most
 *     (A + 2) 2^-24.  For A = 1 it is bit-identical to the power that rsl_detect / rsl_detect_cfar /
 *     rsl_detect_oscfar compute for that cell.
 *     F = 0 is valid and launches nothing.  RSL_ERR_INVALID: a null pointer with F > 0, A, S or C <= 0, A > 32 (the
 *     width of c_amask).  Timed under RSL_K_DETECT. */
int rsl_power_integrate(rsl_handle h, const void* rds, int F, int A, int S, int C, void* power);

/* The three detection rules on a real power map: power f32 [F, S, C], F maps, one per frame (rsl_power_integrate's
 *     output, or any non-negative map).  rule selects
 *       RSL_RULE_THRESHOLD  rsl_detect's rule (guard_*, train_*, rank and alpha are ignored),
 *       RSL_RULE_CA         rsl_detect_cfar's rule (rank is ignored),
 *       RSL_RULE_OS         rsl_detect_oscfar's rule,
 *     word for word as specified there, with p read from the map instead of formed from a complex value: the same
 *     window (Doppler wraps, range truncates), n(i) and k(i), the same strict comparisons, the add-only fp32 training
 *     sum of CA, the exact count of OS, the 3x3 rule, the range gate and the floor (double)p > thr_power.  The kernels
 *     are those of the per-antenna entry points, instantiated for a real element.
 *     Outputs as rsl_detect* with A = 1: mask u64 [F, S, W], row_count i32 [F, S], db_map f32 [F, S, C] (nullable) =
 *     10 log10f(P + 1e-12f), peak_pow f32 [F, S, C] (nullable) row-compact, group 1; rsl_peak_offsets / rsl_peak_emit
 *     take them with A = 1 (every cell is then one entry of antenna 0 and its c_amask is 1).
 *     Factor: in exponential noise the sum of A looks is Gamma(A)-distributed, so alpha for a false-alarm rate differs
 *     from the one-look formulas above; the host layer designs it (rsl/tables.py: cfar_alpha_nci, os_cfar_alpha_nci).
 *     Errors: the cases of the per-antenna function of the rule (RSL_RULE_THRESHOLD: those of rsl_detect); an unknown
 *     rule is RSL_ERR_INVALID.  A negative, non-finite or NaN value in power is the caller's business.
 *     F = 0 is valid and launches nothing.  Timed under RSL_K_DETECT. */
#define RSL_RULE_THRESHOLD 0
#define RSL_RULE_CA 1
#define RSL_RULE_OS 2
int rsl_detect_power(rsl_handle h, const void* power, int F, int S, int C, int rule, int guard_r, int guard_d,
                     int train_r, int train_d, double rank, double alpha, double thr_power, int i_lo, int i_hi,
                     void* mask, void* row_count, void* db_map, void* peak_pow);

/* a7 + a8 fused: range FFT, then Doppler FFT + fftshift + RDS store + peak detection in one kernel (the RDS is
 *     not re-read for detection).  Arguments as rsl_rds and rsl_detect; falls back to the two calls when the
 *     shape is not covered (C not a power of two <= 1024, or its range-bin tiling does not divide S/2).
 *     peak_pow is written group-compact: the peaks of the G rows r0 .. r0+G-1 of one (frame, antenna)
 *     (row = (f*A + a)*S + i, r0 a multiple of G) are contiguous from slot r0*C, in row order and Doppler order
 *     within a row (full cache lines instead of a short run per row).  *peak_pow_group (host, nullable)
 *     receives G (1 = row-compact, as rsl_detect writes it); pass it to rsl_peak_emit.
 *     work (c64-sized scratch, F A C S 8 bytes): at (S, C) = (256, 64), (512, 128) and (1024, 256) the range
 *     spectra travel packed (6 B per value, chirp-class tiles) in its first F A C S 6 bytes and the rest is not
 *     written; at other shapes it holds the c64 range spectra [F, A, C, S] as in rsl_rds.
 *     The range FFT's tile queue is per stream: the first call on a stream allocates 2 KiB of device memory
 *     (kept for the process) and zeroes it on that stream (likewise rsl_rds). */
int rsl_rds_detect(rsl_handle h, const void* cube, int F, int A, int C_total, int chirp0, int C, int S,
                   const void* table, int dc_removal, void* work, void* rds, double thr_power, int i_lo, int i_hi,
                   void* mask, void* row_count, void* db_map, void* peak_pow, int* peak_pow_group);

/* Offsets for the order-preserving compaction of a8's peak list (antenna -> range -> doppler,
 * dechirp.py:246-271) and of the deduplicated (range, doppler) cells that DoA runs on.
 *     entry_row_off i32 [F*A*S], cell_row_off i32 [F*S], scratch i32 [F*S],
 *     entry_base i64 [F+1], cell_base i64 [F+1] (global exclusive offsets; [F] = totals),
 *     frame_counts i64 [2F] (entries, cells per frame), union_mask u64 [F, S, W] (nullable) = OR over antennas. */
int rsl_peak_offsets(rsl_handle h, const void* mask, const void* row_count, int F, int A, int S, int C,
                     void* entry_row_off, void* cell_row_off, void* scratch, void* entry_base, void* cell_base,
                     void* frame_counts, void* union_mask);

/* Emit the peak entries and the unique cells (c_frame i32, c_rc i32 = range_bin*C + doppler_bin, c_amask u32 =
 * antennas with a peak there).  An entry is e_coord u32 = antenna << 26 | range_bin << 13 | doppler_bin (the
 * RSL_COORD_* macros; S, C <= 8192), e_cell i32 = its cell's list position, e_pdb f32 = power_db (nullable;
 * dechirp.py:235-236, computed in fp32 from the fp32 RDS).  Items beyond *_cap are dropped (compare the totals).
 * With union_mask (from rsl_peak_offsets) and peak_pow (from rsl_detect / rsl_rds_detect, in the row grouping
 * peak_pow_group those report; 1 for rsl_detect) the RDS is not read (rds may be NULL); otherwise power_db is
 * recomputed from rds. */
int rsl_peak_emit(rsl_handle h, const void* rds, const void* mask, const void* union_mask, const void* peak_pow,
                  int peak_pow_group, int F, int A, int S, int C, const void* entry_row_off, const void* cell_row_off, const void* entry_base,
                  const void* cell_base, long long entry_cap, long long cell_cap, void* e_coord, void* e_cell,
                  void* e_pdb, void* c_frame, void* c_rc, void* c_amask);
#define RSL_COORD_ANT(x) ((unsigned)(x) >> 26)
#define RSL_COORD_RANGE(x) (((unsigned)(x) >> 13) & 0x1fffu)
#define RSL_COORD_DOPPLER(x) ((unsigned)(x) & 0x1fffu)

/* Host helper: MFMA operand tables of a steering matrix.  steer_c128 is the host [G][M] complex128
 * matrix of AngleEstimator.generate_steering_vector (angle_estimation.py:92-107) over the azimuth grid
 * (angle_estimation.py:59-60).  rsl_steer_table_floats returns the float count of the table; the build
 * writes (1) the f32 [Re; Im] operand for v_mfma_f32_16x16x4_f32 (*ntiles = its 16-row tiles),
 * (2) the Toeplitz-form f16 hi/lo operand for v_mfma_f32_32x32x16_f16, valid when the steering matrix is a
 * uniform linear array (*flags |= RSL_STEER_TOEPLITZ), and (3) the fp64 matrix itself transposed, [M][G] complex128
 * (the last 4 G M floats), which the exact fp64 re-scan of near-tie cells reads. */
long long rsl_steer_table_floats(int G, int M);
int rsl_steer_table_build(const double* steer_c128, int G, int M, float* host_out, int* ntiles, int* flags);

/* a11-a16  extract_spatial_signature + music_spectrum / estimate_angle_music / estimate_angle_beamforming
 *     (angle_estimation.py:67-176, 227-251; robust_angle_estimation.py:236-245).
 *     Cells (c_frame, c_rc) index rds c64 [*, A, S, C]; n = min(*ncell_dev, ncell) if ncell_dev is non-null
 *     (ncell = the lists' capacity: an overflowed list is processed up to its capacity), else ncell.
 *     steer_tab = device copy of the rsl_steer_table_build output (its fp64 section feeds the exact fp64 re-scan of
 *     the cells whose top-2 gap in the f16 hi/lo or f32 scan is inside that scan's error bound, and of MUSIC's
 *     near-degenerate cells, so out_idx is the fp64 argmax of each cell's own signature; keys within 1e-13 relative
 *     count as ties and the lower index wins, as np.argmax.  The scans' bounds are relative to the cell's best value,
 *     so this exactness is established statistically, not by a worst-case bound); steer_c128 (device fp64 [G][M][2], nullable) is no
 *     longer read by rsl_doa / rsl_doa_extras and is kept for ABI compatibility.
 *     method = RSL_METHOD_* | RSL_DOA_TOEPLITZ (optional; with out_spec it applies to the RSL_DOA_SPEC_BLOCKED layout
 *     without out_gmax, the other spectrum requests take the f32 scan).
 *     out_idx i32 [n] = first-index argmax over the G grid points; out_gmax f32 [n] (nullable) = |a^H s|^2
 *     at the argmax (unit-norm s); out_spec f32 [n, G] (nullable; [G][ncell] with RSL_DOA_SPEC_GMAJOR,
 *     [ceil(ncell / 32)][G][32] with RSL_DOA_SPEC_BLOCKED) = MUSIC
 *     1/(M-|a^H s|^2) with the reference's den > 1e-12 rule, or the beamforming |a^H s|^2. */
int rsl_doa(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
            const void* ncell_dev, long long ncell, const void* steer_tab, const void* steer_c128, int G, int method,
            void* out_idx, void* out_gmax, void* out_spec);

/* a11-a16 + a15 + a26 fused: the Toeplitz argmax of rsl_doa (requires RSL_STEER_TOEPLITZ) plus, from the same
 *     signature load, ESPRIT (f64 deg, nullable; angle_estimation.py:178-225, esprit_scale = lambda/(2 pi d))
 *     and the spatial phase angle(s1 conj(s0)) (f64, nullable; velocity_solver.py:136) of each cell.
 *     Returns RSL_ERR_UNSUPPORTED when the grid does not fit the Toeplitz path. */
int rsl_doa_extras(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                   const void* ncell_dev, long long ncell, const void* steer_tab, const void* steer_c128, int G,
                   int method, double esprit_scale, void* out_idx, void* out_gmax, void* esprit_deg, void* phase);

/* Spatially smoothed MUSIC: several directions of arrival per cell from one snapshot of a uniform linear array
 *     (rsl_ssmusic.hip; the reference project has no counterpart, this comment is the specification).
 *     Cells and n as rsl_doa (n = min(*ncell_dev, ncell); n = 0 launches nothing; slots beyond n are not written).
 *     M = A antennas, 3 <= M <= 16; sub-array length L, 2 <= L <= min(M, RSL_SS_MAX_L); K = M - L + 1;
 *     output width nmax, 1 <= nmax <= L - 1; 0 <= num_sources <= nmax (0: estimate the order); rel in (0, 1).
 *     Per cell:
 *     1. x = rds[f, :, r, c].  If sum |x|^2 = 0 the cell is empty: nsrc = 0, every pick -1 / NaN, the eig and spec
 *        rows NaN.  Otherwise s = x / ||x||.
 *     2. R_f[p][q] = (1/K) sum_{k<K} s[k+p] conj(s[k+q]);  R[p][q] = (R_f[p][q] + conj(R_f[L-1-p][L-1-q])) / 2
 *        (forward-backward smoothing; Hermitian and persymmetric L x L; its trace is the mean power of the K
 *        sub-arrays, 1 for L = M).
 *     3. Eigenvalues l_1 >= ... >= l_L, orthonormal eigenvectors v_i, by cyclic complex Jacobi in fp32: at most
 *        RSL_SS_MAX_SWEEPS sweeps (round-robin order); a cell stops rotating once its off-diagonal Frobenius norm
 *        is <= RSL_SS_OFF_TOL ||R||_F at the start of a sweep.
 *     4. k = num_sources if > 0, else the number of i with l_i >= rel l_1, clamped to [1, nmax].
 *     5. den[g] = sum_{i>k} |v_i^H a_g|^2 with a_g = steer_sub_c64[g] (device c64 [G][L]: a_g[l] = exp(j l psi_g),
 *        psi_g = 2 pi d sin(theta_g) / lambda, the first L columns of the array's steering matrix, built by the host
 *        in fp64).  den in [0, L]; the MUSIC pseudo-spectrum is 1 / den.
 *     6. g is a local minimum if den[g] < den[g-1] and den[g] <= den[g+1] (g = 0: den[0] < den[1]; g = G-1:
 *        den[G-1] < den[G-2]).  The picks are the k local minima of smallest den, ties to the lower index, listed in
 *        ascending den; with fewer than k minima the remaining slots are -1 / NaN.
 *     out_nsrc i32 [n] = k; out_idx i32 [n][nmax] = the picks; out_den f32 [n][nmax] (nullable) = den at each pick;
 *     out_eig f32 [n][L] (nullable) = the eigenvalues, descending; out_spec f32 [n][G] (nullable) = the den row.
 *     RSL_ERR_INVALID: M, L, nmax, num_sources or rel out of range (or rel NaN), G < 3, null rds, lists,
 *     steer_sub_c64, out_nsrc or out_idx.  Timed under RSL_K_DOA_SCAN. */
#define RSL_SS_MAX_L 8
#define RSL_SS_MAX_SWEEPS 12
#define RSL_SS_OFF_TOL 1e-8f
int rsl_doa_smoothed(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                     const void* ncell_dev, long long ncell, const void* steer_sub_c64, int G, int L, int nmax,
                     int num_sources, double rel, void* out_nsrc, void* out_idx, void* out_den, void* out_eig,
                     void* out_spec);

/* Range-azimuth maps: the multi-snapshot spatial covariance of every range bin and the Bartlett / Capon (MVDR) power
 *     over an azimuth grid computed from it (rsl_ramap.hip; the reference project has no counterpart, this comment is
 *     the specification).  The Doppler bins of one range row are the snapshots: reflectors that share a range bin but
 *     differ in radial velocity are incoherent across them, so Capon separates them below the beamwidth with the full
 *     aperture.  Both functions are timed under RSL_K_DOA_SCAN.
 *
 *     rsl_range_cov: rds c64 [F, A, S, C], 2 <= A <= RSL_RA_MAX_A, Doppler window 0 <= c0 < c1 <= C, Cw = c1 - c0.
 *       cov[f, r, p, q] = (1/Cw) sum_{c0 <= c < c1} rds[f, p, r, c] conj(rds[f, q, r, c]),  cov c64 [F, S, A, A],
 *     accumulated in fp32 on the matrix pipe (a k-ordered fmaf chain of the real Gram matrix of [Re X; Im X], then one
 *     add or subtract and one multiply by (float)(1/Cw): |cov - exact| <= 2 (Cw + 4) 2^-24 sqrt(cov_pp cov_qq)).
 *     The result is exactly Hermitian: cov[q][p] is the bitwise conjugate of cov[p][q] and the diagonal's imaginary
 *     part is exactly 0.  Row (f, r) depends on its own inputs only: a batch equals its frames run alone, bit for bit.
 *     F = 0 launches nothing.  RSL_ERR_INVALID: A, c0 or c1 out of range, S or C <= 0, null pointers with F > 0.
 *
 *     rsl_range_azimuth: cov c64 [n, A, A], Hermitian positive semi-definite; its upper triangle and the diagonal's
 *     real part define it (the rest is not read).  steer_c64 device c64 [G][A]: any array's steering matrix rounded
 *     to c64 (unit-modulus entries; it need not be uniform linear), G >= 1.  map f32 [n, G]; arg i32 [n] (nullable) =
 *     the first-index argmax of the row.  With t = Re tr(cov_i): if t <= 0 the row is all 0 and arg is 0; otherwise
 *       RSL_RA_BARTLETT  map[g] = Re(a_g^H R a_g) / A^2
 *       RSL_RA_CAPON     map[g] = 1 / Re(a_g^H R_l^-1 a_g),  R_l = R + loading (t / A) I
 *     (fp32; R_l^-1 from a Cholesky factorisation, its triangular inverse T and T^H T).  Both return the source power
 *     + noise / A for a single source in white noise, so their values are directly comparable.  loading lies in
 *     [RSL_RA_MIN_LOADING, 1] and is read by Capon only: cond(R_l) <= A / loading + 1, and below 1e-4 an fp32
 *     factorisation has no digits left.  A cov that is not positive semi-definite is the caller's business (Capon's
 *     factorisation may then give a NaN row, whose arg is 0).
 *     n = 0 launches nothing.  RSL_ERR_INVALID: a bad method, A outside [2, RSL_RA_MAX_A], G < 1, loading out of
 *     range or NaN, n < 0, null cov / steer_c64 / map with n > 0. */
#define RSL_RA_BARTLETT 0
#define RSL_RA_CAPON 1
#define RSL_RA_MAX_A 16
#define RSL_RA_MIN_LOADING 1e-4
int rsl_range_cov(rsl_handle h, const void* rds, int F, int A, int S, int C, int c0, int c1, void* cov);
int rsl_range_azimuth(rsl_handle h, const void* cov, long long n, int A, const void* steer_c64, int G,
                      int method, double loading, void* map, void* arg);

/* a11, a15, a26  normalised signature (c64 [n, A], nullable), ESPRIT closed form (f64 deg, nullable;
 *     angle_estimation.py:178-225 with esprit_scale = lambda / (2 pi d)), spatial phase
 *     angle(s1 conj(s0)) (f64, nullable; velocity_solver.py:136; exactly 0.0 where s0 or s1 is 0), az_out =
 *     az_table[gidx] (f64, nullable).  2 <= A <= 32 (RSL_ERR_INVALID otherwise: the phase needs two antennas). */
int rsl_cell_extras(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                    const void* ncell_dev, long long ncell, double esprit_scale, const void* gidx,
                    const void* az_table, void* sig_out, void* esprit_deg, void* phase, void* az_out);

/* The point cloud: what rsl_cell_refine writes and rsl_scan_register and rsl_map_update read (device side:
 *     rsl_cloud.h).  points f32 [n][RSL_POINT_COLS]: 32-byte rows, the columns in the order of the ids below.
 *     seg i64 [F + 1] (cell_base): frame f owns the rows [clamp(seg[f], 0, n), clamp(seg[f + 1], 0, n)), none when the
 *     segment descends; n is the number of rows in use.  weight f32 [n] (nullable = 1).  A point counts with its
 *     weight when x and y are finite and the weight is > 0, and with 0 otherwise (a NaN weight is not > 0). */
#define RSL_POINT_COLS 8
#define RSL_POINT_RANGE 0
#define RSL_POINT_DOPPLER 1
#define RSL_POINT_AZ 2
#define RSL_POINT_X 3
#define RSL_POINT_Y 4
#define RSL_POINT_POWER_DB 5
#define RSL_POINT_RANGE_OFFSET 6
#define RSL_POINT_DOPPLER_OFFSET 7

/* Point cloud: sub-bin range, Doppler and azimuth and the position of every detected cell (rsl_refine.hip; the
 *     reference project has no counterpart, this comment is the specification).  Cells and n as in rsl_doa:
 *     n = min(*ncell_dev, ncell); slots beyond n are not written; ncell = 0 launches nothing.  rds c64 [*, A, S, C],
 *     2 <= A <= 32; power f32 [*, S, C] (nullable), the map of rsl_power_integrate; gidx i32 [n], the scan's argmax;
 *     az_table f64 [G] radians, strictly increasing inside [-pi/2, pi/2]; steer_c64 device c64 [G][A], any array's
 *     steering matrix rounded to c64; axes4 (host) = {r0, r_step, d0, d_step}.
 *     1. Five powers of cell (f, i, j): P0 = P[f,i,j], Pr+- = P[f,i+-1,j], Pd+- = P[f,i,(j+-1) mod C] (the Doppler axis
 *        wraps, the range axis truncates, as in the CFAR family).  Read from power when given; otherwise each is
 *        formed from rds as rsl_power_integrate defines it (fmaf(re, re, im im) per antenna, added in antenna order
 *        in fp32), so both ways are bit-identical.
 *     2. Offsets dr, dd in [-0.5, 0.5], one estimator per axis, in fp64 from the axis' fp32 powers (pm, p0, pp); every
 *        comparison is on the fp32 values:
 *          RSL_REFINE_NONE  0
 *          RSL_REFINE_LOG   0 if any of the three is <= 0; else with den = ln pm - 2 ln p0 + ln pp: 0 if den >= 0,
 *                           else clamp(0.5 (ln pm - ln pp) / den, -0.5, 0.5)    (log-parabola: Hamming, Blackman)
 *          RSL_REFINE_RECT  0 if p0 <= 0 or pm == pp; else q = max(pm, pp), r = sqrt(q / p0), s = +1 if pp > pm
 *                           else -1: s min(0.5, r / (1 + r))                    (amplitude ratio, no window)
 *          RSL_REFINE_HANN  as RECT with s clamp((2 r - 1) / (r + 1), 0, 0.5)   (amplitude ratio, Hann window)
 *        At i = 0 and i = S - 1, dr = 0.
 *     3. Azimuth, g = gidx[c].  g outside [0, G): az, x and y are NaN, the rest is written as usual.  Otherwise
 *        B_k = |a_k^H z|^2 for k = g-1, g, g+1 in fp64 (z the cell's fp32 signature, a_k the row of steer_c64, both
 *        promoted; z is not normalised, the vertex is scale-free), u_k = sin(az_table[k]),
 *        d01 = (B_g - B_{g-1}) / (u_g - u_{g-1}), d12 likewise, c = (d12 - d01) / (u_{g+1} - u_{g-1}).  If g is 0 or
 *        G - 1, or c >= 0, or c is not finite: az = az_table[g].  Otherwise u* = (u_{g-1} + u_g) / 2 - d01 / (2 c)
 *        clamped to [(u_{g-1} + u_g) / 2, (u_g + u_{g+1}) / 2] and az = asin(u*).  MUSIC's rank-1 spectrum
 *        1 / (M - B) has the same argmax, so the rule serves both methods.
 *     4. out_az f64 [n] (nullable) = az.  out_points (nullable; 16-byte aligned): the rows of the point cloud above,
 *        each value computed in fp64 and rounded once: range = r0 + r_step (i + dr), doppler = d0 + d_step (j + dd)
 *        (the product and the sum each rounded, not fused: a label that cancels to nearly 0 is the same everywhere),
 *        az, x = range cos az, y = range sin az, power_db = 10 log10(P0 + 1e-12), range_offset = dr,
 *        doppler_offset = dd.
 *        No wrap is applied to the Doppler label: bin C - 1 with dd > 0 reads slightly past the axis end.
 *     RSL_ERR_INVALID: A outside [2, 32]; S, C or G <= 0; an unknown mode; a step that is not finite; both outputs
 *     null; out_points not 16-byte aligned; null rds, lists, gidx, az_table, steer_c64 or axes4 with ncell > 0.
 *     Timed under RSL_K_CELL_EXTRAS. */
#define RSL_REFINE_NONE 0
#define RSL_REFINE_LOG 1
#define RSL_REFINE_RECT 2
#define RSL_REFINE_HANN 3
int rsl_cell_refine(rsl_handle h, const void* rds, const void* power, int A, int S, int C, const void* c_frame,
                    const void* c_rc, const void* ncell_dev, long long ncell, const void* gidx, const void* az_table,
                    const void* steer_c64, int G, int range_mode, int doppler_mode, const double* axes4,
                    void* out_points, void* out_az);

/* a13-a15 with num_sources != 1  music_spectrum / estimate_angle_music / estimate_angle_esprit
 *     (angle_estimation.py:109-225) for any num_sources (Python slicing semantics for K <= 0 and K >= M), fp64:
 *     sigs c128 [n][M] (device, the signatures as given; MUSIC normalises them), steer_c128 f64 [G][M][2]
 *     (device), spec f64 [n][G] = 1/den or 0 (den <= 1e-12), deg f64 [n] (0.0 where the reference's ESPRIT
 *     raises, NaN where it returns NaN).  The reference's noise / null-space bases for 2 <= K < M come from LAPACK
 *     round-off; these use a fixed Householder completion (rsl_subspace.hip), so only K = 1, K >= M (MUSIC),
 *     K <= 0 (ESPRIT) and zero signatures are reference-determined.
 *     rsl_esprit_subspace by kk = the column count of U[:, :num_sources] (U is (M-1) x (M-1)): kk = 0 or M <= 2: 0.0
 *     (empty Phi); kk = 1: the closed form; kk = 2: one of the reference's two eigenvalues; kk = M - 1: 0.0 (Phi is
 *     nilpotent, every eigenvalue is 0, and the reference's value there is round-off); 3 <= kk < M - 1: Phi on the
 *     span [s[:-1], s[1:], e_0 .. e_{kk-3}] has two non-zero eigenvalues and a zero one of multiplicity kk - 2; the
 *     value is the first diagonal entry of Phi's Schur form among the two of largest modulus (the first entry as it
 *     is would be a numerically zero eigenvalue, whose argument is round-off, on about 1 % of random signatures and
 *     up to 2 % at kk = M - 2). */
int rsl_music_subspace(rsl_handle h, const void* sigs, long long n, int M, int num_sources, const void* steer_c128,
                       int G, void* spec);
int rsl_esprit_subspace(rsl_handle h, const void* sigs, long long n, int M, int num_sources, double esprit_scale,
                        void* deg);

/* a19  RobustAngleEstimator.compute_angle_confidence (robust_angle_estimation.py:88-138) for n
 *     (cell, grid index) pairs.  steer_c128 f64 [G][M][2] and steer_phase f64 [G][M] = np.angle(a) are
 *     device copies of the host fp64 tables.  conf f64 [n]. */
int rsl_confidence(rsl_handle h, const void* rds, int A, int S, int C, const void* c_frame, const void* c_rc,
                   long long n, const void* gidx, const void* steer_c128, const void* steer_phase, void* conf);

/* a25-a29  VelocitySolver.two_step_optimization / solve_velocity (velocity_solver.py:65-355): exact
 *     box-constrained LS for (v_x, v_y) per segment (segments = frames).  az f64 [N] radians, or (when gidx
 *     i32 [N] is non-null) az = az_table[gidx] with az_table f64 [G], G <= 2048; y f64 [N]
 *     observed phase, amask u32 [N] (nullable; multiplicity = popcount), seg i64 [F+1] (device; bounds
 *     clamped to n = N, the arrays' length: a capacity-sized list that overflowed ends at its capacity),
 *     k = 4 pi dt / lambda, ridge >= 0, bounds4 (host) = {vx_lo, vx_hi, vy_lo, vy_hi};
 *     out f64 [F, 8] = {vx, vy, cost, rmse, max_residual, n, det, 0}; resid/pred f64 [N] nullable.
 *     F = 0 launches nothing.  RSL_ERR_INVALID: F < 0 or n < 0; ridge < 0 or NaN (also at F = 0); gidx with G <= 0,
 *     G > 2048 or without az_table; az and gidx both null; null y, seg, out or bounds4; a box with lo > hi or a NaN.
 *     Timed under RSL_K_VELOCITY. */
int rsl_velocity(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G, const void* y,
                 const void* amask, const void* seg, long long n, int F, double k, double ridge, const double* bounds4,
                 void* out, void* resid, void* pred);

/* Robust ego-velocity solve: Huber / Tukey iteratively re-weighted least squares (k_velocity_robust), an explicitly
 *     selected alternative to rsl_velocity with the same model and inputs (az / gidx + az_table, y, amask, seg, n, k,
 *     ridge, bounds4 as above).  Per frame, cell i has the direction (c_i, s_i) = (cos az_i, sin az_i), the
 *     observation y_i, the multiplicity m_i = popcount(amask[i]) (1 when amask is null) and the residual
 *     r_i(x) = y_i - k (x_0 c_i + x_1 s_i).
 *     Losses, cut-off t = c sigma, both scaled so that rho(r) = r^2 for small r (costs compare with rsl_velocity's):
 *       RSL_LOSS_HUBER  rho = r^2 if |r| <= t, else 2 t |r| - t^2;           u = 1 if |r| <= t, else t / |r|
 *       RSL_LOSS_TUKEY  rho = (t^2/3)(1 - (1 - (r/t)^2)^3) if |r| < t, else t^2/3;  u = (1 - (r/t)^2)^2 if |r| < t, else 0
 *     (t = 0: u = 1 where r = 0, else 0, and such cells count as inliers, for both losses).  The Python layers
 *     default c to 1.345 (Huber) and 4.685 (Tukey).
 *     Iteration: x^0 is exactly rsl_velocity's solution of the frame (same moments, ridge, box, and rule: the
 *     interior solution if feasible, else the best edge).  For j = 1 .. iters: residuals at x^(j-1); sigma = scale
 *     when scale > 0, else (scale <= 0) 1.4826 x the lower weighted median of (float)|r_i|, i.e. the smallest value a
 *     such that the multiplicities of the cells with (float)|r_i| <= a sum to at least half the total (cells with
 *     m_i = 0 do not count; the fp32 rounding is part of the definition, which makes the device's integer radix
 *     select exact and order-independent); weights u_i; x^j = the box-constrained ridge LS with weights m_i u_i, by
 *     the same 2x2 rule.  Stop after iteration j when max|x^j - x^(j-1)| <= tol (tol = 0: run exactly iters
 *     iterations).  Also stop, keeping x and counting as converged, when sigma = 0, when sum m_i u_i = 0, or when the
 *     segment is empty (or holds no multiplicity).
 *     A given scale (the sensor's phase-noise sigma) with RSL_LOSS_TUKEY is the dependable configuration: it
 *     recovered the inlier motion up to 45 % coherent outliers in the prototype.  The estimated scale starts from the
 *     LS fit and breaks down beyond roughly 30 % coherent outliers.
 *     out f64 [F, 8] = {v_x, v_y, cost, rmse_w, n_in, n, sigma, it}: cost = sum m_i rho(r_i) + ridge |v|^2;
 *     rmse_w = sqrt(sum m_i u_i r_i^2 / sum m_i u_i) (0 when the denominator is 0); n_in = sum of m_i over the cells
 *     with |r_i| <= t (Huber) or |r_i| < t (Tukey); n = sum m_i; sigma = the last sigma used; it = the number of
 *     iterations run, negated when the stop rule was not met (never for tol = 0).  weight f32 [N] (nullable): u_i at
 *     the returned x with the sigma of the last iteration; resid f64 [N] (nullable).  All at the returned x.
 *     F = 0 launches nothing.  RSL_ERR_INVALID: loss not 1 or 2; c <= 0 or not finite; scale NaN or +inf; iters < 1
 *     or > 1000; tol < 0 or NaN; ridge < 0; gidx with G > 2048 or without az_table; az and gidx both null; null y,
 *     seg, out or bounds4.  Timed under RSL_K_VELOCITY. */
#define RSL_LOSS_HUBER 1
#define RSL_LOSS_TUKEY 2
int rsl_velocity_robust(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G,
                        const void* y, const void* amask, const void* seg, long long n, int F, double k,
                        double ridge, const double* bounds4, int loss, double c, double scale, int iters,
                        double tol, void* out, void* weight, void* resid);

/* Consensus (RANSAC) ego-velocity solve (k_velocity_consensus): for frames where the static world is not the majority
 *     of the cells.  Both solvers above start from the LS fit and need that majority; this one proposes two-cell
 *     hypotheses, keeps the one the most cells agree with and refits on those cells, so it finds the largest coherent
 *     population even where that is a minority.  Model and inputs are exactly those of rsl_velocity_robust (az / gidx +
 *     az_table, y, amask, seg clamped to n, k, ridge, bounds4).  Per frame f with the cells b .. e, n_f = e - b: the
 *     directions (c_i, s_i), the multiplicity m_i = popcount(amask[i]) (1 when amask is null), the residual
 *     r_i(x) = y_i - k (x_0 c_i + x_1 s_i), the cut-off t = c scale.  scale > 0 is required: it is the sensor's
 *     phase-noise sigma (radians).  The Python layers default c to 3.0.
 *     Hypotheses h = 0 .. hyps - 1: (x0, x1, ., .) = Philox-4x32-10 with the counter (h, low32(frame0 + f),
 *     high32(frame0 + f), 0) and the key (low32(seed), high32(seed)) (the generator of rsl_synth_cube);
 *     i = (x0 n_f) >> 32; j = (x1 (n_f - 1)) >> 32, then j += (j >= i): two distinct local indices into the segment.
 *     det = c_i s_j - c_j s_i; v_x = (y_i s_j - y_j s_i) / (k det); v_y = (c_i y_j - c_j y_i) / (k det).  The
 *     hypothesis is valid iff n_f >= 2, m_i > 0 and m_j > 0, |det| >= min_det (the least |sin| of the pair's azimuth
 *     difference; the Python default 0.1 lies between 5.5 and 6 degrees, so no pair of the 0.5 degree grid sits on it)
 *     and (v_x, v_y) lies inside the box, edges included.
 *     Score: score(h) = sum of m_i over the cells with |r_i(x_h)| <= t, an exact integer.  The winner is the valid
 *     hypothesis with the largest score, ties going to the lowest h.  If no hypothesis is valid, the start is
 *     rsl_velocity's solution of the frame (same moments, ridge, box and rule) and best_h = -1.  An empty frame, or one with sum m_i = 0, has no valid
 *     hypothesis and keeps that LS start untouched, as rsl_velocity_robust does.
 *     Refinement, repeated `refine` times: w_i = m_i where |r_i(x)| <= t, else 0; if sum w_i = 0, stop and keep x;
 *     otherwise x = the box-constrained ridge LS with the weights w_i, by the 2x2 rule of the other two solvers (the
 *     interior solution if feasible, else the best edge).
 *     out f64 [F, 8] = {v_x, v_y, cost, rmse_in, n_in, n, best_h, n_valid}, all at the returned x:
 *     cost = sum m_i min(r_i^2, t^2) + ridge |v|^2; n_in = sum of m_i over the cells with |r_i| <= t (the inliers);
 *     rmse_in = sqrt(sum over the inliers of m_i r_i^2 / n_in) (0 when n_in = 0); n = sum m_i; best_h = the winning
 *     hypothesis or -1; n_valid = the number of valid hypotheses.  weight f32 [N] (nullable): 1 where |r_i| <= t, else
 *     0: the inlier mask, i.e. the static / moving labelling of the cells.  resid f64 [N] (nullable).
 *     Rows [a, b) of a batch equal a launch of those frames alone with frame0 = a: the draws depend on
 *     (seed, frame0 + f, h) only.
 *     F = 0 launches nothing.  RSL_ERR_INVALID: c <= 0 or not finite; scale <= 0 or not finite; hyps outside
 *     1 .. RSL_CONSENSUS_MAX_H; min_det outside (0, 1]; refine outside 0 .. 100; frame0 < 0; ridge < 0; gidx with
 *     G > 2048 or without az_table; az and gidx both null; null y, seg, out or bounds4.  Timed under RSL_K_VELOCITY. */
#define RSL_CONSENSUS_MAX_H 4096
int rsl_velocity_consensus(rsl_handle h, const void* az, const void* gidx, const void* az_table, int G,
                           const void* y, const void* amask, const void* seg, long long n, int F, double k,
                           double ridge, const double* bounds4, double c, double scale, int hyps, double min_det,
                           int refine, unsigned long long seed, long long frame0,
                           void* out, void* weight, void* resid);

/* Scan registration: the yaw increment and the displacement between the point clouds of consecutive frames
 *     (rsl_register.hip, k_scan_register; the reference project has no counterpart, this comment is the
 *     specification).  The Doppler solve of one radar observes only (v_x, v_y); this supplies the rotation.
 *     Inputs (device unless marked host): points, seg, n and weight: the point cloud above, of which x, y and the
 *     weight each point counts with are read; rc i32 [n] (nullable) with C and axes4 (host) = {r0, r_step, ., .} as in
 *     rsl_cell_refine, used for culling only (below);
 *     prev_points / prev_weight / prev_rc (nullable): the cloud frame 0 is registered against, its length
 *     min(prev_n, *prev_n_dev) (prev_n_dev i64 [1], nullable); init f64 [F][3] (nullable = zeros), the start
 *     (theta, t_x, t_y) of every frame, a component that is not finite counting as 0.
 *     Frame pairs: frame f >= 1 is the current cloud P (p_i, w_i), frame f - 1 the reference cloud Q (q_j, u_j);
 *     frame 0 uses prev_*, and without prev_points gets the row {0, 0, 0, 0, 0, 0, 0, 2}.
 *     Unknown: T = (theta, t), p' = R(theta) p + t, which maps current sensor coordinates into the previous frame's:
 *     theta is the yaw increment, t the displacement expressed in the previous body frame.
 *     Kernel: a_ij(T, h) = max(0, 1 - |R(theta) p_i + t - q_j|^2 (1 / h^2)), the biweight kernel: support of radius h,
 *     continuous at the cut-off, no transcendental.
 *     Coarse stage (yaw only, the translation trusted to the start t0): theta_k = theta0 + k dtheta, |k| <= K,
 *     S_k = sum_ij w_i u_j a_ij((theta_k, t0), h_coarse)^3; the first maximum wins and theta starts there.  If every
 *     S_k is 0 (an empty cloud among them): the row is {theta0, t0_x, t0_y, 0, 0, 0, 0, 1}, no fine stage.
 *     Fine stage, steps it = 0 .. iters - 1 (MM / IRLS): h_it = max(h, h_coarse shrink^it), the power formed by
 *     repeated multiplication; g_ij = w_i u_j a_ij(T, h_it)^2; W = sum g, S_p = sum g p_i, S_q = sum g q_j,
 *     D = sum g (p_i . q_j), X = sum g (p_ix q_jy - p_iy q_jx), E = sum g d_ij^2 (d the residual at T).  If
 *     W <= w_min (or NaN): flag 1, T kept, stop.  Otherwise D_c = D - (S_p . S_q) / W, X_c = X - (S_p x S_q) / W,
 *     theta <- atan2(X_c, D_c), t <- S_q / W - R(theta) S_p / W; stop once h_it == h and the largest change of the
 *     three components is below tol.  This is the weighted 2-D Procrustes solution under Tukey's biweight loss summed
 *     over all pairs; the loss is concave in d^2, so at a fixed h no step decreases sum w u a^3.
 *     All sums are fp64 (per thread in a fixed order, then rsl_reduce.h), the pair arithmetic fp64 from the fp32
 *     coordinates: the centred moments cancel many digits at 100 m.  No atomics: rows are run-to-run bit-identical.
 *     out f64 [F][8] = {theta, t_x, t_y, W, rms = sqrt(E / W), S_best / sum_k S_k, updates applied, flag}; W and E are
 *     those of the last step evaluated, i.e. at the T before the last update (0 when iters = 0; rms 0 when W = 0).
 *     omega f64 [F][3] (nullable): frame f's theta goes as {0, 0, theta_f / dt} into row f - 1 (rsl_traj_scan's
 *     convention R_i = R_{i-1} exp(omega_{i-1} dt)), for every flag; row F - 1 is 0.
 *     Culling is implementation, not result: with rc, the partners of a transformed point at range rho' are searched
 *     in the range rows i whose label interval r0 + r_step (i -+ 0.5) meets [rho' - h_it, rho' + h_it], one more row on
 *     each side for the fp32 rounding of the labels (coarse stage: all rho' the candidates can give), found by binary
 *     search on rc inside the reference's segment (rc ascends inside a frame).  Without rc every pair is tested.
 *     One workgroup per frame pair, the whole loop inside the kernel: a call with F = 2 uses one CU.
 *     RSL_ERR_INVALID: h, h_coarse, dtheta, dt or w_min not finite, or h, h_coarse, dtheta, dt <= 0, or w_min < 0;
 *     tol NaN; h_coarse < h; K outside 0 .. RSL_REG_MAX_K; iters outside 0 .. RSL_REG_MAX_ITERS; shrink outside (0, 1];
 *     F, n or prev_n < 0; null points, seg or out with F > 0; rc or prev_rc given with null axes4, C <= 0, or an
 *     r_step that is not finite and > 0.  F = 0 launches nothing.  Timed under RSL_K_AUX. */
#define RSL_REG_MAX_K 64
#define RSL_REG_MAX_ITERS 100
int rsl_scan_register(rsl_handle h, const void* points, const void* seg, int F, long long n, const void* weight,
                      const void* rc, int C, const double* axes4, const void* prev_points, const void* prev_weight,
                      const void* prev_rc, long long prev_n, const void* prev_n_dev, const void* init, double h_fine,
                      double h_coarse, double dtheta, int K, int iters, double shrink, double tol, double w_min,
                      double dt, void* out, void* omega);

/* Grid map: per-scan hit and free-space counts in world coordinates from the frames' point clouds and poses
 *     (rsl_map.hip, k_map_update; the reference project has no counterpart, this comment is the specification).
 *     The map is two planes of unsigned integer counts, and every frame (scan) adds at most 1 to a cell's hit count or
 *     to its free count: the classical per-scan binary update.  Several points in one cell, and the mostly-noise cells
 *     of the threshold detector, do not multiply the evidence.  Integer adds commute, so the planes are bit-identical
 *     from run to run and independent of the frame order and of how the frames are split over launches or ranks, and
 *     rank maps merge by integer addition.  Clamped log-odds are derived from the counts at the end (rsl_map_logodds),
 *     not clamped per update: a per-update clamp would make the map depend on the order of the frames.
 *     Inputs (device unless marked host): points, seg, n and weight: the point cloud above, of which x, y, power_db
 *     and the weight are read; poses f64 [F][7] = (p_x, p_y, p_z, q_w, q_x, q_y, q_z), the rows of the trajectory
 *     reduction: the sensor frame is the body frame (no mounting offset); grid4 (host) = {x0, y0, cell, unused}: the
 *     world position of the corner of cell (0, 0) and the cell size; hits, free_ u32 [ny][nx], both in / out: the call
 *     adds to them and never clears them; free_ nullable: no ray is cast; stats i32 [F][4] (nullable).
 *     Arithmetic: all fp64, every product and sum rounded once in the order written, no fused multiply-add.
 *     inv = 1 / cell (one division, on the host), Rw = (int)ceil(r_max inv) + 1.
 *     Per frame: r00 = 1 - 2 (q_y q_y + q_z q_z), r01 = 2 (q_x q_y - q_w q_z), r10 = 2 (q_x q_y + q_w q_z),
 *     r11 = 1 - 2 (q_x q_x + q_z q_z): the quaternion as given, not normalised; only the planar 2 x 2 block is used and
 *     p_z is ignored.  Origin cell: ox = floor((p_x - x0) inv), oy likewise.  If any of p_x, p_y, r00, r01, r10, r11 is
 *     not finite, or |(p - x0) inv| >= 2^30 in x or y, the frame counts nothing and its stats row is {0, 0, 0, 1}.
 *     Per point, x and y promoted to fp64, accepted iff (1), (2) it counts in the point cloud above (x and y finite,
 *     the weight null or > 0); (3) not (power_db < min_db), so -inf disables the floor; (4) r_min^2 <= x x + y y <=
 *     r_max^2, both squares formed as products on the host; then X = (r00 x + r01 y) + p_x, Y = (r10 x + r11 y) + p_y,
 *     hx = floor((X - x0) inv), hy likewise, and (5) 0 <= hx < nx and 0 <= hy < ny, compared as doubles before any
 *     conversion; (6) |hx - ox| <= Rw and |hy - oy| <= Rw.  H_f is the set of the accepted points' cells.
 *     Free set (only with free_): for every cell (hx, hy) of H_f, dx = |hx - ox|, dy = |hy - oy|, sx = +1 if hx >= ox
 *     else -1, sy likewise, L = max(dx, dy), and for k = 0 .. L - 1 the cell
 *         (ox + sx k, oy + sy ((2 k dy + dx) div (2 dx)))   if dx >= dy,
 *         (ox + sx ((2 k dx + dy) div (2 dy)), oy + sy k)   otherwise:
 *     the closed form of the integer line from the origin cell up to, not including, the hit cell (L distinct,
 *     8-connected cells; the next step would be the hit cell).  Ray cells outside the map are dropped one by one (the
 *     sensor stands outside the map).  Free_f = (the union of the rays' cells) \ H_f: a cell hit in this scan is not
 *     free in this scan.
 *     Update: hits[c] += 1 for c in H_f, free_[c] += 1 for c in Free_f; stats row = {accepted points, |H_f|, |Free_f|,
 *     flag}.  One workgroup per frame with two bitmaps of the (2 Rw + 1)^2 window in LDS: Rw <= RSL_MAP_MAX_RW, two
 *     bitmaps of 767^2 bits = 147,080 B of the CU's 160 KiB.
 *     RSL_ERR_UNSUPPORTED: Rw > RSL_MAP_MAX_RW.  RSL_ERR_INVALID: cell, r_max, x0 or y0 not finite; cell <= 0;
 *     r_min < 0 or NaN; r_max < r_min; min_db NaN or +inf; nx, ny <= 0 or nx ny >= 2^31; F or n < 0; null points, seg,
 *     poses, grid4 or hits with F > 0.  F = 0 launches nothing.  Timed under RSL_K_AUX. */
#define RSL_MAP_MAX_RW 383
int rsl_map_update(rsl_handle h, const void* points, const void* seg, int F, long long n, const void* weight,
                   const void* poses, const double* grid4, int nx, int ny, double r_min, double r_max,
                   double min_db, void* hits, void* free_, void* stats);

/* Log-odds of the grid map's counts (rsl_map.hip, k_map_logodds), elementwise:
 *     out f32 [ncells] = clamp((double)hits l_occ - (double)free l_free, l_min, l_max); each operation rounded in
 *     fp64, the result rounded to f32 once.  free_ nullable = 0.  RSL_ERR_INVALID: a parameter that is not finite;
 *     l_min > l_max; ncells < 0; null hits or out with ncells > 0.  Timed under RSL_K_AUX. */
int rsl_map_logodds(rsl_handle h, const void* hits, const void* free_, long long ncells, double l_occ, double l_free,
                    double l_min, double l_max, void* out);

/* a3-a6  SignalPreprocessor.dechirp_signal / apply_window / remove_dc / process_chirp (dechirp.py:85-166):
 *     out[r, s] = in[r, s] * table[s], then (dc != 0) minus the row's complex mean.  in/out c64 [rows, S]. */
int rsl_preprocess_rows(rsl_handle h, const void* in, long long rows, int S, const void* table, int dc, void* out);

/* a25, a27  compute_phase_difference_model + cost_function (velocity_solver.py:65-176), general 6-DoF:
 *     pred = k (v + w x p).d, d = (cos el cos az, cos el sin az, sin el); pos f64 [n,3], ang f64 [n,2],
 *     x f64 [6] = (v, w) (device); y f64 [n] nullable; wrap != 0 wraps residuals to (-pi, pi]
 *     (velocity_solver_improved.py:255); cost f64 [1] = sum r^2 + ridge |x|^2 (nullable). */
int rsl_phase_model(rsl_handle h, const void* pos, const void* ang, long long n, const void* x, double k,
                    const void* y, int wrap, double ridge, void* pred, void* resid, void* cost);

/* a28  two_step_optimization (velocity_solver.py:178-307) for arbitrary (pos, ang): exact box-constrained
 *     linear least squares over nv = 3 (v, w = 0) or 6 (v, w) unknowns (BVLS active set, fp64).
 *     lo/hi f64 [nv] device bounds; out f64 [nv + 1] = x, cost.  The cost is the per-target sum of squares
 *     sum_i (y_i - k J_i.x)^2 + ridge |x|^2 evaluated at the returned x (the reference's result.fun), never negative;
 *     it is not formed from the normal-equation moments, which cancel at a near-exact fit. */
int rsl_bvls(rsl_handle h, const void* pos, const void* ang, long long n, const void* y, double k, int nv,
             double ridge, const void* lo, const void* hi, void* out);

/* a30  ImprovedVelocitySolver.associate_targets_across_frames (velocity_solver_improved.py:74-129): for each
 *     current target in order, the nearest unused previous target with Euclidean distance < thr (ties to the
 *     lowest index).  cur_xy f64 [nc][2], prev_xy f64 [np][2] (device), scratch u32 [ceil(np/32)],
 *     match i32 [nc] (-1 = none), dist f64 [nc]. */
int rsl_associate(rsl_handle h, const void* cur_xy, int nc, const void* prev_xy, int np, double thr, void* scratch,
                  void* match, void* dist);

/* configs[3] per-frame pattern, peak selection of RobustAngleEstimator.process_targets_robust
 *     (robust_angle_estimation.py:362-369: power_db > thr_db, stable sort by power_db descending, first kmax), for
 *     every cube k of a batch at once.  entry_base i64 [ncube + 1], e_coord u32 / e_pdb f32 [entry_cap] are the
 *     chain's compacted entries (rsl_peak_emit); kmax <= 256.  Outputs (device, slots k * kmax + r): sel_entry i32
 *     (global entry index, -1 past the selection), sel_frame i32 (= k) and sel_rc i32 (range_bin * C + doppler_bin;
 *     a DoA cell list for rsl_doa / rsl_confidence / rsl_cell_extras), sel_n i32 [ncube] = selected count.  The
 *     selection is in the reference's order: power descending, ties in entry (antenna -> range -> Doppler) order. */
int rsl_peak_topk(rsl_handle h, const void* entry_base, long long entry_cap, int ncube, const void* e_coord,
                  const void* e_pdb, double thr_db, int kmax, int C, void* sel_entry, void* sel_frame, void* sel_rc,
                  void* sel_n);

/* configs[3] per-frame pattern: CompleteRadarScenesAnalyzer._create_target_associations
 *     (radarscenes_complete_analysis.py:274-305) for every frame of a batch at once.  Targets of frame f are
 *     [off[f], off[f+1]) of the concatenated f64 arrays range_m, az_rad and s0 (c128: the first component of each
 *     target's spatial signature); off i64 [nframes + 1] on the device.  For target i of frame f > 0: the target j of
 *     frame f-1 with the smallest sqrt((r_i - r_j)^2 + (az_i - az_j)^2), strict '<' against the running minimum and
 *     against thr (first minimum wins; previous targets may be matched many times), in float64 with each difference,
 *     product, sum and the square root rounded to nearest on its own (no fused multiply-add).  Outputs
 *     [off[nframes]]: match i32 (index within frame f-1, -1 = none; always -1 in frame 0), dist f64, phase f64 =
 *     angle(s0_i * conj(s0_j)) (:296; 0 where unmatched). */
int rsl_associate_nearest(rsl_handle h, const void* range_m, const void* az_rad, const void* s0, const void* off,
                          int nframes, long long ntargets, double thr, void* match, void* dist, void* phase);

/* a30, a31  wrapped-phase ego-motion solve: minimises sum_i wrap(y_i - k J_i.x)^2 + R(x) over the box
 *     [lo6, hi6] (host), J_i = [d_i, p_i x d_i] from pos f64 [n][3] and ang f64 [n][2] (az, el).
 *     mode 0: R = 0.01 |v|^2 + 0.01 |w|^2 (velocity_solver_improved.py:223-266);
 *     mode 1: the piecewise penalties of advanced_velocity_optimization.py:153-223 with weight w, max
 *             velocity vmax, max angular velocity wmax and previous motion prev f64 [6] (device, nullable).
 *     nv = 3 (w fixed at 0; step 1) or 6.  Multi-start projected Gauss-Newton from a grid_n x grid_n grid
 *     over (v_x, v_y) plus nextra extra starts extra f64 [nextra][6] (device), iters iterations each;
 *     out f64 [8] (device) = {x[6], cost, start index}.  scratch >= rsl_wrapped_scratch_bytes(n, grid_n, nextra).
 *     "Projected": every start is clipped to the box, and each iteration solves the Newton system on the free
 *     coordinates only.  A coordinate is held while it sits exactly on a bound and the total gradient points out of
 *     the box there; the others take the step of the reduced Hessian, and the trial points x + step d (step 1, 1/2,
 *     ..., 1/32, the first that lowers the cost) are clipped to the box.  A converged descent so ends at the minimiser
 *     over the box of the quadratic piece it is in (a KKT point), not at the clipped unconstrained minimiser; with
 *     no bound active the step is the plain Newton step. */
long long rsl_wrapped_scratch_bytes(long long n, int grid_n, int nextra);

int rsl_wrapped_solve(rsl_handle h, const void* pos, const void* ang, long long n, const void* y, double k, int mode,
                      double w, double vmax, double wmax, const void* prev, const double* lo6, const double* hi6,
                      int nv, int grid_n, const void* extra, int nextra, int iters, void* scratch,
                      long long scratch_bytes, void* out);

/* a30, a31  the same minimisation with a dense multi-start global stage (a heuristic checked by cost <= the reference
 *     DE on recorded runs; it does not guarantee that every basin of the wrapped cost is entered).
 *     Stage 1: projected 2-D Gauss-Newton in (x0, x1) = (v_x, v_y) from every point of a grid with the given spacing
 *     (a fraction of the wrap period 2 pi / k; ceil(width / spacing) points per axis, at most 32768) over
 *     [lo6[0], hi6[0]] x [lo6[1], hi6[1]], with x[2..5] held at base6 (host, clipped to the box; the regulariser's
 *     optimum for them); stage 2: the nv-D Gauss-Newton of rsl_wrapped_solve from the nbest best stage-1 minima
 *     (1..1024) and the extra starts.  out as rsl_wrapped_solve (start index = position among the stage-2 starts).
 *     scratch >= rsl_wrapped_search_scratch_bytes(n, lo6, hi6, spacing, nbest, nextra). */
long long rsl_wrapped_search_scratch_bytes(long long n, const double* lo6, const double* hi6, double spacing,
                                           int nbest, int nextra);
int rsl_wrapped_search(rsl_handle h, const void* pos, const void* ang, long long n, const void* y, double k, int mode,
                       double w, double vmax, double wmax, const void* prev, const double* lo6, const double* hi6,
                       int nv, const double* base6, double spacing, int nbest, const void* extra, int nextra, int iters,
                       void* scratch, long long scratch_bytes, void* out);

/* L4 trajectory  PoseIntegrator.integrate_translational_velocity / integrate_angular_velocity
 *     (pose_integration.py:67-167) as block-wide fp64 prefix scans over one frame block.
 *     vel f64 [F][vstride] (first nv <= 3 components used, missing ones 0), omega f64 [F][ostride] (nullable = 0),
 *     timestamps f64 [F] (nullable: uniform dt); method 0 = trapezoidal, 1 = euler.
 *     pos f64 [F][3] (pos[0] = 0), quat f64 [F][4] (w,x,y,z; quat[0] = identity),
 *     summary f64 [16] (nullable) = {pos[F-1], quat[F-1], v[F-1], v[0], omega[F-1]} for stitching blocks. */
int rsl_traj_scan(rsl_handle h, const void* vel, int vstride, int nv, const void* omega, int ostride,
                  const void* timestamps, double dt, long long F, int method, void* pos, void* quat, void* summary);
/* Stitch: pos[i] += base[0:3], quat[i] = base[3:7] (x) quat[i]; base f64 [7] (device). */
int rsl_traj_apply(rsl_handle h, void* pos, void* quat, long long F, const void* base);
/* Stitch consecutive frame blocks (e.g. one per GPU after an all-gather of the 16-double summaries, rank order):
 *     state f64 [16] (device, in/out) = {pos (3), quat (4), v_last (3), omega_last (3), started, 0, 0}, zero-init
 *     except quat = (1,0,0,0) (plus the initial pose); base f64 [7] (device, out) = offset of block `rank`. */
int rsl_traj_stitch(rsl_handle h, const void* summaries, int R, int rank, double dt, int method, void* state,
                    void* base);
/* uniform_filter1d(x[:, c], size, mode='nearest') per column (pose_integration.py:105-109); x, out f64 [F][ncol]. */
int rsl_traj_smooth(rsl_handle h, const void* x, long long F, int ncol, int size, void* out);

/* SURVEY §8f #3 (evaluation half)  PoseErrorEvaluator (evaluation/compute_pose_error.py:51-361), fp64.
 *     Poses f64 [n][7] = (x, y, z, q0, q1, q2, q3) with q read as scipy quaternions (scalar LAST, normalised), as the
 *     reference's Rotation.from_quat reads them.  scratch >= rsl_pose_error_scratch_bytes(n, nlen) (device).
 *     rsl_pose_align (align_trajectories :51-96 + compute_ape :171-236): align f64 [32] = position rotation R (9,
 *       row-major; Umeyama :98-140), translation t (3), orientation rotation Rq (9; Rotation.mean of gt * est^-1,
 *       :142-169), its quaternion (4, x y z w, w >= 0), scale_factor = cbrt(det R) (1), the two position means (6);
 *       aligned f64 [n][7]; ape_err f64 [3][n] = position, orientation, combined errors; ape_stats f64 [3][5]
 *       (nullable) = {rmse, mean, std, max, n} per series.
 *     rsl_pose_rte (compute_rte :238-306 on rsl_pose_align's aligned poses): lengths f64 [nlen] (device) segment
 *       lengths; err f64 [nlen][n]: the first counts[l] entries of row l are the segment errors (the valid starts of a
 *       positive length are a prefix); counts u64 [nlen]; stats f64 [nlen][5] as above. */
long long rsl_pose_error_scratch_bytes(long long n, int nlen);
int rsl_pose_align(rsl_handle h, const void* est, const void* gt, long long n, void* scratch, void* align,
                   void* aligned, void* ape_err, void* ape_stats);
int rsl_pose_rte(rsl_handle h, const void* aligned, const void* gt, long long n, const void* lengths, int nlen,
                 void* scratch, void* err, void* counts, void* stats);

/* SURVEY §8f #2  FMCWRadarSimulator.synthesize_frame (scripts/simulate_raw.py:147-221) at batch scale.
 *     rsl_synth_pattern: the deterministic part, which does not depend on the chirp index, as fp64 complex
 *       pattern [A][S] (device) from scatterers f64 [n][4] = {range m, azimuth rad, rcs dBsm, radial velocity m/s}
 *       (device); antenna_spacing <= 0 means lambda / 2; S = samples per chirp (int(chirp_duration * fs)).
 *     rsl_synth_cube: cube c64 [F][A][C][S] = pattern + sqrt(noise_power) (n1 + j n2) with standard normal n1, n2
 *       from Philox-4x32-10 (key = seed, counter = global sample index / 2 counted from frame frame0) and
 *       Box-Muller; S must be even.  Frame blocks generated separately (e.g. one per rank) equal one large call. */
int rsl_synth_pattern(rsl_handle h, const void* scatterers, int n, int A, int S, double fc, double bandwidth,
                      double chirp_duration, double antenna_spacing, void* pattern);
int rsl_synth_cube(rsl_handle h, const void* pattern, int F, int A, int C, int S, double noise_power,
                   unsigned long long seed, long long frame0, void* cube);

#ifdef __cplusplus
}
#endif
#endif /* RSL_H */
