"""Batched per-frame chain on one MI355X: cube -> RDS -> peaks -> DoA (MUSIC argmax) -> ESPRIT -> velocity.

This is the throughput path (``bench.py``) and the engine under the drop-in wrappers.  A batch of F
frames is processed with a fixed sequence of asynchronous kernel launches on the current stream and no
host synchronisation: peak lists are written into capacity-sized buffers whose true sizes live on the
device (``entry_base[F]``, ``cell_base[F]``).  Per-antenna detections of one (range, doppler) cell share
one spatial signature (angle_estimation.py:83), so DoA/ESPRIT run once per unique cell and entries map
to cells (``e_cell``); the velocity LS weights each cell by its number of antenna detections, which
reproduces the reference's sums over all targets exactly.

``ChainConfig(detect_on='sum')`` detects once per frame on the antenna-summed power map instead (non-coherent
integration, include/rsl.h rsl_power_integrate / rsl_detect_power): every cell is then one entry of antenna 0 with
weight 1, and the DoA stage runs unchanged on the full RDS.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib, tables
from .runtime import Context, get_context, unpack_coord

C_LIGHT = 3e8


@dataclass
class ChainConfig:
    num_antennas: int = 8
    num_chirps: int = 128
    fc: float = 77e9
    bandwidth: float = 1e9
    chirp_duration: float = 51.2e-6
    pri: float = 100e-6
    sampling_rate: float = 10e6
    window_type: str = 'hann'
    dc_removal: bool = True
    threshold_db: float = -20.0
    min_range: float = 1.0
    max_range: float = 200.0
    antenna_spacing: Optional[float] = None
    search_range: tuple = (-90, 90)
    search_resolution: float = 0.5
    method: str = 'music'
    velocity_lambda: Optional[float] = None    # VelocitySolver default: c / fc
    dt: float = 0.1
    ridge: float = 0.0
    bounds: tuple = (-50.0, 50.0, -50.0, 50.0)
    entry_frac: float = 0.20                   # capacity: peak entries per cube cell (9.4 % measured)
    cell_frac: float = 1.00                    # capacity: unique cells per (range, doppler) cell (54-76 %)
    spectrum: bool = False                     # also write the MUSIC / beamforming spectrum of every cell, f32
                                               # cell-blocked [cells / 32, G, 32] (rsl.runtime.spectrum_rows)
                                               # (angle_estimation.py:299 stores spectrum f64[G] per target)
    detector: str = 'threshold'                # 'threshold': the reference's rule (threshold_db + 3x3 maximum);
                                               # 'cfar': 2-D CA-CFAR + 3x3 maximum, threshold_db kept as a floor
                                               # (-inf switches the floor off)
    cfar_guard: tuple = (2, 2)                 # guard half-sizes (range, doppler)
    cfar_train: tuple = (8, 8)                 # training half-sizes (range, doppler)
    cfar_pfa: float = 1e-4                     # false-alarm rate -> alpha (tables.cfar_alpha)
    cfar_alpha: Optional[float] = None         # factor on the training mean; overrides cfar_pfa when set
    cfar_method: str = 'ca'                    # 'ca': cell averaging (rsl_detect_cfar); 'os': ordered statistic
                                               # (rsl_detect_oscfar), cfar_alpha / cfar_pfa then refer to the
                                               # order statistic (tables.os_cfar_alpha)
    cfar_rank: float = 0.75                    # 'os': the ceil(cfar_rank * cells)-th smallest training cell, (0, 1]
    detect_on: str = 'antenna'                 # 'antenna': the detector runs once per antenna on that antenna's
                                               # |rds|^2 (the reference's way); 'sum': once per frame on the
                                               # antenna-summed power (non-coherent integration: rsl_power_integrate
                                               # + rsl_detect_power): every cell is one entry of antenna 0, cfar_pfa
                                               # is the rate per cell (alpha designed for a sum of num_antennas looks)
                                               # and threshold_db applies to the summed power
    velocity_loss: str = 'ls'                  # 'ls': rsl_velocity (plain box-constrained LS); 'huber' | 'tukey':
                                               # rsl_velocity_robust (IRLS from the LS start, include/rsl.h);
                                               # 'consensus': rsl_velocity_consensus (two-cell hypotheses, for frames
                                               # where the static cells are not the majority; needs velocity_scale)
    velocity_scale: Optional[float] = None     # residual scale sigma (the sensor's phase-noise sigma, radians); None:
                                               # estimated per iteration from the residuals' weighted median, which
                                               # is dependable only below roughly 30 % coherent outliers
    velocity_c: Optional[float] = None         # tuning constant; None: 1.345 (huber) / 4.685 (tukey) / 3.0 (consensus)
    velocity_iters: int = 30
    velocity_tol: float = 1e-9
    velocity_hyps: int = 256                   # 'consensus': hypotheses per frame, 1 .. _lib.CONSENSUS_MAX_H
    velocity_min_det: float = 0.1              # 'consensus': the least |sin| of a pair's azimuth difference, (0, 1]
    velocity_refine: int = 3                   # 'consensus': LS passes on the winner's inliers, 0 .. 100
    velocity_seed: int = 0                     # 'consensus': key of the hypothesis draws
    multi_source: bool = False                 # also run the spatially smoothed MUSIC (rsl_doa_smoothed) on every
                                               # cell: up to ss_max angles per cell in results()['ss_*']; gidx, esprit,
                                               # phase and the velocity solve keep using the one-angle scan
    ss_len: Optional[int] = None               # sub-array length L; None: min(8, A - A // 3)
    ss_sources: int = 0                        # sources per cell; 0: estimated from the eigenvalues (>= ss_rel * the
                                               # largest), which depends on the SNR -- a fixed count is the dependable
                                               # setting
    ss_rel: float = 0.05
    ss_max: int = 3                            # angles kept per cell (lowered to L - 1 where it exceeds it)
    ra_map: Optional[str] = None               # 'bartlett' | 'capon': also form every range bin's spatial covariance
                                               # over its Doppler bins (rsl_range_cov) and the range-azimuth power map
                                               # on the chain's grid (rsl_range_azimuth): results()['ra_map'], ['ra_arg'];
                                               # None: nothing is allocated or launched
    ra_doppler: Optional[tuple] = None         # Doppler window (c0, c1) of the covariance; None: all num_chirps bins
    ra_loading: float = 1e-2                   # Capon's diagonal loading, in [_lib.RA_MIN_LOADING, 1]
    point_cloud: bool = False                  # also refine every cell below the bin and grid spacing
                                               # (rsl_cell_refine, after the DoA scan): results()['points'] f32
                                               # [cells, 8] = {range, doppler, az, x, y, power_db, range offset,
                                               # doppler offset} and ['az_refined']; the range estimator follows
                                               # window_type (tables.refine_mode_for_window), the Doppler axis takes
                                               # 'rect'; False: nothing is allocated or launched
    pc_velocity: bool = False                  # label the points' Doppler column in metres per second
                                               # (tables.point_axes(velocity=True)) instead of the reference's hertz
    velocity_az: str = 'grid'                  # 'grid': the solvers read az_table[gidx]; 'refined': the refined
                                               # azimuths of the point cloud (needs point_cloud)
    registration: bool = False                 # also register every frame's point cloud against the frame before it
                                               # (rsl_scan_register, after the velocity solve; needs point_cloud):
                                               # results()['registration'] f64 [F, 8] = {theta, t_x, t_y, W, rms,
                                               # S_best / sum S, updates, flag} and chain.omega f64 [F, 3] for
                                               # TrajectoryReducer.step(chain.vel, ..., omega=chain.omega).  The start
                                               # is (0, v_x dt, v_y dt) from the velocity rows; a robust or consensus
                                               # solver's vel_weight keeps the movers from voting; the chain's last
                                               # frame is kept as the next run's reference (reset_registration()).
                                               # False: nothing is allocated or launched
    reg_h: float = 0.5                         # the kernel's final radius, metres
    reg_h_coarse: float = 1.0                  # the radius of the yaw search and of the first step
    reg_dtheta: float = math.radians(0.25)     # the yaw search's step, radians
    reg_k: int = 20                            # candidates on each side of the start yaw, 0 .. _lib.REG_MAX_K
    reg_iters: int = 10                        # MM / IRLS steps, 0 .. _lib.REG_MAX_ITERS
    reg_shrink: float = 0.7                    # the radius' factor per step, (0, 1]
    reg_tol: float = 1e-9                      # stop below this change of (theta, t_x, t_y)
    reg_w_min: float = 3.0                     # the least kernel weight a step needs

    def __post_init__(self):
        if self.registration:
            if not self.point_cloud:
                raise ValueError('registration=True needs point_cloud=True')
            pos = lambda v: math.isfinite(float(v)) and float(v) > 0.0
            if not (pos(self.reg_h) and pos(self.reg_h_coarse) and pos(self.reg_dtheta) and pos(self.dt)):
                raise ValueError('registration needs reg_h, reg_h_coarse, reg_dtheta and dt finite and > 0')
            if float(self.reg_h_coarse) < float(self.reg_h):
                raise ValueError(f'reg_h_coarse {self.reg_h_coarse!r} is below reg_h {self.reg_h!r}')
            if not 0 <= int(self.reg_k) <= _lib.REG_MAX_K:
                raise ValueError(f'reg_k must lie in [0, {_lib.REG_MAX_K}], not {self.reg_k!r}')
            if not 0 <= int(self.reg_iters) <= _lib.REG_MAX_ITERS:
                raise ValueError(f'reg_iters must lie in [0, {_lib.REG_MAX_ITERS}], not {self.reg_iters!r}')
            if not 0.0 < float(self.reg_shrink) <= 1.0:
                raise ValueError(f'reg_shrink must lie in (0, 1], not {self.reg_shrink!r}')
            if not (math.isfinite(float(self.reg_w_min)) and float(self.reg_w_min) >= 0.0):
                raise ValueError(f'reg_w_min must be finite and >= 0, not {self.reg_w_min!r}')
        if self.velocity_az not in ('grid', 'refined'):
            raise ValueError(f"velocity_az must be 'grid' or 'refined', not {self.velocity_az!r}")
        if self.velocity_az == 'refined' and not self.point_cloud:
            raise ValueError("velocity_az='refined' needs point_cloud=True")
        if self.point_cloud:
            if not 2 <= int(self.num_antennas) <= 32:
                raise ValueError(f'point_cloud needs 2 to 32 antennas, not {self.num_antennas}')
            tables.refine_mode_for_window(self.window_type)  # ValueError for a window without an estimator
        if self.ra_map is not None and self.ra_map not in _lib.RA_IDS:
            raise ValueError(f"ra_map must be None, 'bartlett' or 'capon', not {self.ra_map!r}")
        if self.ra_doppler is not None:
            if len(tuple(self.ra_doppler)) != 2 or not (0 <= int(self.ra_doppler[0]) < int(self.ra_doppler[1])
                                                        <= int(self.num_chirps)):
                raise ValueError(f'ra_doppler must be (c0, c1) with 0 <= c0 < c1 <= {int(self.num_chirps)}, '
                                 f'not {self.ra_doppler!r}')
        if not _lib.RA_MIN_LOADING <= float(self.ra_loading) <= 1.0:
            raise ValueError(f'ra_loading must lie in [{_lib.RA_MIN_LOADING}, 1], not {self.ra_loading!r}')
        if self.ra_map is not None and not 2 <= int(self.num_antennas) <= _lib.RA_MAX_A:
            raise ValueError(f'ra_map needs 2 to {_lib.RA_MAX_A} antennas, not {self.num_antennas}')
        if self.ss_len is not None and not 2 <= int(self.ss_len) <= _lib.SS_MAX_L:
            raise ValueError(f'ss_len must lie in [2, {_lib.SS_MAX_L}], not {self.ss_len!r}')
        if int(self.ss_max) < 1:
            raise ValueError(f'ss_max must be >= 1, not {self.ss_max!r}')
        if not 0 <= int(self.ss_sources) <= int(self.ss_max):
            raise ValueError(f'ss_sources must lie in [0, ss_max], not {self.ss_sources!r}')
        if not 0.0 < float(self.ss_rel) < 1.0:
            raise ValueError(f'ss_rel must lie in (0, 1), not {self.ss_rel!r}')
        if self.multi_source:
            A = int(self.num_antennas)
            if not 3 <= A <= 16:
                raise ValueError(f'multi_source needs 3 to 16 antennas, not {A}')
            L = self.ss_sub_len
            if L > A:
                raise ValueError(f'ss_len {L} exceeds the {A} antennas')
            if int(self.ss_sources) > min(int(self.ss_max), L - 1):
                raise ValueError(f'ss_sources {self.ss_sources} exceeds the {L - 1} angles a sub-array of {L} resolves')
        if self.velocity_loss not in ('ls', 'huber', 'tukey', 'consensus'):
            raise ValueError("velocity_loss must be 'ls', 'huber', 'tukey' or 'consensus', "
                             f'not {self.velocity_loss!r}')
        if self.velocity_loss == 'consensus':
            if self.velocity_scale is None or not float(self.velocity_scale) > 0.0:
                raise ValueError("velocity_loss='consensus' needs velocity_scale > 0, the phase-noise sigma in radians")
            if not 1 <= int(self.velocity_hyps) <= _lib.CONSENSUS_MAX_H:
                raise ValueError(f'velocity_hyps must lie in [1, {_lib.CONSENSUS_MAX_H}], not {self.velocity_hyps!r}')
            if not 0.0 < float(self.velocity_min_det) <= 1.0:
                raise ValueError(f'velocity_min_det must lie in (0, 1], not {self.velocity_min_det!r}')
            if not 0 <= int(self.velocity_refine) <= 100:
                raise ValueError(f'velocity_refine must lie in [0, 100], not {self.velocity_refine!r}')
        if self.detector not in ('threshold', 'cfar'):
            raise ValueError(f"detector must be 'threshold' or 'cfar', not {self.detector!r}")
        if self.detect_on not in ('antenna', 'sum'):
            raise ValueError(f"detect_on must be 'antenna' or 'sum', not {self.detect_on!r}")
        if self.detect_on == 'sum' and not 1 <= int(self.num_antennas) <= 32:
            raise ValueError(f"detect_on='sum' needs 1 to 32 antennas, not {self.num_antennas}")
        if self.cfar_method not in tables.CFAR_METHODS:
            raise ValueError(f"cfar_method must be 'ca' or 'os', not {self.cfar_method!r}")
        if not 0.0 < float(self.cfar_rank) <= 1.0:
            raise ValueError(f'cfar_rank must lie in (0, 1], not {self.cfar_rank!r}')

    @property
    def ss_sub_len(self) -> int:
        return tables.default_sub_len(self.num_antennas) if self.ss_len is None else int(self.ss_len)

    @property
    def S(self) -> int:
        return tables.samples_per_chirp(self.chirp_duration, self.sampling_rate)

    @property
    def lambda_c(self) -> float:
        return C_LIGHT / self.fc


GUARD_BYTES = 256 * 1024  # sentinel pad on each side of a guarded buffer (RadarChain(guard=True))
GUARD_FILL = 0xA5


class RadarChain:
    def __init__(self, cfg: ChainConfig, frames: int, ctx: Optional[Context] = None, vel_out=None,
                 guard: bool = False, spec_out=None):
        """vel_out: optional device f64 [frames, 8] view receiving the per-frame velocity rows (lets several
        chains on different streams fill consecutive slices of one buffer).
        guard: debug canary — every device buffer of the chain gets its own allocation with GUARD_BYTES of sentinel
        bytes on both sides; guard_violations() lists the buffers whose pads were written (a store that left its own
        buffer: tests/test_gpu_pipelined.py).
        spec_out: optional device f32 tensor receiving the cell-blocked spectrum (cfg.spectrum), of shape
        spectrum_shape(), or 'contiguous': the chain allocates it with Context.empty_contiguous (one physically
        contiguous allocation; the default allocator when the driver cannot provide one, spec_contiguous tells)."""
        self.cfg, self.F = cfg, int(frames)
        self.ctx = ctx or get_context()
        torch, ctx = self.ctx.torch, self.ctx
        self._guards = []
        A, C, S, F = cfg.num_antennas, cfg.num_chirps, cfg.S, self.F
        self.A, self.C, self.S = A, C, S
        tab = tables.chirp_table(cfg.fc, cfg.bandwidth, cfg.chirp_duration, cfg.sampling_rate, cfg.window_type, S)
        self.table = ctx.to_dev(tab.astype(np.complex64))
        self.i_lo, self.i_hi = tables.range_gate(cfg.bandwidth, S, cfg.min_range, cfg.max_range)
        self.thr_p = tables.power_threshold(cfg.threshold_db)
        self.cfar_alpha = None
        if cfg.detector == 'cfar':
            self.cfar_alpha = float(cfg.cfar_alpha) if cfg.cfar_alpha is not None else tables.cfar_design_alpha(
                cfg.cfar_method, cfg.cfar_pfa, cfg.cfar_guard, cfg.cfar_train, cfg.cfar_rank,
                looks=cfg.num_antennas if cfg.detect_on == 'sum' else 1)
        d = cfg.antenna_spacing or cfg.lambda_c / 2
        self.grid = tables.azimuth_grid(cfg.search_range, cfg.search_resolution)
        steer_c128 = tables.steering_matrix(self.grid, np.arange(A) * d, cfg.lambda_c)
        self.steer = ctx.steering(steer_c128)
        self.az_table = ctx.to_dev(np.radians(self.grid).astype(np.float64))
        self.esprit_scale = cfg.lambda_c / (2 * np.pi * d)
        lam_v = cfg.velocity_lambda or cfg.lambda_c
        self.k = 4 * np.pi * cfg.dt / lam_v
        self.method = _lib.METHOD_MUSIC if cfg.method == 'music' else _lib.METHOD_BEAMFORMING
        self.sum = cfg.detect_on == 'sum'
        DA = 1 if self.sum else A  # antenna maps the detector decides on per frame
        self.entry_cap = int(math.ceil(cfg.entry_frac * F * DA * S * C)) + 64
        self.cell_cap = (int(math.ceil(cfg.cell_frac * F * S * C)) + 64 + 3) & ~3  # a multiple of 4 (16-B rows)
        e = self._guarded_empty if guard else ctx.empty
        W = (C + 63) // 64
        self.work = e((F, A, C, S), torch.complex64)
        self.rds = e((F, A, S, C), torch.complex64)
        self.mask = e((F, A, S, W), torch.int64)
        self.row_count = e((F, A, S), torch.int32)
        self.peak_pow = e((F, A, S, C), torch.float32)  # row-compact peak powers (detect -> emit)
        self.power = None
        if self.sum:
            # the fused front end still writes its per-antenna outputs; what it wrote is not read, and the detector of
            # the summed map puts its own (one map per frame) at the start of the same buffers
            self.power = e((F, S, C), torch.float32)  # the antenna-summed map (the integrated range-Doppler map)
            self._front = dict(mask=self.mask, row_count=self.row_count, peak_pow=self.peak_pow)
            self.mask = self.mask.view(-1)[:F * S * W].view(F, 1, S, W)
            self.row_count = self.row_count.view(-1)[:F * S].view(F, 1, S)
            self.peak_pow = self.peak_pow.view(-1)[:F * S * C].view(F, 1, S, C)
        self.offs = dict(entry_row_off=e((F * DA * S,), torch.int32), cell_row_off=e((F * S,), torch.int32),
                         scratch=e((F * S,), torch.int32), entry_base=e((F + 1,), torch.int64),
                         cell_base=e((F + 1,), torch.int64), frame_counts=e((2 * F,), torch.int64),
                         union_mask=e((F, S, W), torch.int64))
        ec, cc = self.entry_cap, self.cell_cap
        self.lists = dict(e_coord=e((ec,), torch.int32), e_cell=e((ec,), torch.int32), e_pdb=e((ec,), torch.float32),
                          c_frame=e((cc,), torch.int32), c_rc=e((cc,), torch.int32), c_amask=e((cc,), torch.int32))
        self.gidx = e((cc,), torch.int32)
        self.ext = dict(esprit=e((cc,), torch.float64), phase=e((cc,), torch.float64), az=e((cc,), torch.float64))
        self.vel = vel_out if vel_out is not None else e((F, 8), torch.float64)
        # IRLS weight of every cell ('consensus': the inlier mask)
        self.vel_weight = e((cc,), torch.float32) if cfg.velocity_loss != 'ls' else None
        self.ncell_dev = self.offs['cell_base'][F:F + 1]
        self.ss = None
        if cfg.multi_source:  # smoothed MUSIC: its own outputs on the same cell lists
            L = cfg.ss_sub_len
            self.ss_nmax = min(int(cfg.ss_max), L - 1)
            self.ss_steer = ctx.steering_sub(steer_c128, L)
            self.ss = dict(nsrc=e((cc,), torch.int32), idx=e((cc, self.ss_nmax), torch.int32),
                           den=e((cc, self.ss_nmax), torch.float32))
        self.ra = None
        if cfg.ra_map is not None:  # range-azimuth map: per-range covariance, then its power over the grid
            self.ra_steer = ctx.steering_c64(steer_c128)
            self.ra_win = (0, C) if cfg.ra_doppler is None else (int(cfg.ra_doppler[0]), int(cfg.ra_doppler[1]))
            self.ra_cov = e((F, S, A, A), torch.complex64)
            self.ra = dict(map=e((F, S, len(self.grid)), torch.float32), arg=e((F, S), torch.int32))
        self.pc = None
        if cfg.point_cloud:  # point cloud: one row and one refined azimuth per cell, from the antenna-summed power
            self.pc_steer = ctx.steering_c64(steer_c128)
            self.pc_modes = (tables.refine_mode_for_window(cfg.window_type), 'rect')
            self.pc_axes = tables.point_axes(cfg, S, C, velocity=cfg.pc_velocity)
            if self.power is None:  # detect_on='antenna': no summed map yet, run_back integrates it
                self.power = e((F, S, C), torch.float32)
            self.pc = dict(points=e((cc, 8), torch.float32), az=e((cc,), torch.float64))
        self.reg = None
        self.omega = None
        if cfg.registration:  # scan registration: one row per frame, and the last frame's cloud kept for the next run
            fc = S * C  # the most cells of one frame
            self.reg = dict(rows=e((F, 8), torch.float64), omega=e((F, 3), torch.float64))
            self.omega = self.reg['omega']
            self.reg_init = e((F, 3), torch.float64)
            self.reg_keep = dict(points=e((fc, 8), torch.float32), rc=e((fc,), torch.int32), n_dev=e((1,), torch.int64),
                                 weight=e((fc,), torch.float32) if self.vel_weight is not None else None)
            self.reg_prev = None  # reg_keep once a run has filled it
            self.reg_idx = torch.arange(fc, dtype=torch.int64, device=ctx.device)
        # one signature gather for DoA + ESPRIT + phase when the Toeplitz path applies (uniform linear array)
        self.fused_doa = bool(self.steer['toeplitz']) and A >= 2 and not cfg.spectrum
        self.spec = None
        self.spec_contiguous = False
        if cfg.spectrum:
            shp = self.spectrum_shape()
            if isinstance(spec_out, str):
                if spec_out != 'contiguous':
                    raise ValueError("spec_out: a tensor, 'contiguous' or None")
                spec_out = ctx.empty_contiguous(shp, torch.float32)  # None: the driver could not provide it
                self.spec_contiguous = spec_out is not None
            if spec_out is not None:
                if tuple(spec_out.shape) != shp or spec_out.dtype != torch.float32 or not spec_out.is_contiguous():
                    raise ValueError(f'spec_out must be a contiguous float32 tensor of shape {shp}')
                self.spec = spec_out
            else:
                self.spec = e(shp, torch.float32)

    def spectrum_shape(self):
        """Shape of the cell-blocked spectrum buffer: [ceil(cell_cap / 32), G, 32] f32."""
        return ((self.cell_cap + 31) // 32, len(self.grid), 32)

    def _guarded_empty(self, shape, dtype):
        torch = self.ctx.torch
        n = 1
        for d in (shape if isinstance(shape, tuple) else (shape,)):
            n *= int(d)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        raw = torch.empty((2 * GUARD_BYTES + nbytes,), dtype=torch.uint8, device=self.ctx.device)
        raw.fill_(GUARD_FILL)
        self._guards.append(raw)
        return raw[GUARD_BYTES:GUARD_BYTES + nbytes].view(dtype).view(shape)

    def guard_violations(self):
        """Indices (allocation order) and byte counts of guarded buffers whose sentinel pads changed (synchronises)."""
        bad = []
        for k, raw in enumerate(self._guards):
            n = int((raw[:GUARD_BYTES] != GUARD_FILL).sum().item() + (raw[-GUARD_BYTES:] != GUARD_FILL).sum().item())
            if n:
                bad.append((k, n))
        return bad

    def run(self, cube, *, esprit: bool = True, velocity: bool = True):
        """Launch the whole chain for cube complex64 [F, A, C, S] on the current stream (asynchronous)."""
        self.run_front(cube)
        self.run_back(esprit=esprit, velocity=velocity)

    def run_front(self, cube, *, emit: bool = True, offsets: bool = True):
        """Memory-bound half: RDS + detection, offsets, peak / cell compaction (current stream). With emit=False the
        compaction is left to run_back(emit=True) (a pipelining split of the same work)."""
        ctx, cfg = self.ctx, self.cfg
        if self.F == 0:  # empty batch: only the (zeroed) bases
            ctx.offsets(self.mask, self.row_count, self.C, bufs=self.offs)
            return
        front = self._front if self.sum else dict(mask=self.mask, row_count=self.row_count, peak_pow=self.peak_pow)
        group = ctx.rds_detect(cube, self.table, self.thr_p, self.i_lo, self.i_hi, rds=self.rds, work=self.work,
                               dc_removal=cfg.dc_removal, **front)
        self._group = group
        if self.sum:  # one decision per cell, on the antenna-summed power
            out = dict(mask=self.mask, row_count=self.row_count, peak_pow=self.peak_pow)
            ctx.integrate_power(self.rds, out=self.power)
            ctx.detect_power(self.power, 'threshold' if cfg.detector == 'threshold' else cfg.cfar_method,
                             cfg.cfar_guard, cfg.cfar_train, cfg.cfar_rank,
                             self.cfar_alpha if self.cfar_alpha is not None else 1.0, self.thr_p, self.i_lo,
                             self.i_hi, out=out)
            self._group = 1
        elif cfg.detector == 'cfar':  # the CFAR detector rewrites the fused detector's mask, counts and peak powers
            out = dict(mask=self.mask, row_count=self.row_count, peak_pow=self.peak_pow)
            ctx.detect_cfar(self.rds, cfg.cfar_guard, cfg.cfar_train, self.cfar_alpha, self.thr_p, self.i_lo,
                            self.i_hi, out=out, method=cfg.cfar_method, rank=cfg.cfar_rank)
            self._group = 1
        if offsets:
            ctx.offsets(self.mask, self.row_count, self.C, bufs=self.offs)
        if emit:
            self._emit()

    def _emit(self):
        self.ctx.emit(self.rds, self.mask, self.offs, self.entry_cap, self.cell_cap, want_pdb=True, bufs=self.lists,
                      peak_pow=self.peak_pow, peak_pow_group=self._group)

    def run_back(self, *, esprit: bool = True, velocity: bool = True, emit: bool = False, offsets: bool = False):
        """Compute-bound half: DoA scan (+ ESPRIT, phase) and the velocity solve, on run_front's lists (emit=True:
        the compaction first, after run_front(emit=False))."""
        ctx, cfg = self.ctx, self.cfg
        L = self.lists
        if self.F == 0:
            return
        if offsets:
            ctx.offsets(self.mask, self.row_count, self.C, bufs=self.offs)
        if emit:
            self._emit()
        if self.fused_doa:
            ctx.doa_extras(self.rds, L['c_frame'], L['c_rc'], self.steer, self.method, n=self.cell_cap,
                           n_dev=self.ncell_dev, esprit_scale=self.esprit_scale, out_idx=self.gidx,
                           esprit=self.ext['esprit'] if esprit else None, phase=self.ext['phase'] if velocity else None)
        else:
            ctx.doa(self.rds, L['c_frame'], L['c_rc'], self.steer, self.method, n=self.cell_cap,
                    n_dev=self.ncell_dev, out_idx=self.gidx, want_spec=self.spec is not None, spec_blocked=True,
                    out_spec=self.spec)
            if esprit or velocity:
                ctx.cell_extras(self.rds, L['c_frame'], L['c_rc'], n=self.cell_cap, n_dev=self.ncell_dev,
                                esprit_scale=self.esprit_scale, want_esprit=esprit, want_phase=velocity,
                                bufs=self.ext)
        if self.ss is not None:
            ctx.doa_smoothed(self.rds, L['c_frame'], L['c_rc'], self.ss_steer, n=self.cell_cap, n_dev=self.ncell_dev,
                             nmax=self.ss_nmax, num_sources=cfg.ss_sources, rel=cfg.ss_rel, out=self.ss)
        if self.ra is not None:
            ctx.range_cov(self.rds, self.ra_win, out=self.ra_cov)
            ctx.range_azimuth(self.ra_cov, self.ra_steer, cfg.ra_map, loading=cfg.ra_loading, out=self.ra)
        if self.pc is not None:
            if not self.sum:
                ctx.integrate_power(self.rds, out=self.power)
            ctx.cell_refine(self.rds, L['c_frame'], L['c_rc'], self.gidx, self.az_table, self.pc_steer,
                            n=self.cell_cap, n_dev=self.ncell_dev, power=self.power, range_mode=self.pc_modes[0],
                            doppler_mode=self.pc_modes[1], axes=self.pc_axes, out=self.pc)
        if not velocity:
            return
        # the problem the three solvers share: the chain's own lists, on the grid-index path
        prob = dict(az=None, y=self.ext['phase'], seg=self.offs['cell_base'], k=self.k, ridge=cfg.ridge,
                    bounds=cfg.bounds, amask=L['c_amask'], out=self.vel, gidx=self.gidx, az_table=self.az_table,
                    n=self.cell_cap)
        if cfg.velocity_az == 'refined':  # the point cloud's azimuths in place of the grid's
            prob.update(az=self.pc['az'], gidx=None, az_table=None)
        if cfg.velocity_loss == 'consensus':
            # vel columns 2-7 become {cost, rmse_in, n_in, n, best_h, n_valid} (include/rsl.h)
            ctx.velocity_consensus(**prob, scale=cfg.velocity_scale, c=cfg.velocity_c, hyps=cfg.velocity_hyps,
                                   min_det=cfg.velocity_min_det, refine=cfg.velocity_refine, seed=cfg.velocity_seed,
                                   frame0=0, want_weight=self.vel_weight)
        elif cfg.velocity_loss != 'ls':
            # vel columns 2-7 become {cost, rmse_w, n_in, n, sigma, it} (include/rsl.h)
            ctx.velocity_robust(**prob, loss=cfg.velocity_loss, c=cfg.velocity_c, scale=cfg.velocity_scale,
                                iters=cfg.velocity_iters, tol=cfg.velocity_tol, want_weight=self.vel_weight)
        else:
            ctx.velocity(**prob)
        if self.reg is not None:
            self._register()

    def _register(self):
        """Scan registration of the batch (after the velocity solve), then the batch's last frame into reg_keep."""
        ctx, cfg, torch = self.ctx, self.cfg, self.ctx.torch
        init = self.reg_init
        init[:, 0] = 0.0
        torch.mul(self.vel[:, :2], float(cfg.dt), out=init[:, 1:])  # the Doppler displacement v dt
        ctx.scan_register(self.pc['points'], self.offs['cell_base'], weight=self.vel_weight, rc=self.lists['c_rc'],
                          C=self.C, axes=self.pc_axes, prev=self.reg_prev, init=init, h=cfg.reg_h,
                          h_coarse=cfg.reg_h_coarse, dtheta=cfg.reg_dtheta, k=cfg.reg_k, iters=cfg.reg_iters,
                          shrink=cfg.reg_shrink, tol=cfg.reg_tol, w_min=cfg.reg_w_min, dt=cfg.dt, n=self.cell_cap,
                          out=self.reg)
        # the last frame's rows, by device-side indices (no host synchronisation): rows past the frame's end are
        # copies of the list's last slot and lie beyond n_dev
        base = self.offs['cell_base'].clamp(0, self.cell_cap)
        keep = self.reg_keep
        idx = (self.reg_idx + base[self.F - 1]).clamp_(max=self.cell_cap - 1)
        torch.index_select(self.pc['points'], 0, idx, out=keep['points'])
        torch.index_select(self.lists['c_rc'], 0, idx, out=keep['rc'])
        if keep['weight'] is not None:
            torch.index_select(self.vel_weight, 0, idx, out=keep['weight'])
        torch.sub(base[self.F:self.F + 1], base[self.F - 1:self.F], out=keep['n_dev'])
        self.reg_prev = keep

    def reset_registration(self):
        """Forget the cloud kept from the last run: the next run's frame 0 has no reference (flag 2)."""
        if self.reg is not None:
            self.reg_prev = None

    def totals(self):
        eb = self.offs['entry_base'][self.F].item()
        cb = self.offs['cell_base'][self.F].item()
        return int(eb), int(cb)

    def results(self):
        """Synchronise and copy the batch results to host numpy arrays."""
        ne, nc = self.totals()
        if ne > self.entry_cap or nc > self.cell_cap:
            raise RuntimeError(f"peak capacity exceeded: entries {ne}/{self.entry_cap}, cells {nc}/{self.cell_cap}")
        L = self.lists
        h = lambda t, n: t[:n].cpu().numpy()
        extra = dict(vel_weight=h(self.vel_weight, nc)) if self.vel_weight is not None else {}
        if self.ss is not None:
            extra.update(ss_nsrc=h(self.ss['nsrc'], nc), ss_gidx=h(self.ss['idx'], nc).astype(np.int64),
                         ss_den=h(self.ss['den'], nc).astype(np.float64))
        if self.ra is not None:  # f32 [F, S, G] and i32 [F, S]: every range bin of every frame
            extra.update(ra_map=self.ra['map'].cpu().numpy(), ra_arg=self.ra['arg'].cpu().numpy())
        if self.reg is not None:
            extra.update(registration=self.reg['rows'].cpu().numpy())
        if self.pc is not None:
            extra.update(points=h(self.pc['points'], nc), az_refined=h(self.pc['az'], nc))
        return dict(entry_base=self.offs['entry_base'].cpu().numpy(), cell_base=self.offs['cell_base'].cpu().numpy(),
                    **dict(zip(('e_ant', 'e_rbin', 'e_dbin'), unpack_coord(h(L['e_coord'], ne)))),
                    e_cell=h(L['e_cell'], ne), e_pdb=h(L['e_pdb'], ne).astype(np.float64), c_frame=h(L['c_frame'], nc),
                    c_rc=h(L['c_rc'], nc), c_amask=h(L['c_amask'], nc), gidx=h(self.gidx, nc),
                    esprit=h(self.ext['esprit'], nc), phase=h(self.ext['phase'], nc),
                    az=np.radians(self.grid)[h(self.gidx, nc)],
                    velocity=self.vel.cpu().numpy(), grid=self.grid, **extra)
