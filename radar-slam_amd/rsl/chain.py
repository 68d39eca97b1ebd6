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
        # every stage refuses its own settings; the order decides which refusal wins
        for stage in (Registration, PointCloud, RangeAzimuth, SmoothedMusic, VelocitySolve, Detector):
            stage.check(self)

    @property
    def ss_sub_len(self) -> int:
        return tables.default_sub_len(self.num_antennas) if self.ss_len is None else int(self.ss_len)

    @property
    def S(self) -> int:
        return tables.samples_per_chirp(self.chirp_duration, self.sampling_rate)

    @property
    def lambda_c(self) -> float:
        return C_LIGHT / self.fc


# --- the stages -------------------------------------------------------------------------------------------------------
# A stage is a plain class that owns one step of the chain: check(cfg) is its share of ChainConfig's refusals; its
# constructor takes the chain, allocates its buffers through chain.alloc (guarded when the chain is) and uploads its
# tables; launch(**over) makes its Context call with its own keyword arguments, `over` laid on top -- the chain calls
# launch(), a tool that measures a variant passes only the difference; results(nc) gives its keys of
# RadarChain.results().  What a stage owns (settings, tables, its buffers: .kw) is bound at construction; the chain's
# buffers are read from the chain at every launch, as a caller may swap one between runs (bench.py rotates chain.spec).

class Detector:
    """What decides the peaks after the fused front end (rds_detect, which writes .front), in one of three forms: the
    front end's own threshold decision stands (.call is None: nothing to launch); 'cfar' rewrites its mask, counts and
    peak powers per antenna; 'sum' decides once per frame on the antenna-summed map chain.power, by any rule."""

    @staticmethod
    def check(cfg):
        if cfg.detector not in ('threshold', 'cfar'):
            raise ValueError(f"detector must be 'threshold' or 'cfar', not {cfg.detector!r}")
        if cfg.detect_on not in ('antenna', 'sum'):
            raise ValueError(f"detect_on must be 'antenna' or 'sum', not {cfg.detect_on!r}")
        if cfg.detect_on == 'sum' and not 1 <= int(cfg.num_antennas) <= 32:
            raise ValueError(f"detect_on='sum' needs 1 to 32 antennas, not {cfg.num_antennas}")
        if cfg.cfar_method not in tables.CFAR_METHODS:
            raise ValueError(f"cfar_method must be 'ca' or 'os', not {cfg.cfar_method!r}")
        if not 0.0 < float(cfg.cfar_rank) <= 1.0:
            raise ValueError(f'cfar_rank must lie in (0, 1], not {cfg.cfar_rank!r}')

    def __init__(self, ch, front):
        cfg, F, S, C = ch.cfg, ch.F, ch.S, ch.C
        self.ch, self.front, self.out, self.call, self.alpha = ch, front, front, None, None
        if cfg.detector == 'cfar':
            self.alpha = float(cfg.cfar_alpha) if cfg.cfar_alpha is not None else tables.cfar_design_alpha(
                cfg.cfar_method, cfg.cfar_pfa, cfg.cfar_guard, cfg.cfar_train, cfg.cfar_rank,
                looks=cfg.num_antennas if ch.sum else 1)
        win = dict(guard=cfg.cfar_guard, train=cfg.cfar_train, rank=cfg.cfar_rank, thr_power=ch.thr_p, i_lo=ch.i_lo,
                   i_hi=ch.i_hi)
        if ch.sum:
            # the fused front end still writes its per-antenna outputs; what it wrote is not read, and the detector of
            # the summed map puts its own (one map per frame) at the start of the same buffers
            W = front['mask'].shape[-1]
            self.out = dict(mask=front['mask'].view(-1)[:F * S * W].view(F, 1, S, W),
                            row_count=front['row_count'].view(-1)[:F * S].view(F, 1, S),
                            peak_pow=front['peak_pow'].view(-1)[:F * S * C].view(F, 1, S, C))
            self.call, self.reads = 'detect_power', 'power'  # the launcher, and the chain buffer it decides on
            self.kw = dict(win, rule='threshold' if cfg.detector == 'threshold' else cfg.cfar_method,
                           alpha=self.alpha if self.alpha is not None else 1.0, out=self.out)
        elif cfg.detector == 'cfar':
            self.call, self.reads = 'detect_cfar', 'rds'
            self.kw = dict(win, alpha=self.alpha, method=cfg.cfar_method, out=self.out)

    def launch(self, **over):
        ch = self.ch
        return getattr(ch.ctx, self.call)(**{self.reads: getattr(ch, self.reads), **self.kw, **over})


class FusedDoa:
    """DoA argmax, ESPRIT and phase from one signature gather (doa_extras): the uniform linear array's path."""
    spec, spec_contiguous = None, False

    def __init__(self, ch, spec_out=None):
        self.ch = ch
        self.kw = dict(steer=ch.steer, method=ch.method, esprit_scale=ch.esprit_scale)

    def launch(self, esprit=True, velocity=True, **over):
        ch = self.ch
        ch.ctx.doa_extras(**{**ch.cells(), **self.kw, 'out_idx': ch.gidx,
                             'esprit': ch.ext['esprit'] if esprit else None,
                             'phase': ch.ext['phase'] if velocity else None, **over})


class ScanDoa:
    """The steering scan (doa), with the cell-blocked spectrum where cfg.spectrum asks for it, then ESPRIT and phase
    (cell_extras) where either is wanted."""

    def __init__(self, ch, spec_out=None):
        ctx, torch = ch.ctx, ch.ctx.torch
        self.ch, self.spec, self.spec_contiguous = ch, None, False  # spec: as allocated; the chain's is the live one
        if ch.cfg.spectrum:
            shp = ch.spectrum_shape()
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
                self.spec = ch.alloc(shp, torch.float32)
        self.kw = dict(steer=ch.steer, method=ch.method, spec_blocked=True)

    def launch(self, esprit=True, velocity=True, **over):
        ch = self.ch
        cells = ch.cells()
        ch.ctx.doa(**{**cells, **self.kw, 'out_idx': ch.gidx, 'want_spec': ch.spec is not None, 'out_spec': ch.spec,
                      **over})
        if esprit or velocity:
            ch.ctx.cell_extras(**cells, esprit_scale=ch.esprit_scale, want_esprit=esprit, want_phase=velocity,
                               bufs=ch.ext)


class SmoothedMusic:
    """cfg.multi_source: the spatially smoothed MUSIC (doa_smoothed) on the chain's cell lists, up to nmax angles per
    cell in its own outputs."""

    @staticmethod
    def check(cfg):
        if cfg.ss_len is not None and not 2 <= int(cfg.ss_len) <= _lib.SS_MAX_L:
            raise ValueError(f'ss_len must lie in [2, {_lib.SS_MAX_L}], not {cfg.ss_len!r}')
        if int(cfg.ss_max) < 1:
            raise ValueError(f'ss_max must be >= 1, not {cfg.ss_max!r}')
        if not 0 <= int(cfg.ss_sources) <= int(cfg.ss_max):
            raise ValueError(f'ss_sources must lie in [0, ss_max], not {cfg.ss_sources!r}')
        if not 0.0 < float(cfg.ss_rel) < 1.0:
            raise ValueError(f'ss_rel must lie in (0, 1), not {cfg.ss_rel!r}')
        if cfg.multi_source:
            A = int(cfg.num_antennas)
            if not 3 <= A <= 16:
                raise ValueError(f'multi_source needs 3 to 16 antennas, not {A}')
            L = cfg.ss_sub_len
            if L > A:
                raise ValueError(f'ss_len {L} exceeds the {A} antennas')
            if int(cfg.ss_sources) > min(int(cfg.ss_max), L - 1):
                raise ValueError(f'ss_sources {cfg.ss_sources} exceeds the {L - 1} angles a sub-array of {L} resolves')

    def __init__(self, ch):
        cfg, e, torch, cc, L = ch.cfg, ch.alloc, ch.ctx.torch, ch.cell_cap, ch.cfg.ss_sub_len
        self.ch = ch
        self.nmax = min(int(cfg.ss_max), L - 1)
        self.steer = ch.ctx.steering_sub(ch.steer_c128, L)
        self.out = dict(nsrc=e((cc,), torch.int32), idx=e((cc, self.nmax), torch.int32),
                        den=e((cc, self.nmax), torch.float32))
        self.kw = dict(steer_sub=self.steer, nmax=self.nmax, num_sources=cfg.ss_sources, rel=cfg.ss_rel, out=self.out)

    def launch(self, **over):
        return self.ch.ctx.doa_smoothed(**{**self.ch.cells(), **self.kw, **over})

    def results(self, nc):
        o = self.out
        return dict(ss_nsrc=o['nsrc'][:nc].cpu().numpy(), ss_gidx=o['idx'][:nc].cpu().numpy().astype(np.int64),
                    ss_den=o['den'][:nc].cpu().numpy().astype(np.float64))


class RangeAzimuth:
    """cfg.ra_map: every range bin's spatial covariance over its Doppler window (cov(): range_cov), then its Bartlett
    or Capon power over the chain's grid (launch(): range_azimuth on that covariance)."""

    @staticmethod
    def check(cfg):
        if cfg.ra_map is not None and cfg.ra_map not in _lib.RA_IDS:
            raise ValueError(f"ra_map must be None, 'bartlett' or 'capon', not {cfg.ra_map!r}")
        if cfg.ra_doppler is not None:
            if len(tuple(cfg.ra_doppler)) != 2 or not (0 <= int(cfg.ra_doppler[0]) < int(cfg.ra_doppler[1])
                                                       <= int(cfg.num_chirps)):
                raise ValueError(f'ra_doppler must be (c0, c1) with 0 <= c0 < c1 <= {int(cfg.num_chirps)}, '
                                 f'not {cfg.ra_doppler!r}')
        if not _lib.RA_MIN_LOADING <= float(cfg.ra_loading) <= 1.0:
            raise ValueError(f'ra_loading must lie in [{_lib.RA_MIN_LOADING}, 1], not {cfg.ra_loading!r}')
        if cfg.ra_map is not None and not 2 <= int(cfg.num_antennas) <= _lib.RA_MAX_A:
            raise ValueError(f'ra_map needs 2 to {_lib.RA_MAX_A} antennas, not {cfg.num_antennas}')

    def __init__(self, ch):
        cfg, e, torch, F, A, S = ch.cfg, ch.alloc, ch.ctx.torch, ch.F, ch.A, ch.S
        self.ch = ch
        self.steer = ch.ctx.steering_c64(ch.steer_c128)
        self.win = (0, ch.C) if cfg.ra_doppler is None else (int(cfg.ra_doppler[0]), int(cfg.ra_doppler[1]))
        self.cov_out = e((F, S, A, A), torch.complex64)
        self.out = dict(map=e((F, S, len(ch.grid)), torch.float32), arg=e((F, S), torch.int32))
        self.kw = dict(cov=self.cov_out, steer_c64=self.steer, method=cfg.ra_map, loading=cfg.ra_loading, out=self.out)

    def cov(self, **over):
        return self.ch.ctx.range_cov(**{'rds': self.ch.rds, 'doppler': self.win, 'out': self.cov_out, **over})

    def launch(self, with_cov=True, **over):
        """with_cov=False: the map alone, on the covariance as it stands."""
        if with_cov:
            self.cov()
        return self.ch.ctx.range_azimuth(**{**self.kw, **over})

    def results(self, nc):  # f32 [F, S, G] and i32 [F, S]: every range bin of every frame
        return dict(ra_map=self.out['map'].cpu().numpy(), ra_arg=self.out['arg'].cpu().numpy())


class PowerSum:
    """The antenna-summed power map chain.power (integrate_power): what the 'sum' detector decides on and what the
    point cloud refines on, integrated once per run, before whichever comes first."""

    def __init__(self, ch):
        self.ch = ch
        self.out = ch.alloc((ch.F, ch.S, ch.C), ch.ctx.torch.float32)

    def launch(self, **over):
        return self.ch.ctx.integrate_power(**{'rds': self.ch.rds, 'out': self.ch.power, **over})


class PointCloud:
    """cfg.point_cloud: one row and one refined azimuth per cell (cell_refine, after the DoA scan), from the
    antenna-summed power map chain.power."""

    @staticmethod
    def check(cfg):
        if cfg.velocity_az not in ('grid', 'refined'):
            raise ValueError(f"velocity_az must be 'grid' or 'refined', not {cfg.velocity_az!r}")
        if cfg.velocity_az == 'refined' and not cfg.point_cloud:
            raise ValueError("velocity_az='refined' needs point_cloud=True")
        if cfg.point_cloud:
            if not 2 <= int(cfg.num_antennas) <= 32:
                raise ValueError(f'point_cloud needs 2 to 32 antennas, not {cfg.num_antennas}')
            tables.refine_mode_for_window(cfg.window_type)  # ValueError for a window without an estimator

    def __init__(self, ch):
        cfg, e, torch, cc = ch.cfg, ch.alloc, ch.ctx.torch, ch.cell_cap
        self.ch = ch
        self.steer = ch.ctx.steering_c64(ch.steer_c128)
        self.modes = (tables.refine_mode_for_window(cfg.window_type), 'rect')
        self.axes = tables.point_axes(cfg, ch.S, ch.C, velocity=cfg.pc_velocity)
        self.out = dict(points=e((cc, 8), torch.float32), az=e((cc,), torch.float64))
        self.kw = dict(az_table=ch.az_table, steer_c64=self.steer, range_mode=self.modes[0],
                       doppler_mode=self.modes[1], axes=self.axes, out=self.out)

    def launch(self, **over):
        ch = self.ch
        return ch.ctx.cell_refine(**{**ch.cells(), 'gidx': ch.gidx, 'power': ch.power, **self.kw, **over})

    def results(self, nc):
        return dict(points=self.out['points'][:nc].cpu().numpy(), az_refined=self.out['az'][:nc].cpu().numpy())


class VelocitySolve:
    """The ego-velocity solve: one of the three solvers on the one problem they share, the chain's own lists, with
    the azimuths of the grid (az_table[gidx]) or the point cloud's refined ones."""

    @staticmethod
    def check(cfg):
        if cfg.velocity_loss not in ('ls', 'huber', 'tukey', 'consensus'):
            raise ValueError("velocity_loss must be 'ls', 'huber', 'tukey' or 'consensus', "
                             f'not {cfg.velocity_loss!r}')
        if cfg.velocity_loss == 'consensus':
            if cfg.velocity_scale is None or not float(cfg.velocity_scale) > 0.0:
                raise ValueError("velocity_loss='consensus' needs velocity_scale > 0, the phase-noise sigma in radians")
            if not 1 <= int(cfg.velocity_hyps) <= _lib.CONSENSUS_MAX_H:
                raise ValueError(f'velocity_hyps must lie in [1, {_lib.CONSENSUS_MAX_H}], not {cfg.velocity_hyps!r}')
            if not 0.0 < float(cfg.velocity_min_det) <= 1.0:
                raise ValueError(f'velocity_min_det must lie in (0, 1], not {cfg.velocity_min_det!r}')
            if not 0 <= int(cfg.velocity_refine) <= 100:
                raise ValueError(f'velocity_refine must lie in [0, 100], not {cfg.velocity_refine!r}')

    def __init__(self, ch):
        cfg, loss = ch.cfg, ch.cfg.velocity_loss
        self.ch = ch
        # IRLS weight of every cell ('consensus': the inlier mask)
        self.weight = ch.alloc((ch.cell_cap,), ch.ctx.torch.float32) if loss != 'ls' else None
        prob = dict(k=ch.k, ridge=cfg.ridge, bounds=cfg.bounds, n=ch.cell_cap)
        if cfg.velocity_az == 'refined':  # the point cloud's azimuths in place of the grid's
            prob.update(az=ch.pc.out['az'], gidx=None, az_table=None)
        if loss == 'consensus':
            # vel columns 2-7 become {cost, rmse_in, n_in, n, best_h, n_valid} (include/rsl.h)
            self.call = 'velocity_consensus'
            prob.update(scale=cfg.velocity_scale, c=cfg.velocity_c, hyps=cfg.velocity_hyps, seed=cfg.velocity_seed,
                        min_det=cfg.velocity_min_det, refine=cfg.velocity_refine, frame0=0, want_weight=self.weight)
        elif loss != 'ls':
            # vel columns 2-7 become {cost, rmse_w, n_in, n, sigma, it} (include/rsl.h)
            self.call = 'velocity_robust'
            prob.update(loss=loss, c=cfg.velocity_c, scale=cfg.velocity_scale, iters=cfg.velocity_iters,
                        tol=cfg.velocity_tol, want_weight=self.weight)
        else:
            self.call = 'velocity'
        self.kw = prob

    def launch(self, **over):
        ch = self.ch  # the chain's own lists, on the grid-index path unless .kw says otherwise
        return getattr(ch.ctx, self.call)(**{
            'az': None, 'gidx': ch.gidx, 'az_table': ch.az_table, 'y': ch.ext['phase'], 'seg': ch.offs['cell_base'],
            'amask': ch.lists['c_amask'], 'out': ch.vel, **self.kw, **over})

    def results(self, nc):
        return dict(vel_weight=self.weight[:nc].cpu().numpy()) if self.weight is not None else {}


class Registration:
    """cfg.registration: every frame's point cloud against the frame before it (scan_register, after the velocity
    solve), from the start (0, v_x dt, v_y dt) of the velocity rows; the batch's last frame is kept as the next run's
    reference (.prev: None until a run has filled .keep)."""

    @staticmethod
    def check(cfg):
        if not cfg.registration:
            return
        if not cfg.point_cloud:
            raise ValueError('registration=True needs point_cloud=True')
        pos = lambda v: math.isfinite(float(v)) and float(v) > 0.0
        if not (pos(cfg.reg_h) and pos(cfg.reg_h_coarse) and pos(cfg.reg_dtheta) and pos(cfg.dt)):
            raise ValueError('registration needs reg_h, reg_h_coarse, reg_dtheta and dt finite and > 0')
        if float(cfg.reg_h_coarse) < float(cfg.reg_h):
            raise ValueError(f'reg_h_coarse {cfg.reg_h_coarse!r} is below reg_h {cfg.reg_h!r}')
        if not 0 <= int(cfg.reg_k) <= _lib.REG_MAX_K:
            raise ValueError(f'reg_k must lie in [0, {_lib.REG_MAX_K}], not {cfg.reg_k!r}')
        if not 0 <= int(cfg.reg_iters) <= _lib.REG_MAX_ITERS:
            raise ValueError(f'reg_iters must lie in [0, {_lib.REG_MAX_ITERS}], not {cfg.reg_iters!r}')
        if not 0.0 < float(cfg.reg_shrink) <= 1.0:
            raise ValueError(f'reg_shrink must lie in (0, 1], not {cfg.reg_shrink!r}')
        if not (math.isfinite(float(cfg.reg_w_min)) and float(cfg.reg_w_min) >= 0.0):
            raise ValueError(f'reg_w_min must be finite and >= 0, not {cfg.reg_w_min!r}')

    def __init__(self, ch):
        cfg, e, torch, F = ch.cfg, ch.alloc, ch.ctx.torch, ch.F
        fc = ch.S * ch.C  # the most cells of one frame
        self.ch = ch
        self.out = dict(rows=e((F, 8), torch.float64), omega=e((F, 3), torch.float64))
        self.init = e((F, 3), torch.float64)
        self.keep = dict(points=e((fc, 8), torch.float32), rc=e((fc,), torch.int32), n_dev=e((1,), torch.int64),
                         weight=e((fc,), torch.float32) if ch.vel_weight is not None else None)
        self.prev = None
        self.idx = torch.arange(fc, dtype=torch.int64, device=ch.ctx.device)
        self.kw = dict(points=ch.pc.out['points'], C=ch.C, axes=ch.pc.axes, init=self.init, h=cfg.reg_h,
                       h_coarse=cfg.reg_h_coarse, dtheta=cfg.reg_dtheta, k=cfg.reg_k, iters=cfg.reg_iters,
                       shrink=cfg.reg_shrink, tol=cfg.reg_tol, w_min=cfg.reg_w_min, dt=cfg.dt, n=ch.cell_cap,
                       out=self.out)

    def launch(self, **over):
        """The start from the velocity rows, the registration of the batch (prev: the kept cloud unless `over` says
        otherwise), then the batch's last frame into .keep."""
        ch, keep, torch = self.ch, self.keep, self.ch.ctx.torch
        points, seg, rc, weight = self.kw['points'], ch.offs['cell_base'], ch.lists['c_rc'], ch.vel_weight
        self.init[:, 0] = 0.0
        torch.mul(ch.vel[:, :2], float(ch.cfg.dt), out=self.init[:, 1:])  # the Doppler displacement v dt
        ch.ctx.scan_register(**{'seg': seg, 'weight': weight, 'rc': rc, 'prev': self.prev, **self.kw, **over})
        # the last frame's rows, by device-side indices (no host synchronisation): rows past the frame's end are
        # copies of the list's last slot and lie beyond n_dev
        base = seg.clamp(0, ch.cell_cap)
        idx = (self.idx + base[ch.F - 1]).clamp_(max=ch.cell_cap - 1)
        torch.index_select(points, 0, idx, out=keep['points'])
        torch.index_select(rc, 0, idx, out=keep['rc'])
        if keep['weight'] is not None:
            torch.index_select(weight, 0, idx, out=keep['weight'])
        torch.sub(base[ch.F:ch.F + 1], base[ch.F - 1:ch.F], out=keep['n_dev'])
        self.prev = keep

    def results(self, nc):
        return dict(registration=self.out['rows'].cpu().numpy())


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
        d = cfg.antenna_spacing or cfg.lambda_c / 2
        self.grid = tables.azimuth_grid(cfg.search_range, cfg.search_resolution)
        self.steer_c128 = tables.steering_matrix(self.grid, np.arange(A) * d, cfg.lambda_c)  # host; the stages' tables
        self.steer = ctx.steering(self.steer_c128)
        self.az_table = ctx.to_dev(np.radians(self.grid).astype(np.float64))
        self.esprit_scale = cfg.lambda_c / (2 * np.pi * d)
        lam_v = cfg.velocity_lambda or cfg.lambda_c
        self.k = 4 * np.pi * cfg.dt / lam_v
        self.method = _lib.METHOD_MUSIC if cfg.method == 'music' else _lib.METHOD_BEAMFORMING
        self.sum = cfg.detect_on == 'sum'
        DA = 1 if self.sum else A  # antenna maps the detector decides on per frame
        self.entry_cap = int(math.ceil(cfg.entry_frac * F * DA * S * C)) + 64
        self.cell_cap = (int(math.ceil(cfg.cell_frac * F * S * C)) + 64 + 3) & ~3  # a multiple of 4 (16-B rows)
        e = self.alloc = self._guarded_empty if guard else ctx.empty  # the stages allocate through it too
        W = (C + 63) // 64
        self.work = e((F, A, C, S), torch.complex64)
        self.rds = e((F, A, S, C), torch.complex64)
        # mask, per-row counts and row-compact peak powers (detect -> emit): rds_detect's, then the detector's
        front = dict(mask=e((F, A, S, W), torch.int64), row_count=e((F, A, S), torch.int32),
                     peak_pow=e((F, A, S, C), torch.float32))
        integrate = PowerSum(self) if self.sum or cfg.point_cloud else None
        self.power = integrate.out if integrate is not None else None
        self.det = Detector(self, front)
        self.mask, self.row_count, self.peak_pow = (self.det.out[k] for k in ('mask', 'row_count', 'peak_pow'))
        self.cfar_alpha = self.det.alpha
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
        self.ncell_dev = self.offs['cell_base'][F:F + 1]
        # the stages, in launch order.  One signature gather for DoA + ESPRIT + phase when the Toeplitz path applies
        # (uniform linear array)
        self.fused_doa = bool(self.steer['toeplitz']) and A >= 2 and not cfg.spectrum
        self.doa = (FusedDoa if self.fused_doa else ScanDoa)(self, spec_out)
        self.spec, self.spec_contiguous = self.doa.spec, self.doa.spec_contiguous
        self.ss = SmoothedMusic(self) if cfg.multi_source else None
        self.ra = RangeAzimuth(self) if cfg.ra_map is not None else None
        self.pc = PointCloud(self) if cfg.point_cloud else None
        self.solve = VelocitySolve(self)
        self.vel_weight = self.solve.weight
        self.reg = Registration(self) if cfg.registration else None
        self.omega = self.reg.out['omega'] if self.reg is not None else None
        on = lambda *stages: [st for st in stages if st is not None]
        self.detect = on(integrate if self.sum else None, self.det if self.det.call else None)
        self.before_solve = on(self.ss, self.ra, None if self.sum else integrate, self.pc)
        self.after_solve = on(self.reg)

    def cells(self):
        """What every per-cell launch reads: the RDS, the cell lists, their capacity and true size (on the device)."""
        L = self.lists
        return dict(rds=self.rds, c_frame=L['c_frame'], c_rc=L['c_rc'], n=self.cell_cap, n_dev=self.ncell_dev)

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

    def _offsets(self):
        self.ctx.offsets(self.mask, self.row_count, self.C, bufs=self.offs)

    def run_front(self, cube, *, emit: bool = True, offsets: bool = True):
        """Memory-bound half: RDS + detection, offsets, peak / cell compaction (current stream). With emit=False the
        compaction is left to run_back(emit=True) (a pipelining split of the same work)."""
        if self.F == 0:  # empty batch: only the (zeroed) bases
            self._offsets()
            return
        group = self.ctx.rds_detect(cube, self.table, self.thr_p, self.i_lo, self.i_hi, rds=self.rds, work=self.work,
                                    dc_removal=self.cfg.dc_removal, **self.det.front)
        for st in self.detect:
            st.launch()
        self._group = 1 if self.detect else group  # peak_pow's row grouping: 1 once a detector has rewritten it
        if offsets:
            self._offsets()
        if emit:
            self._emit()

    def _emit(self):
        self.ctx.emit(self.rds, self.mask, self.offs, self.entry_cap, self.cell_cap, want_pdb=True, bufs=self.lists,
                      peak_pow=self.peak_pow, peak_pow_group=self._group)

    def run_back(self, *, esprit: bool = True, velocity: bool = True, emit: bool = False, offsets: bool = False):
        """Compute-bound half: DoA scan (+ ESPRIT, phase), the optional stages and the velocity solve, on run_front's
        lists (emit=True: the compaction first, after run_front(emit=False))."""
        if self.F == 0:
            return
        if offsets:
            self._offsets()
        if emit:
            self._emit()
        self.doa.launch(esprit=esprit, velocity=velocity)
        for st in self.before_solve:
            st.launch()
        if not velocity:
            return
        self.solve.launch()
        for st in self.after_solve:
            st.launch()

    def reset_registration(self):
        """Forget the cloud kept from the last run: the next run's frame 0 has no reference (flag 2)."""
        if self.reg is not None:
            self.reg.prev = None

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
        extra = {}
        for st in (self.ss, self.ra, self.pc, self.solve, self.reg):
            extra.update(st.results(nc) if st is not None else {})
        return dict(entry_base=self.offs['entry_base'].cpu().numpy(), cell_base=self.offs['cell_base'].cpu().numpy(),
                    **dict(zip(('e_ant', 'e_rbin', 'e_dbin'), unpack_coord(h(L['e_coord'], ne)))),
                    e_cell=h(L['e_cell'], ne), e_pdb=h(L['e_pdb'], ne).astype(np.float64), c_frame=h(L['c_frame'], nc),
                    c_rc=h(L['c_rc'], nc), c_amask=h(L['c_amask'], nc), gidx=h(self.gidx, nc),
                    esprit=h(self.ext['esprit'], nc), phase=h(self.ext['phase'], nc),
                    az=np.radians(self.grid)[h(self.gidx, nc)],
                    velocity=self.vel.cpu().numpy(), grid=self.grid, **extra)
