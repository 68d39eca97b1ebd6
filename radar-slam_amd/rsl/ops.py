"""Per-call device operations with host (numpy) inputs/outputs, used by the reference-compatible classes.

Each function uploads its operands, launches librsl kernels on the context's device, and returns numpy
arrays in the reference's dtypes (complex128 / float64 upcast from the fp32 device results where the
kernel computes in fp32).  Device tensors (torch) are accepted wherever an RDS/cube is expected and are
then used in place without a copy.
"""
from __future__ import annotations

import math
from ctypes import c_double
from typing import Optional, Sequence, Tuple

import numpy as np

from . import _lib, tables
from .runtime import POINT_COLUMNS, Context, emit_compact_supported, get_context, unpack_coord


def _ctx(ctx: Optional[Context]) -> Context:
    return ctx or get_context()


def _is_dev(x) -> bool:
    return hasattr(x, 'is_cuda') and bool(getattr(x, 'is_cuda', False))


def as_dev_c64(ctx: Context, x):
    torch = ctx.torch
    if _is_dev(x):
        return x if x.dtype == torch.complex64 else x.to(torch.complex64)
    a = np.asarray(x)
    if not np.iscomplexobj(a):
        a = a.astype(np.complex128)
    return ctx.to_dev(a.astype(np.complex64))


def dev(ctx: Context, x, dtype, npdtype):
    """x (None, a host array or a device tensor) as a contiguous device tensor of `dtype` (npdtype on the host)."""
    if x is None:
        return None
    if _is_dev(x):
        return (x if x.dtype == dtype else x.to(dtype)).contiguous()
    return ctx.to_dev(np.ascontiguousarray(np.asarray(x, dtype=npdtype)))


def to_host(t, dtype=None):
    a = t.cpu().numpy()
    return a.astype(dtype) if dtype is not None else a


# -- a3..a7 --------------------------------------------------------------------------------------------
def preprocess_rows(rows, table: np.ndarray, dc: bool, ctx: Optional[Context] = None) -> np.ndarray:
    """rows [..., S] * table[S], then optional complex-mean removal per row (dechirp.py:108,120,139)."""
    c = _ctx(ctx)
    a = np.asarray(rows)
    shape = a.shape
    S = shape[-1]
    if np.asarray(table).shape[0] != S:
        raise ValueError(f"operands could not be broadcast together with shapes ({S},) ({np.asarray(table).shape[0]},) ")
    d_in = as_dev_c64(c, a.reshape(-1, S))
    d_tab = c.to_dev(np.asarray(table, dtype=np.complex128).astype(np.complex64))
    out = c.empty(d_in.shape, c.torch.complex64)
    c.call('rsl_preprocess_rows', d_in, d_in.shape[0], S, d_tab, dc, out)
    return to_host(out, np.complex128).reshape(shape)


def range_doppler(frames, table: np.ndarray, *, chirp0=0, num_chirps=None, dc_removal=True,
                  ctx: Optional[Context] = None, keep_on_device=False):
    """frames [A, C, S] or [F, A, C, S] -> RDS [.., A, S, C] (c128 host, or c64 device tensor)."""
    c = _ctx(ctx)
    single = (frames.ndim == 3)
    d = as_dev_c64(c, frames)
    if single:
        d = d.unsqueeze(0)
    d = d.contiguous()
    d_tab = c.to_dev(np.asarray(table).astype(np.complex64))
    rds = c.rds(d, d_tab, chirp0=chirp0, num_chirps=num_chirps, dc_removal=dc_removal)
    if keep_on_device:
        return rds[0] if single else rds
    out = to_host(rds, np.complex128)
    return out[0] if single else out


# -- a8 -------------------------------------------------------------------------------------------------
def _dev_rds4(c: Context, rds):
    """rds [A, S, C] or [F, A, S, C] -> the contiguous complex64 device tensor [F, A, S, C] (F = 1 for three axes)."""
    d = as_dev_c64(c, rds)
    if d.dim() == 3:
        d = d.unsqueeze(0)
    return d.contiguous()


def _peak_result(c: Context, d, mask, rc, db, want_db, peak_pow=None, pdb_from_db=False):
    """The peak dictionary of detect_peaks from a detector's outputs (mask, row_count, dB map) on the device RDS d:
    offsets, emit and the host unpack.  power_db is the emit's; with pdb_from_db it is gathered from the dB map."""
    F, C = d.shape[0], d.shape[3]
    offs = c.offsets(mask, rc, C)
    ne = int(offs['entry_base'][F].item())
    nc = int(offs['cell_base'][F].item())
    lists = c.emit(d, mask, offs, ne, nc, want_pdb=not pdb_from_db, peak_pow=peak_pow)
    ant, rbin, dbin = unpack_coord(to_host(lists['e_coord'][:ne]))
    if pdb_from_db:
        fr = np.searchsorted(to_host(offs['entry_base']), np.arange(ne), side='right') - 1
        pdb = to_host(db, np.float64)[fr, 0, rbin, dbin]
    else:
        pdb = to_host(lists['e_pdb'][:ne], np.float64)
    res = dict(antenna=ant.astype(np.int64), range_bin=rbin.astype(np.int64), doppler_bin=dbin.astype(np.int64),
               power_db=pdb, entry_base=to_host(offs['entry_base']), cells=nc)
    if want_db:
        res['power_spectrum_db'] = to_host(db, np.float64)
        if F == 1:
            res['power_spectrum_db'] = res['power_spectrum_db'][0]
    return res


def _detect_peaks(rds, ctx: Optional[Context], want_db, detector):
    """The peak dictionary of detect_peaks from ``detector(c, d)`` -> (mask, row_count, dB map) on the device RDS d."""
    c = _ctx(ctx)
    d = _dev_rds4(c, rds)
    mask, rc, db = detector(c, d)
    return _peak_result(c, d, mask, rc, db, want_db)


def detect_peaks(rds, *, threshold_db=-20.0, i_lo=0, i_hi=1 << 30, want_db=True, ctx: Optional[Context] = None):
    """rds [A, S, C] -> (antenna, range_bin, doppler_bin, power_db) arrays in reference order + dB map."""
    return _detect_peaks(rds, ctx, want_db, lambda c, d: c.detect(d, tables.power_threshold(threshold_db), i_lo, i_hi,
                                                                  want_db=want_db))


def detect_peaks_cfar(rds, *, guard=(2, 2), train=(8, 8), pfa=1e-4, alpha=None, threshold_db=-math.inf, i_lo=0,
                      i_hi=1 << 30, want_db=True, ctx: Optional[Context] = None, method='ca', rank=0.75):
    """rds [A, S, C] -> the dictionary of detect_peaks, with a CFAR detector in place of the fixed threshold: guard /
    train (range, doppler) half-sizes; threshold_db remains as a floor (-inf: none).
    method 'ca' (rsl_detect_cfar): alpha on the training mean (default: from pfa and the full-window count,
    tables.cfar_alpha).  method 'os' (rsl_detect_oscfar): alpha on the training cells' order statistic of rank
    ceil(rank * cells) (default: tables.os_cfar_alpha for the full window)."""
    if method not in tables.CFAR_METHODS:
        raise ValueError(f"method must be 'ca' or 'os', not {method!r}")
    thr = tables.power_threshold(threshold_db)
    if alpha is None:
        alpha = tables.cfar_design_alpha(method, pfa, guard, train, rank)
    return _detect_peaks(rds, ctx, want_db, lambda c, d: c.detect_cfar(d, guard, train, alpha, thr, i_lo, i_hi,
                                                                       want_db=want_db, method=method, rank=rank))


# -- non-coherent integration: detection on the antenna-summed power map --------------------------------
def integrate_power(rds, ctx: Optional[Context] = None, keep_on_device=False):
    """rds [A, S, C] or [F, A, S, C] -> the antenna-summed power map [S, C] or [F, S, C] (rsl_power_integrate: fp32
    sum of |rds|^2 over the antennas in antenna order; float64 host array, or the float32 device tensor)."""
    c = _ctx(ctx)
    single = (rds.ndim == 3)
    p = c.integrate_power(_dev_rds4(c, rds))
    if not keep_on_device:
        p = to_host(p, np.float64)
    return p[0] if single else p


def detect_peaks_integrated(rds, *, detector='cfar', method='ca', rank=0.75, guard=(2, 2), train=(8, 8), pfa=1e-4,
                            alpha=None, threshold_db=-math.inf, i_lo=0, i_hi=1 << 30, want_db=True,
                            ctx: Optional[Context] = None):
    """rds [A, S, C] -> the dictionary of detect_peaks, detected once on the antenna-summed power map instead of once
    per antenna (rsl_power_integrate + rsl_detect_power).  detector 'cfar': method 'ca' / 'os' as detect_peaks_cfar,
    alpha from pfa for a sum of A looks (tables.cfar_design_alpha(..., looks=A)) unless given, threshold_db a floor on
    the summed power (-inf: none); detector 'threshold': the fixed threshold_db on the summed power.  Every peak is
    one entry: antenna is all zeros, power_db is that of the summed power and power_spectrum_db is [1, S, C]."""
    if detector not in ('threshold', 'cfar'):
        raise ValueError(f"detector must be 'threshold' or 'cfar', not {detector!r}")
    if method not in tables.CFAR_METHODS:
        raise ValueError(f"method must be 'ca' or 'os', not {method!r}")
    c = _ctx(ctx)
    d = _dev_rds4(c, rds)
    F, A, S, C = d.shape
    rule = 'threshold' if detector == 'threshold' else method
    if alpha is None:
        alpha = tables.cfar_design_alpha(method, pfa, guard, train, rank, looks=A) if detector == 'cfar' else 1.0
    power = c.integrate_power(d)
    pk = c.empty((F, 1, S, C), c.torch.float32)
    # without the compact path emit would recompute power_db from the RDS: gather it from the dB map instead
    on_dev = emit_compact_supported(C, True, True, True)
    mask, rc, db = c.detect_power(power, rule, guard, train, rank, alpha, tables.power_threshold(threshold_db), i_lo,
                                  i_hi, want_db=want_db or not on_dev, out=dict(peak_pow=pk))
    return _peak_result(c, d, mask, rc, db, want_db, peak_pow=pk, pdb_from_db=not on_dev)


# -- signatures as a pseudo-RDS [N, A, 1, 1] -------------------------------------------------------------
def _sig_cells(c: Context, sigs: np.ndarray):
    torch = c.torch
    s = np.atleast_2d(np.asarray(sigs))
    N, A = s.shape
    d = as_dev_c64(c, s.reshape(N, A, 1, 1)).contiguous()
    fr = c.to_dev(np.arange(N, dtype=np.int32))
    rc = c.to_dev(np.zeros(N, dtype=np.int32))
    return d, fr, rc, N


def _rds_cells(c: Context, rds, rbins, dbins):
    d = _dev_rds4(c, rds)
    _, A, S, C = d.shape
    rb = np.asarray(rbins, dtype=np.int64)
    db = np.asarray(dbins, dtype=np.int64)
    if rb.size and (rb.min() < 0 or rb.max() >= S or db.min() < 0 or db.max() >= C):
        raise IndexError('range/doppler bin out of bounds')
    fr = c.to_dev(np.zeros(rb.size, dtype=np.int32))
    rc = c.to_dev((rb * C + db).astype(np.int32))
    return d, fr, rc, int(rb.size)


def doa(method: str, steer_c128: np.ndarray, *, sigs=None, rds=None, rbins=None, dbins=None, want_spec=False,
        ctx: Optional[Context] = None):
    """Argmax grid index (+ optional f64 spectrum [N, G]) for MUSIC / beamforming; signatures either given
    explicitly ([N, M], normalised in-kernel as the reference does) or gathered from an RDS."""
    c = _ctx(ctx)
    if sigs is not None:
        d, fr, rc, N = _sig_cells(c, sigs)
    else:
        d, fr, rc, N = _rds_cells(c, rds, rbins, dbins)
    if N == 0:
        return np.zeros(0, np.int64), (np.zeros((0, steer_c128.shape[0])) if want_spec else None)
    st = c.steering(steer_c128)
    m = _lib.METHOD_MUSIC if method == 'music' else _lib.METHOD_BEAMFORMING
    idx, _, spec = c.doa(d, fr, rc, st, m, n=N, want_spec=want_spec)
    return to_host(idx[:N]).astype(np.int64), (to_host(spec[:N], np.float64) if want_spec else None)


def doa_smoothed(steer_c128: np.ndarray, *, sigs=None, rds=None, rbins=None, dbins=None, sub_len=None, num_sources=0,
                 rel=0.05, nmax=3, want_eig=False, want_spec=False, grid_deg=None, ctx: Optional[Context] = None):
    """Spatially smoothed MUSIC (rsl_doa_smoothed, specified in include/rsl.h): up to nmax angles per cell from one
    snapshot of a uniform linear array with the [G, M] steering matrix steer_c128; signatures given ([N, M]) or
    gathered from an RDS.  sub_len=None: tables.default_sub_len(M); nmax is lowered to sub_len - 1 where it exceeds
    it.  num_sources=0 estimates the order per cell as the number of eigenvalues >= rel * the largest: rel depends on
    the SNR, and forward-backward smoothing leaves some relative phases of two coherent sources close to rank 1, so a
    fixed num_sources is the dependable setting.  Returns a dict of host arrays: nsrc i32 [N], gidx i64 [N, nmax] (-1
    where a slot is empty), deg f64 [N, nmax] (grid_deg[gidx]; without grid_deg the angle of a half-wavelength array
    with that phase step; NaN where empty), den f64 [N, nmax] (null spectrum at the pick, ascending), and on request
    eig f64 [N, L] (descending) and spec f64 [N, G] (the whole null spectrum; MUSIC's pseudo-spectrum is 1 / spec)."""
    c = _ctx(ctx)
    st = np.asarray(steer_c128)
    G, M = st.shape
    L = tables.default_sub_len(M) if sub_len is None else int(sub_len)
    if not 3 <= M <= 16:
        raise ValueError(f'doa_smoothed: {M} antennas outside [3, 16]')
    if not 2 <= L <= min(M, _lib.SS_MAX_L):
        raise ValueError(f'doa_smoothed: sub_len {L} outside [2, {min(M, _lib.SS_MAX_L)}]')
    nmax, num_sources = min(int(nmax), L - 1), int(num_sources)
    if not 1 <= nmax <= L - 1:
        raise ValueError(f'doa_smoothed: nmax {nmax} outside [1, {L - 1}]')
    if not 0 <= num_sources <= nmax:
        raise ValueError(f'doa_smoothed: num_sources {num_sources} outside [0, {nmax}]')
    if not 0.0 < float(rel) < 1.0:
        raise ValueError(f'doa_smoothed: rel {rel} outside (0, 1)')
    if G < 3:
        raise ValueError('doa_smoothed: at least 3 grid points')
    sub = c.steering_sub(st, L)
    if sigs is not None:
        if np.atleast_2d(np.asarray(sigs)).shape[1] != M:
            raise ValueError(f'doa_smoothed: signatures of {np.atleast_2d(np.asarray(sigs)).shape[1]} antennas, '
                             f'steering matrix of {M}')
        d, fr, rc, N = _sig_cells(c, sigs)
    else:
        d, fr, rc, N = _rds_cells(c, rds, rbins, dbins)
        if d.shape[1] != M:
            raise ValueError(f'doa_smoothed: RDS of {d.shape[1]} antennas, steering matrix of {M}')
    if grid_deg is None:
        psi = np.angle(st[:, 1] * st[:, 0].conj())
        grid_deg = np.degrees(np.arcsin(np.clip(psi / np.pi, -1.0, 1.0)))
    grid_deg = np.asarray(grid_deg, np.float64)
    if N == 0:
        res = dict(nsrc=np.zeros(0, np.int32), gidx=np.zeros((0, nmax), np.int64), deg=np.zeros((0, nmax)),
                   den=np.zeros((0, nmax)))
        if want_eig:
            res['eig'] = np.zeros((0, L))
        if want_spec:
            res['spec'] = np.zeros((0, G))
        return res
    nsrc, idx, den, eig, spec = c.doa_smoothed(d, fr, rc, sub, n=N, nmax=nmax, num_sources=num_sources, rel=rel,
                                               want_eig=want_eig, want_spec=want_spec)
    gi = to_host(idx[:N]).astype(np.int64)
    res = dict(nsrc=to_host(nsrc[:N]), gidx=gi, deg=np.where(gi >= 0, grid_deg[np.clip(gi, 0, None)], np.nan),
               den=to_host(den[:N], np.float64))
    if want_eig:
        res['eig'] = to_host(eig[:N], np.float64)
    if want_spec:
        res['spec'] = to_host(spec[:N], np.float64)
    return res


# -- range-azimuth maps: per-range covariance, Bartlett and Capon ----------------------------------------
def _ra_check_rds(fn: str, rds, doppler):
    """Shape, antenna-count and window checks of an RDS [A, S, C] or [F, A, S, C]; returns the window (c0, c1)."""
    shape = tuple(int(d) for d in rds.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f'{fn}: rds must be [A, S, C] or [F, A, S, C], not {len(shape)} axes')
    A, S, C = shape[-3:]
    if not 2 <= A <= _lib.RA_MAX_A:
        raise ValueError(f'{fn}: {A} antennas outside [2, {_lib.RA_MAX_A}]')
    if S < 1 or C < 1:
        raise ValueError(f'{fn}: empty range or Doppler axis {shape}')
    c0, c1 = (0, C) if doppler is None else (int(doppler[0]), int(doppler[1]))
    if not 0 <= c0 < c1 <= C:
        raise ValueError(f'{fn}: Doppler window ({c0}, {c1}) outside 0 <= c0 < c1 <= {C}')
    return c0, c1


def range_covariance(rds, doppler=None, ctx: Optional[Context] = None, keep_on_device=False):
    """rds [A, S, C] or [F, A, S, C] -> the multi-snapshot spatial covariance of every range bin, [S, A, A] or
    [F, S, A, A] (rsl_range_cov): the mean of x x^H over the Doppler bins doppler = (c0, c1) (None: all), accumulated
    in fp32 and exactly Hermitian.  complex128 host array, or the complex64 device tensor."""
    win = _ra_check_rds('range_covariance', rds, doppler)
    c = _ctx(ctx)
    single = len(rds.shape) == 3
    cov = c.range_cov(_dev_rds4(c, rds), win)
    if not keep_on_device:
        cov = to_host(cov, np.complex128)
    return cov[0] if single else cov


def range_azimuth_map(steer_c128: np.ndarray, *, rds=None, cov=None, method='capon', doppler=None, loading=1e-2,
                      want_arg=False, ctx: Optional[Context] = None):
    """The range-azimuth power map (rsl_range_azimuth, specified in include/rsl.h) over the grid of the [G, A]
    steering matrix steer_c128 (any array geometry), from an RDS [A, S, C] / [F, A, S, C] (its per-range covariance
    over the Doppler window is formed first, rsl_range_cov) or from given Hermitian covariances cov [.., A, A].
    method 'bartlett': a^H R a / A^2; 'capon': 1 / (a^H R_l^-1 a) with R_l = R + loading (tr R / A) I, loading in
    [1e-4, 1].  Returns a dict of host arrays: map f64 [.., S, G] ([.., G] from cov), arg i64 (the first-index argmax
    of every row, on request) and, when computed from an RDS, cov c128 [.., S, A, A]."""
    st = np.asarray(steer_c128)
    if st.ndim != 2 or st.shape[0] < 1:
        raise ValueError('range_azimuth_map: steer_c128 must be [G, A] with G >= 1')
    G, A = st.shape
    if method not in _lib.RA_IDS:
        raise ValueError(f"range_azimuth_map: method must be 'bartlett' or 'capon', not {method!r}")
    if not _lib.RA_MIN_LOADING <= float(loading) <= 1.0:
        raise ValueError(f'range_azimuth_map: loading {loading} outside [{_lib.RA_MIN_LOADING}, 1]')
    if (rds is None) == (cov is None):
        raise ValueError('range_azimuth_map: give exactly one of rds and cov')
    if not 2 <= A <= _lib.RA_MAX_A:
        raise ValueError(f'range_azimuth_map: {A} antennas outside [2, {_lib.RA_MAX_A}]')
    if rds is not None:
        win = _ra_check_rds('range_azimuth_map', rds, doppler)
        if int(rds.shape[-3]) != A:
            raise ValueError(f'range_azimuth_map: RDS of {int(rds.shape[-3])} antennas, steering matrix of {A}')
    else:
        shape = tuple(int(d) for d in cov.shape)
        if len(shape) < 2 or shape[-1] != shape[-2]:
            raise ValueError(f'range_azimuth_map: cov must be [.., A, A], not {shape}')
        if shape[-1] != A:
            raise ValueError(f'range_azimuth_map: covariances of {shape[-1]} antennas, steering matrix of {A}')
    c = _ctx(ctx)
    res = {}
    if rds is not None:
        single = len(rds.shape) == 3
        d_cov = c.range_cov(_dev_rds4(c, rds), win)
        if single:
            d_cov = d_cov[0]
        res['cov'] = to_host(d_cov, np.complex128)
    else:
        d_cov = as_dev_c64(c, cov).contiguous()
        if d_cov.dim() == 2:
            d_cov = d_cov.unsqueeze(0)
    m, arg = c.range_azimuth(d_cov, c.steering_c64(st), method, loading=loading, want_arg=want_arg)
    if rds is None and len(cov.shape) == 2:
        m, arg = m[0], (arg[0] if arg is not None else None)
    res['map'] = to_host(m, np.float64)
    if want_arg:
        res['arg'] = to_host(arg).astype(np.int64)
    return res


def subspace_music(sigs, steer_c128: np.ndarray, num_sources: int, ctx: Optional[Context] = None) -> np.ndarray:
    """MUSIC spectrum f64 [n, G] for any num_sources (angle_estimation.py:109-154; rsl_music_subspace)."""
    c = _ctx(ctx)
    s = np.ascontiguousarray(np.atleast_2d(np.asarray(sigs, dtype=np.complex128)))
    st = np.ascontiguousarray(np.asarray(steer_c128, dtype=np.complex128))
    n, M = s.shape
    G = st.shape[0]
    ds, dst = c.to_dev(s.view(np.float64)), c.to_dev(st.view(np.float64))
    out = c.empty((n, G), c.torch.float64)
    c.call('rsl_music_subspace', ds, n, M, num_sources, dst, G, out)
    return to_host(out)


def subspace_esprit(sigs, num_sources: int, esprit_scale: float, ctx: Optional[Context] = None) -> np.ndarray:
    """ESPRIT angles (deg) f64 [n] for any num_sources (angle_estimation.py:178-225; rsl_esprit_subspace)."""
    c = _ctx(ctx)
    s = np.ascontiguousarray(np.atleast_2d(np.asarray(sigs, dtype=np.complex128)))
    n, M = s.shape
    ds = c.to_dev(s.view(np.float64))
    out = c.empty((n,), c.torch.float64)
    c.call('rsl_esprit_subspace', ds, n, M, num_sources, esprit_scale, out)
    return to_host(out)


def cell_extras(*, sigs=None, rds=None, rbins=None, dbins=None, esprit_scale=1 / math.pi, want_sig=False,
                want_esprit=False, want_phase=False, ctx: Optional[Context] = None):
    c = _ctx(ctx)
    if sigs is not None:
        d, fr, rc, N = _sig_cells(c, sigs)
    else:
        d, fr, rc, N = _rds_cells(c, rds, rbins, dbins)
    if N == 0:
        A = d.shape[1]
        return (np.zeros((0, A), np.complex128) if want_sig else None, np.zeros(0) if want_esprit else None,
                np.zeros(0) if want_phase else None)
    sig, esp, ph, _ = c.cell_extras(d, fr, rc, n=N, esprit_scale=esprit_scale, want_sig=want_sig,
                                    want_esprit=want_esprit, want_phase=want_phase)
    return (to_host(sig[:N], np.complex128) if want_sig else None, to_host(esp[:N]) if want_esprit else None,
            to_host(ph[:N]) if want_phase else None)


def refine_cells(steer_c128: np.ndarray, az_deg_grid, *, rds, rbins, dbins, gidx=None, power=None, method='music',
                 range_mode='hann', doppler_mode='rect', axes=(0.0, 1.0, 0.0, 1.0), ctx: Optional[Context] = None):
    """The point cloud of the cells (rbins, dbins) of an RDS [A, S, C] (rsl_cell_refine, specified in include/rsl.h):
    sub-bin range and Doppler offsets, the azimuth refined below the grid spacing, the position.  steer_c128 [G, A]
    and az_deg_grid [G] describe the scan's grid; gidx=None runs ops.doa(method) first.  power: the antenna-summed map
    [S, C] (ops.integrate_power) or None: formed from the RDS.  axes = (r0, r_step, d0, d_step)
    (tables.point_axes).  Returns a dict of host arrays: the f32 columns POINT_COLUMNS of the row (az in radians),
    'points' f32 [N, 8] (the rows as written), 'az_refined' f64 [N] (radians), 'azimuth_deg' f64 [N] and 'gidx'."""
    c = _ctx(ctx)
    st = np.asarray(steer_c128)
    grid = np.asarray(az_deg_grid, np.float64)
    if st.ndim != 2 or grid.shape != (st.shape[0],):
        raise ValueError('refine_cells: steer_c128 [G, A] and az_deg_grid [G] expected')
    d, fr, rc, N = _rds_cells(c, rds, rbins, dbins)
    if d.shape[1] != st.shape[1]:
        raise ValueError(f'refine_cells: RDS of {d.shape[1]} antennas, steering matrix of {st.shape[1]}')
    if gidx is None:
        gidx, _ = doa(method, st, rds=d, rbins=rbins, dbins=dbins, ctx=c)
    gi = np.asarray(gidx, dtype=np.int32)
    if gi.shape != (N,):
        raise ValueError(f'refine_cells: gidx must have one entry per cell ({N})')
    if N == 0:
        res = {k: np.zeros(0, np.float32) for k in POINT_COLUMNS}
        res.update(points=np.zeros((0, 8), np.float32), az_refined=np.zeros(0), azimuth_deg=np.zeros(0), gidx=gi)
        return res
    pw = None
    if power is not None:
        pw = power if _is_dev(power) else c.to_dev(np.asarray(power, dtype=np.float32))
        pw = pw.reshape(-1, pw.shape[-2], pw.shape[-1]).contiguous()
    pts, az = c.cell_refine(d, fr, rc, c.to_dev(gi), c.to_dev(np.radians(grid)), c.steering_c64(st), n=N, power=pw,
                            range_mode=range_mode, doppler_mode=doppler_mode, axes=axes)
    pts, az = to_host(pts[:N]), to_host(az[:N])
    res = {k: pts[:, i] for i, k in enumerate(POINT_COLUMNS)}
    res.update(points=pts, az_refined=az, azimuth_deg=np.degrees(az), gidx=gi)
    return res


REGISTRATION_COLUMNS = ('theta', 't_x', 't_y', 'support', 'rms', 'peak_ratio', 'updates', 'flag')


def register_scans(points, seg, *, weight=None, rc=None, C: int = 0, axes=None, prev=None, init=None,
                   ctx: Optional[Context] = None, **params):
    """Scan registration of F point clouds, each against the one before it (rsl_scan_register, specified in
    include/rsl.h): points f32 [N, 8] (the rows of refine_cells / the chain's 'points': POINT_COLUMNS; x and y are read),
    seg [F + 1] the frames' first rows (the chain's cell_base), weight [N] or None (the static / moving labels:
    'vel_weight'), rc i32 [N] with C and axes (tables.point_axes) to cull the pair search by range rows, prev: None or
    dict(points, weight, rc) of the cloud frame 0 is registered against, init f64 [F, 3] = (theta, t_x, t_y) start
    values (the Doppler displacement v dt).  params: h, h_coarse, dtheta, k, iters, shrink, tol, w_min, dt
    (Context.scan_register).  Host arrays or device tensors.  Returns a dict of host arrays: 'rows' f64 [F, 8] =
    REGISTRATION_COLUMNS, each column under its name, and 'omega' f64 [F, 3] for rsl_traj_scan
    (omega[f - 1] = {0, 0, theta_f / dt})."""
    c = _ctx(ctx)
    f32, i32 = (c.torch.float32, np.float32), (c.torch.int32, np.int32)
    cols = len(POINT_COLUMNS)
    pts = dev(c, points, *f32)
    if pts.dim() != 2 or int(pts.shape[1]) != cols:
        raise ValueError(f'register_scans: points [N, {cols}] expected')
    sg = dev(c, seg, c.torch.int64, np.int64)
    if sg.dim() != 1 or int(sg.shape[0]) < 1:
        raise ValueError('register_scans: seg [F + 1] expected')
    pv = None
    if prev is not None and prev.get('points') is not None:
        pv = dict(points=dev(c, prev['points'], *f32).reshape(-1, cols), weight=dev(c, prev.get('weight'), *f32),
                  rc=dev(c, prev.get('rc'), *i32), n=prev.get('n'), n_dev=prev.get('n_dev'))
    F = int(sg.shape[0]) - 1
    it = dev(c, init, c.torch.float64, np.float64)
    if it is not None:
        it = it.reshape(F, 3)
    rows, om = c.scan_register(pts, sg, weight=dev(c, weight, *f32), rc=dev(c, rc, *i32), C=C, axes=axes, prev=pv,
                               init=it, **params)
    rows, om = to_host(rows[:F]), to_host(om[:F])
    res = {k: rows[:, i] for i, k in enumerate(REGISTRATION_COLUMNS)}
    res.update(rows=rows, omega=om)
    return res


def grid_map(points, seg, poses, *, weight=None, free: bool = True, ctx: Optional[Context] = None, **params):
    """The grid map of F point clouds seen from F poses (mapping.GridMap; rsl_map_update and rsl_map_logodds, specified
    in include/rsl.h): points f32 [N, 8] (the rows of refine_cells / the chain's 'points': POINT_COLUMNS; x, y and
    power_db are read), seg [F + 1] the frames' first rows, poses f64 [F, 7] = (p_x, p_y, p_z, q_w, q_x, q_y, q_z), weight
    [N] or None (the static / moving labels: 'vel_weight').  params: origin, shape = (ny, nx), cell, r_min, r_max,
    min_db, l_occ, l_free, l_min, l_max (GridMap), checked before any device use.  Host arrays or device tensors.
    Returns a dict of host arrays: hits u32 [ny, nx], free u32 [ny, nx] (None with free=False), logodds f32 [ny, nx],
    stats i32 [F, 4] = {accepted points, hit cells, free cells, flag}."""
    from . import mapping
    mapping.check_params(**params)
    points, seg, poses = (x if _is_dev(x) else np.asarray(x) for x in (points, seg, poses))
    for name, x, cols in (('points', points, len(POINT_COLUMNS)), ('poses', poses, 7)):
        if len(x.shape) != 2 or int(x.shape[1]) != cols:
            raise ValueError(f'grid_map: {name} [*, {cols}] expected')
    F = int(seg.shape[0]) - 1
    if len(seg.shape) != 1 or F < 0 or int(poses.shape[0]) != F:
        raise ValueError('grid_map: seg [F + 1] and poses [F, 7] expected')
    c = _ctx(ctx)
    torch = c.torch
    gm = mapping.GridMap(c, free=free, **params)
    if F > 0:
        gm.update(dev(c, points, torch.float32, np.float32), dev(c, seg, torch.int64, np.int64),
                  dev(c, poses, torch.float64, np.float64), weight=dev(c, weight, torch.float32, np.float32))
    res = gm.results()
    if res['stats'] is None:
        res['stats'] = np.zeros((0, 4), np.int32)
    return res


def confidence(sigs, az_deg: Sequence[float], antenna_positions, lambda_c, ctx: Optional[Context] = None):
    """compute_angle_confidence for N (signature, angle) pairs (robust_angle_estimation.py:88-138)."""
    c = _ctx(ctx)
    d, fr, rc, N = _sig_cells(c, sigs)
    az = np.atleast_1d(np.asarray(az_deg, dtype=np.float64))
    steer = tables.steering_matrix(az, np.asarray(antenna_positions), lambda_c)
    st = c.steering(steer)
    gi = c.to_dev(np.arange(N, dtype=np.int32))
    conf = c.confidence(d, fr, rc, gi, st, N)
    return to_host(conf[:N])


def _pos_ang(c: Context, pos, ang, pad=False):
    """(n, device pos f64 [3 n], device ang f64 [2 n]) of n targets' host positions [n, 3] and angles [n, 2]; with pad
    an empty set still gets valid pointers."""
    pos = np.ascontiguousarray(np.asarray(pos, np.float64).reshape(-1, 3))
    ang = np.ascontiguousarray(np.asarray(ang, np.float64).reshape(-1, 2))
    n = pos.shape[0]
    if pad and not n:
        pos, ang = np.zeros(3), np.zeros(2)
    return n, c.to_dev(pos.reshape(-1)), c.to_dev(ang.reshape(-1))


def phase_model(pos, ang, x6, k, y=None, wrap=False, ridge=0.0, ctx: Optional[Context] = None):
    c = _ctx(ctx)
    n, dp, da = _pos_ang(c, pos, ang, pad=True)
    torch = c.torch
    dx = c.to_dev(np.asarray(x6, np.float64).reshape(6))
    dy = c.to_dev(np.asarray(y, np.float64)) if y is not None and n else None
    pred = c.empty((max(n, 1),), torch.float64)
    resid = c.empty((max(n, 1),), torch.float64) if dy is not None else None
    cost = c.empty((1,), torch.float64) if dy is not None else None
    c.call('rsl_phase_model', dp, da, n, dx, k, dy, wrap, ridge, pred, resid, cost)
    out = dict(pred=to_host(pred[:n]))
    if dy is not None:
        out['resid'] = to_host(resid[:n])
        out['cost'] = float(cost.item())
    return out


def bvls(pos, ang, y, k, lo, hi, ridge=0.0, ctx: Optional[Context] = None):
    """Exact box-constrained linear LS of the 3- or 6-DoF phase model; returns (x, cost)."""
    c = _ctx(ctx)
    n, dp, da = _pos_ang(c, pos, ang)
    nv = len(lo)
    torch = c.torch
    dy = c.to_dev(np.asarray(y, np.float64))
    dlo, dhi = c.to_dev(np.asarray(lo, np.float64)), c.to_dev(np.asarray(hi, np.float64))
    out = c.empty((nv + 1,), torch.float64)
    c.call('rsl_bvls', dp, da, n, dy, k, nv, ridge, dlo, dhi, out)
    o = to_host(out)
    return o[:nv], float(o[nv])


def _vel_segment(cx: Context, az, y, amask):
    """One host segment on the device for the velocity solvers: (az f64 [n], y f64 [n], amask as i32 bits or None,
    seg = [0, n], n)."""
    az = np.ascontiguousarray(np.asarray(az, np.float64).reshape(-1))
    yy = np.ascontiguousarray(np.asarray(y, np.float64).reshape(-1))
    if az.shape != yy.shape:
        raise ValueError(f'az and y must have the same length, not {az.shape[0]} and {yy.shape[0]}')
    n = yy.shape[0]
    pad = lambda a: a if n else np.zeros(1, a.dtype)  # an empty segment still needs a valid pointer
    d_az, d_y = cx.to_dev(pad(az)), cx.to_dev(pad(yy))
    d_m = None
    if amask is not None:
        am = np.asarray(amask).astype(np.int64).reshape(-1)
        if am.shape[0] != n:
            raise ValueError('amask must have the length of y')
        d_m = cx.to_dev(pad((am & 0xffffffff).astype(np.uint32).view(np.int32)))
    return d_az, d_y, d_m, cx.to_dev(np.array([0, n], np.int64)), n


def solve_velocity_robust(az, y, *, k, loss='tukey', c=None, scale=None, iters=30, tol=1e-9, ridge=0.0,
                          bounds=(-50.0, 50.0, -50.0, 50.0), amask=None, ctx: Optional[Context] = None):
    """Huber / Tukey IRLS solve of one host segment (rsl_velocity_robust, one frame): az radians [N], y observed phase
    [N], amask optional antenna masks (multiplicity = popcount).  scale=None estimates sigma from the residuals'
    median (dependable only below roughly 30 % coherent outliers); give the sensor's phase-noise sigma where it is
    known.  Returns the out row by name (velocity [2], cost, rmse_w, num_inliers, num_targets, scale, iterations,
    converged) plus weights and residuals [N]."""
    cx = _ctx(ctx)
    d_az, d_y, d_m, seg, n = _vel_segment(cx, az, y, amask)
    out, w, r = cx.velocity_robust(d_az, d_y, seg, k=k, loss=loss, c=c, scale=scale, iters=iters, tol=tol, ridge=ridge,
                                   bounds=bounds, amask=d_m, n=n, want_weight=True, want_resid=True)
    o = to_host(out)[0]
    return dict(velocity=o[:2].copy(), cost=float(o[2]), rmse_w=float(o[3]), num_inliers=int(o[4]),
                num_targets=int(o[5]), scale=float(o[6]), iterations=int(abs(o[7])), converged=bool(o[7] >= 0),
                weights=to_host(w, np.float64)[:n], residuals=to_host(r)[:n])


def solve_velocity_consensus(az, y, *, k, scale, c=None, hyps=256, min_det=0.1, refine=3, seed=0, ridge=0.0,
                             bounds=(-50.0, 50.0, -50.0, 50.0), amask=None, ctx: Optional[Context] = None):
    """Consensus (RANSAC) solve of one host segment (rsl_velocity_consensus, one frame, frame0 = 0): az radians [N], y
    observed phase [N], amask optional antenna masks (multiplicity = popcount), scale the sensor's phase-noise sigma in
    radians (required; the cut-off is c * scale, c=None: 3.0).  Finds the largest coherent population even where it is
    a minority of the cells.  Returns the out row by name (velocity [2], cost, rmse_in, num_inliers, num_targets,
    best_hypothesis, num_valid) plus weights (the inlier mask) and residuals [N]."""
    cx = _ctx(ctx)
    d_az, d_y, d_m, seg, n = _vel_segment(cx, az, y, amask)
    out, w, r = cx.velocity_consensus(d_az, d_y, seg, k=k, scale=scale, c=c, hyps=hyps, min_det=min_det, refine=refine,
                                      seed=seed, ridge=ridge, bounds=bounds, amask=d_m, n=n, want_weight=True,
                                      want_resid=True)
    o = to_host(out)[0]
    return dict(velocity=o[:2].copy(), cost=float(o[2]), rmse_in=float(o[3]), num_inliers=int(o[4]),
                num_targets=int(o[5]), best_hypothesis=int(o[6]), num_valid=int(o[7]),
                weights=to_host(w, np.float64)[:n], residuals=to_host(r)[:n])


# -- a30 / a31: cross-frame association and wrapped-phase solve ------------------------------------------
def associate(cur_xy, prev_xy, thr: float, ctx: Optional[Context] = None):
    """Greedy nearest-unused association (velocity_solver_improved.py:74-129) on the device.
    Returns (match int64 [Nc] with -1 for none, dist float64 [Nc])."""
    c = _ctx(ctx)
    torch = c.torch
    cur = np.ascontiguousarray(np.asarray(cur_xy, np.float64).reshape(-1, 2))
    prev = np.ascontiguousarray(np.asarray(prev_xy, np.float64).reshape(-1, 2))
    nc, npv = cur.shape[0], prev.shape[0]
    if nc == 0:
        return np.zeros(0, np.int64), np.zeros(0)
    dc = c.to_dev(cur.reshape(-1))
    dp = c.to_dev(prev.reshape(-1)) if npv else None
    scratch = c.empty((max((npv + 31) // 32, 1),), torch.int32)
    match = c.empty((nc,), torch.int32)
    dist = c.empty((nc,), torch.float64)
    c.call('rsl_associate', dc, nc, dp, npv, thr, scratch, match, dist)
    return to_host(match).astype(np.int64), to_host(dist)


def _wrapped_call(c: Context, name, pos, ang, y, k, mode, w, vmax, wmax, prev, lo, hi, nv, own, extra, iters,
                  scratch_bytes):
    """One call of rsl_wrapped_solve / rsl_wrapped_search (name) on host operands: own are the entry point's arguments
    between nv and extra, scratch_bytes(n, lo6, hi6, nextra) its scratch size.  Returns (x6, cost)."""
    torch = c.torch
    n, dp, da = _pos_ang(c, pos, ang)
    ex = None if extra is None else np.ascontiguousarray(np.asarray(extra, np.float64).reshape(-1, 6))
    nextra = 0 if ex is None else ex.shape[0]
    lo6 = (c_double * 6)(*[float(v) for v in lo])
    hi6 = (c_double * 6)(*[float(v) for v in hi])
    nbytes = int(scratch_bytes(n, lo6, hi6, nextra))
    scratch = c.empty(((nbytes + 7) // 8,), torch.float64)
    dy = c.to_dev(np.asarray(y, np.float64))
    dprev = c.to_dev(np.asarray(prev, np.float64).reshape(6)) if prev is not None else None
    dex = c.to_dev(ex.reshape(-1)) if nextra else None
    out = c.empty((8,), torch.float64)
    c.call(name, dp, da, n, dy, k, mode, w, vmax, wmax, dprev, lo6, hi6, nv, *own, dex, nextra, iters, scratch, nbytes,
           out)
    o = to_host(out)
    return o[:6].copy(), float(o[6])


def wrapped_solve(pos, ang, y, k, *, mode: int, lo, hi, nv: int = 6, w: float = 0.01, vmax: float = 50.0,
                  wmax: float = 10.0, prev=None, extra=None, grid_n: int = 512, iters: int = 12,
                  ctx: Optional[Context] = None):
    """Global minimisation of the wrapped-phase cost (rsl_wrapped_solve): mode 0 = Improved regularisation,
    mode 1 = Advanced penalties.  Returns (x6, cost)."""
    c = _ctx(ctx)
    return _wrapped_call(c, 'rsl_wrapped_solve', pos, ang, y, k, mode, w, vmax, wmax, prev, lo, hi, nv, (grid_n,),
                         extra, iters, lambda n, lo6, hi6, nextra: c.lib.rsl_wrapped_scratch_bytes(n, grid_n, nextra))


def wrapped_search(pos, ang, y, k, *, mode: int, lo, hi, nv: int = 6, w: float = 0.01, vmax: float = 50.0,
                   wmax: float = 10.0, prev=None, extra=None, spacing_frac: float = 0.5, nbest: int = 64,
                   iters: int = 12, ctx: Optional[Context] = None):
    """Basin-resolving global minimisation of the wrapped-phase cost (rsl_wrapped_search): 2-D Gauss-Newton in
    (v_x, v_y) from a grid whose spacing is spacing_frac of the wrap period 2 pi / k, then the nv-D refinement from the
    nbest best basins and the extra starts.  Returns (x6, cost)."""
    c = _ctx(ctx)
    # x[2..5] during the 2-D stage: the regulariser's optimum for them (0; with a previous motion, Advanced's temporal
    # term w 0.1 |x - prev|^2 against 10 w v_z^2: v_z = prev_z / 101, w = prev_w)
    base = np.zeros(6)
    if prev is not None and mode == 1:
        p = np.asarray(prev, np.float64).reshape(6)
        base[2] = p[2] * 0.1 / 10.1
        base[3:] = p[3:] if nv == 6 else 0.0
    # at least 64 points per axis (a smooth landscape when k is small, e.g. the pipeline's lambda = fc / c); the width
    # of a collapsed axis (adaptive bounds with lo == hi) does not count: that axis gets one point (search_grid), and
    # the other keeps its own spacing instead of a 32768-point line of starts
    widths = [w for w in (float(hi[0]) - float(lo[0]), float(hi[1]) - float(lo[1])) if w > 1e-9]
    width = min(widths) if widths else 1e-9
    spacing = min(float(spacing_frac) * 2 * math.pi / abs(float(k)), width / 64)

    def scratch_bytes(n, lo6, hi6, nextra):
        nbytes = int(c.lib.rsl_wrapped_search_scratch_bytes(n, lo6, hi6, spacing, int(nbest), nextra))
        if nbytes < 0:
            raise ValueError('rsl_wrapped_search_scratch_bytes: bad arguments')
        return nbytes

    return _wrapped_call(c, 'rsl_wrapped_search', pos, ang, y, k, mode, w, vmax, wmax, prev, lo, hi, nv,
                         (base, spacing, nbest), extra, iters, scratch_bytes)


