"""Device runtime: one librsl handle per (device, stream), torch tensors as device memory (plumbing).

Every function here launches HIP kernels of librsl.so on torch's current stream of the context's
device.  There is no CPU path: constructing a Context without a HIP device raises RuntimeError.
"""
from __future__ import annotations

import ctypes
import math
import threading
from ctypes import byref, c_double, c_float, c_int, c_longlong, c_void_p
from typing import Dict, Optional

import numpy as np

from . import _lib
from . import tables

_P = c_void_p


def unpack_coord(coord: np.ndarray):
    """Host unpack of the emit's packed entries (include/rsl.h RSL_COORD_*): antenna, range_bin, doppler_bin."""
    u = np.asarray(coord).view(np.uint32)
    return ((u >> 26).astype(np.int32), ((u >> 13) & 0x1fff).astype(np.int32), (u & 0x1fff).astype(np.int32))


def emit_compact_supported(C: int, union_mask: bool, peak_pow: bool, want_pdb: bool) -> bool:
    """Whether rsl_peak_emit takes its compact path (power_db from the peak powers) and not the general one, which
    recomputes power_db from the RDS: the rule of emit_compact_supported in csrc/rsl_internal.h."""
    W = (C + 63) // 64
    return bool(union_mask and (peak_pow or not want_pdb) and not W & (W - 1) and W <= 64)


# The columns of a point-cloud row, in order: RSL_POINT_* in include/rsl.h, which also states what a cloud is.
POINT_COLUMNS = ('range', 'doppler', 'az', 'x', 'y', 'power_db', 'range_offset', 'doppler_offset')


def _per_point(fn, t, dtype, rows, what):
    """A per-point array (weight, rc) of fn's cloud: None, or one axis of `dtype` with at least `rows` entries."""
    if t is not None and (t.dtype != dtype or t.dim() != 1 or int(t.shape[0]) < rows):
        raise ValueError(f"{fn}: {what} must be {str(dtype).replace('torch.', '')} with one entry per point")


def check_cloud(fn, points, seg, n, weight, empty, what=''):
    """The one check of a point cloud (include/rsl.h) before fn hands it to the library: points contiguous float32
    [rows, 8]; seg contiguous int64 [F + 1] (None: a cloud without segments, scan_register's prev, what='prev ');
    weight None or float32 with an entry for each of the N = min(n, rows) rows in use.  Shapes and dtypes only, so CPU
    tensors serve; the one allocation, empty((1, 8), float32), stands in for empty points (an empty tensor has no
    address; the functions want one).  Returns (points, N)."""
    import torch
    cols = len(POINT_COLUMNS)
    if points.dim() != 2 or int(points.shape[1]) != cols or points.dtype != torch.float32 or not points.is_contiguous():
        raise ValueError(f"{fn}: {what}points must be contiguous float32 [{'M' if what else 'N'}, {cols}]")
    N = int(points.shape[0]) if n is None else min(int(n), int(points.shape[0]))
    if int(points.shape[0]) == 0:
        points = empty((1, cols), torch.float32)
    if seg is not None and (seg.dtype != torch.int64 or seg.dim() != 1 or int(seg.shape[0]) < 1 or
                            not seg.is_contiguous()):
        raise ValueError(f'{fn}: seg must be contiguous int64 [F + 1]')
    _per_point(fn, weight, torch.float32, N, what + 'weight')
    return points, N


_HIP = None


def _hip():
    """The HIP runtime (libamdhip64, already loaded by torch-ROCm) for the few calls torch does not expose."""
    global _HIP
    if _HIP is None:
        h = ctypes.CDLL('libamdhip64.so')
        h.hipExtMallocWithFlags.argtypes = [ctypes.POINTER(c_void_p), ctypes.c_size_t, ctypes.c_uint]
        h.hipExtMallocWithFlags.restype = c_int
        h.hipFree.argtypes = [c_void_p]
        h.hipFree.restype = c_int
        _HIP = h
    return _HIP


class _DeviceBlock:
    """Owner of a raw device allocation exposed to torch through __cuda_array_interface__ (torch keeps this object
    alive as long as the tensor's storage; hipFree when it goes)."""
    _TYPESTR = {'float32': '<f4', 'float64': '<f8', 'int32': '<i4', 'int64': '<i8', 'complex64': '<c8', 'uint8': '|u1'}

    def __init__(self, ptr, nbytes, shape, dtype, hip):
        self.ptr, self.nbytes, self.hip = ptr, nbytes, hip
        self.__cuda_array_interface__ = {'shape': tuple(int(d) for d in shape),
                                         'typestr': self._TYPESTR[str(dtype).replace('torch.', '')],
                                         'data': (ptr, False), 'version': 2, 'strides': None}

    def __del__(self):
        if self.ptr:
            self.hip.hipFree(c_void_p(self.ptr))
            self.ptr = 0


def _ptr(t) -> Optional[c_void_p]:
    if t is None:
        return None
    return c_void_p(t.data_ptr())


class Context:
    """A librsl handle bound to one HIP device; launches go to torch's current stream."""

    def __init__(self, device: int = 0):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("rsl: no HIP device visible — the MI355X product path has no CPU fallback")
        self.torch = torch
        self.lib = _lib.load()
        self.device = torch.device('cuda', device)
        h = c_void_p()
        rc = self.lib.rsl_create(byref(h), device)
        if rc != 0:
            raise RuntimeError(f"rsl_create(device={device}) failed with code {rc}")
        self.h = h
        self._steer_cache: Dict = {}

    def __del__(self):
        try:
            if getattr(self, 'h', None):
                self.lib.rsl_destroy(self.h)
        except Exception:
            pass

    # -- plumbing -------------------------------------------------------------------------------
    def _bind(self):
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        self.lib.rsl_set_stream(self.h, c_void_p(s))

    def check(self, rc: int, what: str):
        if rc == 0:
            return
        msg = self.lib.rsl_last_error(self.h).decode(errors='replace')
        if rc in (_lib.RSL_ERR_INVALID, _lib.RSL_ERR_UNSUPPORTED):
            raise ValueError(f"{what}: {msg}")
        raise RuntimeError(f"{what}: {msg}")

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    def call(self, name: str, *args):
        """Entry point `name` of librsl on torch's current stream: the arguments after the handle as its
        _lib.SIGNATURES row takes them (tensors or None for device pointers, numbers, sequences for the small host
        arrays).  A status other than RSL_OK raises as check does; a tensor that is not on this context's device raises
        ValueError before the library is entered."""
        conv = _lib.marshal(name, args)
        for i in _lib.POINTER_SLOTS[name]:
            if hasattr(args[i], 'data_ptr') and args[i].device != self.device:
                raise ValueError(f'{name}: argument {i + 1} is a tensor on {args[i].device}, not on {self.device}')
        self._bind()
        self.check(getattr(self.lib, name)(self.h, *conv), name)  # args stay referenced until the call has returned

    def _buf(self, bufs, name, shape, dtype, want=True):
        """The caller's preallocated buffer ``bufs[name]`` where there is one (it is filled whether wanted or not),
        else a new tensor, or None when it is not wanted."""
        t = bufs.get(name) if bufs else None
        return t if t is not None or not want else self.empty(shape, dtype)

    def empty_contiguous(self, shape, dtype):
        """A device tensor in its own physically contiguous allocation (hipExtMallocWithFlags with
        hipDeviceMallocContiguous), freed when the tensor goes away; None when the driver cannot provide it.  For the
        large streamed outputs whose store rate depends on how the VRAM manager backs them (the configs[1] spectrum:
        DESIGN §5)."""
        torch = self.torch
        n = 1
        for d in shape:
            n *= int(d)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        hip = _hip()
        p = c_void_p()
        torch.cuda.set_device(self.device)
        if hip.hipExtMallocWithFlags(byref(p), ctypes.c_size_t(max(nbytes, 1)), 0x4) != 0 or not p.value:
            hip.hipGetLastError()
            return None
        owner = _DeviceBlock(p.value, nbytes, shape, dtype, hip)
        return torch.as_tensor(owner, device=self.device)

    def to_dev(self, arr: np.ndarray, dtype=None):
        t = self.torch.from_numpy(np.ascontiguousarray(arr))
        if dtype is not None:
            t = t.to(dtype)
        return t.to(self.device, non_blocking=False)

    def sync(self):
        self.call('rsl_sync')

    # -- timing ---------------------------------------------------------------------------------
    def timing(self, on: bool = True):
        self.lib.rsl_timing_enable(self.h, int(on))

    def timing_reset(self):
        self.lib.rsl_timing_reset(self.h)

    def timing_read(self) -> Dict[str, tuple]:
        out = {}
        for k, name in enumerate(_lib.K_NAMES):
            ms, n = c_double(), c_longlong()
            self.lib.rsl_timing_read(self.h, k, byref(ms), byref(n))
            out[name] = (ms.value, n.value)
        return out

    def timing_spans(self) -> Dict[str, list]:
        """Per kernel id: [(start_ms, end_ms), ...] of every launch since timing_reset, on one device clock (ms after
        the reset's reference event), in launch order."""
        out = {}
        if not hasattr(self.lib, 'rsl_timing_spans'):  # an older library under RSL_LIBRARY (A/B runs)
            return out
        for k, name in enumerate(_lib.K_NAMES):
            n = self.lib.rsl_timing_spans(self.h, k, 0, None, None)
            if n > 0:
                a, b = (c_double * n)(), (c_double * n)()
                self.lib.rsl_timing_spans(self.h, k, n, a, b)
                out[name] = list(zip(a, b))
        return out

    # -- a7 -------------------------------------------------------------------------------------
    def rds(self, cube, table, *, chirp0: int = 0, num_chirps: Optional[int] = None, dc_removal: bool = True,
            out=None, work=None):
        """cube complex64 [F, A, Ct, S] (device) -> rds complex64 [F, A, S, C]."""
        torch = self.torch
        F, A, Ct, S = cube.shape
        C = Ct - chirp0 if num_chirps is None else num_chirps
        if out is None:
            out = self.empty((F, A, S, C), torch.complex64)
        if work is None:
            work = self.empty((F, A, C, S), torch.complex64)
        self.call('rsl_rds', cube, F, A, Ct, chirp0, C, S, table, dc_removal, work, out)
        return out

    # -- a7 + a8 fused -----------------------------------------------------------------------------
    def rds_detect(self, cube, table, thr_power: float, i_lo: int, i_hi: int, *, rds, work, mask, row_count,
                   peak_pow=None, db_map=None, chirp0: int = 0, num_chirps: Optional[int] = None,
                   dc_removal: bool = True):
        """cube [F, A, Ct, S] -> rds [F, A, S, C] + detection outputs, Doppler FFT and detection in one kernel.
        Returns the row grouping of ``peak_pow`` (pass it to ``emit``)."""
        F, A, Ct, S = cube.shape
        C = Ct - chirp0 if num_chirps is None else num_chirps
        group = c_int(1)
        self.call('rsl_rds_detect', cube, F, A, Ct, chirp0, C, S, table, dc_removal, work, rds, thr_power, i_lo, i_hi,
                  mask, row_count, db_map, peak_pow, byref(group))
        return int(group.value)

    # -- a8 -------------------------------------------------------------------------------------
    def _detect_out(self, rds, want_db, out):
        """Outputs of a detector on rds [F, A, S, C]: (mask, row_count, db map or None, peak_pow or None); mask,
        row_count and peak_pow from ``out`` where given (peak_pow is never allocated here)."""
        torch = self.torch
        F, A, S, C = rds.shape
        mask = self._buf(out, 'mask', (F, A, S, (C + 63) // 64), torch.int64)
        rc = self._buf(out, 'row_count', (F, A, S), torch.int32)
        db = self.empty((F, A, S, C), torch.float32) if want_db else None
        return mask, rc, db, (out or {}).get('peak_pow')

    def detect(self, rds, thr_power: float, i_lo: int, i_hi: int, want_db: bool = False, out=None):
        F, A, S, C = rds.shape
        mask, rc, db, pk = self._detect_out(rds, want_db, out)
        self.call('rsl_detect', rds, F, A, S, C, thr_power, i_lo, i_hi, mask, rc, db, pk)
        return mask, rc, db

    def detect_cfar(self, rds, guard, train, alpha: float, thr_power: float, i_lo: int, i_hi: int,
                    want_db: bool = False, out=None, *, method: str = 'ca', rank: float = 0.75):
        """CFAR detector: guard / train = (range, doppler) half-sizes, thr_power the power floor (negative: none).
        method 'ca' (rsl_detect_cfar): alpha on the training mean.  method 'os' (rsl_detect_oscfar): alpha on the
        training cells' order statistic of rank k = ceil(rank * cells) (rank in (0, 1]).  Outputs as detect (peak_pow
        row-compact, group 1)."""
        F, A, S, C = rds.shape
        mask, rc, db, pk = self._detect_out(rds, want_db, out)
        head = (rds, F, A, S, C, guard[0], guard[1], train[0], train[1])
        tail = (alpha, thr_power, i_lo, i_hi, mask, rc, db, pk)
        if method == 'os':
            self.call('rsl_detect_oscfar', *head, rank, *tail)
        else:
            self.call('rsl_detect_cfar', *head, *tail)
        return mask, rc, db

    def detect_oscfar(self, rds, guard, train, rank: float, alpha: float, thr_power: float, i_lo: int, i_hi: int,
                      want_db: bool = False, out=None):
        """detect_cfar with method 'os'."""
        return self.detect_cfar(rds, guard, train, alpha, thr_power, i_lo, i_hi, want_db, out, method='os', rank=rank)

    # -- non-coherent integration -----------------------------------------------------------------
    def integrate_power(self, rds, out=None):
        """rds complex64 [F, A, S, C] -> the antenna-summed power map float32 [F, S, C] (rsl_power_integrate: the
        fp32 sum of the per-antenna powers in antenna order; A <= 32)."""
        torch = self.torch
        if rds.dim() != 4 or rds.dtype != torch.complex64:
            raise ValueError('integrate_power: rds must be complex64 [F, A, S, C]')
        F, A, S, C = rds.shape
        if out is None:
            out = self.empty((F, S, C), torch.float32)
        self.call('rsl_power_integrate', rds, F, A, S, C, out)
        return out

    def detect_power(self, power, rule, guard, train, rank: float, alpha: float, thr_power: float, i_lo: int,
                     i_hi: int, want_db: bool = False, out=None):
        """One of the three detection rules on a power map float32 [F, S, C] (rsl_detect_power).  rule: 'threshold'
        (guard, train, rank and alpha are ignored), 'ca' or 'os', or the _lib.RULE_* id.  Returns (mask [F, 1, S, W],
        row_count [F, 1, S], dB map [F, 1, S, C] or None): a unit antenna axis, so that offsets and emit take them as
        they are.  out: optional preallocated mask / row_count / peak_pow (row-compact, group 1)."""
        torch = self.torch
        if power.dim() != 3 or power.dtype != torch.float32:
            raise ValueError('detect_power: power must be float32 [F, S, C]')
        if isinstance(rule, str):
            if rule not in _lib.RULE_IDS:
                raise ValueError(f"rule must be 'threshold', 'ca' or 'os', not {rule!r}")
            rule = _lib.RULE_IDS[rule]
        F, S, C = power.shape
        mask, rc, db, pk = self._detect_out(power.unsqueeze(1), want_db, out)
        self.call('rsl_detect_power', power, F, S, C, rule, guard[0], guard[1], train[0], train[1], rank, alpha,
                  thr_power, i_lo, i_hi, mask, rc, db, pk)
        return mask, rc, db

    def offsets(self, mask, row_count, C: int, bufs=None):
        torch = self.torch
        F, A, S, W = mask.shape
        eo = self._buf(bufs, 'entry_row_off', (F * A * S,), torch.int32)
        co = self._buf(bufs, 'cell_row_off', (F * S,), torch.int32)
        sc = self._buf(bufs, 'scratch', (F * S,), torch.int32)
        eb = self._buf(bufs, 'entry_base', (F + 1,), torch.int64)
        cb = self._buf(bufs, 'cell_base', (F + 1,), torch.int64)
        fc = self._buf(bufs, 'frame_counts', (2 * F,), torch.int64)
        um = self._buf(bufs, 'union_mask', (F, S, W), torch.int64)
        self.call('rsl_peak_offsets', mask, row_count, F, A, S, C, eo, co, sc, eb, cb, fc, um)
        return dict(entry_row_off=eo, cell_row_off=co, scratch=sc, entry_base=eb, cell_base=cb, frame_counts=fc,
                    union_mask=um)

    def emit(self, rds, mask, offs, entry_cap: int, cell_cap: int, want_pdb: bool = True, bufs=None,
             peak_pow=None, peak_pow_group: int = 1):
        """Compact peak entries and unique cells.  With ``peak_pow`` (from detect, row grouping 1; or rds_detect,
        the grouping it returned) and the offsets' union mask the RDS is not re-read.  The antenna count is the
        mask's: masks of an antenna-summed map (detect_power, one antenna) go with the full RDS."""
        torch = self.torch
        F, _, S, C = rds.shape
        A = int(mask.shape[1])
        if want_pdb and A != rds.shape[1] and not emit_compact_supported(C, offs.get('union_mask') is not None,
                                                                         peak_pow is not None, True):
            # rsl_peak_emit would recompute power_db from the RDS, which is not the map these masks were taken on
            raise ValueError('emit: masks of another antenna count than the RDS need peak_pow, the union mask and a '
                             'power-of-two count of mask words per row (or want_pdb=False)')

        def get(name, n, dt):
            return self._buf(bufs, name, (max(n, 1),), dt)
        # e_coord = antenna << 26 | range_bin << 13 | doppler_bin (u32 bits in an int32 tensor; unpack_coord)
        e_co, e_c = get('e_coord', entry_cap, torch.int32), get('e_cell', entry_cap, torch.int32)
        e_pdb = get('e_pdb', entry_cap, torch.float32) if want_pdb else None
        c_f, c_rc, c_am = (get('c_frame', cell_cap, torch.int32), get('c_rc', cell_cap, torch.int32),
                           get('c_amask', cell_cap, torch.int32))
        self.call('rsl_peak_emit', rds, mask, offs.get('union_mask'), peak_pow, peak_pow_group, F, A, S, C,
                  offs['entry_row_off'], offs['cell_row_off'], offs['entry_base'], offs['cell_base'], entry_cap,
                  cell_cap, e_co, e_c, e_pdb, c_f, c_rc, c_am)
        return dict(e_coord=e_co, e_cell=e_c, e_pdb=e_pdb, c_frame=c_f, c_rc=c_rc, c_amask=c_am)

    # -- steering tables -------------------------------------------------------------------------
    def _steer_cached(self, kind, steer_c128, build):
        """The one cache of everything uploaded from a steering matrix: build() runs once per (kind, matrix).  The key
        holds the matrix's bytes themselves, not their hash: two matrices with one hash must not share a table."""
        key = (kind, steer_c128.dtype.str, steer_c128.shape, steer_c128.tobytes())
        if key not in self._steer_cache:
            self._steer_cache[key] = build()
        return self._steer_cache[key]

    def steering(self, steer_c128: np.ndarray):
        """Upload a [G, M] complex128 steering matrix: MFMA operand table (f32), fp64 copy, np.angle copy."""
        def build():
            G, M = steer_c128.shape
            host = np.zeros(self.lib.rsl_steer_table_floats(G, M), dtype=np.float32)
            flat = np.ascontiguousarray(steer_c128.astype(np.complex128)).view(np.float64)
            nt, fl = c_int(), c_int()
            rc = self.lib.rsl_steer_table_build(flat.ctypes.data_as(ctypes.POINTER(c_double)), G, M,
                                                host.ctypes.data_as(ctypes.POINTER(c_float)), byref(nt), byref(fl))
            if rc != 0:
                raise ValueError(f"rsl_steer_table_build failed (G={G}, M={M})")
            return dict(G=G, M=M, tab=self.to_dev(host), c128=self.to_dev(flat.copy()),
                        toeplitz=bool(fl.value & _lib.STEER_TOEPLITZ),
                        phase=self.to_dev(np.angle(steer_c128).astype(np.float64)))
        return self._steer_cached('mfma', steer_c128, build)

    # -- a11-a16 ----------------------------------------------------------------------------------
    def doa(self, rds, c_frame, c_rc, steer, method: int, *, n: Optional[int] = None, n_dev=None,
            want_gmax: bool = False, want_spec: bool = False, out_idx=None, fast: bool = True,
            spec_gmajor: bool = False, spec_blocked: bool = False, out_spec=None):
        """Steering-scan argmax per cell.  fast=True (default) uses the Toeplitz f16-MFMA path when the
        steering matrix is a uniform linear array and either no spectrum or the cell-blocked spectrum (without
        gmax) is requested; fast=False forces the f32 [Re; Im] MFMA scan.  want_spec: the spectrum, f32 [n, G]; [G, n] (n = the capacity) with spec_gmajor;
        [ceil(n / 32), G, 32] with spec_blocked (see spectrum_rows)."""
        torch = self.torch
        _, A, S, C = rds.shape
        cap = int(c_frame.shape[0]) if n is None else int(n)
        idx = out_idx if out_idx is not None else self.empty((max(cap, 1),), torch.int32)
        gmax = self.empty((max(cap, 1),), torch.float32) if want_gmax else None
        spec = out_spec
        if want_spec and spec is None:
            G = steer['G']
            shape = ((max(cap, 1) + 31) // 32, G, 32) if spec_blocked else (G, max(cap, 1)) if spec_gmajor else \
                (max(cap, 1), G)
            spec = self.empty(shape, torch.float32)
        m = int(method)
        if want_spec and spec_blocked:
            m |= _lib.DOA_SPEC_BLOCKED
        elif want_spec and spec_gmajor:
            m |= _lib.DOA_SPEC_GMAJOR
        if fast and steer['toeplitz'] and (not want_spec or (spec_blocked and not want_gmax)):
            m |= _lib.DOA_TOEPLITZ  # the f16-MFMA Toeplitz scan (argmax, or with the cell-blocked spectrum)
        self.call('rsl_doa', rds, A, S, C, c_frame, c_rc, n_dev, cap, steer['tab'], steer['c128'], steer['G'], m, idx,
                  gmax, spec)
        return idx, gmax, spec

    def doa_extras(self, rds, c_frame, c_rc, steer, method: int, *, n: int, n_dev=None, esprit_scale: float,
                   out_idx, esprit=None, phase=None, gmax=None):
        """Fused Toeplitz DoA argmax + ESPRIT + spatial phase from one signature load (rsl_doa_extras)."""
        _, A, S, C = rds.shape
        self.call('rsl_doa_extras', rds, A, S, C, c_frame, c_rc, n_dev, n, steer['tab'], steer['c128'], steer['G'],
                  method, esprit_scale, out_idx, gmax, esprit, phase)
        return out_idx, esprit, phase

    def steering_sub(self, steer_c128: np.ndarray, L: int):
        """Upload the sub-array steering vectors of rsl_doa_smoothed: device c64 [G, L] (tables.subarray_steering;
        ValueError for a non-uniform array)."""
        return self._steer_cached(('sub', int(L)), steer_c128,
                                  lambda: self.to_dev(tables.subarray_steering(steer_c128, L).astype(np.complex64)))

    def doa_smoothed(self, rds, c_frame, c_rc, steer_sub, *, n: Optional[int] = None, n_dev=None, nmax: int = 3,
                     num_sources: int = 0, rel: float = 0.05, want_den: bool = True, want_eig: bool = False,
                     want_spec: bool = False, out=None):
        """Forward-backward spatially smoothed MUSIC (rsl_doa_smoothed; the estimator is specified in include/rsl.h):
        up to nmax angles per cell.  steer_sub: device c64 [G, L] (steering_sub); num_sources = 0 estimates the order
        from the eigenvalues (those >= rel * the largest).  out: optional dict of preallocated nsrc i32 [cap], idx i32
        [cap, nmax], den f32 [cap, nmax], eig f32 [cap, L], spec f32 [cap, G].  Returns (nsrc, idx, den, eig, spec),
        None where not requested; slots beyond n = min(*n_dev, cap) are left as they were."""
        torch = self.torch
        _, A, S, C = rds.shape
        G, L = int(steer_sub.shape[0]), int(steer_sub.shape[1])
        cap = int(c_frame.shape[0]) if n is None else int(n)
        rows = max(cap, 1)
        nmax = int(nmax)
        nsrc = self._buf(out, 'nsrc', (rows,), torch.int32)
        idx = self._buf(out, 'idx', (rows, max(nmax, 1)), torch.int32)
        den = self._buf(out, 'den', (rows, max(nmax, 1)), torch.float32, want_den)
        eig = self._buf(out, 'eig', (rows, L), torch.float32, want_eig)
        spec = self._buf(out, 'spec', (rows, G), torch.float32, want_spec)
        self.call('rsl_doa_smoothed', rds, A, S, C, c_frame, c_rc, n_dev, cap, steer_sub, G, L, nmax, num_sources, rel,
                  nsrc, idx, den, eig, spec)
        return nsrc, idx, den, eig, spec

    # -- range-azimuth maps -----------------------------------------------------------------------
    def range_cov(self, rds, doppler=None, out=None):
        """rds complex64 [F, A, S, C] -> the spatial covariance of every range bin over the Doppler window
        doppler = (c0, c1) (None: all C bins), complex64 [F, S, A, A], exactly Hermitian (rsl_range_cov)."""
        torch = self.torch
        if rds.dim() != 4 or rds.dtype != torch.complex64:
            raise ValueError('range_cov: rds must be complex64 [F, A, S, C]')
        F, A, S, C = rds.shape
        c0, c1 = (0, C) if doppler is None else (int(doppler[0]), int(doppler[1]))
        if out is None:
            out = self.empty((F, S, A, A), torch.complex64)
        self.call('rsl_range_cov', rds, F, A, S, C, c0, c1, out)
        return out

    def steering_c64(self, steer_c128: np.ndarray):
        """Upload a steering matrix [G, A] rounded to complex64 (the table of rsl_range_azimuth), cached."""
        st = np.ascontiguousarray(np.asarray(steer_c128, dtype=np.complex128))
        return self._steer_cached('c64', st, lambda: self.to_dev(st.astype(np.complex64)))

    def range_azimuth(self, cov, steer_c64, method, loading: float = 1e-2, want_arg: bool = False, out=None):
        """cov complex64 [.., A, A] (Hermitian) -> the Bartlett or Capon power over the grid of steer_c64 (device c64
        [G, A], steering_c64), float32 [.., G], and on request the first-index argmax of every row, int32 [..]
        (rsl_range_azimuth).  method: 'bartlett' / 'capon' or the _lib.RA_* id; loading is read by Capon only.
        out: optional dict of preallocated map / arg.  Returns (map, arg or None)."""
        torch = self.torch
        if cov.dim() < 3 or cov.dtype != torch.complex64 or cov.shape[-1] != cov.shape[-2]:
            raise ValueError('range_azimuth: cov must be complex64 [.., A, A]')
        if isinstance(method, str):
            if method not in _lib.RA_IDS:
                raise ValueError(f"range_azimuth: method must be 'bartlett' or 'capon', not {method!r}")
            method = _lib.RA_IDS[method]
        A = int(cov.shape[-1])
        if steer_c64.dim() != 2 or steer_c64.dtype != torch.complex64 or int(steer_c64.shape[1]) != A:
            raise ValueError(f'range_azimuth: steer_c64 must be complex64 [G, {A}]')
        G = int(steer_c64.shape[0])
        lead = tuple(cov.shape[:-2])
        n = 1
        for d in lead:
            n *= int(d)
        m = self._buf(out, 'map', lead + (G,), torch.float32)
        arg = self._buf(out, 'arg', lead, torch.int32, want_arg)
        self.call('rsl_range_azimuth', cov, n, A, steer_c64, G, method, loading, m, arg)
        return m, arg

    def cell_extras(self, rds, c_frame, c_rc, *, n: int, n_dev=None, esprit_scale: float = 1 / math.pi,
                    want_sig=False, want_esprit=False, want_phase=False, gidx=None, az_table=None, bufs=None):
        torch = self.torch
        _, A, S, C = rds.shape
        cap = max(int(n), 1)
        sig = self.empty((cap, A), torch.complex64) if want_sig else None
        esp = self._buf(bufs, 'esprit', (cap,), torch.float64) if want_esprit else None
        ph = self._buf(bufs, 'phase', (cap,), torch.float64) if want_phase else None
        az = self._buf(bufs, 'az', (cap,), torch.float64) if az_table is not None else None
        self.call('rsl_cell_extras', rds, A, S, C, c_frame, c_rc, n_dev, n, esprit_scale, gidx, az_table, sig, esp, ph,
                  az)
        return sig, esp, ph, az

    def cell_refine(self, rds, c_frame, c_rc, gidx, az_table, steer_c64, *, n: Optional[int] = None, n_dev=None,
                    power=None, range_mode='hann', doppler_mode='rect', axes=(0.0, 1.0, 0.0, 1.0),
                    want_points: bool = True, want_az: bool = True, out=None):
        """The point cloud of a cell list (rsl_cell_refine; specified in include/rsl.h): sub-bin range and Doppler
        offsets from the five powers around each cell, the azimuth at the parabola vertex around gidx, the position.
        gidx i32 [n]; az_table f64 [G] radians; steer_c64 device c64 [G, A] (steering_c64); power f32 [F, S, C]
        (integrate_power) or None: the powers are then formed from rds.  range_mode / doppler_mode: 'none' | 'log' |
        'rect' | 'hann' or the _lib.REFINE_* id; axes = (r0, r_step, d0, d_step) (tables.point_axes).  out: optional
        dict of preallocated points f32 [cap, 8] / az f64 [cap].  Returns (points, az), None where not requested; slots
        beyond n = min(*n_dev, cap) are left as they were."""
        torch = self.torch
        _, A, S, C = rds.shape

        def mode_id(m, what):
            if isinstance(m, str):
                if m not in _lib.REFINE_IDS:
                    raise ValueError(f"cell_refine: {what} must be 'none', 'log', 'rect' or 'hann', not {m!r}")
                return _lib.REFINE_IDS[m]
            return int(m)
        rm, dm = mode_id(range_mode, 'range_mode'), mode_id(doppler_mode, 'doppler_mode')
        if steer_c64 is not None and (steer_c64.dim() != 2 or steer_c64.dtype != torch.complex64 or
                                      int(steer_c64.shape[1]) != A):
            raise ValueError(f'cell_refine: steer_c64 must be complex64 [G, {A}]')
        G = int(steer_c64.shape[0]) if steer_c64 is not None else 0
        if az_table is not None and int(az_table.shape[0]) != G:
            raise ValueError(f'cell_refine: az_table must have the steering table\'s {G} entries')
        if power is not None and (power.dtype != torch.float32 or tuple(power.shape[-2:]) != (S, C)):
            raise ValueError('cell_refine: power must be float32 [F, S, C]')
        cap = int(c_frame.shape[0]) if n is None else int(n)
        rows = max(cap, 1)
        shape = (rows, len(POINT_COLUMNS))
        pts = self._buf(out, 'points', shape, torch.float32, want_points)
        az = self._buf(out, 'az', (rows,), torch.float64, want_az)
        self.call('rsl_cell_refine', rds, power, A, S, C, c_frame, c_rc, n_dev, cap, gidx, az_table, steer_c64, G, rm,
                  dm, axes, pts, az)
        return pts, az

    def scan_register(self, points, seg, *, weight=None, rc=None, C: int = 0, axes=None, prev=None, init=None,
                      h: float = 0.5, h_coarse: float = 1.0, dtheta: float = math.radians(0.25), k: int = 20,
                      iters: int = 10, shrink: float = 0.7, tol: float = 1e-9, w_min: float = 3.0, dt: float = 0.1,
                      n: Optional[int] = None, want_omega: bool = True, out=None):
        """Scan registration (rsl_scan_register; the estimator is specified in include/rsl.h): the yaw increment and
        the displacement of every frame's point cloud against the frame before it.  points f32 [N, 8] (the rows of
        cell_refine), seg i64 [F + 1] (cell_base; clamped to n, default N), weight f32 [N] or None, rc i32 [N] or None
        with C and axes = (r0, r_step, ...) (tables.point_axes) for the culling, init f64 [F, 3] or None.  prev: None,
        or a dict of the cloud frame 0 is registered against: points f32 [M, 8], and optionally weight f32 [M], rc i32
        [M], n (rows in use, default M) and n_dev (device i64 [1], the rows in use where only the device knows them).
        out: optional dict of preallocated rows f64 [F, 8] / omega f64 [F, 3].  Returns (rows, omega or None):
        rows = {theta, t_x, t_y, W, rms, S_best / sum S, updates, flag}, omega[f - 1] = {0, 0, theta_f / dt}."""
        torch = self.torch
        points, N = check_cloud('scan_register', points, seg, n, weight, self.empty)
        F = int(seg.shape[0]) - 1
        _per_point('scan_register', rc, torch.int32, N, 'rc')
        pv = dict(prev) if prev else {}
        pp = pv.get('points')
        M = 0
        if pp is not None:  # an empty reference is still a reference (flag 1, not 2)
            pp, M = check_cloud('scan_register', pp, None, pv.get('n'), pv.get('weight'), self.empty, 'prev ')
            _per_point('scan_register', pv.get('rc'), torch.int32, M, 'prev rc')
        if init is not None and (init.dtype != torch.float64 or tuple(init.shape) != (F, 3) or
                                 not init.is_contiguous()):
            raise ValueError(f'scan_register: init must be contiguous float64 [{F}, 3]')
        rows = self._buf(out, 'rows', (max(F, 1), 8), torch.float64)
        om = self._buf(out, 'omega', (max(F, 1), 3), torch.float64) if want_omega else None
        self.call('rsl_scan_register', points, seg, F, N, weight, rc, C, axes, pp, pv.get('weight'), pv.get('rc'), M,
                  pv.get('n_dev'), init, h, h_coarse, dtheta, k, iters, shrink, tol, w_min, dt, rows, om)
        return rows, om

    def map_update(self, points, seg, poses, hits, *, grid, free=None, weight=None, r_min: float = 0.5,
                   r_max: float = 75.0, min_db: float = -math.inf, n: Optional[int] = None, want_stats: bool = True,
                   out=None):
        """Grid map update (rsl_map_update, specified in include/rsl.h): every frame adds 1 to the hit count of the
        cells its accepted points fall into and, with `free`, 1 to the free count of the cells on the rays from the
        sensor's cell to them.  points f32 [N, 8] (the rows of cell_refine), seg i64 [F + 1] (cell_base; clamped to n,
        default N), poses f64 [F, 7] = (p, q) (TrajectoryReducer.poses), weight f32 [N] or None, grid = (x0, y0, cell);
        hits / free: contiguous int32 (the bits are unsigned counts) [ny, nx], added to in place, free None: no rays.
        out: optional dict of a preallocated stats i32 [F, 4].  Returns stats = {accepted points, hit cells, free
        cells, flag (1: pose not finite or too far from the map)} per frame, or None."""
        torch = self.torch
        points, N = check_cloud('map_update', points, seg, n, weight, self.empty)
        F = int(seg.shape[0]) - 1
        if poses.dtype != torch.float64 or poses.dim() != 2 or int(poses.shape[0]) < F or int(poses.shape[1]) != 7 or \
                not poses.is_contiguous():
            raise ValueError(f'map_update: poses must be contiguous float64 [{F}, 7]')
        for name, t in (('hits', hits), ('free', free)):
            if t is not None and (t.dtype != torch.int32 or t.dim() != 2 or not t.is_contiguous()
                                  or t.shape != hits.shape):
                raise ValueError(f'map_update: {name} must be a contiguous int32 [ny, nx] plane')
        ny, nx = int(hits.shape[0]), int(hits.shape[1])
        stats = self._buf(out, 'stats', (max(F, 1), 4), torch.int32) if want_stats else None
        self.call('rsl_map_update', points, seg, F, N, weight, poses, (grid[0], grid[1], grid[2], 0.0), nx, ny, r_min,
                  r_max, min_db, hits, free, stats)
        return stats

    def map_logodds(self, hits, free=None, *, l_occ: float = 0.85, l_free: float = 0.4, l_min: float = -4.0,
                    l_max: float = 4.0, out=None):
        """Clamped log-odds of the grid map's counts (rsl_map_logodds): f32, shaped as hits,
        clamp(hits l_occ - free l_free, l_min, l_max) in fp64, rounded to f32 once."""
        torch = self.torch
        for name, t in (('hits', hits), ('free', free)):
            if t is not None and (t.dtype != torch.int32 or not t.is_contiguous()
                                  or t.shape != hits.shape):
                raise ValueError(f'map_logodds: {name} must be a contiguous int32 plane')
        lo = out if out is not None else self.empty(tuple(hits.shape), torch.float32)
        self.call('rsl_map_logodds', hits, free, hits.numel(), l_occ, l_free, l_min, l_max, lo)
        return lo

    def confidence(self, rds, c_frame, c_rc, gidx, steer, n: int):
        torch = self.torch
        _, A, S, C = rds.shape
        conf = self.empty((max(n, 1),), torch.float64)
        self.call('rsl_confidence', rds, A, S, C, c_frame, c_rc, n, gidx, steer['c128'], steer['phase'], conf)
        return conf

    # -- configs[3] per-frame pattern ------------------------------------------------------------
    def peak_topk(self, entry_base, entry_cap: int, e_coord, e_pdb, *, thr_db: float, kmax: int, C: int):
        """Per cube k: the first kmax peak entries by power_db descending (stable; robust_angle_estimation.py:362-369).
        Returns (sel_entry, sel_frame, sel_rc) i32 [ncube * kmax] and sel_n i32 [ncube]."""
        torch = self.torch
        ncube = int(entry_base.shape[0]) - 1
        n = max(ncube * int(kmax), 1)
        se, sf, sr = (self.empty((n,), torch.int32) for _ in range(3))
        sn = self.empty((max(ncube, 1),), torch.int32)
        self.call('rsl_peak_topk', entry_base, entry_cap, ncube, e_coord, e_pdb, thr_db, kmax, C, se, sf, sr, sn)
        return se, sf, sr, sn

    def associate_nearest(self, range_m, az_rad, s0, off, *, thr: float = 5.0):
        """The analyser's association (radarscenes_complete_analysis.py:274-305) for every frame of a batch:
        range_m, az_rad f64 [N], s0 c128 [N] (first signature components), off i64 [nframes + 1] (device).
        Returns (match i32 [N] within the previous frame, -1 = none; dist f64 [N]; phase f64 [N])."""
        torch = self.torch
        nframes = int(off.shape[0]) - 1
        N = int(range_m.shape[0])
        match = self.empty((max(N, 1),), torch.int32)
        dist = self.empty((max(N, 1),), torch.float64)
        phase = self.empty((max(N, 1),), torch.float64)
        self.call('rsl_associate_nearest', range_m, az_rad, s0, off, nframes, N, thr, match, dist, phase)
        return match, dist, phase

    # -- a25-a29 ---------------------------------------------------------------------------------
    def _vel_problem(self, y, seg, n, az_table, out, want_weight, want_resid):
        """What the three velocity solvers derive from their shared inputs: F, N (n, default len(y), clamped to it), G,
        the row buffer, and the optional weight (want_weight: True, or a device f32 [N] buffer to fill) and resid
        buffers."""
        torch = self.torch
        F = int(seg.shape[0]) - 1
        o = out if out is not None else self.empty((max(F, 1), 8), torch.float64)
        N = int(y.shape[0]) if n is None else min(int(n), int(y.shape[0]))
        G = int(az_table.shape[0]) if az_table is not None else 0
        if want_weight is True:
            weight = self.empty((max(N, 1),), torch.float32)
        else:
            weight = None if want_weight is False or want_weight is None else want_weight
        resid = self.empty((max(N, 1),), torch.float64) if want_resid else None
        return F, N, G, o, weight, resid

    def velocity(self, az, y, seg, *, k: float, ridge: float = 0.0, bounds=(-50.0, 50.0, -50.0, 50.0),
                 amask=None, want_resid=False, out=None, gidx=None, az_table=None, n=None):
        """n: the per-target arrays' length (default len(y)); the segments in seg are clamped to it."""
        F, N, G, o, _, resid = self._vel_problem(y, seg, n, az_table, out, False, want_resid)
        pred = self.empty((max(N, 1),), self.torch.float64) if want_resid else None
        self.call('rsl_velocity', az, gidx, az_table, G, y, amask, seg, N, F, k, ridge, bounds, o, resid, pred)
        return o, resid, pred

    def velocity_robust(self, az, y, seg, *, k: float, loss, c: Optional[float] = None, scale: Optional[float] = None,
                        iters: int = 30, tol: float = 1e-9, ridge: float = 0.0, bounds=(-50.0, 50.0, -50.0, 50.0),
                        amask=None, gidx=None, az_table=None, n=None, out=None, want_weight=False, want_resid=False):
        """Huber / Tukey IRLS velocity solve (rsl_velocity_robust; the estimator is specified in include/rsl.h).
        loss: 'huber' | 'tukey' or the _lib.LOSS_* id; c=None: the loss's default tuning constant; scale=None: sigma
        estimated per iteration from the residuals' weighted median (dependable only below roughly 30 % coherent
        outliers; pass the sensor's phase-noise sigma where it is known).  want_weight: True, or a device f32 [N]
        buffer to fill.  Returns (out f64 [F, 8], weight f32 [N] or None, resid f64 [N] or None)."""
        if isinstance(loss, str):
            if loss not in _lib.LOSS_IDS:
                raise ValueError(f"loss must be 'huber' or 'tukey', not {loss!r}")
            loss = _lib.LOSS_IDS[loss]
        loss = int(loss)
        if c is None:
            c = _lib.LOSS_DEFAULT_C.get(loss, 1.0)  # an unknown id is rejected by the library
        F, N, G, o, weight, resid = self._vel_problem(y, seg, n, az_table, out, want_weight, want_resid)
        self.call('rsl_velocity_robust', az, gidx, az_table, G, y, amask, seg, N, F, k, ridge, bounds, loss, c,
                  0.0 if scale is None else scale, iters, tol, o, weight, resid)
        return o, weight, resid

    def velocity_consensus(self, az, y, seg, *, k: float, scale: float, c: Optional[float] = None, hyps: int = 256,
                           min_det: float = 0.1, refine: int = 3, seed: int = 0, frame0: int = 0, ridge: float = 0.0,
                           bounds=(-50.0, 50.0, -50.0, 50.0), amask=None, gidx=None, az_table=None, n=None, out=None,
                           want_weight=False, want_resid=False):
        """Consensus (RANSAC) velocity solve (rsl_velocity_consensus; the estimator is specified in include/rsl.h): for
        frames where the static cells are not the majority.  scale: the sensor's phase-noise sigma in radians
        (required); c=None: 3.0, the cut-off is c * scale; hyps two-cell hypotheses per frame, drawn from
        (seed, frame0 + f, h); min_det: the least |sin| of a pair's azimuth difference; refine: LS passes on the
        winner's inliers.  want_weight: True, or a device f32 [N] buffer to fill with the inlier mask.  Returns
        (out f64 [F, 8] = {v_x, v_y, cost, rmse_in, n_in, n, best_h, n_valid}, weight f32 [N] or None, resid f64 [N]
        or None)."""
        if scale is None:
            raise ValueError('velocity_consensus needs scale, the phase-noise sigma in radians')
        if c is None:
            c = _lib.CONSENSUS_DEFAULT_C
        seed, frame0 = int(seed), int(frame0)
        if not 0 <= seed < 2 ** 64:
            raise ValueError(f'seed must lie in [0, 2^64), not {seed!r}')
        if not -2 ** 63 <= frame0 < 2 ** 63:
            raise ValueError(f'frame0 must fit 64 bits, not {frame0!r}')
        F, N, G, o, weight, resid = self._vel_problem(y, seg, n, az_table, out, want_weight, want_resid)
        self.call('rsl_velocity_consensus', az, gidx, az_table, G, y, amask, seg, N, F, k, ridge, bounds, c, scale,
                  hyps, min_det, refine, seed, frame0, o, weight, resid)
        return o, weight, resid


_ctx_lock = threading.Lock()
_ctx: Dict[int, Context] = {}


def spectrum_rows(spec_blocked, n: int):
    """Cell-major [n, G] view (a device copy) of a cell-blocked spectrum [ceil(cap / 32), G, 32]."""
    nb, G, _ = spec_blocked.shape
    return spec_blocked.permute(0, 2, 1).reshape(nb * 32, G)[:n]


def get_context(device: Optional[int] = None) -> Context:
    import torch
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    with _ctx_lock:
        c = _ctx.get(device)
        if c is None:
            c = Context(device)
            _ctx[device] = c
        return c
