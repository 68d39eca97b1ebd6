"""ctypes binding of librsl.so (C ABI declared in include/rsl.h).

The library is built in-tree by ``__graft_entry__.build()`` (``make -C radar-slam_amd/csrc``) into
``radar-slam_amd/lib/librsl.so``.  There is no fallback: if the library is missing, importing the
product path raises ``ImportError``.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import c_double, c_float, c_int, c_longlong, c_ulonglong, c_void_p, c_char_p, POINTER

PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.environ.get('RSL_LIBRARY', os.path.join(PKG_ROOT, 'lib', 'librsl.so'))

RSL_OK, RSL_ERR_INVALID, RSL_ERR_UNSUPPORTED, RSL_ERR_HIP = 0, 1, 2, 3
METHOD_BEAMFORMING, METHOD_MUSIC = 0, 1
DOA_TOEPLITZ = 0x100
DOA_SPEC_GMAJOR = 0x200
DOA_SPEC_BLOCKED = 0x400
STEER_TOEPLITZ = 1
RULE_THRESHOLD, RULE_CA, RULE_OS = 0, 1, 2  # RSL_RULE_*: the detection rule of rsl_detect_power
RULE_IDS = {'threshold': RULE_THRESHOLD, 'ca': RULE_CA, 'os': RULE_OS}
SS_MAX_L = 8  # RSL_SS_MAX_L: the longest sub-array of rsl_doa_smoothed
RA_BARTLETT, RA_CAPON = 0, 1  # RSL_RA_*: the method of rsl_range_azimuth
RA_IDS = {'bartlett': RA_BARTLETT, 'capon': RA_CAPON}
RA_MAX_A = 16  # RSL_RA_MAX_A: the most antennas of rsl_range_cov / rsl_range_azimuth
RA_MIN_LOADING = 1e-4  # RSL_RA_MIN_LOADING: the least diagonal loading of the Capon map
REFINE_NONE, REFINE_LOG, REFINE_RECT, REFINE_HANN = 0, 1, 2, 3  # RSL_REFINE_*: the offset estimators of rsl_cell_refine
REFINE_IDS = {'none': REFINE_NONE, 'log': REFINE_LOG, 'rect': REFINE_RECT, 'hann': REFINE_HANN}
REG_MAX_K, REG_MAX_ITERS = 64, 100  # RSL_REG_MAX_K, RSL_REG_MAX_ITERS: the limits of rsl_scan_register
MAP_MAX_RW = 383  # RSL_MAP_MAX_RW: the largest half window, in cells, of rsl_map_update
LOSS_HUBER, LOSS_TUKEY = 1, 2
LOSS_IDS = {'huber': LOSS_HUBER, 'tukey': LOSS_TUKEY}
LOSS_DEFAULT_C = {LOSS_HUBER: 1.345, LOSS_TUKEY: 4.685}  # 95 % efficiency at the normal distribution
CONSENSUS_MAX_H = 4096  # RSL_CONSENSUS_MAX_H: the most hypotheses of rsl_velocity_consensus
CONSENSUS_DEFAULT_C = 3.0  # cut-off of the consensus solver in units of the phase-noise sigma
K_NAMES = ['range_fft', 'doppler_fft', 'detect', 'offsets', 'emit', 'doa_scan', 'cell_extras', 'confidence',
           'velocity', 'aux']

_P = c_void_p
# the handle and the problem the three velocity solvers share: az, gidx, az_table, G, y, amask, seg, n, F, k, ridge,
# bounds4
_VEL = [_P, _P, _P, _P, c_int, _P, _P, _P, c_longlong, c_int, c_double, c_double, POINTER(c_double)]
# name -> (restype, argtypes); must mirror include/rsl.h (tests/test_abi_host.py checks every type, both directions)
SIGNATURES = {
    'rsl_version': (c_int, []),
    'rsl_create': (c_int, [POINTER(c_void_p), c_int]),
    'rsl_destroy': (c_int, [_P]),
    'rsl_last_error': (c_char_p, [_P]),
    'rsl_set_stream': (c_int, [_P, _P]),
    'rsl_sync': (c_int, [_P]),
    'rsl_fft_supported': (c_int, [c_int]),
    'rsl_timing_enable': (c_int, [_P, c_int]),
    'rsl_timing_reset': (c_int, [_P]),
    'rsl_timing_read': (c_int, [_P, c_int, POINTER(c_double), POINTER(c_longlong)]),
    'rsl_timing_spans': (c_int, [_P, c_int, c_int, POINTER(c_double), POINTER(c_double)]),
    'rsl_rds': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P]),
    'rsl_rds_detect': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P, c_int, _P, _P, c_double, c_int,
                               c_int, _P, _P, _P, _P, POINTER(c_int)]),
    'rsl_detect': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_double, c_int, c_int, _P, _P, _P, _P]),
    'rsl_detect_cfar': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_double,
                                c_int, c_int, _P, _P, _P, _P]),
    'rsl_detect_oscfar': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_double,
                                  c_double, c_int, c_int, _P, _P, _P, _P]),
    'rsl_power_integrate': (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    'rsl_detect_power': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_double,
                                 c_double, c_int, c_int, _P, _P, _P, _P]),
    'rsl_peak_offsets': (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P]),
    'rsl_peak_emit': (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P, _P, _P, c_longlong,
                              c_longlong, _P, _P, _P, _P, _P, _P]),
    'rsl_steer_table_floats': (c_longlong, [c_int, c_int]),
    'rsl_steer_table_build': (c_int, [POINTER(c_double), c_int, c_int, POINTER(c_float), POINTER(c_int),
                                      POINTER(c_int)]),
    'rsl_doa': (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, c_longlong, _P, _P, c_int, c_int, _P, _P, _P]),
    'rsl_doa_extras': (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, c_longlong, _P, _P, c_int, c_int, c_double,
                               _P, _P, _P, _P]),
    'rsl_doa_smoothed': (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, c_longlong, _P, c_int, c_int, c_int, c_int,
                                 c_double, _P, _P, _P, _P, _P]),
    'rsl_range_cov': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    'rsl_range_azimuth': (c_int, [_P, _P, c_longlong, c_int, _P, c_int, c_int, c_double, _P, _P]),
    'rsl_cell_extras': (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, c_longlong, c_double, _P, _P, _P, _P,
                                _P, _P]),
    'rsl_cell_refine': (c_int, [_P, _P, _P, c_int, c_int, c_int, _P, _P, _P, c_longlong, _P, _P, _P, c_int, c_int, c_int,
                                POINTER(c_double), _P, _P]),
    'rsl_scan_register': (c_int, [_P, _P, _P, c_int, c_longlong, _P, _P, c_int, POINTER(c_double), _P, _P, _P, c_longlong,
                                  _P, _P, c_double, c_double, c_double, c_int, c_int, c_double, c_double, c_double,
                                  c_double, _P, _P]),
    'rsl_map_update': (c_int, [_P, _P, _P, c_int, c_longlong, _P, _P, POINTER(c_double), c_int, c_int, c_double, c_double,
                               c_double, _P, _P, _P]),
    'rsl_map_logodds': (c_int, [_P, _P, _P, c_longlong, c_double, c_double, c_double, c_double, _P]),
    'rsl_confidence': (c_int, [_P, _P, c_int, c_int, c_int, _P, _P, c_longlong, _P, _P, _P, _P]),
    'rsl_velocity': (c_int, _VEL + [_P, _P, _P]),
    'rsl_velocity_robust': (c_int, _VEL + [c_int, c_double, c_double, c_int, c_double, _P, _P, _P]),
    'rsl_velocity_consensus': (c_int, _VEL + [c_double, c_double, c_int, c_double, c_int, c_ulonglong, c_longlong,
                                              _P, _P, _P]),
    'rsl_preprocess_rows': (c_int, [_P, _P, c_longlong, c_int, _P, c_int, _P]),
    'rsl_phase_model': (c_int, [_P, _P, _P, c_longlong, _P, c_double, _P, c_int, c_double, _P, _P, _P]),
    'rsl_associate': (c_int, [_P, _P, c_int, _P, c_int, c_double, _P, _P, _P]),
    'rsl_peak_topk': (c_int, [_P, _P, c_longlong, c_int, _P, _P, c_double, c_int, c_int, _P, _P, _P, _P]),
    'rsl_associate_nearest': (c_int, [_P, _P, _P, _P, _P, c_int, c_longlong, c_double, _P, _P, _P]),
    'rsl_wrapped_scratch_bytes': (c_longlong, [c_longlong, c_int, c_int]),
    'rsl_wrapped_search_scratch_bytes': (c_longlong, [c_longlong, POINTER(c_double), POINTER(c_double), c_double, c_int, c_int]),
    'rsl_wrapped_search': (c_int, [_P, _P, _P, c_longlong, _P, c_double, c_int, c_double, c_double, c_double, _P,
                                   POINTER(c_double), POINTER(c_double), c_int, POINTER(c_double), c_double, c_int, _P,
                                   c_int, c_int, _P, c_longlong, _P]),
    'rsl_wrapped_solve': (c_int, [_P, _P, _P, c_longlong, _P, c_double, c_int, c_double, c_double, c_double, _P,
                                  POINTER(c_double), POINTER(c_double), c_int, c_int, _P, c_int, c_int, _P,
                                  c_longlong, _P]),
    'rsl_traj_scan': (c_int, [_P, _P, c_int, c_int, _P, c_int, _P, c_double, c_longlong, c_int, _P, _P, _P]),
    'rsl_traj_apply': (c_int, [_P, _P, _P, c_longlong, _P]),
    'rsl_traj_stitch': (c_int, [_P, _P, c_int, c_int, c_double, c_int, _P, _P]),
    'rsl_traj_smooth': (c_int, [_P, _P, c_longlong, c_int, c_int, _P]),
    'rsl_synth_pattern': (c_int, [_P, _P, c_int, c_int, c_int, c_double, c_double, c_double, c_double, _P]),
    'rsl_synth_cube': (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_double, c_ulonglong, c_longlong, _P]),
    'rsl_pose_error_scratch_bytes': (c_longlong, [c_longlong, c_int]),
    'rsl_music_subspace': (c_int, [_P, _P, c_longlong, c_int, c_int, _P, c_int, _P]),
    'rsl_esprit_subspace': (c_int, [_P, _P, c_longlong, c_int, c_int, c_double, _P]),
    'rsl_pose_align': (c_int, [_P, _P, _P, c_longlong, _P, _P, _P, _P, _P]),
    'rsl_pose_rte': (c_int, [_P, _P, _P, c_longlong, _P, c_int, _P, _P, _P, _P]),
    'rsl_bvls': (c_int, [_P, _P, _P, c_longlong, _P, c_double, c_int, c_double, _P, _P, _P]),
}


def _pointer(a):
    """A c_void_p slot: None stays None, a tensor (anything with data_ptr()) gives its address, an int or a c_void_p
    passes."""
    if a is None:
        return None
    addr = getattr(a, 'data_ptr', None)
    return a if addr is None else c_void_p(addr())


def _host_array(ctype):
    """A POINTER(ctype) slot: None and what ctypes already takes (an array, a pointer, byref) pass; a Python sequence
    or a numpy array becomes a ctype array of its length."""
    scalar = float if ctype in (c_double, c_float) else int

    def conv(a):
        if a is None or isinstance(a, ctypes.Array) or not hasattr(a, '__len__'):
            return a
        return (ctype * len(a))(*[scalar(x) for x in a])
    return conv


def _converter(ctype):
    if ctype is c_void_p:
        return _pointer
    if ctype in (c_int, c_longlong, c_ulonglong):
        return int
    if ctype is c_double:
        return float
    return _host_array(ctype._type_)


# name -> one converter per argument after the handle, for every entry point that takes the handle first and returns
# the c_int status: the calls Context.call makes
CONVERTERS = {name: tuple(_converter(t) for t in args[1:]) for name, (res, args) in SIGNATURES.items()
              if res is c_int and args and args[0] is c_void_p}
# name -> the positions (after the handle) of its c_void_p slots: the device pointers
POINTER_SLOTS = {name: tuple(i for i, t in enumerate(SIGNATURES[name][1][1:]) if t is c_void_p) for name in CONVERTERS}


def marshal(name, args):
    """The arguments of entry point `name` after the handle, converted as its SIGNATURES row says (a pure function: no
    library, no device).  TypeError when the count differs."""
    conv = CONVERTERS[name]
    if len(args) != len(conv):
        raise TypeError(f'{name}: {len(conv)} arguments after the handle expected, {len(args)} given')
    return [f(a) for f, a in zip(conv, args)]


_lib = None


def load():
    """Load librsl.so once and declare every entry point's signature."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"librsl.so not found at {LIB_PATH}: build it with __graft_entry__.build() "
                          f"or `make -C radar-slam_amd/csrc` (there is no CPU fallback)")
    lib = ctypes.CDLL(LIB_PATH)
    # a non-default library (RSL_LIBRARY: an older build for an A/B comparison) may lack newer entry points; the
    # product library must export every one (tests/test_abi.py)
    lenient = 'RSL_LIBRARY' in os.environ
    for name, (res, args) in SIGNATURES.items():
        if lenient and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
