"""CPU: rsl._lib.marshal, the argument conversion of Context.call, on every kind of slot of the signature table.  It
needs no library and no device: the tensors are torch CPU tensors."""
import ctypes
from ctypes import POINTER, c_double, c_int, c_longlong, c_ulonglong, c_void_p

import numpy as np
import pytest
import torch

from rsl import _lib


def test_converters_cover_exactly_the_status_entry_points():
    """One converter per argument after the handle, for exactly the entry points that take the handle first and return
    the c_int status; every slot type of theirs is one marshal knows."""
    want = {n for n, (res, args) in _lib.SIGNATURES.items() if res is c_int and args and args[0] is c_void_p}
    assert set(_lib.CONVERTERS) == want == set(_lib.POINTER_SLOTS)
    assert {'rsl_version', 'rsl_create', 'rsl_last_error', 'rsl_fft_supported', 'rsl_steer_table_build',
            'rsl_steer_table_floats', 'rsl_wrapped_scratch_bytes', 'rsl_wrapped_search_scratch_bytes',
            'rsl_pose_error_scratch_bytes'}.isdisjoint(want)
    assert {'rsl_sync', 'rsl_rds', 'rsl_scan_register', 'rsl_bvls'} <= want
    for n in want:
        args = _lib.SIGNATURES[n][1][1:]
        assert len(_lib.CONVERTERS[n]) == len(args)
        assert _lib.POINTER_SLOTS[n] == tuple(i for i, t in enumerate(args) if t is c_void_p)
        for t in args:
            assert t in (c_void_p, c_int, c_longlong, c_ulonglong, c_double) or \
                t in (POINTER(c_double), POINTER(c_int), POINTER(c_longlong)), (n, t)
    assert len(_lib.CONVERTERS['rsl_scan_register']) == 25 and _lib.marshal('rsl_sync', ()) == []


def test_pointer_slots():
    # rsl_power_integrate: rds, F, A, S, C, out
    t = torch.zeros(4, dtype=torch.complex64)
    got = _lib.marshal('rsl_power_integrate', (t, 1, 2, 4, 8, None))
    assert isinstance(got[0], c_void_p) and got[0].value == t.data_ptr() and got[5] is None
    p = c_void_p(64)
    got = _lib.marshal('rsl_power_integrate', (p, 1, 2, 4, 8, 4096))
    assert got[0] is p and got[5] == 4096
    view = t[2:]
    assert _lib.marshal('rsl_power_integrate', (view, 1, 2, 4, 8, None))[0].value == t.data_ptr() + 16


def test_integer_and_double_slots():
    # rsl_synth_cube: pattern, F, A, C, S, noise_power (double), seed (unsigned long long), frame0 (long long), cube
    got = _lib.marshal('rsl_synth_cube', (None, True, np.int64(3), 2.0, np.float32(5.0), 1, 2 ** 64 - 1, -2 ** 40,
                                          None))
    assert got == [None, 1, 3, 2, 5, 1.0, 2 ** 64 - 1, -2 ** 40, None]
    assert [type(v) for v in got[1:8]] == [int, int, int, int, float, int, int]
    # what ctypes makes of them: nothing is truncated on the way into a 64-bit slot
    assert c_ulonglong(got[6]).value == 2 ** 64 - 1 and c_longlong(got[7]).value == -2 ** 40
    got = _lib.marshal('rsl_synth_cube', (None, 1, 1, 1, 1, np.float64(0.25), np.uint64(7), 0, None))
    assert got[5] == 0.25 and type(got[5]) is float and got[6] == 7 and type(got[6]) is int
    with pytest.raises((TypeError, ValueError)):
        _lib.marshal('rsl_synth_cube', (None, 'one', 1, 1, 1, 0.0, 0, 0, None))
    with pytest.raises(TypeError):
        _lib.marshal('rsl_synth_cube', (None, None, 1, 1, 1, 0.0, 0, 0, None))


@pytest.mark.parametrize('box', [(-50.0, 50.0, -1, 1), [-50.0, 50.0, -1, 1], np.array([-50.0, 50.0, -1.0, 1.0]),
                                 np.array([-50, 50, -1, 1], np.float32)], ids=['tuple', 'list', 'f64', 'f32'])
def test_host_array_slots(box):
    # rsl_velocity: az, gidx, az_table, G, y, amask, seg, n, F, k, ridge, bounds4 (const double*), out, resid, pred
    got = _lib.marshal('rsl_velocity', (None, None, None, 0, None, None, None, 0, 0, 1, 0, box, None, None, None))
    b = got[11]
    assert isinstance(b, ctypes.Array) and b._type_ is c_double and len(b) == 4 and list(b) == [-50.0, 50.0, -1.0, 1.0]
    assert got[9] == 1.0 and type(got[9]) is float


def test_host_array_slots_pass_ctypes_through():
    a4 = (c_double * 4)(1.0, 2.0, 3.0, 4.0)
    args = [None, None, None, 0, None, None, None, 0, 0, 1.0, 0.0, a4, None, None, None]
    assert _lib.marshal('rsl_velocity', args)[11] is a4
    args[11] = None
    assert _lib.marshal('rsl_velocity', args)[11] is None
    ptr = ctypes.cast(a4, POINTER(c_double))
    args[11] = ptr
    assert _lib.marshal('rsl_velocity', args)[11] is ptr
    # rsl_rds_detect's last slot is the int* the row grouping comes back through
    group = c_int(1)
    ref = ctypes.byref(group)
    got = _lib.marshal('rsl_rds_detect', (None,) + (0,) * 6 + (None, 0, None, None, 0.0, 0, 0, None, None, None, None,
                                                            ref))
    assert got[-1] is ref and len(got) == 19


def test_argument_count():
    with pytest.raises(TypeError, match=r'rsl_power_integrate: 6 arguments after the handle expected, 5 given'):
        _lib.marshal('rsl_power_integrate', (None, 1, 2, 4, 8))
    with pytest.raises(TypeError, match=r'rsl_sync: 0 arguments after the handle expected, 1 given'):
        _lib.marshal('rsl_sync', (None,))
    with pytest.raises(KeyError):
        _lib.marshal('rsl_version', ())
