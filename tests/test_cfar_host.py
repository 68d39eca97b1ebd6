"""CPU checks of the CA-CFAR detector's host surface: the C ABI symbol, the alpha tables, the chain option and the
numpy oracle (tests/cfar_ref.py) that the GPU tests compare against."""
import ctypes
import os
import re

import numpy as np
import pytest

import cfar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'rsl.h')
LIB = os.path.join(ROOT, 'radar-slam_amd', 'lib', 'librsl.so')


def test_header_declares_detect_cfar():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'int\s+rsl_detect_cfar\s*\(([^)]*)\)', src)
    assert m, 'rsl_detect_cfar not declared in include/rsl.h'
    names = [a.strip().split()[-1].lstrip('*') for a in m.group(1).split(',')]
    assert names == ['h', 'rds', 'F', 'A', 'S', 'C', 'guard_r', 'guard_d', 'train_r', 'train_d', 'alpha', 'thr_power',
                     'i_lo', 'i_hi', 'mask', 'row_count', 'db_map', 'peak_pow']
    assert re.search(r'#define\s+RSL_CFAR_MAX_C\s+512\b', src)


def test_library_exports_detect_cfar_and_rejects_null_handle():
    from rsl import _lib
    assert 'rsl_detect_cfar' in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, 'rsl_detect_cfar')
    rc = lib.rsl_detect_cfar(None, None, 1, 1, 64, 64, 2, 2, 8, 8, 9.0, -1.0, 0, 63, None, None, None, None)
    assert rc == _lib.RSL_ERR_INVALID == 1


def test_cfar_tables():
    from rsl import tables
    assert tables.cfar_training_cells((2, 2), (8, 8)) == 416
    assert tables.cfar_training_cells((1, 1), (4, 4)) == 112
    assert tables.cfar_training_cells((0, 1), (0, 6)) == 12
    assert tables.cfar_training_cells((1, 0), (5, 0)) == 10
    assert tables.cfar_alpha(1e-2, 416) == pytest.approx(4.63, abs=0.01)
    assert tables.cfar_alpha(1e-4, 416) == pytest.approx(9.31, abs=0.01)
    assert tables.cfar_alpha(1e-4, 12) == pytest.approx(13.9, abs=0.05)
    # Pfa = (1 + alpha / N)^-N inverted exactly
    for n in (10, 112, 416):
        a = tables.cfar_alpha(1e-3, n)
        assert (1 + a / n) ** (-n) == pytest.approx(1e-3, rel=1e-12)
    with pytest.raises(ValueError):
        tables.cfar_alpha(0.0, 16)


def test_chain_config_detector_option():
    from rsl.chain import ChainConfig
    assert ChainConfig().detector == 'threshold'
    c = ChainConfig(detector='cfar', cfar_pfa=1e-2)
    assert (c.cfar_guard, c.cfar_train, c.cfar_alpha) == ((2, 2), (8, 8), None)
    with pytest.raises(ValueError):
        ChainConfig(detector='nope')


@pytest.mark.parametrize('window', [(1, 1, 2, 2), (0, 1, 0, 3), (1, 0, 3, 0), (2, 1, 3, 3)])
def test_oracle_agrees_with_brute_force(window):
    rng = np.random.default_rng(3)
    z = (rng.standard_normal((12, 9)) + 1j * rng.standard_normal((12, 9))).astype(np.complex64)
    z[4, 4] = 30.0
    z[0, 8] = 20.0
    for alpha in (1.5, 4.0):
        ref = R.cfar_reference(z, window, alpha)
        assert (ref['mask'] == R.brute_force(R.power(z), window, alpha)).all()
    # the count of training cells: full window in the middle rows, truncated at the range edges
    _, n = R.training_sum(R.power(z), window)
    gr, gd, tr, td = window
    full = (2 * (gr + tr) + 1) * (2 * (gd + td) + 1) - (2 * gr + 1) * (2 * gd + 1)
    assert n[6] == full and n[11] == n[0]
    assert n[0] < full if tr else n[0] == full  # a Doppler-only window loses nothing at the range edges


def test_oracle_gate_and_floor():
    rng = np.random.default_rng(4)
    z = (rng.standard_normal((2, 20, 16)) + 1j * rng.standard_normal((2, 20, 16))).astype(np.complex64)
    free = R.cfar_reference(z, (1, 1, 2, 2), 2.0)['mask']
    gated = R.cfar_reference(z, (1, 1, 2, 2), 2.0, gate=(3, 10))['mask']
    assert (gated[:, 3:11] == free[:, 3:11]).all() and not gated[:, :3].any() and not gated[:, 11:].any()
    floor = R.cfar_reference(z, (1, 1, 2, 2), 2.0, thr_power=6.0)
    assert (floor['mask'] == (free & (floor['p'] > 6.0))).all()
    words = np.zeros((2, 20, 1), np.uint64)
    for a, i, j in zip(*np.nonzero(free)):
        words[a, i, 0] |= np.uint64(1) << np.uint64(j)
    assert (R.mask_bool(words, 16) == free).all()
