"""CPU checks of the CA-CFAR detector's host surface: the C ABI symbol, the alpha tables, the chain option and the
numpy oracle (tests/cfar_ref.py) that the GPU tests compare against.  What the OS-CFAR host file checks in the same
way is in tests/cfar_cases.py."""
import re

import numpy as np
import pytest

import cfar_cases as K
import cfar_ref as R


def test_header_declares_detect_cfar():
    K.header_declares('rsl_detect_cfar', [])
    assert re.search(r'#define\s+RSL_CFAR_MAX_C\s+512\b', K.header_source())


def test_library_exports_detect_cfar_and_rejects_null_handle():
    K.library_exports_and_rejects_null_handle('rsl_detect_cfar', [])


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
    # the factor of a design is one of the two tables, bit for bit
    assert tables.CFAR_METHODS == ('ca', 'os')
    assert tables.cfar_design_alpha('ca', 1e-2, (2, 2), (8, 8)) == tables.cfar_alpha(1e-2, 416)
    assert tables.cfar_design_alpha('os', 1e-2, (2, 2), (8, 8), 0.5) == tables.os_cfar_alpha(1e-2, 416, 208)


def test_chain_config_detector_option():
    from rsl.chain import ChainConfig
    assert ChainConfig().detector == 'threshold'
    c = ChainConfig(detector='cfar', cfar_pfa=1e-2)
    assert (c.cfar_guard, c.cfar_train, c.cfar_alpha) == ((2, 2), (8, 8), None)
    with pytest.raises(ValueError):
        ChainConfig(detector='nope')


@pytest.mark.parametrize('window', [(1, 1, 2, 2), (0, 1, 0, 3), (1, 0, 3, 0), (2, 1, 3, 3)])
def test_oracle_agrees_with_brute_force(window):
    z = K.brute_force_map()
    for alpha in (1.5, 4.0):
        ref = R.reference(z, window, alpha, method='ca')
        assert (ref['mask'] == R.brute_force(R.power(z), window, alpha)).all()
    K.check_training_cells(R.training_sum(R.power(z), window)[1], window)


def test_oracle_gate_and_floor():
    rng = np.random.default_rng(4)
    z = (rng.standard_normal((2, 20, 16)) + 1j * rng.standard_normal((2, 20, 16))).astype(np.complex64)
    free = R.reference(z, (1, 1, 2, 2), 2.0)['mask']
    gated = R.reference(z, (1, 1, 2, 2), 2.0, gate=(3, 10))['mask']
    assert (gated[:, 3:11] == free[:, 3:11]).all() and not gated[:, :3].any() and not gated[:, 11:].any()
    floor = R.reference(z, (1, 1, 2, 2), 2.0, thr_power=6.0)
    assert (floor['mask'] == (free & (floor['p'] > 6.0))).all()
    words = np.zeros((2, 20, 1), np.uint64)
    for a, i, j in zip(*np.nonzero(free)):
        words[a, i, 0] |= np.uint64(1) << np.uint64(j)
    assert (R.mask_bool(words, 16) == free).all()
