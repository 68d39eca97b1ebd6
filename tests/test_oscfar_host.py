"""CPU checks of the OS-CFAR detector's host surface: the C ABI symbol, the rank and alpha tables, the chain option
and the 'os' method of the numpy oracle (tests/cfar_ref.py) that the GPU tests compare against.  What the CA-CFAR
host file checks in the same way is in tests/cfar_cases.py."""
import math
import re

import numpy as np
import pytest

import cfar_cases as K
import cfar_ref as R


# -- 1. header and library ---------------------------------------------------------------------------------
def test_header_declares_detect_oscfar():
    K.header_declares('rsl_detect_oscfar', ['rank'])
    assert re.search(r'#define\s+RSL_VERSION\s+2\b', K.header_source())  # additive: the ABI version stays


def test_library_exports_detect_oscfar_and_rejects_null_handle():
    K.library_exports_and_rejects_null_handle('rsl_detect_oscfar', [0.75])


# -- 2. alpha ----------------------------------------------------------------------------------------------
def pfa_of(alpha, n, k):
    """The product formula, factor by factor."""
    out = 1.0
    for m in range(k):
        out *= (n - m) / (n - m + alpha)
    return out


def test_os_cfar_alpha():
    from rsl import tables
    for pfa in (1e-2, 1e-4, 1e-6):
        assert tables.os_cfar_alpha(pfa, 1, 1) == pytest.approx(1 / pfa - 1, rel=1e-12)
        assert tables.os_cfar_alpha(pfa, 2, 2) == pytest.approx((-3 + math.sqrt(1 + 8 / pfa)) / 2, rel=1e-12)
    for n, k in ((12, 9), (112, 84), (416, 312), (416, 208)):
        for pfa in (1e-2, 1e-4):
            assert pfa_of(tables.os_cfar_alpha(pfa, n, k), n, k) == pytest.approx(pfa, rel=1e-10)
    assert tables.os_cfar_alpha(1e-6, 16, 12) == pytest.approx(20.95, abs=0.01)  # Rohling's published value
    assert tables.os_cfar_alpha(1e-2, 416, 312) == pytest.approx(3.36, abs=0.01)
    assert tables.os_cfar_alpha(1e-4, 416, 312) == pytest.approx(6.78, abs=0.01)
    assert tables.os_cfar_alpha(1e-4, 12, 9) == pytest.approx(13.17, abs=0.01)
    for bad in ((0.0, 16, 12), (1.0, 16, 12), (-0.1, 16, 12), (1e-4, 16, 0), (1e-4, 16, 17), (1e-4, 0, 0)):
        with pytest.raises(ValueError):
            tables.os_cfar_alpha(*bad)


# -- 3. rank -----------------------------------------------------------------------------------------------
def test_os_cfar_rank():
    from rsl import tables
    assert tables.os_cfar_rank(416, .75) == 312
    assert tables.os_cfar_rank(112, .75) == 84
    assert tables.os_cfar_rank(12, .75) == 9
    assert tables.os_cfar_rank(10, .75) == 8
    assert tables.os_cfar_rank(10, .5) == 5
    for n in (1, 5, 416, 1088):
        assert tables.os_cfar_rank(n, 1.0) == n
    assert tables.os_cfar_rank(5, 0.01) == 1
    for bad in (0.0, -0.1, 1.0001, float('nan')):
        with pytest.raises(ValueError):
            tables.os_cfar_rank(10, bad)
    with pytest.raises(ValueError):
        tables.os_cfar_rank(0, 0.5)
    for n in (1, 7, 45, 84, 416):  # the oracle applies the same rule
        for rank in (1e-6, 0.5, 0.75, 1.0):
            assert R.rank_of(n, rank) == tables.os_cfar_rank(n, rank)


# -- 4. chain option ---------------------------------------------------------------------------------------
def test_chain_config_cfar_method():
    from rsl.chain import ChainConfig
    c = ChainConfig()
    assert (c.cfar_method, c.cfar_rank) == ('ca', 0.75)
    c = ChainConfig(detector='cfar', cfar_method='os', cfar_rank=0.5)
    assert (c.cfar_method, c.cfar_rank) == ('os', 0.5)
    with pytest.raises(ValueError):
        ChainConfig(detector='cfar', cfar_method='go')
    with pytest.raises(ValueError):
        ChainConfig(detector='cfar', cfar_method='os', cfar_rank=0)
    with pytest.raises(ValueError):
        ChainConfig(detector='cfar', cfar_method='os', cfar_rank=1.5)
    with pytest.raises(ValueError):
        ChainConfig(detector='os-cfar')  # the selector is a field of detector='cfar', not a detector name


# -- 5. oracle against the counting form -------------------------------------------------------------------
@pytest.mark.parametrize('window', [(1, 1, 2, 2), (0, 1, 0, 3), (1, 0, 3, 0), (2, 1, 3, 3)])
def test_oracle_agrees_with_counting_brute_force(window):
    z = K.brute_force_map()
    p32 = R.power(z).astype(np.float32)
    for rank in (0.5, 0.75, 1.0):
        for alpha in (1.5, 4.0):
            ref = R.reference(z, window, alpha, method='os', rank=rank)
            assert not ref['near'].any()
            assert (ref['mask'] == R.brute_force_count(p32, window, rank, alpha)).all(), (rank, alpha)
    ref = R.reference(z, window, 1.5, method='os', rank=0.75)
    k = ref['k']
    assert k[6] == R.rank_of(K.check_training_cells(ref['n'], window), 0.75)
    if window[2]:  # a truncated edge row keeps the fraction, not the rank
        assert k[0] < k[6] and k[11] < k[6]
    else:
        assert k[0] == k[6]


# -- 6. three reflectors inside each other's window --------------------------------------------------------
def test_masking_scene():
    from rsl import tables
    z = K.masking_scene()
    window, targets = (0, 1, 0, 6), [(20, 10), (20, 13), (20, 16)]
    n = tables.cfar_training_cells(window[:2], window[2:])
    assert n == 12
    ca = R.reference(z, window, tables.cfar_alpha(1e-4, n), method='ca')['mask']
    assert not any(ca[t] for t in targets)  # the targets raise each other's training mean
    k = tables.os_cfar_rank(n, 0.75)
    assert k == 9
    os_ = R.reference(z, window, tables.os_cfar_alpha(1e-4, n, k), method='os', rank=0.75)['mask']
    assert sorted(zip(*np.nonzero(os_))) == targets


# -- 7. false-alarm rate -----------------------------------------------------------------------------------
def test_false_alarm_rate():
    """Level crossings p > alpha x_(k) of unit-power noise at the design Pfa 1e-2: +-20 % is about 3.5 binomial sigma
    at 30 k interior cells (sigma = sqrt(1e-2 * 0.99 / 30208) = 5.7e-4)."""
    from rsl import tables
    rng = np.random.default_rng(2024)
    S, Cn = 256, 128
    z = ((rng.standard_normal((S, Cn)) + 1j * rng.standard_normal((S, Cn))) / math.sqrt(2)).astype(np.complex64)
    window = (1, 1, 4, 4)
    alpha = tables.cfar_design_alpha('os', 1e-2, window[:2], window[2:], 0.75)
    ref = R.reference(z, window, alpha, method='os', rank=0.75)
    inner = slice(10, S - 10)
    rate = float((ref['p'][inner] > ref['level'][inner]).mean())
    print(f'\nOS-CFAR level crossings: {rate:.5f} at design 1e-2')
    assert 0.8e-2 <= rate <= 1.2e-2
