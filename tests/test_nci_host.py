"""CPU checks of detection on the antenna-summed power map (non-coherent integration): the oracle helper
tests/nci_ref.py pinned to tests/cfar_ref.py, the false-alarm designs for a sum of L looks (rsl/tables.py), the scene
that motivates the feature (on the oracle alone) and the host surface of rsl_power_integrate / rsl_detect_power."""
import math
import re

import numpy as np
import pytest

import cfar_cases as K
import cfar_ref as R
import nci_ref as N

DEFAULT_N = 416  # training cells of the default window (2, 2, 8, 8)


# -- the helper is the existing oracle ----------------------------------------------------------------------
@pytest.mark.parametrize('method,rank', [('ca', None), ('os', 0.75)])
def test_reference_power_is_cfar_reference(method, rank):
    cases = [(K.brute_force_map(), (1, 1, 2, 2), 1.5), (K.brute_force_map(), (2, 1, 3, 3), 4.0),
             (K.noise((2, 64, 32), 21), (1, 1, 4, 4), 3.0), (K.noise((2, 64, 32), 21), K.DEFAULT, 5.0)]
    for z, window, alpha in cases:
        for kw in (dict(), dict(thr_power=1.5, gate=(3, z.shape[-2] - 4))):
            want = R.reference(z, window, alpha, method=method, rank=rank, **kw)
            got = N.reference_power(R.power(z), window, alpha, method=method, rank=rank, **kw)
            assert set(got) == set(want)
            for key in ('mask', 'level', 'near', 'p', 'nbmax'):
                assert np.array_equal(got[key], want[key]), (key, window)
    assert N.near_cap is R.near_cap and N.diff is R.diff


def test_reference_power_threshold_rule():
    z = K.noise((2, 20, 16), 4)
    p = R.power(z)
    free = N.reference_power(p, None, 0.0, method='threshold')
    assert (free['mask'] == (p >= R.neighbour_max(p))).all()
    thr = N.reference_power(p, None, 0.0, method='threshold', thr_power=1.0, gate=(3, 10))
    assert (thr['mask'][:, 3:11] == (free['mask'] & (p > 1.0))[:, 3:11]).all()
    assert not thr['mask'][:, :3].any() and not thr['mask'][:, 11:].any()


def test_integrate_is_the_antenna_sum():
    z = K.noise((2, 3, 5, 4), 1)
    want = sum(R.power(z[:, a]) for a in range(3))
    assert np.allclose(N.integrate(z), want, rtol=1e-15) and N.integrate(z).shape == (2, 5, 4)


# -- the designs for a sum of L looks -----------------------------------------------------------------------
@pytest.mark.parametrize('guard,train', [((2, 2), (8, 8)), ((1, 1), (4, 4))])
def test_design_alpha_with_one_look_is_todays(guard, train):
    from rsl import tables
    for method in ('ca', 'os'):
        for pfa in (1e-2, 1e-4):
            assert tables.cfar_design_alpha(method, pfa, guard, train, 0.75, looks=1) == \
                tables.cfar_design_alpha(method, pfa, guard, train, 0.75)


def test_ca_known_answers():
    from rsl import tables
    assert tables.cfar_alpha_nci(1e-2, 16, 8) == pytest.approx(2.071078504113302, rel=1e-9)
    assert tables.cfar_alpha_nci(1e-3, 264, 8) == pytest.approx(2.460614244475849, rel=1e-9)
    for L, a in ((3, 2.8092), (4, 2.5166), (8, 2.0027), (16, 1.6729)):
        assert tables.cfar_design_alpha('ca', 1e-2, (2, 2), (8, 8), looks=L) == pytest.approx(a, abs=1e-4)
    # one look: today's closed form
    assert tables.cfar_pfa_nci(4.0, 16, 1) == pytest.approx((1 + 4.0 / 16) ** -16, rel=1e-13)
    assert tables.cfar_alpha_nci(1e-3, DEFAULT_N, 1) == pytest.approx(tables.cfar_alpha(1e-3, DEFAULT_N), rel=1e-12)


@pytest.mark.parametrize('n,L,p', [(16, 8, 1e-2), (264, 8, 1e-3), (DEFAULT_N, 4, 1e-4), (DEFAULT_N, 16, 1e-6),
                                   (12, 2, 1e-2), (1088, 32, 1e-4)])
def test_ca_round_trip(n, L, p):
    from rsl import tables
    assert tables.cfar_pfa_nci(tables.cfar_alpha_nci(p, n, L), n, L) == pytest.approx(p, rel=1e-9)


@pytest.mark.parametrize('n,k', [(DEFAULT_N, 312), (16, 12), (80, 60), (10, 1), (12, 12), (1088, 816)])
def test_os_with_one_look_is_rohlings_product(n, k):
    from rsl import tables
    for alpha in (0.5, 3.0, 20.0):
        assert tables.os_cfar_pfa_nci(alpha, n, k, 1) == pytest.approx(tables.os_cfar_pfa(alpha, n, k), rel=1e-8)


@pytest.mark.parametrize('n,k,L,p', [(80, 60, 8, 1e-2), (DEFAULT_N, 312, 8, 1e-4), (DEFAULT_N, 208, 4, 1e-6),
                                     (12, 9, 2, 1e-2), (1088, 816, 16, 1e-3)])
def test_os_round_trip(n, k, L, p):
    from rsl import tables
    assert tables.os_cfar_pfa_nci(tables.os_cfar_alpha_nci(p, n, k, L), n, k, L) == pytest.approx(p, rel=1e-6)


def test_alpha_falls_with_looks_and_rises_as_pfa_falls():
    from rsl import tables
    for design in (lambda p, L: tables.cfar_alpha_nci(p, DEFAULT_N, L),
                   lambda p, L: tables.os_cfar_alpha_nci(p, DEFAULT_N, 312, L),
                   lambda p, L: tables.cfar_design_alpha('os', p, (1, 1), (4, 4), 0.75, looks=L)):
        by_looks = [design(1e-4, L) for L in (1, 2, 3, 4, 8, 16)]
        assert all(a > b for a, b in zip(by_looks, by_looks[1:])), by_looks
        by_pfa = [design(p, 8) for p in (1e-2, 1e-3, 1e-4, 1e-6)]
        assert all(a < b for a, b in zip(by_pfa, by_pfa[1:])), by_pfa


def test_design_arguments():
    from rsl import tables
    for bad in (0, 33, 2.5):
        with pytest.raises(ValueError):
            tables.cfar_alpha_nci(1e-2, 16, bad)
        with pytest.raises(ValueError):
            tables.os_cfar_alpha_nci(1e-2, 16, 12, bad)
    with pytest.raises(ValueError):
        tables.cfar_alpha_nci(0.0, 16, 8)
    with pytest.raises(ValueError):
        tables.os_cfar_alpha_nci(1e-2, 16, 17, 8)


def test_designs_by_monte_carlo():
    """N = 80 training cells, L = 8 looks, Pfa 1e-2, 4e5 seeded draws: the observed rate of each design lies within
    four binomial standard deviations of the design rate."""
    from rsl import tables
    n, L, pfa, draws, k = 80, 8, 1e-2, 400_000, 60
    sd = math.sqrt(pfa * (1 - pfa) / draws)
    rng = np.random.default_rng(2024)
    cut = rng.gamma(L, size=draws)
    # CA: the training sum of n Gamma(L) cells is Gamma(n L)
    a_ca = tables.cfar_alpha_nci(pfa, n, L)
    rate = float((cut > a_ca * rng.gamma(n * L, size=draws) / n).mean())
    print(f'\nCA alpha {a_ca:.6f}: rate {rate:.5f}, design {pfa}, sd {sd:.2e}')
    assert abs(rate - pfa) <= 4 * sd
    # OS: the k-th smallest of n Gamma(L) cells, in blocks
    a_os = tables.os_cfar_alpha_nci(pfa, n, k, L)
    hits = 0
    for b in range(0, draws, 50_000):
        xk = np.partition(rng.gamma(L, size=(50_000, n)), k - 1, axis=1)[:, k - 1]
        hits += int((cut[b:b + 50_000] > a_os * xk).sum())
    rate = hits / draws
    print(f'OS alpha {a_os:.6f}: rate {rate:.5f}, design {pfa}, sd {sd:.2e}')
    assert abs(rate - pfa) <= 4 * sd


# -- the motivating scene, on the oracle alone ----------------------------------------------------------------
def test_motivating_scene_on_the_oracle():
    from rsl import tables
    z, cells = N.motivating_scene()
    assert len(cells) == 54
    ii, jj = np.array(cells).T
    window, pfa = (2, 2, 8, 8), 1e-4
    per = R.reference(z, window, tables.cfar_design_alpha('ca', pfa, window[:2], window[2:]), method='ca')
    union = per['mask'][0].any(axis=0)
    held = int(union[ii, jj].sum())
    print(f'\nper-antenna union: {held} of 54 reflectors, {int(union.sum()) - held} other cells')
    assert held < 40
    alpha = tables.cfar_design_alpha('ca', pfa, window[:2], window[2:], looks=8)
    summed = N.reference_power(N.integrate(z), window, alpha, method='ca')['mask'][0]
    held_s = int(summed[ii, jj].sum())
    print(f'integrated: {held_s} of 54 reflectors, {int(summed.sum()) - held_s} other cells')
    assert held_s == 54
    assert int(summed.sum()) - held_s <= 5


# -- host surface -----------------------------------------------------------------------------------------------
def _declared(fn):
    m = re.search(rf'int\s+{fn}\s*\(([^)]*)\)', K.header_source())
    assert m, f'{fn} not declared in include/rsl.h'
    return [a.strip().split()[-1].lstrip('*') for a in m.group(1).split(',')]


def test_header_declares_the_entry_points():
    assert _declared('rsl_power_integrate') == ['h', 'rds', 'F', 'A', 'S', 'C', 'power']
    assert _declared('rsl_detect_power') == ['h', 'power', 'F', 'S', 'C', 'rule', 'guard_r', 'guard_d', 'train_r',
                                             'train_d', 'rank', 'alpha', 'thr_power', 'i_lo', 'i_hi', 'mask',
                                             'row_count', 'db_map', 'peak_pow']
    src = K.header_source()
    for name, value in (('RSL_RULE_THRESHOLD', 0), ('RSL_RULE_CA', 1), ('RSL_RULE_OS', 2)):
        assert re.search(rf'#define\s+{name}\s+{value}\b', src)
    assert re.search(r'#define\s+RSL_K_COUNT\s+10\b', src) and re.search(r'#define\s+RSL_VERSION\s+2\b', src)


def test_library_exports_and_rejects_null_handle():
    from rsl import _lib
    assert (_lib.RULE_THRESHOLD, _lib.RULE_CA, _lib.RULE_OS) == (0, 1, 2)
    lib = _lib.load()
    for fn in ('rsl_power_integrate', 'rsl_detect_power'):
        assert fn in _lib.SIGNATURES and hasattr(lib, fn)
    assert lib.rsl_power_integrate(None, None, 1, 8, 64, 64, None) == _lib.RSL_ERR_INVALID == 1
    assert lib.rsl_detect_power(None, None, 1, 64, 64, _lib.RULE_CA, 2, 2, 8, 8, 0.75, 9.0, -1.0, 0, 63, None, None,
                                None, None) == _lib.RSL_ERR_INVALID


def test_chain_config_detect_on_option():
    from rsl.chain import ChainConfig
    assert ChainConfig().detect_on == 'antenna'
    assert ChainConfig(detect_on='sum', detector='cfar').detect_on == 'sum'
    with pytest.raises(ValueError):
        ChainConfig(detect_on='x')


def test_integrate_kernel_has_no_packed_fp32(tmp_path):
    """k_power_integrate runs in the chain step with detect_on='sum': like the kernels test_no_packed_fp32.py guards it
    is compiled under no-packed-fp32-ops; both of its forms must be in the library and hold no v_pk_* FP32."""
    import os
    from collections import Counter
    import test_no_packed_fp32 as T
    if not all(os.path.exists(os.path.join(T.LLVM, tool)) for tool in ('llvm-objdump', 'llvm-objcopy')):
        pytest.skip('ROCm llvm tools absent')
    funcs = Counter()
    for j, co in enumerate(T.gfx950_code_objects(T.LIB, str(tmp_path))):
        funcs.update(T.packed_fp32_by_function(co, str(tmp_path), f'co{j}'))
    mine = {n: c for n, c in funcs.items() if re.search(r'\brsl::k_power_integrate<', n)}
    assert len(mine) == 2, list(mine)
    assert not any(mine.values()), mine
    # the real-element instances of the three detectors exist next to the complex ones
    for k in ('k_detect', 'k_detect_cfar', 'k_detect_oscfar'):
        for elem in ('float', 'HIP_vector_type<float, 2u>'):
            assert any(re.search(rf'\brsl::{k}<{re.escape(elem)}>', n) for n in funcs), (k, elem)
