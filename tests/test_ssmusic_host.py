"""CPU checks of the spatially smoothed MUSIC's host surface: the numpy oracle (tests/ssmusic_ref.py) that the GPU tests
compare against -- its resolution against beamforming, its two forms of the null spectrum, its covariance -- and the
C ABI symbol, the ctypes row, the sub-array steering table and the chain options."""
import os
import re

import numpy as np
import pytest

import ssmusic_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'rsl.h')
GRID = np.arange(-90.0, 90.25, 0.5)


@pytest.mark.parametrize('L', [5, 6])
def test_oracle_resolves_what_beamforming_cannot(L):
    """Two coherent sources 10 degrees apart (beamwidth of 8 elements: about 14 degrees), 30 dB: smoothed MUSIC finds
    both within +-2 degrees in >= 95 % of the cells, the two highest beamforming peaks in <= 5 %."""
    M = 8
    sigs, theta = R.two_sources(2000, M, 10, 30, 11)
    steer = R.steering(GRID, M)
    ref = R.reference(sigs, steer[:, :L], L, 3, num_sources=2)
    picks = np.where(ref['idx'] >= 0, GRID[np.clip(ref['idx'], 0, None)], np.nan)
    rate = R.resolved(picks, theta)
    bf = R.beamforming_two_peaks(sigs, steer)
    bf_rate = R.resolved(np.where(bf >= 0, GRID[np.clip(bf, 0, None)], np.nan), theta)
    print(f'L={L}: smoothed MUSIC {rate:.3f}, beamforming peaks {bf_rate:.3f}')
    assert rate >= 0.95
    assert bf_rate <= 0.05
    assert (ref['nsrc'] == 2).all() and (ref['idx'][:, 2] == -1).all()
    # picks are listed in ascending den
    assert (np.diff(ref['den'][:, :2], axis=1) >= 0).all()


@pytest.mark.parametrize('M,L', [(8, 6), (16, 8), (4, 3)])
def test_oracle_noise_and_signal_side_agree(M, L):
    sigs, _ = R.two_sources(200, M, 15, 30, 3)
    st = R.steering(GRID, M)[:, :L]
    for k in (0, 1, min(2, L - 1)):
        a = R.reference(sigs, st, L, L - 1, num_sources=k)
        b = R.reference(sigs, st, L, L - 1, num_sources=k, signal_side=True)
        assert np.abs(a['spec'] - b['spec']).max() <= 1e-12
        # den in [0, ||a_g||^2], and ||a_g||^2 = L up to the c64 rounding of the steering values
        assert a['spec'].min() >= -1e-12 and a['spec'].max() <= L * (1 + 1e-6)


def test_oracle_covariance_is_hermitian_with_trace_one():
    for M, L in ((8, 6), (8, 8), (16, 8), (3, 2)):
        sigs = R.noise_sigs(50, M, 2).astype(np.complex128)
        sigs /= np.linalg.norm(sigs, axis=1, keepdims=True)
        Rm = R.covariance(sigs, L)
        assert np.abs(Rm - Rm.conj().transpose(0, 2, 1)).max() <= 1e-15
        # trace = the mean power of the sub-arrays; persymmetric by the backward term
        K = M - L + 1
        tr = np.array([(np.abs(sigs[:, k:k + L]) ** 2).sum(axis=1) for k in range(K)]).mean(axis=0)
        assert np.abs(np.trace(Rm, axis1=1, axis2=2).real - tr).max() <= 1e-14
        assert np.abs(Rm - Rm[:, ::-1, ::-1].conj()).max() <= 1e-15
    # L = M (one sub-array): trace exactly the signature's power, 1
    Rm = R.covariance(sigs, 3)
    assert np.abs(np.trace(Rm, axis1=1, axis2=2).real - 1.0).max() <= 1e-14


def test_oracle_degenerate_cells():
    st = R.steering(GRID, 8)[:, :6]
    sigs = np.zeros((2, 8), np.complex64)
    sigs[1] = R.steering([GRID[200]], 8)[0]
    ref = R.reference(sigs, st, 6, 3)
    assert ref['nsrc'].tolist() == [0, 1]
    assert (ref['idx'][0] == -1).all() and np.isnan(ref['den'][0]).all() and np.isnan(ref['spec'][0]).all()
    assert ref['idx'][1].tolist() == [200, -1, -1] and ref['den'][1, 0] <= 1e-12


def test_header_declares_doa_smoothed():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    m = re.search(r'int\s+rsl_doa_smoothed\s*\(([^)]*)\)', src)
    assert m, 'rsl_doa_smoothed not declared in include/rsl.h'
    names = [a.strip().split()[-1].lstrip('*') for a in m.group(1).split(',')]
    assert names == ['h', 'rds', 'A', 'S', 'C', 'c_frame', 'c_rc', 'ncell_dev', 'ncell', 'steer_sub_c64', 'G', 'L',
                     'nmax', 'num_sources', 'rel', 'out_nsrc', 'out_idx', 'out_den', 'out_eig', 'out_spec']
    assert re.search(r'#define\s+RSL_SS_MAX_L\s+8\b', src)
    assert re.search(r'#define\s+RSL_SS_MAX_SWEEPS\s+\d+\b', src) and re.search(r'#define\s+RSL_SS_OFF_TOL\s+\S+', src)
    assert re.search(r'#define\s+RSL_VERSION\s+2\b', src) and re.search(r'#define\s+RSL_K_COUNT\s+10\b', src)


def test_library_exports_doa_smoothed_and_rejects_null_handle():
    from rsl import _lib
    assert 'rsl_doa_smoothed' in _lib.SIGNATURES
    assert len(_lib.SIGNATURES['rsl_doa_smoothed'][1]) == 20
    lib = _lib.load()
    assert hasattr(lib, 'rsl_doa_smoothed')
    rc = lib.rsl_doa_smoothed(None, None, 8, 1, 1, None, None, None, 4, None, 361, 6, 3, 0, 0.05, None, None, None,
                              None, None)
    assert rc == _lib.RSL_ERR_INVALID == 1


def test_subarray_steering():
    from rsl import tables
    lam = 3e8 / 77e9
    st = tables.steering_matrix(GRID, np.arange(8) * lam / 2, lam)
    sub = tables.subarray_steering(st, 6)
    assert sub.shape == (len(GRID), 6) and sub.dtype == np.complex128
    assert np.array_equal(sub, st[:, :6])
    assert np.abs(sub - R.steering(GRID, 6)).max() <= 1e-12
    # an array whose first element is not the phase reference: the same sub-array vectors
    off = tables.steering_matrix(GRID, (np.arange(8) + 3) * lam / 2, lam)
    assert np.abs(tables.subarray_steering(off, 6) - sub).max() <= 1e-12
    pos = np.arange(8) * lam / 2
    pos[3] += 0.1 * lam
    with pytest.raises(ValueError):
        tables.subarray_steering(tables.steering_matrix(GRID, pos, lam), 6)
    with pytest.raises(ValueError):
        tables.subarray_steering(st, 9)
    with pytest.raises(ValueError):
        tables.subarray_steering(st, 1)
    assert [tables.default_sub_len(m) for m in (3, 4, 8, 12, 16)] == [2, 3, 6, 8, 8]


def test_chain_config_multi_source_options():
    from rsl.chain import ChainConfig
    c = ChainConfig()
    assert (c.multi_source, c.ss_len, c.ss_sources, c.ss_rel, c.ss_max) == (False, None, 0, 0.05, 3)
    c = ChainConfig(multi_source=True, ss_len=5, ss_sources=2, ss_rel=0.01, ss_max=4)
    assert c.ss_sub_len == 5
    assert ChainConfig(multi_source=True).ss_sub_len == 6
    assert ChainConfig(num_antennas=16, multi_source=True).ss_sub_len == 8
    for bad in (dict(ss_len=1), dict(ss_len=9), dict(ss_max=0), dict(ss_sources=-1), dict(ss_sources=4),
                dict(ss_rel=0.0), dict(ss_rel=1.0), dict(ss_rel=float('nan')),
                dict(multi_source=True, num_antennas=2), dict(multi_source=True, num_antennas=17),
                dict(multi_source=True, num_antennas=4, ss_len=6),
                dict(multi_source=True, num_antennas=4, ss_sources=3)):
        with pytest.raises(ValueError):
            ChainConfig(**bad)
