"""GPU tests of the CA-CFAR detector (rsl_detect_cfar / k_detect_cfar) against the fp64 numpy oracle in
tests/cfar_ref.py.  The cases themselves are in tests/cfar_cases.py, shared with test_gpu_oscfar.py; this file runs
them with the CA detector and holds what only the CA chain is asked."""
import numpy as np
import pytest

import cfar_cases as K
import parity as P
import radar_oracle as O
from cfar_cases import BAD, CA, CH, LARGEST, WINDOWS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def chains(ctx):
    return K.chains(ctx)


# -- 1. oracle parity ----------------------------------------------------------------------------------
@pytest.mark.parametrize('pfa', [1e-2, 1e-4])
@pytest.mark.parametrize('window', WINDOWS)
def test_oracle_parity(ctx, window, pfa):
    K.oracle_parity(ctx, CA, window, pfa)


# -- 2. strong cells: the add-only training sum -----------------------------------------------------------
@pytest.mark.parametrize('window', WINDOWS)
def test_strong_cells(ctx, window):
    K.strong_cells(ctx, CA, window)


# -- 3. shapes; the last: the kernel's largest LDS request (162 816 B), on the noise map of the OS case ---------
@pytest.mark.parametrize('S,C,window', [(50, 100, K.DEFAULT), (21, 21, K.DEFAULT), (200, 64, K.DEFAULT),
                                        (130, 128, K.DEFAULT), (40, 512, K.DEFAULT), (40, 512, LARGEST)],
                         ids=['50-100', '21-21', '200-64', '130-128', '40-512', '40-512-largest'])
def test_shapes(ctx, S, C, window):
    K.shapes(ctx, CA, S, C, window)


# -- 4. degenerate maps -----------------------------------------------------------------------------------
def test_degenerate_maps(ctx):
    K.degenerate_maps(ctx, CA)


# -- 5. arguments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,guard,train,alpha', BAD)
def test_bad_arguments(ctx, shape, guard, train, alpha):
    K.bad_arguments(ctx, CA, shape, guard, train, alpha)


def test_empty_batch_launches_nothing(ctx):
    K.empty_batch_launches_nothing(ctx, CA)


# -- 6. chain ---------------------------------------------------------------------------------------------
def test_chain_cfar_entries_and_cells(chains):
    from rsl import tables
    K.chain_entries_and_cells(chains['cfar'], CA, tables.cfar_alpha(1e-2, 416))


def test_chain_cfar_cells_match_default_chain(chains):
    K.chain_cells_match_default_chain(chains['cfar'], chains['plain'])


def test_chain_cfar_velocity(chains):
    r = chains['cfar']
    cb, grid = r['cell_base'], r['grid']
    for f in range(2):
        sl = slice(cb[f], cb[f + 1])
        w = np.array([bin(int(m) & 0xffffffff).count('1') for m in r['c_amask'][sl]])
        az = np.repeat(np.radians(grid[r['gidx'][sl]]), w)
        y = np.repeat(r['phase'][sl], w)
        assert len(y) >= 3
        vx, vy, cost = O.velocity_ls(az, y, lambda_c=3e8 / 77e9)
        v = r['velocity'][f]
        assert abs(v[2] - cost) <= P.VEL_COST_RTOL * cost
        assert abs(v[0] - vx) < P.VEL_ATOL and abs(v[1] - vy) < P.VEL_ATOL
        assert int(v[5]) == len(y)


def test_chain_threshold_detector_unchanged(chains):
    K.chain_same_results(chains['plain'], chains['threshold'])


def test_chain_cfar_no_detection(chains):
    K.chain_no_detection(chains['none-ca'])


def test_chain_rejects_unknown_detector():
    import rsl
    with pytest.raises(ValueError):
        rsl.ChainConfig(**CH, detector='os-cfar')


# -- 7. drop-in -------------------------------------------------------------------------------------------
def test_dropin_cfar(ctx):
    pre, rds, out, got = K.dropin_against_ops(ctx)
    assert out['power_spectrum_db'].shape == rds.shape
    # the default range gate (1 m .. 200 m) only removes rows
    gated = pre.extract_range_doppler_peaks_cfar(rds, pfa=1e-2)
    assert set((p['antenna'], int(p['range_bin']), int(p['doppler_bin'])) for p in gated['peaks']) <= set(got)
