"""GPU tests of the OS-CFAR detector (rsl_detect_oscfar / k_detect_oscfar) against the fp64 numpy oracle in
tests/cfar_ref.py.  The cases themselves are in tests/cfar_cases.py, shared with test_gpu_cfar.py; this file runs them
with the OS detector (rank 0.75 where the case does not say) and holds what only OS-CFAR is asked: ranks, masking."""
import pytest

import cfar_cases as K
import cfar_ref as R
from cfar_cases import BAD, CA, DEFAULT, LARGEST, OS, WINDOWS

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def chains(ctx):
    return K.chains(ctx)


# -- 1. oracle parity ----------------------------------------------------------------------------------
@pytest.mark.parametrize('pfa', [1e-2, 1e-4])
@pytest.mark.parametrize('rank', [0.75, 0.5])
@pytest.mark.parametrize('window', WINDOWS)
def test_oracle_parity(ctx, window, rank, pfa):
    """Rows 0 .. hr-1 and S-hr .. S-1 have a truncated window (k = 45 against 84 at (1, 1, 4, 4), rank 0.75).  The
    narrow OS band may hold 2 cells at the most."""
    K.oracle_parity(ctx, ('os', rank), window, pfa, cap=2)


# -- 2. strong cells --------------------------------------------------------------------------------------
@pytest.mark.parametrize('window', WINDOWS)
def test_strong_cells(ctx, window):
    K.strong_cells(ctx, OS, window)


# -- 3. masking: three equal reflectors inside each other's window ------------------------------------------
def test_masking_on_device(ctx):
    host = K.masking_scene()[None, None]
    dev = ctx.to_dev(host)
    window, targets = (0, 1, 0, 6), [(20, 10), (20, 13), (20, 16)]
    ca = K.run(ctx, CA, dev, window, K.alpha_for(CA, window, 1e-4))
    cm = R.mask_bool(ca['mask'], 32)[0, 0]
    assert not any(cm[t] for t in targets)
    alpha = K.alpha_for(OS, window, 1e-4)
    got = K.run(ctx, OS, dev, window, alpha)
    gm = K.check_against_oracle('masking', OS, host, window, alpha, got)[0, 0]
    assert all(gm[t] for t in targets)


# -- 4. shapes; the last: the largest window (hr = hd = RSL_CFAR_MAX_HALF) at [1, 1, 40, 512] ------------------
@pytest.mark.parametrize('S,C,window', [(50, 100, DEFAULT), (21, 21, DEFAULT), (200, 64, DEFAULT),
                                        (130, 128, DEFAULT), (40, 512, DEFAULT), (40, 512, LARGEST)])
def test_shapes(ctx, S, C, window):
    K.shapes(ctx, OS, S, C, window)


# -- 5. degenerate maps -----------------------------------------------------------------------------------
def test_degenerate_maps(ctx):
    K.degenerate_maps(ctx, OS)


@pytest.mark.parametrize('rank,alpha', [(1.0, 0.6), (1e-6, 30.0)])
def test_extreme_ranks(ctx, rank, alpha):
    """rank 1: the window maximum (k = n(i)); a tiny rank: the minimum (k = 1)."""
    host = K.noise((1, 2, 48, 64), 77)
    window, det = (1, 1, 4, 4), ('os', rank)
    got = K.run(ctx, det, ctx.to_dev(host), window, alpha)
    gm = K.check_against_oracle(f'rank {rank}', det, host, window, alpha, got)
    assert gm.any() and not gm.all()


# -- 6. arguments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,guard,train,alpha', BAD)
def test_bad_arguments(ctx, shape, guard, train, alpha):
    K.bad_arguments(ctx, OS, shape, guard, train, alpha)


@pytest.mark.parametrize('rank', [0.0, -0.1, 1.0001, float('nan')])
def test_bad_rank(ctx, rank):
    torch = ctx.torch
    rds = torch.zeros((1, 1, 64, 64), dtype=torch.complex64, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.detect_oscfar(rds, (2, 2), (8, 8), rank, 5.0, -1.0, 0, 63)


# -- 7. empty batch ---------------------------------------------------------------------------------------
def test_empty_batch_launches_nothing(ctx):
    K.empty_batch_launches_nothing(ctx, OS)


# -- 8. chain ---------------------------------------------------------------------------------------------
def test_chain_oscfar_entries_and_cells(chains):
    from rsl import tables
    K.chain_entries_and_cells(chains['os'], OS, tables.os_cfar_alpha(1e-2, 416, 312))


def test_chain_oscfar_cells_match_default_chain(chains):
    K.chain_cells_match_default_chain(chains['os'], chains['plain'])


def test_chain_method_ca_is_the_cfar_chain(chains):
    a, b = chains['cfar'], chains['ca']
    assert a['chain'].cfar_alpha == b['chain'].cfar_alpha
    K.chain_same_results(a, b)


def test_chain_oscfar_no_detection(chains):
    K.chain_no_detection(chains['none-os'])


# -- 9. drop-in -------------------------------------------------------------------------------------------
def test_dropin_oscfar(ctx):
    from rsl import ops
    _, rds, _, _ = K.dropin_against_ops(ctx, method='os')
    ca = ops.detect_peaks_cfar(rds, pfa=1e-2, ctx=ctx)  # the default method is 'ca', as before
    assert ca['antenna'].tolist() == ops.detect_peaks_cfar(rds, pfa=1e-2, method='ca', ctx=ctx)['antenna'].tolist()
    with pytest.raises(ValueError):
        ops.detect_peaks_cfar(rds, pfa=1e-2, method='go', ctx=ctx)
