"""GPU tests of the robust velocity solve (rsl_velocity_robust / k_velocity_robust) against the fp64 numpy oracle in
tests/vel_robust_ref.py, with the tolerances derived in that module's docstring.  Every comparison first asserts, on the
oracle alone, what its tolerance presupposes (condition number, cells at the cut-off, contraction rate)."""
import numpy as np
import pytest

import radar_oracle as O
import vel_robust_ref as R

pytestmark = pytest.mark.gpu

K = R.K_CHAIN
LOSSES = [('huber', R.LOSS_HUBER), ('tukey', R.LOSS_TUKEY)]
# one launch; 512 and 4096 are the thread and trip boundaries of the 512 x 8 loop; the empty frame sits in the middle
PARITY_LENGTHS = [513, 1, 4097, 0, 2, 9000, 3, 511, 512]
RIDGE = 1e5  # about k^2: keeps the 1- to 3-cell frames well posed (condition number <= 1 + 1.04 * sum m <= 26)


def dev(ctx, d, az_path=False, with_mask=True):
    """Device copies of a concat()-style dictionary."""
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
    return dict(az=ctx.to_dev(pad(d['az'])) if az_path else None, gidx=None if az_path else ctx.to_dev(pad(d['gidx'])),
                y=ctx.to_dev(pad(d['y'])), amask=ctx.to_dev(pad(d['amask'])) if with_mask else None,
                seg=ctx.to_dev(d['seg']))


def run_gpu(ctx, d, dd, *, G=361, n=None, **kw):
    """rsl_velocity_robust on the arrays of dev(); weight / resid buffers pre-filled with NaN (untouched slots stay)."""
    torch = ctx.torch
    N = len(d['y'])
    tab = ctx.to_dev(R.grid_rad(G)) if dd['gidx'] is not None else None
    w = torch.full((max(N, 1),), float('nan'), dtype=torch.float32, device=ctx.device)
    out, w, r = ctx.velocity_robust(dd['az'], dd['y'], dd['seg'], k=K, amask=dd['amask'], gidx=dd['gidx'],
                                    az_table=tab, n=N if n is None else n, want_weight=w, want_resid=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), w.cpu().numpy().astype(np.float64)[:N], r.cpu().numpy()[:N]


def make_batch(lengths, share=0.25, seed0=100, **kw):
    return R.concat([R.planted(n, share, seed=seed0 + i, **kw) for i, n in enumerate(lengths)])


@pytest.fixture(scope='module')
def parity_batch(ctx):
    d = make_batch(PARITY_LENGTHS)
    assert (d['m'] == 0).any() and d['seg'][-1] == sum(PARITY_LENGTHS)
    return d, dev(ctx, d)


# -- 1. parity with the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize('scale', [0.05, None], ids=['fixed', 'auto'])
@pytest.mark.parametrize('loss', ['huber', 'tukey'])
def test_oracle_parity(ctx, parity_batch, loss, scale):
    d, dd = parity_batch
    kw = dict(loss=loss, scale=scale, iters=20, tol=0.0, ridge=RIDGE)
    ref = R.robust_batch(d['az'], d['y'], d['m'], d['seg'], k=K, **kw)
    out, w, r = run_gpu(ctx, d, dd, **kw)
    print()
    R.compare(f'{loss}/{scale}', out, w, r, ref, tol=0.0)
    assert (out[:, 7] >= 0).all()  # tol = 0 never reports a missed stop rule
    assert not np.isnan(w).any() and not np.isnan(r).any()  # every cell of every frame was written


# -- 2. other paths ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['huber', 'tukey'])
def test_az_path_without_masks(ctx, loss):
    d = make_batch([3, 513], seed0=200, mmax=0)
    dd = dev(ctx, d, az_path=True, with_mask=False)
    for scale in (0.05, None):
        kw = dict(loss=loss, scale=scale, iters=12, tol=0.0, ridge=RIDGE)
        ref = R.robust_batch(d['az'], d['y'], None, d['seg'], k=K, **kw)
        out, w, r = run_gpu(ctx, d, dd, **kw)
        print()
        R.compare(f'az {loss}/{scale}', out, w, r, ref, tol=0.0)
        assert (out[:, 5] == [3, 513]).all()


@pytest.mark.parametrize('loss', ['huber', 'tukey'])
def test_small_grid(ctx, loss):
    d = make_batch([100, 7], seed0=300, G=5)
    dd = dev(ctx, d)
    kw = dict(loss=loss, scale=None, iters=12, tol=0.0, ridge=RIDGE)
    ref = R.robust_batch(d['az'], d['y'], d['m'], d['seg'], k=K, **kw)
    out, w, r = run_gpu(ctx, d, dd, G=5, **kw)
    print()
    R.compare(f'G=5 {loss}', out, w, r, ref, tol=0.0)


# -- 3. early stop ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss,scale', [('tukey', 0.05), ('huber', 0.05), ('tukey', None)])
def test_early_stop(ctx, loss, scale):
    d = make_batch([40, 3000], seed0=400)
    dd = dev(ctx, d)
    kw = dict(loss=loss, scale=scale, iters=200, tol=1e-9)
    ref = R.robust_batch(d['az'], d['y'], d['m'], d['seg'], k=K, **kw)
    assert (ref['out'][:, 7] > 1).all() and (ref['out'][:, 7] < 200).all()  # the oracle stopped early
    out, w, r = run_gpu(ctx, d, dd, **kw)
    print()
    R.compare(f'early {loss}/{scale}', out, w, r, ref, tol=1e-9)
    assert (out[:, 7] > 0).all()
    # two iterations are not enough: the count is reported negated
    out2, _, _ = run_gpu(ctx, d, dd, loss=loss, scale=scale, iters=2, tol=1e-9)
    assert (out2[:, 7] == -2).all(), out2[:, 7]


# -- 4. LS equivalence ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bounds', [R.BOX, (-0.001, 0.001, -0.0015, 0.0005)], ids=['interior', 'box-active'])
def test_ls_equivalence(ctx, parity_batch, bounds):
    """A cut-off beyond every residual makes every weight 1: each iteration is the LS solve again."""
    d, dd = parity_batch
    tab = ctx.to_dev(R.grid_rad())
    ls, _, _ = ctx.velocity(None, dd['y'], dd['seg'], k=K, ridge=RIDGE, bounds=bounds, amask=dd['amask'],
                            gidx=dd['gidx'], az_table=tab, n=len(d['y']))
    ls = ls.cpu().numpy()
    out, w, _ = run_gpu(ctx, d, dd, loss='huber', c=1e30, scale=1.0, iters=3, tol=0.0, ridge=RIDGE, bounds=bounds)
    if bounds is not R.BOX:  # the LS optimum of the long frames is outside the box
        big = np.array(PARITY_LENGTHS) > 100
        at = (np.abs(ls[big, 0]) == 0.001) | (ls[big, 1] == -0.0015) | (ls[big, 1] == 0.0005)
        assert at.all()
    err = np.abs(out[:, :2] - ls[:, :2]) / np.maximum(np.abs(ls[:, :2]), 1e-300)
    print(f'\nLS equivalence: worst relative difference {err.max():.2e}')
    assert (err <= 1e-13).all()
    assert (out[:, 5] == ls[:, 5]).all()
    full = np.array(PARITY_LENGTHS) > 0  # the empty frame stops before the first iteration
    assert (out[full, 7] == 3).all() and out[~full, 7] == 0 and (w == 1.0).all()
    assert (out[:, 4] == out[:, 5]).all()  # every cell is an inlier


# -- 5. degenerate cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('loss', ['huber', 'tukey'])
def test_exact_fit_stops_with_zero_scale(ctx, loss):
    d = make_batch([50, 600], seed0=500)
    d['y'] = np.zeros_like(d['y'])  # fits v = 0 exactly: every residual is 0, so the estimated sigma is 0
    dd = dev(ctx, d)
    out, w, r = run_gpu(ctx, d, dd, loss=loss, scale=None, iters=20, tol=1e-9)
    assert (out[:, :2] == 0).all() and (out[:, 6] == 0).all()
    assert (out[:, 7] == 0).all() and not np.signbit(out[:, 7]).any()  # converged before the first iteration
    assert (w == 1.0).all() and (r == 0).all()
    assert (out[:, 2] == 0).all() and (out[:, 3] == 0).all()
    assert (out[:, 4] == out[:, 5]).all() and (out[:, 5] == [d['m'][:50].sum(), d['m'][50:].sum()]).all()


@pytest.mark.parametrize('scale', [0.05, None], ids=['fixed', 'auto'])
def test_all_masks_zero(ctx, scale):
    d = make_batch([50, 600], seed0=500)
    d['amask'] = np.zeros_like(d['amask'])
    d['m'] = np.zeros_like(d['m'])
    dd = dev(ctx, d)
    out, w, r = run_gpu(ctx, d, dd, loss='tukey', scale=scale, iters=20, tol=1e-9, ridge=RIDGE)
    ref = R.robust_batch(d['az'], d['y'], d['m'], d['seg'], k=K, loss='tukey', scale=scale, iters=20, tol=1e-9,
                         ridge=RIDGE)
    assert np.isfinite(out).all()
    assert (out[:, 5] == 0).all() and (out[:, 4] == 0).all() and (out[:, 7] == 0).all()
    assert (out[:, :2] == ref['out'][:, :2]).all() and (out[:, 6] == ref['out'][:, 6]).all()
    assert not np.isnan(w).any() and not np.isnan(r).any()


def test_segments_are_clamped(ctx):
    d = make_batch([300, 400, 200], seed0=600)
    dd = dev(ctx, d)
    n = 520  # frame 1 is cut short, frame 2 becomes empty
    kw = dict(loss='tukey', scale=0.05, iters=10, tol=0.0)
    ref = R.robust_batch(d['az'], d['y'], d['m'], d['seg'], n=n, k=K, **kw)
    out, w, r = run_gpu(ctx, d, dd, n=n, **kw)
    print()
    R.compare('clamped', out, w, r, ref, tol=0.0)
    assert out[2, 5] == 0 and out[1, 5] == d['m'][300:520].sum()
    assert np.isnan(w[n:]).all()  # nothing was written past n


def test_empty_batch_launches_nothing(ctx, parity_batch):
    d, dd = parity_batch
    torch = ctx.torch
    tab = ctx.to_dev(R.grid_rad())
    ctx.timing(True)
    try:
        ctx.timing_reset()
        seg0 = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
        ctx.velocity_robust(None, dd['y'], seg0, k=K, loss='tukey', gidx=dd['gidx'], az_table=tab, amask=dd['amask'])
        assert ctx.timing_read()['velocity'][1] == 0
        ctx.velocity_robust(None, dd['y'], dd['seg'], k=K, loss='tukey', gidx=dd['gidx'], az_table=tab,
                            amask=dd['amask'])
        assert ctx.timing_read()['velocity'][1] == 1  # timed under RSL_K_VELOCITY
    finally:
        ctx.timing_reset()
        ctx.timing(False)


# -- 6. value ----------------------------------------------------------------------------------------------------------
def test_rejects_a_second_motion(ctx):
    frames = [R.planted(600, 0.35, seed=700 + i) for i in range(4)]
    d = R.concat(frames)
    dd = dev(ctx, d)
    tab = ctx.to_dev(R.grid_rad())
    out, _, _ = run_gpu(ctx, d, dd, loss='tukey', scale=0.05)
    ls, _, _ = ctx.velocity(None, dd['y'], dd['seg'], k=K, amask=dd['amask'], gidx=dd['gidx'], az_table=tab)
    ls = ls.cpu().numpy()
    v = frames[0]['v_in']
    err, err_ls = np.abs(out[:, :2] - v).max(1), np.abs(ls[:, :2] - v).max(1)
    print(f'\n35 % outliers: tukey error {err}, LS error {err_ls}, iterations {out[:, 7]}')
    assert (err < 1e-4).all()
    assert (err_ls > 1e-3).all()
    assert (out[:, 7] > 0).all()


# -- 7. arguments ------------------------------------------------------------------------------------------------------
GOOD = dict(loss=R.LOSS_TUKEY, c=4.685, scale=0.05, iters=30, tol=1e-9, ridge=0.0)


@pytest.mark.parametrize('bad', [dict(loss=0), dict(loss=3), dict(c=0.0), dict(c=-1.0), dict(c=float('inf')),
                                 dict(c=float('nan')), dict(scale=float('nan')), dict(scale=float('inf')),
                                 dict(iters=0), dict(iters=1001), dict(tol=-1e-9), dict(tol=float('nan')),
                                 dict(ridge=-1.0)], ids=lambda b: '-'.join(f'{k}={v}' for k, v in b.items()))
def test_bad_scalars(ctx, parity_batch, bad):
    d, dd = parity_batch
    tab = ctx.to_dev(R.grid_rad())
    with pytest.raises(ValueError):
        ctx.velocity_robust(None, dd['y'], dd['seg'], k=K, gidx=dd['gidx'], az_table=tab, **{**GOOD, **bad})


def test_bad_pointers(ctx, parity_batch):
    d, dd = parity_batch
    torch = ctx.torch
    tab = ctx.to_dev(R.grid_rad())
    big = torch.zeros((2049,), dtype=torch.float64, device=ctx.device)
    az = torch.zeros((len(d['y']),), dtype=torch.float64, device=ctx.device)
    with pytest.raises(ValueError):  # G > 2048 with gidx
        ctx.velocity_robust(None, dd['y'], dd['seg'], k=K, gidx=dd['gidx'], az_table=big, **GOOD)
    with pytest.raises(ValueError):  # gidx without az_table
        ctx.velocity_robust(None, dd['y'], dd['seg'], k=K, gidx=dd['gidx'], az_table=None, **GOOD)
    with pytest.raises(ValueError):  # neither az nor gidx
        ctx.velocity_robust(None, dd['y'], dd['seg'], k=K, **GOOD)
    lib, F, N = ctx.lib, len(PARITY_LENGTHS), len(d['y'])
    from ctypes import c_double, c_void_p
    b4 = (c_double * 4)(*R.BOX)
    out = torch.zeros((F, 8), dtype=torch.float64, device=ctx.device)
    p = lambda t: c_void_p(t.data_ptr())
    base = dict(az=p(az), y=p(dd['y']), seg=p(dd['seg']), out=p(out), b4=b4)
    for null in ('y', 'seg', 'out', 'b4'):
        a = {**base, null: None}
        rc = lib.rsl_velocity_robust(ctx.h, a['az'], None, None, 0, a['y'], None, a['seg'], N, F, K, 0.0, a['b4'],
                                     R.LOSS_TUKEY, 4.685, 0.05, 30, 1e-9, a['out'], None, None)
        assert rc == 1, (null, rc)  # RSL_ERR_INVALID
        with pytest.raises(ValueError):
            ctx.check(rc, 'rsl_velocity_robust')
    # the unknown loss name is rejected before the library is called
    with pytest.raises(ValueError):
        ctx.velocity_robust(az, dd['y'], dd['seg'], k=K, loss='ransac')


# -- 8. chain ----------------------------------------------------------------------------------------------------------
CH = dict(num_antennas=8, num_chirps=64, chirp_duration=25.6e-6)
CHAIN_SCALE, CHAIN_ITERS = 0.3, 15


@pytest.fixture(scope='module')
def chains(ctx):
    import rsl
    frames = []
    for s in (1000, 1001):
        np.random.seed(s)
        frames.append(O.synthesize_frame(O.TEST_SCENE, chirp_duration=25.6e-6, num_chirps=64, num_antennas=8))
    cube = ctx.to_dev(np.stack(frames).astype(np.complex64))
    out = {}
    for name, kw in (('plain', {}), ('ls', dict(velocity_loss='ls', velocity_scale=CHAIN_SCALE, velocity_iters=3)),
                     ('tukey', dict(velocity_loss='tukey', velocity_scale=CHAIN_SCALE, velocity_iters=CHAIN_ITERS,
                                    velocity_tol=0.0))):
        ch = rsl.RadarChain(rsl.ChainConfig(**CH, **kw), 2, ctx)
        ch.run(cube)
        res = ch.results()
        res['chain'] = ch
        out[name] = res
    return out


def test_chain_tukey_matches_oracle(chains):
    r = chains['tukey']
    ch = r['chain']
    nc = int(r['cell_base'][-1])
    assert nc >= 6 and r['vel_weight'].shape == (nc,) and r['vel_weight'].dtype == np.float32
    az = np.radians(r['grid'])[r['gidx']]
    ref = R.robust_batch(az, r['phase'], R.popcount(r['c_amask']), r['cell_base'], k=ch.k, loss='tukey',
                         scale=CHAIN_SCALE, iters=CHAIN_ITERS, tol=0.0)
    print()
    R.compare('chain', r['velocity'], r['vel_weight'].astype(np.float64), None, ref, tol=0.0)
    # and the solve was a different one from the plain chain's
    assert (r['velocity'][:, 7] == CHAIN_ITERS).all()
    assert (r['velocity'][:, :2] != chains['plain']['velocity'][:, :2]).any()


def test_chain_ls_unchanged(chains):
    a, b = chains['plain'], chains['ls']
    assert b['chain'].vel_weight is None and 'vel_weight' not in b and 'vel_weight' not in a
    for k in ('cell_base', 'c_amask', 'gidx', 'phase', 'velocity'):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


# -- 9. drop-in ----------------------------------------------------------------------------------------------------------
def test_dropin_solve_velocity_robust(ctx):
    from src.velocity_solver.velocity_solver import VelocitySolver
    d = R.planted(40, 0.25, seed=800, mmax=0)
    targets = [dict(range_m=10.0 + i, azimuth_rad=float(a), spatial_signature=np.exp(1j * np.arange(8) * ph))
               for i, (a, ph) in enumerate(zip(d['az'], d['y']))]
    vs = VelocitySolver()
    y = vs.compute_observed_phase_differences(None, targets)  # the phases the solver itself observes (fp32 signatures)
    assert np.abs(y - d['y']).max() < 1e-5
    got = vs.solve_velocity_robust(None, targets, dt=0.1, loss='tukey', scale=0.05)
    ref = R.robust_batch(d['az'], y, None, np.array([0, 40]), k=vs._k(0.1), loss='tukey', scale=0.05, iters=30,
                         tol=1e-9)
    fr = ref['frames'][0]
    assert got['success'] and got['num_targets'] == 40
    row = np.array([[got['velocity'][0], got['velocity'][1], got['cost'], got['rmse'], got['num_inliers'], 40,
                     got['scale'], got['iterations'] if fr['it'] > 0 else -got['iterations']]])
    print()
    R.compare('drop-in', row, got['weights'], got['residuals'], ref, tol=1e-9)
    assert got['velocity'][2] == 0 and (got['angular_velocity'] == 0).all()
    assert got['weights'].shape == (40,) and got['residuals'].shape == (40,)
    few = vs.solve_velocity_robust(None, targets[:2], dt=0.1)
    assert few == {'success': False, 'message': 'Insufficient targets'}
