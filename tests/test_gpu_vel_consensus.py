"""GPU tests of the consensus velocity solve (rsl_velocity_consensus / k_velocity_consensus) against the fp64 numpy
oracle in tests/vel_consensus_ref.py.  best_h, n_valid, n_in, n and the inlier mask are compared exactly; every
comparison first asserts, on the oracle alone, what that exactness presupposes (no decision within 1e-9 of its
boundary, condition number of the last refinement): that module's docstring has the derivation."""
import numpy as np
import pytest

import radar_oracle as O
import vel_consensus_ref as C
import vel_robust_ref as R

pytestmark = pytest.mark.gpu

K = R.K_CHAIN
SCALE = 0.05
# one launch: the empty frame sits in the middle; 63 / 64 / 65 straddle a wave, CHUNK - 1 / CHUNK / CHUNK + 1 one trip
# of the LDS staging loop (5000 takes five), 600 and 5000 are the sizes of the prototype
PARITY_LENGTHS = [600, 1, C.CHUNK + 1, 0, 2, 5000, 3, 17, 63, C.CHUNK - 1, 64, 65, C.CHUNK]
HYPS = [1, 255, 256, 257, 4096]  # 256 threads: one hypothesis per thread and the first of the second round
RIDGE = 1e5  # about k^2: keeps the 1- to 3-cell frames well posed, as in test_gpu_vel_robust.py
ACTIVE_BOX = (-0.001, 0.001, -0.0015, 0.0005)


def make_batch(lengths, seed0=100, **kw):
    return C.concat([C.scene(n, seed0 + i, **kw) for i, n in enumerate(lengths)])


def dev(ctx, d, az_path=False, with_mask=True):
    """Device copies of a concat()-style dictionary."""
    pad = lambda a: a if len(a) else np.zeros(1, a.dtype)
    return dict(az=ctx.to_dev(pad(d['az'])) if az_path else None, gidx=None if az_path else ctx.to_dev(pad(d['gidx'])),
                y=ctx.to_dev(pad(d['y'])), amask=ctx.to_dev(pad(d['amask'])) if with_mask else None,
                seg=ctx.to_dev(d['seg']))


def run_gpu(ctx, d, dd, *, G=361, n=None, seg=None, **kw):
    """rsl_velocity_consensus on the arrays of dev(); weight / resid buffers pre-filled with NaN (untouched slots
    stay)."""
    torch = ctx.torch
    N = len(d['y'])
    tab = ctx.to_dev(R.grid_rad(G)) if dd['gidx'] is not None else None
    w = torch.full((max(N, 1),), float('nan'), dtype=torch.float32, device=ctx.device)
    kw.setdefault('scale', SCALE)
    out, w, r = ctx.velocity_consensus(dd['az'], dd['y'], dd['seg'] if seg is None else seg, k=K, amask=dd['amask'],
                                       gidx=dd['gidx'], az_table=tab, n=N if n is None else n, want_weight=w,
                                       want_resid=True, **kw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), w.cpu().numpy().astype(np.float64)[:N], r.cpu().numpy()[:N]


def oracle(d, with_mask=True, **kw):
    kw.setdefault('scale', SCALE)
    return C.consensus_batch(d['az'], d['y'], d['m'] if with_mask else None, d['seg'], k=K, **kw)


@pytest.fixture(scope='module')
def parity_batch(ctx):
    d = make_batch(PARITY_LENGTHS)
    assert (d['m'] == 0).any() and d['seg'][-1] == sum(PARITY_LENGTHS)
    return d, dev(ctx, d)


@pytest.fixture(scope='module')
def az_batch(ctx):
    d = make_batch(PARITY_LENGTHS, seed0=200, mmax=0)
    return d, dev(ctx, d, az_path=True, with_mask=False)


# -- 1. parity with the oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize('hyps', HYPS)
def test_oracle_parity(ctx, parity_batch, hyps):
    d, dd = parity_batch
    kw = dict(hyps=hyps, seed=11, ridge=RIDGE)
    ref = oracle(d, **kw)
    out, w, r = run_gpu(ctx, d, dd, **kw)
    print()
    C.compare(f'gidx/{hyps}', out, w, r, ref)
    assert not np.isnan(w).any() and not np.isnan(r).any()  # every cell of every frame was written
    big = np.array(PARITY_LENGTHS) >= 17
    if hyps >= 255:
        assert (out[big, 6] >= 0).all() and (out[big, 7] > 0).all()
    assert (out[~big, 7] <= hyps).all() and (out[np.array(PARITY_LENGTHS) < 2, 6] == -1).all()


@pytest.mark.parametrize('hyps', HYPS)
def test_az_path_without_masks(ctx, az_batch, hyps):
    d, dd = az_batch
    kw = dict(hyps=hyps, seed=12, ridge=RIDGE)
    ref = oracle(d, with_mask=False, **kw)
    out, w, r = run_gpu(ctx, d, dd, **kw)
    print()
    C.compare(f'az/{hyps}', out, w, r, ref)
    assert (out[:, 5] == PARITY_LENGTHS).all()


# -- 2. few valid hypotheses ---------------------------------------------------------------------------------
def test_small_grid(ctx):
    """G = 7: a pair on one grid point is degenerate (det = 0), so n_valid is well below hyps."""
    d = make_batch([100, 7, 40], seed0=300, G=7)
    dd = dev(ctx, d)
    kw = dict(hyps=256, seed=3, ridge=RIDGE)
    ref = oracle(d, **kw)
    assert (ref['out'][:, 7] < 230).all() and (ref['out'][:, 7] > 0).all()
    out, w, r = run_gpu(ctx, d, dd, G=7, **kw)
    print()
    C.compare('G=7', out, w, r, ref)


@pytest.mark.parametrize('kw', [dict(refine=0), dict(refine=3, c=1e30)], ids=['refine0', 'all-inliers'])
def test_one_azimuth_falls_back_on_ls(ctx, kw):
    """Every pair of a frame on one azimuth has det = 0: no valid hypothesis, and the start is rsl_velocity's solution
    (refine = 0 returns it; with every cell an inlier each refinement is that LS solve again).  Within 1e-13, as
    test_gpu_vel_robust.py::test_ls_equivalence holds the robust solver's start: the two kernels add the same moments
    in another order (a few 2^-53 relative), and the rank-one normal matrix k^2 M + ridge I amplifies that by its
    condition number 1 + k^2 sum m / ridge, which the ridge of 1e7 keeps at 3 and 26 for these two frames."""
    ridge = 1e7
    d = make_batch([50, 600], seed0=400)
    d['gidx'][:] = 77
    d['az'][:] = R.grid_rad()[77]
    dd = dev(ctx, d)
    tab = ctx.to_dev(R.grid_rad())
    ls, _, _ = ctx.velocity(None, dd['y'], dd['seg'], k=K, ridge=ridge, amask=dd['amask'], gidx=dd['gidx'],
                            az_table=tab, n=len(d['y']))
    ls = ls.cpu().numpy()
    out, w, _ = run_gpu(ctx, d, dd, hyps=256, ridge=ridge, **kw)
    err = np.abs(out[:, :2] - ls[:, :2]) / np.maximum(np.abs(ls[:, :2]), 1e-300)
    print(f'\none azimuth: worst relative difference to rsl_velocity {err.max():.2e}')
    assert (out[:, 6] == -1).all() and (out[:, 7] == 0).all()
    assert (err <= 1e-13).all()
    assert (out[:, 5] == ls[:, 5]).all() and (ls[:, :2] != 0).all()
    if 'c' in kw:
        assert (out[:, 4] == out[:, 5]).all() and (w == 1.0).all()  # every cell is an inlier


# -- 3. degenerate cases ---------------------------------------------------------------------------------------
def test_all_masks_zero(ctx):
    d = make_batch([50, 600], seed0=500)
    d['amask'] = np.zeros_like(d['amask'])
    d['m'] = np.zeros_like(d['m'])
    dd = dev(ctx, d)
    out, w, r = run_gpu(ctx, d, dd, hyps=256, ridge=RIDGE)
    ref = oracle(d, hyps=256, ridge=RIDGE)
    assert np.isfinite(out).all()
    assert (out[:, 4:6] == 0).all() and (out[:, 6] == -1).all() and (out[:, 7] == 0).all()
    assert (out[:, :2] == ref['out'][:, :2]).all() and (out[:, 2] == RIDGE * (out[:, :2] ** 2).sum(1)).all()
    assert not np.isnan(w).any() and not np.isnan(r).any()


def test_single_cell_frames(ctx):
    d = make_batch([1, 1, 1], seed0=510, mmax=0)
    dd = dev(ctx, d)
    ref = oracle(d, hyps=64, ridge=RIDGE)
    out, w, r = run_gpu(ctx, d, dd, hyps=64, ridge=RIDGE)
    print()
    C.compare('n_f = 1', out, w, r, ref)
    assert (out[:, 6] == -1).all() and (out[:, 7] == 0).all() and (out[:, 5] == 1).all()


def test_refine_zero_returns_the_raw_hypothesis(ctx):
    d = make_batch([600, 40], seed0=520)
    dd = dev(ctx, d)
    kw = dict(hyps=256, seed=5, refine=0)
    ref = oracle(d, **kw)
    out, w, r = run_gpu(ctx, d, dd, **kw)
    print()
    C.compare('refine 0', out, w, r, ref)
    for f, fr in enumerate(ref['frames']):
        assert fr['passes'] == 0 and fr['best_h'] >= 0
        xh = fr['x_h'][fr['best_h']]
        assert np.abs(out[f, :2] - xh).max() <= 1e-12 * np.abs(xh).max()  # a two-cell solve, condition <= 20
        assert out[f, 4] == fr['scores'][fr['best_h']]  # n_in at the raw winner is its score


def test_box_active(ctx):
    """Every motion of the scene lies outside the box: most hypotheses are invalid, and with a cut-off wide enough
    (c = 10) for a hypothesis inside the box to count cells of the populations outside it, the refinement lands on the
    box by the edge rule."""
    d = make_batch([600, 300], seed0=530)
    dd = dev(ctx, d)
    kw = dict(hyps=1024, seed=6, c=10.0, bounds=ACTIVE_BOX)
    ref = oracle(d, **kw)
    free = oracle(d, hyps=1024, seed=6, c=10.0)
    assert (ref['out'][:, 7] < free['out'][:, 7]).all() and (ref['out'][:, 7] > 0).all()
    out, w, r = run_gpu(ctx, d, dd, **kw)
    print()
    C.compare('box', out, w, r, ref)
    lx, hx, ly, hy = ACTIVE_BOX
    on_edge = (out[:, 0] == lx) | (out[:, 0] == hx) | (out[:, 1] == ly) | (out[:, 1] == hy)
    assert on_edge.all(), out[:, :2]
    assert ((out[:, 0] >= lx) & (out[:, 0] <= hx) & (out[:, 1] >= ly) & (out[:, 1] <= hy)).all()


# -- 4. draws ------------------------------------------------------------------------------------------------
def test_frame0_composes_and_seed_matters(ctx):
    lengths = [40, 100, 0, 300, 2, 77]
    d = make_batch(lengths, seed0=600)
    dd = dev(ctx, d)
    kw = dict(hyps=256, seed=9, ridge=RIDGE)
    base = 2 ** 32 - 3  # the frame index crosses 2^32: the counter's third word
    out, w, r = run_gpu(ctx, d, dd, frame0=base, **kw)
    ref = oracle(d, frame0=base, **kw)
    print()
    C.compare('frame0', out, w, r, ref)
    a, b = 2, 5
    sub = ctx.to_dev(d['seg'][a:b + 1])
    out2, w2, r2 = run_gpu(ctx, d, dd, seg=sub, frame0=base + a, **kw)
    assert out2[:b - a].tobytes() == out[a:b].tobytes()
    sl = slice(d['seg'][a], d['seg'][b])
    assert w2[sl].tobytes() == w[sl].tobytes() and r2[sl].tobytes() == r[sl].tobytes()
    assert np.isnan(w2[:sl.start]).all() and np.isnan(w2[sl.stop:]).all()
    out0, _, _ = run_gpu(ctx, d, dd, frame0=0, **kw)
    assert (out0[:, 6] != out[:, 6]).any()
    out3, _, _ = run_gpu(ctx, d, dd, frame0=base, hyps=256, seed=10, ridge=RIDGE)
    assert (out3[:, 6] != out[:, 6]).any()


# -- 5. segments, empty batch, arguments ---------------------------------------------------------------------
def test_segments_are_clamped(ctx):
    d = make_batch([300, 400, 200], seed0=700)
    dd = dev(ctx, d)
    n = 520  # frame 1 is cut short, frame 2 becomes empty
    ref = oracle(d, n=n, hyps=256, seed=2)
    out, w, r = run_gpu(ctx, d, dd, n=n, hyps=256, seed=2)
    print()
    C.compare('clamped', out, w, r, ref)
    assert out[2, 5] == 0 and out[2, 6] == -1 and out[1, 5] == d['m'][300:520].sum()
    assert np.isnan(w[n:]).all() and np.isnan(r[n:]).all()  # nothing was written past n


def test_empty_batch_launches_nothing(ctx, parity_batch):
    d, dd = parity_batch
    torch = ctx.torch
    tab = ctx.to_dev(R.grid_rad())
    kw = dict(k=K, scale=SCALE, gidx=dd['gidx'], az_table=tab, amask=dd['amask'])
    ctx.timing(True)
    try:
        ctx.timing_reset()
        seg0 = torch.zeros((1,), dtype=torch.int64, device=ctx.device)
        o = torch.full((1, 8), float('nan'), dtype=torch.float64, device=ctx.device)
        w = torch.full((len(d['y']),), float('nan'), dtype=torch.float32, device=ctx.device)
        ctx.velocity_consensus(None, dd['y'], seg0, out=o, want_weight=w, **kw)
        assert ctx.timing_read()['velocity'][1] == 0
        assert torch.isnan(o).all() and torch.isnan(w).all()
        ctx.velocity_consensus(None, dd['y'], dd['seg'], **kw)
        assert ctx.timing_read()['velocity'][1] == 1  # timed under RSL_K_VELOCITY
    finally:
        ctx.timing_reset()
        ctx.timing(False)


GOOD = dict(c=3.0, scale=SCALE, hyps=256, min_det=0.1, refine=3, seed=0, frame0=0, ridge=0.0)
NAN, INF = float('nan'), float('inf')


@pytest.mark.parametrize('bad', [dict(c=0.0), dict(c=-1.0), dict(c=INF), dict(c=NAN), dict(scale=0.0),
                                 dict(scale=-0.05), dict(scale=INF), dict(scale=NAN), dict(hyps=0), dict(hyps=4097),
                                 dict(min_det=0.0), dict(min_det=-0.1), dict(min_det=1.0001), dict(min_det=NAN),
                                 dict(refine=-1), dict(refine=101), dict(frame0=-1), dict(ridge=-1.0)],
                         ids=lambda b: '-'.join(f'{k}={v}' for k, v in b.items()))
def test_bad_scalars(ctx, parity_batch, bad):
    d, dd = parity_batch
    tab = ctx.to_dev(R.grid_rad())
    with pytest.raises(ValueError):
        ctx.velocity_consensus(None, dd['y'], dd['seg'], k=K, gidx=dd['gidx'], az_table=tab, **{**GOOD, **bad})


def test_good_scalar_limits(ctx, parity_batch):
    d, dd = parity_batch
    tab = ctx.to_dev(R.grid_rad())
    for ok in (dict(hyps=1), dict(hyps=4096), dict(min_det=1.0), dict(refine=0), dict(refine=100)):
        ctx.velocity_consensus(None, dd['y'], dd['seg'], k=K, gidx=dd['gidx'], az_table=tab, **{**GOOD, **ok})
    ctx.torch.cuda.synchronize()


def test_bad_pointers(ctx, parity_batch):
    d, dd = parity_batch
    torch = ctx.torch
    big = torch.zeros((2049,), dtype=torch.float64, device=ctx.device)
    az = torch.zeros((len(d['y']),), dtype=torch.float64, device=ctx.device)
    with pytest.raises(ValueError):  # G > 2048 with gidx
        ctx.velocity_consensus(None, dd['y'], dd['seg'], k=K, gidx=dd['gidx'], az_table=big, **GOOD)
    with pytest.raises(ValueError):  # gidx without az_table
        ctx.velocity_consensus(None, dd['y'], dd['seg'], k=K, gidx=dd['gidx'], az_table=None, **GOOD)
    with pytest.raises(ValueError):  # neither az nor gidx
        ctx.velocity_consensus(None, dd['y'], dd['seg'], k=K, **GOOD)
    with pytest.raises(ValueError):  # the scale is required
        ctx.velocity_consensus(az, dd['y'], dd['seg'], k=K, scale=None)
    lib, F, N = ctx.lib, len(PARITY_LENGTHS), len(d['y'])
    from ctypes import c_double, c_void_p
    b4 = (c_double * 4)(*R.BOX)
    out = torch.zeros((F, 8), dtype=torch.float64, device=ctx.device)
    p = lambda t: c_void_p(t.data_ptr())
    base = dict(az=p(az), y=p(dd['y']), seg=p(dd['seg']), out=p(out), b4=b4)
    for null in ('y', 'seg', 'out', 'b4'):
        a = {**base, null: None}
        rc = lib.rsl_velocity_consensus(ctx.h, a['az'], None, None, 0, a['y'], None, a['seg'], N, F, K, 0.0, a['b4'],
                                        3.0, SCALE, 256, 0.1, 3, 0, 0, a['out'], None, None)
        assert rc == 1, (null, rc)  # RSL_ERR_INVALID
        with pytest.raises(ValueError):
            ctx.check(rc, 'rsl_velocity_consensus')


# -- 6. value -------------------------------------------------------------------------------------------------
def test_finds_the_minority_motion(ctx):
    """The scene of tests/test_vel_consensus_host.py (seeds 0 and 2, each as a launch of its own so that the draws are
    those of frame 0): 40 % static cells against three moving groups of 20 %."""
    tab = ctx.to_dev(R.grid_rad())
    for seed in (0, 2):
        d = C.concat([C.scene(600, seed)])
        dd = dev(ctx, d)
        v = C.scene(600, seed)['motions'][0]
        lab = C.scene(600, seed)['label']
        kw = dict(scale=0.05, c=3.0, hyps=256, seed=7, refine=3)
        ref = oracle(d, **kw)
        pop0 = lab == 0
        share_ref = (d['m'][pop0] * ref['weights'][pop0]).sum() / d['m'][pop0].sum()
        assert share_ref >= 0.95
        out, w, r = run_gpu(ctx, d, dd, **kw)
        tk, _, _ = ctx.velocity_robust(None, dd['y'], dd['seg'], k=K, loss='tukey', scale=0.05, iters=30, tol=1e-9,
                                       amask=dd['amask'], gidx=dd['gidx'], az_table=tab)
        tk = tk.cpu().numpy()
        err, err_tukey = np.abs(out[0, :2] - v).max(), np.abs(tk[0, :2] - v).max()
        share = (d['m'][pop0] * w[pop0]).sum() / d['m'][pop0].sum()
        print(f'\nseed {seed}: consensus error {err:.2e}, tukey error {err_tukey:.2e}, inlier share of population 0 '
              f'{share:.4f} (oracle {share_ref:.4f}), best_h {out[0, 6]:.0f}, n_valid {out[0, 7]:.0f}')
        assert err < 1e-4
        assert err_tukey > 1e-3
        assert share >= 0.95
        C.compare(f'minority/{seed}', out, w, r, ref)


# -- 7. chain --------------------------------------------------------------------------------------------------
CH = dict(num_antennas=8, num_chirps=64, chirp_duration=25.6e-6)
CHAIN_SCALE = 0.3
CHAIN_KW = dict(velocity_hyps=300, velocity_seed=4, velocity_refine=2)


@pytest.fixture(scope='module')
def chains(ctx):
    import rsl
    frames = []
    for s in (1000, 1001, 1002):
        np.random.seed(s)
        frames.append(O.synthesize_frame(O.TEST_SCENE, chirp_duration=25.6e-6, num_chirps=64, num_antennas=8))
    cube = ctx.to_dev(np.stack(frames).astype(np.complex64))
    out = {}
    for name, kw in (('plain', {}), ('ls', dict(velocity_loss='ls', velocity_scale=CHAIN_SCALE, **CHAIN_KW)),
                     ('consensus', dict(velocity_loss='consensus', velocity_scale=CHAIN_SCALE, **CHAIN_KW))):
        ch = rsl.RadarChain(rsl.ChainConfig(**CH, **kw), 3, ctx)
        ch.run(cube)
        res = ch.results()
        res['chain'] = ch
        out[name] = res
    return out


def test_chain_consensus_matches_oracle(chains):
    r = chains['consensus']
    ch = r['chain']
    nc = int(r['cell_base'][-1])
    assert ch.S == 256 and nc >= 6 and r['vel_weight'].shape == (nc,) and r['vel_weight'].dtype == np.float32
    az = np.radians(r['grid'])[r['gidx']]
    ref = C.consensus_batch(az, r['phase'], R.popcount(r['c_amask']), r['cell_base'], k=ch.k, scale=CHAIN_SCALE,
                            hyps=300, seed=4, refine=2, frame0=0)
    print()
    C.compare('chain', r['velocity'], r['vel_weight'].astype(np.float64), None, ref)
    assert set(np.unique(r['vel_weight'])) <= {0.0, 1.0}
    assert (r['velocity'][:, 6] >= 0).all()  # a hypothesis won in every frame


def test_chain_ls_unchanged(chains):
    a, b = chains['plain'], chains['ls']
    assert b['chain'].vel_weight is None and 'vel_weight' not in b and 'vel_weight' not in a
    for k in ('cell_base', 'c_amask', 'gidx', 'phase', 'velocity'):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    c = chains['consensus']
    for k in ('cell_base', 'c_amask', 'gidx', 'phase'):  # the consensus chain differs in the solve alone
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(c[k]).tobytes(), k


# -- 8. drop-in ------------------------------------------------------------------------------------------------
def test_dropin_solve_velocity_consensus(ctx):
    from src.velocity_solver.velocity_solver import VelocitySolver
    d = C.scene(40, 805, mmax=0)  # a seed whose phases stay inside (-pi, pi): the solver observes them wrapped
    assert np.abs(d['y']).max() < 3.0
    targets = [dict(range_m=10.0 + i, azimuth_rad=float(a), spatial_signature=np.exp(1j * np.arange(8) * ph))
               for i, (a, ph) in enumerate(zip(d['az'], d['y']))]
    vs = VelocitySolver()
    y = vs.compute_observed_phase_differences(None, targets)  # the phases the solver itself observes (fp32 signatures)
    assert np.abs(y - d['y']).max() < 1e-5
    got = vs.solve_velocity_consensus(None, targets, dt=0.1, scale=0.05, seed=13)
    ref = C.consensus_batch(d['az'], y, None, np.array([0, 40]), k=vs._k(0.1), scale=0.05, seed=13)
    assert got['success'] and got['num_targets'] == 40
    row = np.array([[got['velocity'][0], got['velocity'][1], got['cost'], got['rmse'], got['num_inliers'], 40,
                     got['best_hypothesis'], got['num_valid']]])
    print()
    C.compare('drop-in', row, got['weights'], got['residuals'], ref)
    assert got['velocity'][2] == 0 and (got['angular_velocity'] == 0).all()
    assert got['weights'].shape == (40,) and got['residuals'].shape == (40,)
    assert np.abs(got['velocity'][:2] - d['motions'][0]).max() < 1e-3  # the largest population's motion
    few = vs.solve_velocity_consensus(None, targets[:2], dt=0.1, scale=0.05)
    assert few == {'success': False, 'message': 'Insufficient targets'}
