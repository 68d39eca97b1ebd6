"""Grid map on the device (rsl_map_update, rsl_map_logodds) against tests/map_ref.py, the fp64 restatement of the
specification in include/rsl.h.  Every comparison is exact: the planes are integer counts, the cell of every point is
found in fp64 with each operation rounded once on both sides, and the log-odds are compared bit for bit.

The case (map_ref.gpu_case): ny = 80, nx = 96, cell 0.5 m, r_max 20 m, so Rw = 41 and the window is 83 wide (neither 83
nor 83^2 is a multiple of 32); F = 6 frames of 40, 0, 300, 700, 3 and 50 points, the last segment's end 1000 past the
arrays; yaws in all four quadrants (every octant, both branches of the line), one pose outside the map (clipped rays),
one pose with a NaN (flag 1), and planted points for every rule; the builder asserts that each occurs."""
import numpy as np
import pytest

import map_ref as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def case():
    c = M.gpu_case()
    c['ref'] = {}
    for w in (False, True):
        for fr in (False, True):
            c['ref'][w, fr] = M.map_update(c['points'], c['seg'], c['poses'], c['grid'], c['shape'], n=c['n'],
                                           weight=c['weight'] if w else None, want_free=fr, **c['params'])
    return c


def upload(ctx, c):
    return dict(points=ctx.to_dev(c['points']), seg=ctx.to_dev(c['seg']), poses=ctx.to_dev(c['poses']),
                weight=ctx.to_dev(c['weight']))


def planes(ctx, shape, free=True):
    torch = ctx.torch
    z = lambda: torch.zeros(shape, dtype=torch.int32, device=ctx.device)  # noqa: E731
    return z(), (z() if free else None)


def host(t):
    return t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('with_stats', [True, False], ids=['stats', 'nostats'])
@pytest.mark.parametrize('with_free', [True, False], ids=['free', 'nofree'])
@pytest.mark.parametrize('with_weight', [True, False], ids=['weight', 'noweight'])
def test_update_matches_reference(ctx, case, with_weight, with_free, with_stats):
    d = upload(ctx, case)
    hits, free = planes(ctx, case['shape'], with_free)
    st = ctx.map_update(d['points'], d['seg'], d['poses'], hits, grid=case['grid'], free=free,
                        weight=d['weight'] if with_weight else None, n=case['n'], want_stats=with_stats,
                        **case['params'])
    rh, rf, rs = case['ref'][with_weight, with_free]
    assert np.array_equal(host(hits), rh)
    if with_free:
        assert np.array_equal(host(free), rf)
    if with_stats:
        assert st.dtype == ctx.torch.int32 and np.array_equal(st.cpu().numpy(), rs)
    else:
        assert st is None


def test_second_launch_doubles_and_runs_agree(ctx, case):
    d = upload(ctx, case)
    rh, rf, rs = case['ref'][True, True]
    got = []
    for _ in range(2):
        hits, free = planes(ctx, case['shape'])
        for rep in (1, 2):
            st = ctx.map_update(d['points'], d['seg'], d['poses'], hits, grid=case['grid'], free=free,
                                weight=d['weight'], n=case['n'], **case['params'])
            assert np.array_equal(host(hits), rep * rh) and np.array_equal(host(free), rep * rf)
            assert np.array_equal(st.cpu().numpy(), rs)
        got.append((host(hits).tobytes(), host(free).tobytes()))
    assert got[0] == got[1]


def test_gridmap_rank_merge_and_logodds(ctx, case):
    """Two GridMaps fed frames [0, 3) and [3, 6), added, equal one fed all six; the log-odds are those of the counts."""
    import rsl
    d = upload(ctx, case)
    x0, y0, cell = case['grid']
    kw = dict(origin=(x0, y0), cell=cell, shape=case['shape'], l_occ=0.7, l_free=0.3, l_min=-1.1, l_max=1.3,
              **case['params'])
    whole, a, b = (rsl.GridMap(ctx, **kw) for _ in range(3))
    st = whole.update(d['points'], d['seg'], d['poses'], weight=d['weight'], n=case['n'])
    assert tuple(st.shape) == (6, 4)
    a.update(d['points'], d['seg'][:4].contiguous(), d['poses'][:3].contiguous(), weight=d['weight'], n=case['n'])
    b.update(d['points'], d['seg'][3:].contiguous(), d['poses'][3:].contiguous(), weight=d['weight'], n=case['n'])
    rh, rf, rs = case['ref'][True, True]
    res = whole.results()
    assert res['hits'].dtype == np.uint32 and np.array_equal(res['hits'], rh) and np.array_equal(res['free'], rf)
    assert np.array_equal(res['stats'], rs)
    assert np.array_equal(host(a.hits + b.hits), rh) and np.array_equal(host(a.free + b.free), rf)
    assert np.array_equal(np.concatenate([a.results()['stats'], b.results()['stats']]), rs)
    # counts large enough for both clamps: ten more updates
    for _ in range(10):
        whole.update(d['points'], d['seg'], d['poses'], weight=d['weight'], n=case['n'])
    res = whole.results()
    assert np.array_equal(res['hits'], 11 * rh) and np.array_equal(res['free'], 11 * rf)
    want = M.map_logodds(res['hits'], res['free'], 0.7, 0.3, -1.1, 1.3)
    assert res['logodds'].dtype == np.float32 and res['logodds'].tobytes() == want.tobytes()
    assert (want == np.float32(1.3)).any() and (want == np.float32(-1.1)).any() and len(np.unique(want)) > 3
    p = whole.probability().cpu().numpy()
    assert np.allclose(p, 1.0 / (1.0 + np.exp(-want.astype(np.float64))), atol=1e-6)
    nofree = rsl.GridMap(ctx, free=False, **kw)
    nofree.update(d['points'], d['seg'], d['poses'], weight=d['weight'], n=case['n'])
    res = nofree.results()
    assert res['free'] is None and np.array_equal(res['hits'], rh)
    assert res['logodds'].tobytes() == M.map_logodds(rh, None, 0.7, 0.3, -1.1, 1.3).tobytes()
    whole.reset()
    assert not whole.results()['hits'].any() and not whole.results()['free'].any()


def test_large_window_above_64k_lds(ctx):
    """Cell 0.25 m and r_max 77 m: Rw = 309, the window 619 wide, two bitmaps of 47.9 KB: the > 64 KiB launch path."""
    rng = np.random.default_rng(5)
    F, per = 2, 3000
    r, a = rng.uniform(0.0, 80.0, F * per), rng.uniform(-np.pi, np.pi, F * per)
    pts = np.zeros((F * per, 8), np.float32)
    pts[:, 3], pts[:, 4] = r * np.cos(a), r * np.sin(a)
    seg = np.array([0, per, 2 * per], np.int64)
    poses = np.array([M.yaw_pose(70.3, 65.1, 0.4), M.yaw_pose(12.0, 150.0, -2.0)])  # the second near the left edge
    grid, shape = (0.0, 0.0, 0.25), (640, 620)
    assert M.half_window(0.25, 77.0) == 309
    rh, rf, rs = M.map_update(pts, seg, poses, grid, shape, r_min=0.5, r_max=77.0)
    assert rs[:, 1].min() > 1000 and rs[1, 0] < rs[0, 0]  # the second frame loses points to the map's edge
    hits, free = planes(ctx, shape)
    st = ctx.map_update(ctx.to_dev(pts), ctx.to_dev(seg), ctx.to_dev(poses), hits, grid=grid, free=free, r_min=0.5,
                        r_max=77.0)
    assert np.array_equal(st.cpu().numpy(), rs)
    assert np.array_equal(host(hits), rh) and np.array_equal(host(free), rf)


def test_window_above_the_limit_is_refused(ctx, case):
    import rsl
    d = upload(ctx, case)
    hits, free = planes(ctx, case['shape'])
    with pytest.raises(ValueError, match='RSL_MAP_MAX_RW'):
        ctx.map_update(d['points'], d['seg'], d['poses'], hits, grid=(0.0, 0.0, 0.1), free=free, r_max=75.0)
    assert not host(hits).any() and not host(free).any()
    with pytest.raises(ValueError, match='383'):
        rsl.GridMap(ctx, origin=(0.0, 0.0), cell=0.1, shape=case['shape'], r_max=75.0)
    with pytest.raises(ValueError):
        ctx.map_update(d['points'], d['seg'], d['poses'], hits, grid=(0.0, 0.0, -0.5), free=free)
    with pytest.raises(ValueError):
        ctx.map_logodds(hits, free, l_min=1.0, l_max=0.0)


def test_ops_and_dropin(ctx, case):
    from rsl import ops
    from src.pose_integration.pose_integration import PoseIntegrator
    x0, y0, cell = case['grid']
    kw = dict(origin=(x0, y0), cell=cell, shape=case['shape'], **case['params'])
    n = case['n']
    seg = np.minimum(case['seg'], n)
    res = ops.grid_map(case['points'], seg, case['poses'], weight=case['weight'], ctx=ctx, **kw)
    rh, rf, rs = case['ref'][True, True]
    assert np.array_equal(res['hits'], rh) and np.array_equal(res['free'], rf) and np.array_equal(res['stats'], rs)
    assert res['logodds'].tobytes() == M.map_logodds(rh, rf).tobytes()
    scans = [[dict(x_m=float(p[3]), y_m=float(p[4]), power_db=float(p[5]), weight=float(w))
              for p, w in zip(case['points'][b:e], case['weight'][b:e])] for b, e in zip(seg[:-1], seg[1:])]
    out = PoseIntegrator().grid_map(scans, case['poses'][:, :3], case['poses'][:, 3:], **kw)
    assert np.array_equal(out['hits'], rh) and np.array_equal(out['free'], rf) and np.array_equal(out['stats'], rs)


A, C, S, F = 8, 16, 64, 3
TC = S / 10e6
CFG = dict(num_antennas=A, num_chirps=C, chirp_duration=TC, detector='cfar', detect_on='sum', cfar_guard=(1, 1),
           cfar_train=(0, 4), cfar_pfa=1e-4)
WORLD = [(2.1, -35.0), (2.9, 20.0), (3.8, -8.0), (4.6, 41.0), (5.3, -27.0), (6.2, 9.0), (7.0, -46.0), (7.7, 30.0),
         (8.4, -15.0), (4.1, -52.0), (5.8, 52.0), (3.3, 48.0)]


def test_update_chain(ctx):
    """Plumbing only (the generator's cubes do not focus in range: README): GridMap.update_chain equals the reference on
    the chain's own downloaded points, cell_base and vel_weight, with synthetic poses."""
    import rsl
    sc = [dict(range_sc=r, azimuth_sc=float(np.radians(a)), rcs=20.0, vr=0.0) for r, a in WORLD]
    cube = rsl.SyntheticCubes(ctx, sc, chirp_duration=TC, num_chirps=C, num_antennas=A, noise_power=1e-4).generate(
        F, seed=77, frame0=0)
    poses = np.array([M.yaw_pose(3.0 + 0.4 * f, 4.0 + 0.1 * f, 0.3 * f - 0.2, z=0.5) for f in range(F)])
    kw = dict(origin=(-8.0, -8.0), cell=0.25, shape=(96, 104), r_min=0.5, r_max=12.0)
    for extra in (dict(), dict(velocity_loss='tukey', velocity_scale=0.3)):
        ch = rsl.RadarChain(rsl.ChainConfig(**CFG, point_cloud=True, **extra), F, ctx)
        ch.run(cube)
        res = ch.results()
        w = res.get('vel_weight')
        assert (w is not None) == bool(extra)
        gm = rsl.GridMap(ctx, **kw)
        st = gm.update_chain(ch, ctx.to_dev(poses))
        rh, rf, rs = M.map_update(res['points'], res['cell_base'], poses, (-8.0, -8.0, 0.25), (96, 104), r_min=0.5,
                                  r_max=12.0, weight=w)
        assert (rs[:, 1] >= 4).all() and not rs[:, 3].any(), rs
        out = gm.results()
        assert np.array_equal(st.cpu().numpy(), rs) and np.array_equal(out['stats'], rs)
        assert np.array_equal(out['hits'], rh) and np.array_equal(out['free'], rf)
    plain = rsl.RadarChain(rsl.ChainConfig(**CFG), F, ctx)
    with pytest.raises(ValueError, match='point_cloud=True'):
        rsl.GridMap(ctx, **kw).update_chain(plain, ctx.to_dev(poses))
