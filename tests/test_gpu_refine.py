"""GPU: rsl_cell_refine (rsl_refine.hip) against the fp64 restatement of its specification, tests/refine_ref.py, on
the case list refine_ref.gpu_case builds (tests/test_refine_host.py shows on a CPU that the reference is sound and
that these inputs catch six plausible mistakes).

Shapes: F = 3, S = 16, C = 8, G = 37 (a 5 degree grid), A in {2, 3, 4, 8, 16, 32} (the fixed instances 4, 8, 16 and the
runtime one), 700 cells with repeats (three blocks, the last partly filled), every corner of every frame, both grid
ends, an all-zero cell, pm == pp, gidx = G and -1, and a gidx at a minimum of the beam.

Tolerances.
    out_points  2 ulp of fp32 per field against the reference's fp64 value rounded once: one for the final rounding
                falling either way, one spare.  The reference reads the very fp32 power map the kernel read, and every
                decision compares fp32 values, so no cell is excluded.
    out_az      100 x the largest |fp64 - long double| difference of the reference's azimuth on these very cells,
                computed when the test runs (refine_ref.az_tol).  On this case list the difference is
                    A = 2: 1.7e-13   3: 1.4e-14   4: 2.1e-14   8: 7.2e-15   16: 3.0e-16   32: 3.6e-16 rad
                (the vertex divides by the second difference of three nearly equal beam values: the wider the beam,
                the more digits cancel), so the tolerance runs from 3.0e-14 to 1.7e-11 rad.
    measured on an MI355X: every field of every case 0 ulp from the reference; azimuth 1.3e-13 rad at A = 2, 8.9e-15 at
    3, 6.2e-15 at 4, 8.9e-16 at 8, 2.2e-16 at 16 and 32 (all below the reference's own spread); the chain's points 0 ulp,
    its azimuths within 6.9e-15 rad (reference spread 3.4e-14).
"""
from ctypes import c_double, c_void_p

import numpy as np
import pytest

import parity as P
import radar_oracle as O
import refine_ref as R

pytestmark = pytest.mark.gpu

# every estimator on each axis
MODE_PAIRS = [(R.HANN, R.RECT), (R.LOG, R.HANN), (R.RECT, R.LOG), (R.NONE, R.NONE)]


@pytest.fixture(scope='module')
def dev(ctx):
    """The case of every A on the device, with the power map rsl_power_integrate forms of it."""
    out = {}
    for A in R.GPU_A:
        c = R.gpu_case(A)
        d = dict(case=c, **{k: ctx.to_dev(c[k].copy()) for k in ('rds', 'frame', 'rc', 'gidx', 'az_table', 'steer')})
        d['power'] = ctx.integrate_power(d['rds'])
        d['power_host'] = d['power'].cpu().numpy()
        out[A] = d
    return out


def run(ctx, d, modes, power='map', **kw):
    return ctx.cell_refine(d['rds'], d['frame'], d['rc'], d['gidx'], d['az_table'], d['steer'],
                           power=d['power'] if power == 'map' else None, range_mode=modes[0], doppler_mode=modes[1],
                           axes=R.AXES, **kw)


@pytest.mark.parametrize('A', R.GPU_A)
def test_against_reference(ctx, dev, A):
    d = dev[A]
    c = d['case']
    assert np.array_equal(d['power_host'], R.power_f32(c['rds'])), 'the reference power sum is not the device\'s'
    for modes in MODE_PAIRS:
        pts, az = run(ctx, d, modes)
        pts, az = pts.cpu().numpy(), az.cpu().numpy()
        assert pts.shape == (R.N_, 8) and pts.dtype == np.float32 and az.shape == (R.N_,) and az.dtype == np.float64
        ref = R.refine(c['rds'], d['power_host'], c['frame'], c['rc'], c['gidx'], c['az_table'], c['steer'], *modes,
                       R.AXES)
        ulp = R.ulp_distance(pts, ref['points'])
        tol, spread = R.az_tol(c, *modes)
        want = ref['az'].astype(np.float64)
        assert np.array_equal(np.isnan(az), np.isnan(want))
        err = np.abs(az - want)[~np.isnan(want)]
        print(f'A = {A} modes {modes}: points worst {ulp.max():.1f} ulp (by column {ulp.max(axis=0)}), azimuth worst '
              f'{err.max():.2e} rad (reference spread {spread:.2e}, tolerance {tol:.2e})')
        assert (ulp <= R.POINTS_TOL_ULP).all(), (A, modes, np.argwhere(ulp > R.POINTS_TOL_ULP)[:5])
        assert (err <= tol).all(), (A, modes, err.max(), tol)
        # the cells the list was forced to hold
        nm = c['named']
        assert np.isnan(pts[nm['gover'], 2:5]).all() and np.isnan(pts[nm['gunder'], 2:5]).all()
        assert not np.isnan(pts[[nm['gover'], nm['gunder']]][:, [0, 1, 5, 6, 7]]).any()
        assert pts[nm['equal'], 7] == 0.0 and pts[nm['zero'], 6] == 0.0 and pts[nm['zero'], 7] == 0.0
        assert az[nm['g0']] == c['az_table'][0] and az[nm['gend']] == c['az_table'][-1]
        assert az[nm['lowest']] == c['az_table'][c['gidx'][nm['lowest']]]
        i = c['rc'] // R.C_
        assert (pts[(i == 0) | (i == R.S_ - 1), 6] == 0.0).all()
        if modes[0] == R.NONE:
            assert (pts[:, 6] == 0.0).all() and (pts[:, 7] == 0.0).all()


@pytest.mark.parametrize('A', R.GPU_A)
def test_null_power_is_bit_identical(ctx, dev, A):
    d = dev[A]
    for modes in MODE_PAIRS[:2]:
        a = run(ctx, d, modes)
        b = run(ctx, d, modes, power=None)
        for x, y in zip(a, b):
            assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes(), (A, modes)


def test_outputs_one_at_a_time(ctx, dev):
    d = dev[8]
    pts, az = run(ctx, d, MODE_PAIRS[0])
    p2, a2 = run(ctx, d, MODE_PAIRS[0], want_az=False)
    assert a2 is None and p2.cpu().numpy().tobytes() == pts.cpu().numpy().tobytes()
    p3, a3 = run(ctx, d, MODE_PAIRS[0], want_points=False)
    assert p3 is None and a3.cpu().numpy().tobytes() == az.cpu().numpy().tobytes()


@pytest.mark.parametrize('A', [3, 8])
def test_device_count_below_capacity(ctx, dev, A):
    torch = ctx.torch
    d = dev[A]
    full_p, full_a = (t.cpu().numpy() for t in run(ctx, d, MODE_PAIRS[0]))
    for count in (0, 1, 300, R.N_, R.N_ + 50):
        n = min(count, R.N_)
        out = dict(points=torch.full((R.N_, 8), -7.0, dtype=torch.float32, device=ctx.device),
                   az=torch.full((R.N_,), -7.0, dtype=torch.float64, device=ctx.device))
        ndev = torch.tensor([count], dtype=torch.int64, device=ctx.device)
        pts, az = run(ctx, d, MODE_PAIRS[0], n_dev=ndev, out=out)
        assert pts is out['points'] and az is out['az']
        pts, az = pts.cpu().numpy(), az.cpu().numpy()
        assert pts[:n].tobytes() == full_p[:n].tobytes() and az[:n].tobytes() == full_a[:n].tobytes(), count
        assert (pts[n:] == -7.0).all() and (az[n:] == -7.0).all(), count  # the canary beyond the count


def test_empty_list_launches_nothing(ctx, dev):
    torch = ctx.torch
    d = dev[4]
    out = dict(points=torch.full((4, 8), -7.0, dtype=torch.float32, device=ctx.device),
               az=torch.full((4,), -7.0, dtype=torch.float64, device=ctx.device))
    ctx.timing(True)
    try:
        ctx.timing_reset()
        run(ctx, d, MODE_PAIRS[0], n=0, out=out)
        # null lists are fine with no cell
        ctx.cell_refine(d['rds'], d['frame'][:0], d['rc'][:0], None, None, d['steer'], n=0, out=out)
        assert ctx.timing_read()['cell_extras'][1] == 0
        run(ctx, d, MODE_PAIRS[0])
        assert ctx.timing_read()['cell_extras'][1] == 1  # timed under RSL_K_CELL_EXTRAS
    finally:
        ctx.timing_reset()
        ctx.timing(False)
    assert (out['points'].cpu().numpy() == -7.0).all() and (out['az'].cpu().numpy() == -7.0).all()


def test_argument_errors(ctx, dev):
    torch = ctx.torch
    lib = ctx.lib
    d = dev[4]
    pts = torch.zeros((R.N_, 8), dtype=torch.float32, device=ctx.device)
    az = torch.zeros((R.N_,), dtype=torch.float64, device=ctx.device)
    p = lambda t: None if t is None else c_void_p(t.data_ptr())
    a4 = (c_double * 4)(*R.AXES)
    good = dict(rds=p(d['rds']), power=p(d['power']), A=4, S=R.S_, C=R.C_, frame=p(d['frame']), rc=p(d['rc']),
                ndev=None, n=R.N_, gidx=p(d['gidx']), tab=p(d['az_table']), steer=p(d['steer']), G=R.G_, rm=R.HANN,
                dm=R.RECT, axes=a4, pts=p(pts), az=p(az))

    def call(**kw):
        a = {**good, **kw}
        return lib.rsl_cell_refine(ctx.h, a['rds'], a['power'], a['A'], a['S'], a['C'], a['frame'], a['rc'], a['ndev'],
                                   a['n'], a['gidx'], a['tab'], a['steer'], a['G'], a['rm'], a['dm'], a['axes'],
                                   a['pts'], a['az'])
    ctx._bind()
    assert call() == 0
    assert call(power=None) == 0 and call(pts=None) == 0 and call(az=None) == 0
    nan4 = lambda k, v: (c_double * 4)(*[v if i == k else x for i, x in enumerate(R.AXES)])
    bad = [dict(A=1), dict(A=33), dict(A=0), dict(S=0), dict(C=0), dict(G=0), dict(G=-3), dict(rm=4), dict(rm=-1),
           dict(dm=4), dict(dm=-1), dict(axes=nan4(1, float('nan'))), dict(axes=nan4(1, float('inf'))),
           dict(axes=nan4(3, float('nan'))), dict(axes=nan4(3, -float('inf'))), dict(rds=None), dict(frame=None),
           dict(rc=None), dict(gidx=None), dict(tab=None), dict(steer=None), dict(axes=None),
           dict(pts=None, az=None), dict(pts=None, az=None, n=0), dict(pts=c_void_p(pts.data_ptr() + 4))]
    for kw in bad:
        rc = call(**kw)
        assert rc == 1, (list(kw), rc)  # RSL_ERR_INVALID
        with pytest.raises(ValueError):
            ctx.check(rc, 'rsl_cell_refine')
    assert lib.rsl_cell_refine(None, *[None] * 2, 4, 4, 4, *[None] * 3, 0, *[None] * 3, 4, 0, 0, None, None, None) == 1
    # a start that is not finite is the caller's business (only the steps are checked), and the wrapper's own checks
    assert call(axes=nan4(0, float('nan'))) == 0
    with pytest.raises(ValueError):
        run(ctx, d, ('parabola', 'rect'))
    with pytest.raises(ValueError):
        run(ctx, d, ('hann', 'sinc'))
    with pytest.raises(ValueError):
        ctx.cell_refine(d['rds'], d['frame'], d['rc'], d['gidx'], d['az_table'], dev[8]['steer'])
    with pytest.raises(ValueError):
        ctx.cell_refine(d['rds'], d['frame'], d['rc'], d['gidx'], d['az_table'][:5], d['steer'])
    with pytest.raises(ValueError):
        ctx.cell_refine(d['rds'], d['frame'], d['rc'], d['gidx'], d['az_table'], d['steer'],
                        power=d['power'].to(torch.float64))


def test_ops_and_dropin(ctx, dev):
    """ops.refine_cells on one frame (gidx given, and from its own scan), and the target dicts of the drop-in."""
    from rsl import ops, tables
    from src.angle_estimation.angle_estimation import AngleEstimator
    c = R.gpu_case(8)
    f0 = np.nonzero((c['frame'] == 0) & (c['gidx'] >= 0) & (c['gidx'] < R.G_))[0]
    rb, db = c['rc'][f0] // R.C_, c['rc'][f0] % R.C_
    steer128 = tables.steering_matrix(R.grid_deg(), np.arange(8) * 0.5, 1.0)
    assert np.array_equal(steer128.astype(np.complex64), c['steer'])
    res = ops.refine_cells(steer128, R.grid_deg(), rds=c['rds'][0], rbins=rb, dbins=db, gidx=c['gidx'][f0],
                           range_mode='hann', doppler_mode='rect', axes=R.AXES, ctx=ctx)
    ref = R.refine(c['rds'][:1], None, np.zeros(len(f0), int), c['rc'][f0], c['gidx'][f0], c['az_table'], c['steer'],
                   R.HANN, R.RECT, R.AXES)
    assert (R.ulp_distance(res['points'], ref['points']) <= R.POINTS_TOL_ULP).all()
    assert set(res) == set(ops.POINT_COLUMNS) | {'points', 'az_refined', 'azimuth_deg', 'gidx'}
    for k, name in enumerate(ops.POINT_COLUMNS):
        assert np.array_equal(res[name], res['points'][:, k], equal_nan=True)
    own = ops.refine_cells(steer128, R.grid_deg(), rds=c['rds'][0], rbins=rb[:40], dbins=db[:40], range_mode='hann',
                           doppler_mode='rect', axes=R.AXES, ctx=ctx)
    assert own['points'].shape == (40, 8) and own['gidx'].shape == (40,) and not np.isnan(own['points']).any()
    assert ops.refine_cells(steer128, R.grid_deg(), rds=c['rds'][0], rbins=[], dbins=[], gidx=[],
                            ctx=ctx)['points'].shape == (0, 8)
    # the drop-in: a plane wave between two grid points, one off-bin tone
    est = AngleEstimator(num_antennas=8)
    S, C, true = 32, 16, 17.13
    n, m = np.arange(S), np.arange(C)
    from scipy.signal import windows
    x = windows.hann(S)[:, None] * np.exp(2j * np.pi * (9.3 * n[:, None] / S + 5.2 * m[None, :] / C))
    X = np.fft.fft2(x)
    rds = (O.steering_vector(true)[:, None, None] * X[None]).astype(np.complex64)
    peak = dict(range_bin=9, doppler_bin=5, range_m=9 * 0.5, doppler_hz=5 * 100.0 - 800.0, power_db=0.0, antenna=0)
    info = dict(peaks=[peak], range_bins_m=np.arange(S) * 0.5, doppler_bins_hz=np.arange(C) * 100.0 - 800.0)
    plain = est.process_targets(rds, info)
    got = est.process_targets_refined(rds, info)
    assert len(got) == 1 and set(got[0]) == set(plain[0]) | {
        'range_m_refined', 'doppler_hz_refined', 'azimuth_deg_refined', 'x_m', 'y_m', 'range_offset', 'doppler_offset'}
    t = got[0]
    assert t['azimuth_deg'] == plain[0]['azimuth_deg'] == 17.0
    assert abs(t['azimuth_deg_refined'] - true) < 1e-3
    # the biases of the two estimators at these sizes (tests/test_refine_host.py), with 1.5x headroom
    assert abs(t['range_offset'] - 0.3) < 1.5 * 6.1e-2 and abs(t['doppler_offset'] - 0.2) < 1.5 * 6.2e-4
    assert t['range_m_refined'] == pytest.approx(0.5 * (9 + t['range_offset']), rel=1e-6)
    assert t['doppler_hz_refined'] == pytest.approx(100.0 * (5 + t['doppler_offset']) - 800.0, rel=1e-6)
    az = np.radians(t['azimuth_deg_refined'])
    assert t['x_m'] == pytest.approx(t['range_m_refined'] * np.cos(az), rel=1e-6)
    assert t['y_m'] == pytest.approx(t['range_m_refined'] * np.sin(az), rel=1e-6)
    assert est.process_targets_refined(rds, dict(peaks=[]), window_type='blackman') == []


# -- the chain ---------------------------------------------------------------------------------------------------------
TINY = dict(num_antennas=8, num_chirps=16, chirp_duration=3.2e-6)  # the smallest shape of tests/test_gpu_chain.py
DEFAULT_KEYS = {'entry_base', 'cell_base', 'e_ant', 'e_rbin', 'e_dbin', 'e_cell', 'e_pdb', 'c_frame', 'c_rc',
                'c_amask', 'gidx', 'esprit', 'phase', 'az', 'velocity', 'grid'}


def make_cube(ctx, A, C, Tc, seeds):
    frames = []
    for s in seeds:
        np.random.seed(s)
        frames.append(O.synthesize_frame(O.TEST_SCENE, chirp_duration=Tc, num_chirps=C, num_antennas=A))
    return ctx.to_dev(np.stack(frames).astype(np.complex64))


@pytest.fixture(scope='module')
def tiny(ctx):
    import rsl
    cube = make_cube(ctx, 8, 16, 3.2e-6, (1000, 1001))
    out = {}
    for name, kw in (('plain', {}), ('pc', dict(point_cloud=True)),
                     ('pc_sum', dict(point_cloud=True, detect_on='sum', pc_velocity=True, window_type='blackman')),
                     ('sum', dict(detect_on='sum', window_type='blackman'))):
        ch = rsl.RadarChain(rsl.ChainConfig(**TINY, **kw), 2, ctx)
        ch.run(cube)
        res = ch.results()
        res['chain'] = ch
        out[name] = res
    return out


@pytest.mark.parametrize('name', ['pc', 'pc_sum'])
def test_chain_points(tiny, name):
    from rsl import tables
    r = tiny[name]
    ch = r['chain']
    cfg = ch.cfg
    nc = int(r['cell_base'][-1])
    assert nc >= 6 and r['points'].shape == (nc, 8) and r['points'].dtype == np.float32
    assert r['az_refined'].shape == (nc,) and r['az_refined'].dtype == np.float64
    rds, power = ch.rds.cpu().numpy(), ch.power.cpu().numpy()
    assert np.array_equal(power, R.power_f32(rds))  # integrated in run_back, or the detector's own map
    steer = tables.steering_matrix(ch.grid, np.arange(8) * cfg.lambda_c / 2, cfg.lambda_c).astype(np.complex64)
    axes = tables.point_axes(cfg, ch.S, ch.C, velocity=cfg.pc_velocity)
    modes = (R.MODES[tables.refine_mode_for_window(cfg.window_type)], R.RECT)
    assert modes[0] == (R.HANN if name == 'pc' else R.LOG)
    args = (rds, power, r['c_frame'], r['c_rc'], r['gidx'], np.radians(ch.grid), steer, *modes, axes)
    ref, wide = R.refine(*args), R.refine(*args, wide=True)
    ulp = R.ulp_distance(r['points'], ref['points'])
    spread = float(np.abs(ref['az'].astype(wide['az'].dtype) - wide['az']).max())
    err = np.abs(r['az_refined'] - ref['az'])
    print(f'{name}: {nc} cells, points worst {ulp.max():.1f} ulp, azimuth worst {err.max():.2e} rad (reference spread '
          f'{spread:.2e})')
    assert (ulp <= R.POINTS_TOL_ULP).all() and (err <= 100 * spread).all()
    # the labels at integer bins are the reference project's, and the refined azimuth stays next to its grid point
    i, j = r['c_rc'] // ch.C, r['c_rc'] % ch.C
    whole = r['points'][:, 6] == 0
    assert np.allclose(r['points'][whole, 0], tables.range_axis(cfg.bandwidth, ch.S)[i[whole]], rtol=1e-6)
    if not cfg.pc_velocity:
        lab = tables.doppler_axis(cfg.sampling_rate, ch.C)
        step = lab[1] - lab[0]
        assert np.allclose(r['points'][:, 1] - step * r['points'][:, 7], lab[j], rtol=0, atol=1e-6 * abs(lab[0]))
    else:
        vstep = cfg.lambda_c / (2 * ch.C * cfg.pri)
        assert axes[3] == vstep and axes[2] == -(ch.C // 2) * vstep
    inner = (r['gidx'] > 0) & (r['gidx'] < len(ch.grid) - 1)
    assert (np.abs(np.degrees(r['az_refined']) - ch.grid[r['gidx']])[inner] < 0.5).all()  # between its neighbours
    assert (r['az_refined'] != r['az'])[inner].mean() > 0.9
    # everything the chain computed before is as it was
    base = tiny['plain' if name == 'pc' else 'sum']
    for k in DEFAULT_KEYS - {'grid'}:
        assert np.ascontiguousarray(r[k]).tobytes() == np.ascontiguousarray(base[k]).tobytes(), k


def test_chain_defaults_unchanged(tiny):
    import rsl
    r = tiny['plain']
    assert set(r) - {'chain'} == DEFAULT_KEYS
    ch = r['chain']
    assert ch.pc is None and ch.power is None and not hasattr(ch, 'pc_steer')
    assert tiny['sum']['chain'].pc is None
    cfg = rsl.ChainConfig()
    assert (cfg.point_cloud, cfg.pc_velocity, cfg.velocity_az) == (False, False, 'grid')
    for kw in (dict(velocity_az='vertex'), dict(velocity_az='refined'), dict(point_cloud=True, window_type='kaiser'),
               dict(point_cloud=True, num_antennas=1)):
        with pytest.raises(ValueError):
            rsl.ChainConfig(**kw)


CH = dict(num_antennas=8, num_chirps=64, chirp_duration=25.6e-6)  # the solver tests' chain shape
SCALE = 0.3
SOLVERS = {'ls': {}, 'tukey': dict(velocity_loss='tukey', velocity_scale=SCALE, velocity_iters=15, velocity_tol=0.0),
           'consensus': dict(velocity_loss='consensus', velocity_scale=SCALE, velocity_hyps=300, velocity_seed=4,
                             velocity_refine=2)}


@pytest.fixture(scope='module')
def refined_chains(ctx):
    import rsl
    cube = make_cube(ctx, 8, 64, 25.6e-6, (1000, 1001))
    out = {}
    for name, kw in SOLVERS.items():
        ch = rsl.RadarChain(rsl.ChainConfig(**CH, point_cloud=True, velocity_az='refined', **kw), 2, ctx)
        ch.run(cube)
        res = ch.results()
        res['chain'] = ch
        out[name] = res
    ch = rsl.RadarChain(rsl.ChainConfig(**CH), 2, ctx)
    ch.run(cube)
    out['grid'] = ch.results()
    return out


@pytest.mark.parametrize('loss', list(SOLVERS))
def test_chain_velocity_on_refined_azimuths(ctx, refined_chains, loss):
    """The chain's solve equals the per-call solver fed the chain's refined azimuths (the device's, and the solver's
    fp64 oracle at the tolerances of its own tests), and it is another solve than the grid's."""
    import vel_consensus_ref as VC
    import vel_robust_ref as VR
    r = refined_chains[loss]
    ch = r['chain']
    nc = int(r['cell_base'][-1])
    az, y, m, seg = r['az_refined'], r['phase'], VR.popcount(r['c_amask']), r['cell_base']
    assert nc >= 6 and not np.isnan(az).any()
    d = dict(az=ch.pc.out['az'], y=ch.ext['phase'], seg=ch.offs['cell_base'], amask=ch.lists['c_amask'], k=ch.k,
             n=ch.cell_cap)
    print()
    if loss == 'ls':
        own, _, _ = ctx.velocity(**d)
        for f in range(2):
            sl = slice(seg[f], seg[f + 1])
            vx, vy, cost = O.velocity_ls(np.repeat(az[sl], m[sl]), np.repeat(y[sl], m[sl]), lambda_c=3e8 / ch.cfg.fc)
            v = r['velocity'][f]
            print(f'ls frame {f}: chain ({v[0]:.6e}, {v[1]:.6e}) oracle ({vx:.6e}, {vy:.6e})')
            assert abs(v[0] - vx) < P.VEL_ATOL and abs(v[1] - vy) < P.VEL_ATOL
            assert abs(v[2] - cost) <= P.VEL_COST_RTOL * cost
    elif loss == 'tukey':
        own, _, _ = ctx.velocity_robust(**d, loss='tukey', scale=SCALE, iters=15, tol=0.0)
        ref = VR.robust_batch(az, y, m, seg, k=ch.k, loss='tukey', scale=SCALE, iters=15, tol=0.0)
        VR.compare('chain', r['velocity'], r['vel_weight'].astype(np.float64), None, ref, tol=0.0)
    else:
        own, _, _ = ctx.velocity_consensus(**d, scale=SCALE, hyps=300, seed=4, refine=2, frame0=0)
        ref = VC.consensus_batch(az, y, m, seg, k=ch.k, scale=SCALE, hyps=300, seed=4, refine=2, frame0=0)
        VC.compare('chain', r['velocity'], r['vel_weight'].astype(np.float64), None, ref)
    assert np.abs(own.cpu().numpy()[:, :2] - r['velocity'][:, :2]).max() < P.VEL_ATOL
    g = refined_chains['grid']
    for k in ('cell_base', 'c_rc', 'gidx', 'phase'):
        assert np.ascontiguousarray(g[k]).tobytes() == np.ascontiguousarray(r[k]).tobytes(), k
    if loss == 'ls':
        assert (g['velocity'][:, :2] != r['velocity'][:, :2]).any()
