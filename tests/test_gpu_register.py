"""rsl_scan_register on the device against its fp64 restatement (tests/register_ref.py).

The case list (register_ref.gpu_case): F = 4 frames of 40, 0, 300 and 700 points and a previous cloud of 60; the last
segment's end lies 1000 past the arrays (the clamp); a NaN point and ten weights <= 0 in the last frame.  Run with and
without rc, prev and weight, at K in {0, 20} and iters in {0, 10} (VARIANTS: every value of every option beside every
value of every other one at least once).

  flags, update counts  exact
  theta, t, W, rms      per column within 100 x the largest |fp64 - long double| difference of the reference on these
                        very variants, with a floor of 1e-12 (register_ref.tol, computed when the test runs).
                        Measured device error: theta 2.8e-16 rad, t 1.1e-14 m, W 1.6e-12 (of 5e2), rms 6.2e-16 m,
                        against tolerances of 1e-12, 1e-12, 7.1e-11 and 1e-12
  coarse winners        the iters = 0 variants return theta at the winner; the reference's best and second-best scores
                        differ by more than 1e-3 relative in every pair (asserted), so none is excluded
  determinism           two launches give the same bits
  omega                 row f - 1 = {0, 0, theta_f / dt}, row F - 1 = 0
"""
import functools
import itertools

import numpy as np
import pytest

import register_ref as R

pytestmark = pytest.mark.gpu

# (rc, prev, weight, K, iters)
VARIANTS = [(1, 1, 1, 20, 10), (0, 1, 1, 20, 10), (1, 0, 1, 20, 10), (1, 1, 0, 20, 10), (1, 1, 1, 0, 10),
            (1, 1, 1, 20, 0), (0, 0, 0, 0, 0), (0, 0, 0, 20, 10), (1, 0, 0, 0, 10), (0, 1, 0, 0, 0), (0, 0, 1, 0, 0)]
OVER = 1000  # the last segment's end beyond the arrays


def test_variants_cover_every_pair_of_options():
    for a, b in itertools.combinations(range(5), 2):
        seen = {(v[a], v[b]) for v in VARIANTS}
        assert len(seen) == 4, (a, b, seen)


def host_args(c, prev, weight):
    seg = c['seg'].copy()
    seg[-1] += OVER
    return dict(points=c['points'], seg=seg, weight=c['weight'] if weight else None,
                prev=c['prev'] if prev else None, init=c['init'])


@functools.lru_cache(maxsize=None)
def reference_rows():
    """The reference of every distinct (prev, weight, K, iters) in fp64 and long double, with its traces: computed once
    per session (tests/test_gpu_cloud.py takes its tolerances from the same rows), shared and left unchanged."""
    c = R.gpu_case()
    out = {}
    for _, prev, weight, K, iters in VARIANTS:
        key = (prev, weight, K, iters)
        if key in out:
            continue
        a = host_args(c, prev, weight)
        tr = {}
        r64, o64 = R.register(**a, K=K, iters=iters, traces=tr)
        wide, _ = R.register(**a, K=K, iters=iters, dtype=R.WIDE)
        out[key] = dict(rows=r64, omega=o64, wide=wide, traces=tr)
    return out


@pytest.fixture(scope='module')
def refs():
    return reference_rows()


@pytest.fixture(scope='module')
def tols(refs):
    return R.tol([(r['rows'], r['wide']) for r in refs.values()])


@pytest.fixture(scope='module')
def dev(ctx):
    c = R.gpu_case()
    seg = c['seg'].copy()
    seg[-1] += OVER
    d = {k: ctx.to_dev(c[k].copy()) for k in ('points', 'rc', 'weight', 'init')}
    d['seg'] = ctx.to_dev(seg)
    d['prev'] = {k: ctx.to_dev(v.copy()) for k, v in c['prev'].items()}
    return d


def run(ctx, d, rc, prev, weight, K, iters, **kw):
    args = dict(weight=d['weight'] if weight else None, prev=d['prev'] if prev else None, init=d['init'], k=K,
                iters=iters)
    if rc:
        args.update(rc=d['rc'], C=R.C_, axes=R.AXES)
    elif prev:
        args['prev'] = {k: v for k, v in d['prev'].items() if k != 'rc'}
    args.update(kw)
    rows, om = ctx.scan_register(d['points'], d['seg'], **args)
    return rows.cpu().numpy(), None if om is None else om.cpu().numpy()


def test_reference_gaps(refs):
    """Every coarse search of the case list has a clear winner: the comparison of winners below excludes none."""
    n = 0
    for key, r in refs.items():
        for f, tr in r['traces'].items():
            s = np.sort(tr['scores'])[::-1]
            if len(s) > 1 and s[0] > 0:
                assert (s[0] - s[1]) > 1e-3 * s[0], (key, f)
                n += 1
    assert n >= 8


@pytest.mark.parametrize('variant', VARIANTS, ids=lambda v: 'rc%d-prev%d-w%d-K%d-it%d' % v)
def test_against_reference(ctx, dev, refs, tols, variant):
    rc, prev, weight, K, iters = variant
    ref = refs[(prev, weight, K, iters)]
    tol, spread = tols
    rows, om = run(ctx, dev, *variant)
    want = ref['rows']
    err = np.abs(rows[:, :5] - want[:, :5]).max(axis=0)
    print(f'{variant}: device error {err}, tolerance {tol}, reference spread {spread}')
    assert np.array_equal(rows[:, 7], want[:, 7]), (rows[:, 7], want[:, 7])   # flags
    assert np.array_equal(rows[:, 6], want[:, 6]), (rows[:, 6], want[:, 6])   # updates applied
    assert list(want[:, 7]) == [0 if prev else 2, 1, 1, 0]
    assert (err <= tol).all(), (err, tol)
    assert (np.abs(rows[:, 5] - want[:, 5]) <= 1e-9).all()
    if iters == 0:  # the coarse winners, exactly: theta sits on the reference's candidate
        k_dev = np.rint((rows[:, 0] - dev['init'].cpu().numpy()[:, 0]) / R.DEFAULTS['dtheta'])
        k_ref = np.rint((want[:, 0] - R.gpu_case()['init'][:, 0]) / R.DEFAULTS['dtheta'])
        assert np.array_equal(k_dev, k_ref)
        assert not rows[:, 3:5].any() and not rows[:, 6].any()
    # omega: frame f's yaw rate in row f - 1, the last row 0
    dt = R.DEFAULTS['dt']
    assert np.array_equal(om[:-1, 2], rows[1:, 0] / dt) and not om[-1].any() and not om[:, :2].any()
    assert (np.abs(om - ref['omega']) <= tol[0] / dt).all()
    # two launches of the same problem: the same bits
    again, om2 = run(ctx, dev, *variant)
    assert again.tobytes() == rows.tobytes() and om2.tobytes() == om.tobytes()


def test_clamp_nan_and_weights(ctx, dev, tols):
    """The segment end past the arrays changes nothing, and the NaN point and the weights <= 0 count as absent: the
    rows equal those of the list without these points: exactly in flags and counts, and at the tolerance elsewhere (the
    lanes meet the remaining pairs in another order)."""
    c = R.gpu_case()
    rows, _ = run(ctx, dev, 1, 1, 1, 20, 10)
    exact = ctx.scan_register(dev['points'], ctx.to_dev(c['seg'].copy()), weight=dev['weight'], rc=dev['rc'], C=R.C_,
                              axes=R.AXES, prev=dev['prev'], init=dev['init'])[0].cpu().numpy()
    assert exact.tobytes() == rows.tobytes()
    w = R.effective_weight(c['points'], c['weight'])
    keep = w > 0
    assert (~keep).sum() == 11 and keep[:c['seg'][3]].all()
    seg = c['seg'].copy()
    seg[-1] -= 11
    got = ctx.scan_register(ctx.to_dev(c['points'][keep].copy()), ctx.to_dev(seg), weight=ctx.to_dev(c['weight'][keep]),
                            rc=ctx.to_dev(c['rc'][keep].copy()), C=R.C_, axes=R.AXES, prev=dev['prev'],
                            init=dev['init'])[0].cpu().numpy()
    assert np.array_equal(got[:, 6:], rows[:, 6:])
    assert (np.abs(got[:, :5] - rows[:, :5]).max(axis=0) <= tols[0]).all()


def test_outputs_and_empty_batch(ctx, dev):
    rows, om = run(ctx, dev, 1, 1, 1, 20, 10, want_omega=False)
    assert om is None and rows.shape == (4, 8)
    torch = ctx.torch
    buf = dict(rows=torch.full((4, 8), 7.0, dtype=torch.float64, device=ctx.device),
               omega=torch.full((4, 3), 7.0, dtype=torch.float64, device=ctx.device))
    r2, o2 = ctx.scan_register(dev['points'], dev['seg'], weight=dev['weight'], rc=dev['rc'], C=R.C_, axes=R.AXES,
                               prev=dev['prev'], init=dev['init'], out=buf)
    assert r2 is buf['rows'] and o2 is buf['omega'] and r2.cpu().numpy().tobytes() == rows.tobytes()
    # F = 0 launches nothing and touches nothing
    ctx.timing(True)
    ctx.timing_reset()
    r0, o0 = ctx.scan_register(dev['points'], dev['seg'][:1], out=buf)
    ctx.sync()
    n_aux = ctx.timing_read()['aux'][1]
    ctx.timing(False)
    assert n_aux == 0 and r0.cpu().numpy().tobytes() == rows.tobytes()
    # F = 1: one pair against prev, the only omega row is 0
    r1, o1 = ctx.scan_register(dev['points'], dev['seg'][:2], prev=dev['prev'], init=dev['init'][:1].contiguous(),
                               weight=dev['weight'], rc=dev['rc'], C=R.C_, axes=R.AXES)
    assert r1.cpu().numpy().tobytes() == rows[:1].tobytes() and not o1.cpu().numpy().any()


def test_argument_errors(ctx, dev):
    ok = dict(weight=dev['weight'], rc=dev['rc'], C=R.C_, axes=R.AXES, prev=dev['prev'], init=dev['init'])
    nan = float('nan')
    bad = [dict(h=0.0), dict(h=nan), dict(h=-1.0), dict(h_coarse=0.4), dict(h_coarse=float('inf')), dict(dtheta=0.0),
           dict(dtheta=nan), dict(dt=0.0), dict(dt=nan), dict(w_min=nan), dict(w_min=-1.0), dict(tol=nan),
           dict(k=-1), dict(k=R.MAX_K + 1), dict(iters=-1), dict(iters=R.MAX_ITERS + 1), dict(shrink=0.0),
           dict(shrink=1.5), dict(shrink=nan), dict(axes=None), dict(C=0), dict(axes=(0.0, 0.0, 0.0, 1.0)),
           dict(axes=(0.0, nan, 0.0, 1.0))]
    for kw in bad:
        with pytest.raises(ValueError):
            ctx.scan_register(dev['points'], dev['seg'], **{**ok, **kw})
    with pytest.raises(ValueError):  # prev_rc alone needs the axes too
        ctx.scan_register(dev['points'], dev['seg'], prev=dev['prev'])
    with pytest.raises(ValueError):
        ctx.scan_register(dev['points'][:, :7].contiguous(), dev['seg'])
    with pytest.raises(ValueError):  # the kernel would read an int32 seg as int64, past its end
        ctx.scan_register(dev['points'], dev['seg'].to(ctx.torch.int32))
    with pytest.raises(ValueError):
        ctx.scan_register(dev['points'], dev['seg'], init=dev['init'][:2].contiguous())
    from rsl import _lib
    assert (_lib.REG_MAX_K, _lib.REG_MAX_ITERS) == (R.MAX_K, R.MAX_ITERS) == (64, 100)
    # the limits themselves are accepted
    rows, _ = ctx.scan_register(dev['points'], dev['seg'], **ok, k=R.MAX_K, iters=R.MAX_ITERS, shrink=1.0, tol=0.0)
    assert rows.cpu().numpy()[3, 7] == 0


def test_ops_and_dropin(ctx, dev, refs, tols):
    from rsl import ops
    from src.angle_estimation.angle_estimation import AngleEstimator
    c = R.gpu_case()
    a = host_args(c, 1, 1)
    res = ops.register_scans(a['points'], a['seg'], weight=a['weight'], rc=c['rc'], C=R.C_, axes=R.AXES,
                             prev=c['prev'], init=a['init'], ctx=ctx)
    rows, _ = run(ctx, dev, 1, 1, 1, 20, 10)
    assert res['rows'].tobytes() == rows.tobytes() and res['omega'].shape == (4, 3)
    assert set(res) == set(ops.REGISTRATION_COLUMNS) | {'rows', 'omega'}
    for k, name in enumerate(ops.REGISTRATION_COLUMNS):
        assert np.array_equal(res[name], rows[:, k])
    # the drop-in on target dicts: frame 3 against frame 2, no rc (the lists carry none)
    seg = c['seg']
    w = R.effective_weight(c['points'], c['weight'])

    def targets(b, e):
        return [dict(x_m=float(p[3]), y_m=float(p[4]), weight=float(wi)) for p, wi in zip(c['points'][b:e], w[b:e])
                if np.isfinite(p[3])]
    est = AngleEstimator(num_antennas=8)
    got = est.register_scans(targets(seg[2], seg[3]), targets(seg[3], seg[4]), init=c['init'][3])
    want = refs[(1, 1, 20, 10)]['rows'][3]
    tol = tols[0]
    assert got['flag'] == 0 and got['updates'] == want[6]
    assert abs(got['theta_rad'] - want[0]) <= tol[0] and abs(got['t_x'] - want[1]) <= tol[1]
    assert abs(got['t_y'] - want[2]) <= tol[2] and abs(got['support'] - want[3]) <= tol[3]
    assert got['theta_deg'] == np.degrees(got['theta_rad'])
    truth = c['truth'][3]
    assert abs(got['theta_rad'] - truth[0]) < np.radians(0.03) and abs(got['t_x'] - truth[1]) < 0.02
    none = est.register_scans([], targets(seg[3], seg[4]))
    assert none['flag'] == 1 and none['theta_rad'] == 0.0 and none['support'] == 0.0
