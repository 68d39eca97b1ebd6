"""The three velocity kernels at the edges of their cell loops.  The loaders step by threads x 8 cells (4096 per trip in
k_velocity / k_velocity_robust, 2048 in k_velocity_consensus, whose scoring chunk is 1024), so a loader, a clamp or a
chunk boundary can go wrong first at frames of 0, 1, 2 cells and of one cell below, at and above those steps.  One batch
per solver holds such frames in a row, on the grid-index path with masks (zero masks included) and on the azimuth path
without; n one below the last segment's end puts the clamp on a trip edge.  References and tolerances are those of
test_gpu_vel_robust.py (test_oracle_parity, test_ls_equivalence), test_gpu_vel_consensus.py (test_oracle_parity) and,
for rsl_velocity's per-cell outputs, test_gpu_vel_groups.py (test_velocity_grid_path): tests/vel_robust_ref.py and
tests/vel_consensus_ref.py derive the first two sets."""
import numpy as np
import pytest

import test_gpu_vel_consensus as TC
import test_gpu_vel_robust as TR
import vel_consensus_ref as C
import vel_robust_ref as R

pytestmark = pytest.mark.gpu

K, RIDGE = R.K_CHAIN, TR.RIDGE
TRIP = 512 * 8    # cells per loader trip of k_velocity and k_velocity_robust
CTRIP = 256 * 8   # of k_velocity_consensus; C.CHUNK cells per scoring chunk
LS_LENGTHS = [TRIP + 1, 0, 1, TRIP - 1, 2, TRIP]  # the last frame ends on a trip edge: n - 1 clamps it there
CV_LENGTHS = [CTRIP + 1, 0, 1, C.CHUNK - 1, 2, C.CHUNK, C.CHUNK + 1, CTRIP - 1, CTRIP]
assert C.CHUNK == 1024
PATHS = ['gidx', 'az']


def ls_batch(path):
    """The frames of LS_LENGTHS; path 'gidx': grid indices with masks, 'az': azimuths, every multiplicity 1."""
    d = TR.make_batch(LS_LENGTHS, seed0=800, mmax=8 if path == 'gidx' else 0)
    assert path == 'az' or (d['m'] == 0).any()
    return d


def cv_batch(path):
    d = TC.make_batch(CV_LENGTHS, seed0=900, mmax=8 if path == 'gidx' else 0)
    assert path == 'az' or (d['m'] == 0).any()
    return d


def clamps(d):
    """n: the arrays' length, and one below the last segment's end."""
    return [len(d['y']), len(d['y']) - 1]


def ls_ref(d, path, n, bounds=R.BOX):
    """rsl_velocity's rows {vx, vy, cost, rmse, n} from the oracle's moments and box solve."""
    seg = np.minimum(d['seg'], n)
    m = d['m'].astype(np.float64) if path == 'gidx' else np.ones(len(d['y']))
    cs, sn = np.cos(d['az']), np.sin(d['az'])
    rows = np.zeros((len(seg) - 1, 5))
    for f in range(len(seg) - 1):
        sl = slice(seg[f], max(seg[f], seg[f + 1]))
        x = R.box_solve(R.moments(m[sl], cs[sl], sn[sl], d['y'][sl]), K, RIDGE, bounds)
        r = d['y'][sl] - K * (x[0] * cs[sl] + x[1] * sn[sl])
        r2, w = float((m[sl] * r * r).sum()), m[sl].sum()
        rows[f] = [x[0], x[1], r2 + RIDGE * (x * x).sum(), np.sqrt(r2 / w) if w > 0 else 0.0, w]
    return rows, seg


def robust_ref(d, path, n, loss, scale):
    kw = dict(loss=loss, scale=scale, iters=20, tol=0.0, ridge=RIDGE)  # test_oracle_parity's
    return R.robust_batch(d['az'], d['y'], d['m'] if path == 'gidx' else None, d['seg'], n=n, k=K, **kw), kw


def consensus_ref(d, path, n, hyps):
    kw = dict(hyps=hyps, seed=11, ridge=RIDGE)  # test_oracle_parity's
    return TC.oracle(d, with_mask=path == 'gidx', n=n, **kw), kw


@pytest.fixture(scope='module')
def batches(ctx):
    out = {}
    for path in PATHS:
        for name, d in (('ls', ls_batch(path)), ('cv', cv_batch(path))):
            out[name, path] = d, TR.dev(ctx, d, az_path=path == 'az', with_mask=path == 'gidx')
    return out


@pytest.mark.parametrize('path', PATHS)
def test_ls_trip_edges(ctx, batches, path):
    d, dd = batches['ls', path]
    tab = ctx.to_dev(R.grid_rad()) if path == 'gidx' else None
    cs, sn = np.cos(d['az']), np.sin(d['az'])
    m = d['m'] if path == 'gidx' else np.ones(len(d['y']), np.int64)
    print()
    for n in clamps(d):
        rows, seg = ls_ref(d, path, n)
        o, r, p = ctx.velocity(dd['az'], dd['y'], dd['seg'], k=K, ridge=RIDGE, amask=dd['amask'], gidx=dd['gidx'],
                               az_table=tab, n=n, want_resid=True)
        o2, _, _ = ctx.velocity(dd['az'], dd['y'], dd['seg'], k=K, ridge=RIDGE, amask=dd['amask'], gidx=dd['gidx'],
                                az_table=tab, n=n)
        ctx.torch.cuda.synchronize()
        o, o2, r, p = o.cpu().numpy(), o2.cpu().numpy(), r.cpu().numpy(), p.cpu().numpy()
        assert np.array_equal(o, o2)  # the one-pass form of the grid path gives the rows of the per-cell pass
        for f, want in enumerate(rows):
            g = o[f]
            ex = np.abs(g[:2] - want[:2]).max() / max(np.abs(want[:2]).max(), 1e-3)
            ec, er = (abs(g[q] - want[q]) / want[q] if want[q] != 0 else abs(g[q]) for q in (2, 3))
            print(f'ls/{path} n {n} frame {f} (cells {seg[f + 1] - seg[f]}): x err {ex:.2e}, cost {ec:.2e}, '
                  f'rmse {er:.2e}')
            assert g[5] == want[4] and g[7] == 0.0
            assert ex <= R.XTOL and ec <= R.COST_RTOL and er <= R.COST_RTOL, (path, n, f, g, want)
            # the per-cell outputs and max |r| as test_velocity_grid_path checks them: against the residuals at the
            # kernel's own solution, within 1e-10 and 1e-12 max(1, max |r|)
            sl = slice(seg[f], max(seg[f], seg[f + 1]))
            own = d['y'][sl] - K * (g[0] * cs[sl] + g[1] * sn[sl])
            rm = np.abs(own[m[sl] > 0]).max(initial=0.0)
            assert abs(g[4] - rm) <= 1e-12 * max(1.0, rm), (path, n, f, g[4], rm)
            assert np.allclose(r[sl], own, rtol=0, atol=1e-10)
            assert np.allclose(d['y'][sl] - p[sl], own, rtol=0, atol=1e-10)
        if path == 'gidx':  # test_ls_equivalence: with every weight 1 the robust kernel's iterations are this solve
            ro, w, _ = TR.run_gpu(ctx, d, dd, n=n, loss='huber', c=1e30, scale=1.0, iters=3, tol=0.0, ridge=RIDGE)
            err = np.abs(ro[:, :2] - o[:, :2]) / np.maximum(np.abs(o[:, :2]), 1e-300)
            print(f'ls/{path} n {n}: robust at every weight 1 against LS, worst relative difference {err.max():.2e}')
            assert (err <= 1e-13).all() and (ro[:, 5] == o[:, 5]).all() and (w[:seg[-1]] == 1.0).all()


@pytest.mark.parametrize('scale', [0.05, None], ids=['fixed', 'auto'])
@pytest.mark.parametrize('loss', ['huber', 'tukey'])
@pytest.mark.parametrize('path', PATHS)
def test_robust_trip_edges(ctx, batches, path, loss, scale):
    d, dd = batches['ls', path]
    print()
    for n in clamps(d):
        ref, kw = robust_ref(d, path, n, loss, scale)
        out, w, r = TR.run_gpu(ctx, d, dd, n=n, **kw)
        R.compare(f'{path}/{loss}/{scale} n {n}', out, w, r, ref, tol=0.0)
        assert not np.isnan(w[:n]).any() and not np.isnan(r[:n]).any()  # every cell of every frame was written
        assert np.isnan(w[n:]).all()                                   # and none past n


@pytest.mark.parametrize('hyps', [256, 1024, 4096])  # the three instantiations: 1, 4, 16 per thread
@pytest.mark.parametrize('path', PATHS)
def test_consensus_trip_edges(ctx, batches, path, hyps):
    d, dd = batches['cv', path]
    print()
    for n in clamps(d):
        ref, kw = consensus_ref(d, path, n, hyps)
        out, w, r = TC.run_gpu(ctx, d, dd, n=n, **kw)
        C.compare(f'{path}/{hyps} n {n}', out, w, r, ref)
        assert not np.isnan(w[:n]).any() and not np.isnan(r[:n]).any()
        assert np.isnan(w[n:]).all()
