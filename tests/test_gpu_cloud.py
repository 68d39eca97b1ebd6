"""One hostile point cloud read by both consumers (rsl_scan_register, rsl_map_update): the rows a frame owns and the
points that count are one rule (include/rsl.h, "The point cloud"), so the two kernels and their two independent numpy
restatements (tests/register_ref.py, tests/map_ref.py) must read the cloud the same way.

The cloud (built once on the host, fixed seed): F = 4 frames of 60, 0, 65 and 65 rows inside a 15 m square, frame 3
being frame 2's reflectors seen after a yaw of 1 degree and an advance of (0.25, -0.05) m.  seg = {-7, 60, 50, 115,
n + 1000}: a negative first entry, a descending pair (frame 1 is empty, frame 2 starts inside frame 0's rows) and a last
entry 1000 past n.  In every frame that has rows: one x = NaN, one y = +inf, and weights 0, -1 and NaN.  The map is
64 x 64 cells of 0.5 m with r_min = 0, r_max = 15 and min_db = -inf, and every pose keeps the whole square inside the map
and inside the window, so the acceptance rule alone decides what the map counts.
"""
import math

import numpy as np
import pytest

import map_ref as M
import register_ref as R
from test_gpu_register import refs, tols  # noqa: F401  (fixtures: the tolerances of the registration test)

pytestmark = pytest.mark.gpu

GRID, SHAPE = (0.0, 0.0, 0.5), (64, 64)
MAP = dict(r_min=0.0, r_max=15.0, min_db=-np.inf)
TRUTH = (math.radians(1.0), 0.25, -0.05)


def build_case():
    rng = np.random.default_rng(4242)
    x, y = rng.uniform(1.0, 11.0, 115), rng.uniform(-7.0, 7.0, 115)  # frame 0: rows [0, 60), frame 2: rows [50, 115)
    x3, y3 = R.transform_world(x[50:], y[50:], TRUTH[0], TRUTH[1:])  # frame 3: rows [115, 180)
    n = 180
    pts = np.zeros((n, 8), np.float32)
    pts[:, 3], pts[:, 4] = np.concatenate([x, x3]), np.concatenate([y, y3])
    pts[:, 5] = rng.uniform(-30.0, 10.0, n)
    seg = np.array([-7, 60, 50, 115, n + 1000], np.int64)
    weight = rng.uniform(0.5, 2.0, n).astype(np.float32)
    for b, e in ((0, 50), (60, 115), (115, n)):  # rows that frame 0, frame 2 and frame 3 do not share
        i = b + rng.permutation(e - b)[:5]
        pts[i[0], 3], pts[i[1], 4] = np.nan, np.inf
        weight[i[2]], weight[i[3]], weight[i[4]] = 0.0, -1.0, np.nan
    poses = np.array([M.yaw_pose(10.0 + 0.3 * f, 16.0 - 0.2 * f, 0.05 * f - 0.1, z=1.0) for f in range(4)])
    return dict(points=pts, seg=seg, weight=weight, poses=poses, n=n)


@pytest.fixture(scope='module')
def case():
    """The cloud and both references, computed once and left unchanged; before any device call the two references
    agree on what counts: per frame, the rows register_ref weighs above 0 are the points map_ref accepts."""
    c = build_case()
    c['map'] = M.map_update(c['points'], c['seg'], c['poses'], GRID, SHAPE, weight=c['weight'], **MAP)
    c['rows'], c['omega'] = R.register(c['points'], c['seg'], weight=c['weight'])
    w = R.effective_weight(c['points'], c['weight'])
    seg = np.clip(c['seg'], 0, c['n'])
    counted = [int((w[b:max(b, e)] > 0).sum()) for b, e in zip(seg[:-1], seg[1:])]
    assert counted == c['map'][2][:, 0].tolist() == [55, 0, 60, 60], (counted, c['map'][2])
    assert not c['map'][2][:, 3].any()
    return c


def test_both_consumers_read_one_hostile_cloud(ctx, case, tols):
    torch = ctx.torch
    pts, seg, w = (ctx.to_dev(case[k]) for k in ('points', 'seg', 'weight'))
    hits, free = (torch.zeros(SHAPE, dtype=torch.int32, device=ctx.device) for _ in range(2))
    st = ctx.map_update(pts, seg, ctx.to_dev(case['poses']), hits, grid=GRID, free=free, weight=w, **MAP)
    rh, rf, rs = case['map']
    assert np.array_equal(st.cpu().numpy(), rs)
    assert np.array_equal(hits.cpu().numpy().view(np.uint32), rh)
    assert np.array_equal(free.cpu().numpy().view(np.uint32), rf)

    rows, om = ctx.scan_register(pts, seg, weight=w)
    rows, want = rows.cpu().numpy(), case['rows']
    tol, _ = tols
    err = np.abs(rows[:, :5] - want[:, :5]).max(axis=0)
    print(f'device error {err}, tolerance {tol}')
    # no previous cloud; the empty frame; its successor, which meets an empty reference; one real pair
    assert want[:, 7].tolist() == [2, 1, 1, 0] and np.array_equal(rows[:, 7], want[:, 7])
    assert np.array_equal(rows[:, 6], want[:, 6]) and want[3, 6] > 0
    assert (err <= tol).all(), (err, tol)
    assert (np.abs(rows[:, 5] - want[:, 5]) <= 1e-9).all()
    assert (np.abs(om.cpu().numpy() - case['omega']) <= tol[0] / R.DEFAULTS['dt']).all()
    assert abs(want[3, 0] - TRUTH[0]) < math.radians(0.03) and np.abs(want[3, 1:3] - TRUTH[1:]).max() < 0.02
