"""CPU: the grid map's specification (include/rsl.h, rsl_map_update / rsl_map_logodds) on its fp64 restatement
tests/map_ref.py, and the host-side argument checks of rsl.mapping.GridMap and rsl.ops.grid_map (no device needed).

The ray formula over all end points in [-20, 20]^2: L = max(|dx|, |dy|) cells, distinct, 8-connected, starting at the
origin cell, the next step being the hit cell.

The scene (map_ref.scene / scene_frames): two walls and 30 poles, 472 occupied cells of 0.25 m; 40 frames at 5 m/s with
the yaw going 0 -> 12 degrees, 0.03 m noise, a 60 degree half field of view, one mover that crosses where nothing stands
behind it.  Measured on the reference when this test was written:
  true poses, mover at weight 0:  every cell with >= 5 hits (418) lies within one cell of a true reflector; 423 of the
                                  472 true cells have positive log-odds; no cell with positive log-odds lies elsewhere;
  mover at weight 1:              40 cells with positive log-odds lie elsewhere (the trail), the rest unchanged;
  yaw ignored (identity quaternions): 164 of 727 cells with >= 5 hits are near the truth, 288 true cells have positive
                                  log-odds and 1055 cells with positive log-odds lie elsewhere.
The bounds asserted: none false with the true poses; a trail of at least 20 cells only at weight 1; at least 400 true
cells found; with the yaw ignored under half of the >= 5-hit cells near the truth and over 500 false cells."""
import math

import numpy as np
import pytest

import map_ref as M


def test_ray_formula_all_end_points():
    for ddx in range(-20, 21):
        for ddy in range(-20, 21):
            rx, ry = M.ray_cells(ddx, ddy)
            L = max(abs(ddx), abs(ddy))
            assert len(rx) == len(ry) == L
            if L == 0:
                continue
            cells = list(zip(rx.tolist(), ry.tolist()))
            assert cells[0] == (0, 0)
            assert len(set(cells)) == L and (ddx, ddy) not in cells
            path = cells + [(ddx, ddy)]
            for (ax, ay), (bx, by) in zip(path[:-1], path[1:]):
                assert max(abs(bx - ax), abs(by - ay)) == 1, (ddx, ddy, path)


CELL, GRID, SHAPE = 0.25, (-10.0, -40.0, 0.25), (360, 400)


@pytest.fixture(scope='module')
def world():
    refl, occ = M.scene(CELL)
    truth = np.zeros(SHAPE, bool)
    for cx, cy in occ:
        truth[cy - int(GRID[1] / CELL), cx - int(GRID[0] / CELL)] = True
    ys, xs = np.nonzero(truth)
    near = np.zeros(SHAPE, bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near[ys + dy, xs + dx] = True
    pts, seg, poses, moving = M.scene_frames(refl)
    return dict(truth=truth, near=near, pts=pts, seg=seg, poses=poses, moving=moving)


def figures(w, weight, poses):
    hits, free, stats = M.map_update(w['pts'], w['seg'], poses, GRID, SHAPE, r_min=0.5, r_max=75.0, weight=weight)
    lo = M.map_logodds(hits, free)
    assert not stats[:, 3].any()
    h5 = hits >= 5
    out = dict(h5=int(h5.sum()), h5_near=int((h5 & w['near']).sum()), found=int((w['truth'] & (lo > 0)).sum()),
               elsewhere=int(((lo > 0) & ~w['near']).sum()))
    print(out)
    return out


def test_scene_true_poses_no_false_cells(world):
    assert int(world['truth'].sum()) == 472 and int(world['moving'].sum()) == 40
    fig = figures(world, (~world['moving']).astype(np.float32), world['poses'])
    assert fig['h5'] >= 400 and fig['h5_near'] == fig['h5']
    assert fig['found'] >= 400
    assert fig['elsewhere'] == 0


def test_scene_mover_leaves_a_trail_only_at_weight_one(world):
    fig = figures(world, np.ones(len(world['pts']), np.float32), world['poses'])
    assert fig['h5_near'] == fig['h5'] and fig['found'] >= 400
    assert 20 <= fig['elsewhere'] <= 40  # at most one cell per frame


def test_scene_collapses_without_the_yaw(world):
    poses = world['poses'].copy()
    poses[:, 3:] = (1.0, 0.0, 0.0, 0.0)
    fig = figures(world, (~world['moving']).astype(np.float32), poses)
    assert fig['h5_near'] < 0.5 * fig['h5']
    assert fig['elsewhere'] > 500


def test_counts_do_not_depend_on_order_or_split(world):
    """Integer adds commute: reversed frames, and two halves added, give the planes of one call."""
    w = world
    F = 8
    seg, poses = w['seg'][:F + 1], w['poses'][:F]
    par = dict(r_min=0.5, r_max=75.0)
    h, f, _ = M.map_update(w['pts'], seg, poses, GRID, SHAPE, **par)
    order = np.arange(F)[::-1]
    rows = np.concatenate([w['pts'][seg[i]:seg[i + 1]] for i in order])
    rseg = np.concatenate([[0], np.cumsum([seg[i + 1] - seg[i] for i in order])])
    h2, f2, _ = M.map_update(rows, rseg, poses[order], GRID, SHAPE, **par)
    assert np.array_equal(h, h2) and np.array_equal(f, f2)
    ha, fa, _ = M.map_update(w['pts'], seg[:5], poses[:4], GRID, SHAPE, **par)
    hb, fb, _ = M.map_update(w['pts'], seg[4:], poses[4:], GRID, SHAPE, hits=ha, free=fa, **par)
    assert np.array_equal(h, hb) and np.array_equal(f, fb)
    assert h.max() <= F and f.max() <= F and not ((h + f) > F).any()  # per scan at most one count per cell


def test_gpu_case_builder():
    case = M.gpu_case()  # asserts that every planted situation occurs
    assert np.diff(case['seg'])[:5].tolist() == [40, 0, 300, 700, 3] and case['seg'][-1] == case['n'] + 1000


GOOD = dict(origin=(0.0, 0.0), shape=(64, 64))
BAD = [dict(cell=0.0), dict(cell=-1.0), dict(cell=math.nan), dict(cell=math.inf), dict(origin=(math.nan, 0.0)),
       dict(origin=(0.0, math.inf)), dict(r_min=-0.1), dict(r_min=math.nan), dict(r_max=math.inf), dict(r_max=math.nan),
       dict(r_min=2.0, r_max=1.0), dict(min_db=math.nan), dict(min_db=math.inf), dict(shape=(0, 64)), dict(shape=(64, -1)),
       dict(shape=(65536, 32768)), dict(cell=0.1, r_max=75.0), dict(l_occ=math.nan), dict(l_free=math.inf),
       dict(l_min=1.0, l_max=-1.0), dict(origin=0.0), dict(shape=64)]


@pytest.mark.parametrize('bad', BAD, ids=[','.join(f'{k}={v}' for k, v in b.items()) for b in BAD])
def test_gridmap_checks_arguments_on_the_host(bad):
    """The conditions of the C function, as ValueError, before any device use (the context is never touched)."""
    from rsl.mapping import GridMap
    from rsl import ops
    with pytest.raises(ValueError):
        GridMap(None, **{**GOOD, **bad})
    pts, seg, poses = np.zeros((4, 8), np.float32), np.array([0, 4]), np.array([M.yaw_pose(1.0, 1.0, 0.0)])
    with pytest.raises(ValueError):
        ops.grid_map(pts, seg, poses, **{**GOOD, **bad})


def test_grid_map_checks_array_shapes_on_the_host():
    from rsl import ops
    from rsl.mapping import check_params
    pts, seg, poses = np.zeros((4, 8), np.float32), np.array([0, 4]), np.array([M.yaw_pose(1.0, 1.0, 0.0)])
    for p, s, q in ((pts[:, :7], seg, poses), (pts, seg, poses[:, :6]), (pts, np.array([0, 2, 4]), poses),
                    (pts, seg.reshape(1, 2), poses)):
        with pytest.raises(ValueError):
            ops.grid_map(p, s, q, **GOOD)
    p = check_params(**GOOD, cell=0.25, r_max=77.0)
    assert p['rw'] == 309 == M.half_window(0.25, 77.0) and p['min_db'] == -math.inf
    assert check_params(**GOOD, cell=0.25, r_max=95.5)['rw'] == 383  # the limit itself is accepted
