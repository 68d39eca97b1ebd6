"""numpy fp64 restatement of rsl_map_update and rsl_map_logodds (the comments in include/rsl.h are the specification).
It follows the comment, not the kernel: sets of cells, no bitmaps, no window.  Every product and sum is one numpy
operation, so each is rounded once, as the device does with contraction off: the planes are compared exactly.

Also the case builders of tests/test_map_host.py and tests/test_gpu_map.py."""
import math

import numpy as np

MAX_RW = 383


def ray_cells(ddx: int, ddy: int):
    """The cells, relative to the origin cell, of the ray to the cell at offset (ddx, ddy): L = max(|ddx|, |ddy|) cells
    from (0, 0) up to, not including, (ddx, ddy)."""
    dx, dy = abs(ddx), abs(ddy)
    sx, sy = (1 if ddx >= 0 else -1), (1 if ddy >= 0 else -1)
    k = np.arange(max(dx, dy), dtype=np.int64)
    if dx == 0 and dy == 0:
        return k, k
    if dx >= dy:
        return sx * k, sy * ((2 * k * dy + dx) // (2 * dx))
    return sx * ((2 * k * dx + dy) // (2 * dy)), sy * k


def half_window(cell: float, r_max: float) -> int:
    return int(math.ceil(r_max * (1.0 / cell))) + 1


def frame_pose(pose, x0, y0, inv):
    """(valid, (r00, r01, r10, r11, p_x, p_y), (ox, oy)) of one pose row."""
    with np.errstate(all='ignore'):
        px, py, _, qw, qx, qy, qz = (np.float64(v) for v in pose)
        r00 = 1.0 - 2.0 * (qy * qy + qz * qz)
        r01 = 2.0 * (qx * qy - qw * qz)
        r10 = 2.0 * (qx * qy + qw * qz)
        r11 = 1.0 - 2.0 * (qx * qx + qz * qz)
        gx, gy = (px - x0) * inv, (py - y0) * inv
        ok = all(np.isfinite(v) for v in (px, py, r00, r01, r10, r11)) and abs(gx) < 2.0 ** 30 and abs(gy) < 2.0 ** 30
    if not ok:
        return False, None, None
    return True, (r00, r01, r10, r11, px, py), (int(np.floor(gx)), int(np.floor(gy)))


def map_update(points, seg, poses, grid, shape, *, r_min, r_max, min_db=-np.inf, weight=None, n=None, hits=None,
               free=None, want_free=True):
    """One rsl_map_update call.  grid = (x0, y0, cell), shape = (ny, nx).  hits / free: planes to add to (copied).
    Returns (hits u32 [ny, nx], free u32 [ny, nx] or None, stats i32 [F, 4])."""
    ny, nx = shape
    x0, y0, cell = (np.float64(v) for v in grid[:3])
    inv = np.float64(1.0) / cell
    Rw = half_window(float(cell), r_max)
    assert Rw <= MAX_RW
    rmin2, rmax2 = np.float64(r_min) * np.float64(r_min), np.float64(r_max) * np.float64(r_max)
    pts = np.asarray(points, np.float32).reshape(-1, 8)
    n = len(pts) if n is None else min(int(n), len(pts))
    seg = np.asarray(seg, np.int64)
    F = len(seg) - 1
    hits = np.zeros((ny, nx), np.uint32) if hits is None else np.array(hits, np.uint32)
    if want_free:
        free = np.zeros((ny, nx), np.uint32) if free is None else np.array(free, np.uint32)
    else:
        free = None
    stats = np.zeros((F, 4), np.int32)
    for f in range(F):
        ok, rot, org = frame_pose(np.asarray(poses, np.float64)[f], x0, y0, inv)
        if not ok:
            stats[f] = (0, 0, 0, 1)
            continue
        r00, r01, r10, r11, px, py = rot
        ox, oy = org
        b, e = min(max(int(seg[f]), 0), n), min(max(int(seg[f + 1]), 0), n)
        p = pts[b:e] if e > b else pts[:0]
        with np.errstate(all='ignore'):
            x, y = p[:, 3].astype(np.float64), p[:, 4].astype(np.float64)
            acc = np.isfinite(x) & np.isfinite(y)
            if weight is not None:
                acc &= np.asarray(weight, np.float32)[b:b + len(p)] > 0
            acc &= ~(p[:, 5].astype(np.float64) < min_db)
            r2 = x * x + y * y
            acc &= (rmin2 <= r2) & (r2 <= rmax2)
            X, Y = (r00 * x + r01 * y) + px, (r10 * x + r11 * y) + py
            hx, hy = np.floor((X - x0) * inv), np.floor((Y - y0) * inv)
            acc &= (0 <= hx) & (hx < nx) & (0 <= hy) & (hy < ny)
            acc &= (np.abs(hx - ox) <= Rw) & (np.abs(hy - oy) <= Rw)
        H = set(zip(hx[acc].astype(np.int64).tolist(), hy[acc].astype(np.int64).tolist()))
        Fr = set()
        if want_free:
            for cx, cy in H:
                rx, ry = ray_cells(cx - ox, cy - oy)
                rx, ry = rx + ox, ry + oy
                m = (rx >= 0) & (rx < nx) & (ry >= 0) & (ry < ny)
                Fr.update(zip(rx[m].tolist(), ry[m].tolist()))
            Fr -= H
            for cx, cy in Fr:
                free[cy, cx] += 1
        for cx, cy in H:
            hits[cy, cx] += 1
        stats[f] = (int(acc.sum()), len(H), len(Fr), 0)
    return hits, free, stats


def map_logodds(hits, free, l_occ=0.85, l_free=0.4, l_min=-4.0, l_max=4.0):
    v = np.asarray(hits, np.uint32).astype(np.float64) * np.float64(l_occ)
    if free is not None:
        v = v - np.asarray(free, np.uint32).astype(np.float64) * np.float64(l_free)
    return np.clip(v, l_min, l_max).astype(np.float32)


def yaw_pose(x, y, yaw, z=0.0):
    return [x, y, z, math.cos(0.5 * yaw), 0.0, 0.0, math.sin(0.5 * yaw)]


# ---- the scene of tests/test_map_host.py -------------------------------------------------------------------------

def scene(cell=0.25, seed=7):
    """Two walls and 30 poles as reflector positions (world), sampled densely enough that every cell a wall crosses
    holds a reflector.  Returns (reflectors [M, 2], the set of occupied cells for the grid origin (0, 0))."""
    rng = np.random.default_rng(seed)
    s = np.arange(0.0, 55.0, cell / 2) + cell / 4
    t = np.arange(0.0, 55.5, cell / 2) + cell / 4
    wall_a = np.stack([5.0 + s, np.full_like(s, 30.0 + cell / 2)], 1)        # 220 cells along x at y = 30
    wall_b = np.stack([np.full_like(t, 60.0 + cell / 2), -25.5 + t], 1)      # 222 cells along y at x = 60
    poles = np.stack([rng.uniform(5.0, 55.0, 30), rng.uniform(-15.0, 25.0, 30)], 1)
    poles = (np.floor(poles / cell) + 0.5) * cell                            # a pole sits in the middle of its cell
    refl = np.concatenate([wall_a, wall_b, poles])
    return refl, set(map(tuple, np.floor(refl / cell).astype(np.int64).tolist()))


def scene_frames(refl, *, frames=40, speed=5.0, dt=0.1, yaw_end=math.radians(12.0), noise=0.03,
                 half_fov=math.radians(60.0), r_max=75.0, mover=True, seed=11):
    """The clouds of a sensor that drives along +x from (0, 0) with the yaw going 0 -> yaw_end: every reflector inside
    the field of view and r_max, in sensor coordinates with Gaussian noise, and one mover that crosses the scene
    (last point of every frame, labelled 1 in `moving`).  Returns (points f32 [N, 8], seg, poses f64 [F, 7],
    moving bool [N])."""
    rng = np.random.default_rng(seed)
    rows, seg, poses, moving = [], [0], [], []
    for f in range(frames):
        yaw = yaw_end * f / (frames - 1)
        p = np.array([speed * dt * f, 0.0])
        poses.append(yaw_pose(p[0], p[1], yaw))
        world = refl
        if mover:
            world = np.concatenate([refl, [[30.0 + 0.8 * f, -20.0 - 0.3 * f]]])  # nothing stands behind its path
        d = world - p
        c, s = math.cos(yaw), math.sin(yaw)
        loc = np.stack([c * d[:, 0] + s * d[:, 1], -s * d[:, 0] + c * d[:, 1]], 1)  # R(yaw)^T d
        rng_ = np.hypot(loc[:, 0], loc[:, 1])
        vis = (np.abs(np.arctan2(loc[:, 1], loc[:, 0])) <= half_fov) & (rng_ <= r_max - 1.0) & (rng_ >= 1.0)
        mv = np.zeros(len(world), bool)
        if mover:
            mv[-1] = True
        loc = loc[vis] + rng.normal(0.0, noise, (int(vis.sum()), 2))
        row = np.zeros((len(loc), 8), np.float32)
        row[:, 3:5] = loc
        rows.append(row)
        moving.append(mv[vis])
        seg.append(seg[-1] + len(loc))
    return np.concatenate(rows), np.array(seg, np.int64), np.array(poses, np.float64), np.concatenate(moving)


# ---- the case of tests/test_gpu_map.py ---------------------------------------------------------------------------

GPU_CASE = dict(ny=80, nx=96, cell=0.5, r_max=20.0, r_min=0.5, min_db=-20.0, origin=(-4.0, -3.0))


def gpu_case(seed=3):
    """F = 6 frames of 40, 0, 300, 700, 3 and 50 points on an 80 x 96 map of 0.5 m cells, r_max 20 m (Rw = 41, window
    83 wide: neither 83 nor 83^2 is a multiple of 32); the last segment's end lies 1000 past the arrays.  Yaws in all
    four quadrants, one pose outside the map, one pose with a NaN; planted points for every rule of the
    specification.  Asserts that each of them occurs.  Returns dict(points, seg, poses, weight, n, grid, shape, params)."""
    g = GPU_CASE
    rng = np.random.default_rng(seed)
    x0, y0 = g['origin']
    cell, nx, ny = g['cell'], g['nx'], g['ny']
    counts = [40, 0, 300, 700, 3, 50]
    yaws = [math.radians(a) for a in (20.0, 0.0, 110.0, -160.0, 0.0, -70.0)]
    centres = [(10.0, 8.0), (20.0, 20.0), (22.25, 17.25), (30.0, 25.0), (5.0, 5.0), (-9.0, 12.0)]  # frame 5: outside
    poses = np.array([yaw_pose(cx, cy, a, z=1.5) for (cx, cy), a in zip(centres, yaws)], np.float64)
    poses[4, 4] = np.nan
    rows, weight = [], []
    for f, cnt in enumerate(counts):
        r = rng.uniform(0.0, 24.0, cnt)  # some below r_min, some beyond r_max
        a = rng.uniform(-math.pi, math.pi, cnt)
        p = np.zeros((cnt, 8), np.float32)
        p[:, 3], p[:, 4] = r * np.cos(a), r * np.sin(a)
        p[:, 5] = rng.uniform(-30.0, 10.0, cnt)  # a quarter below min_db
        w = np.ones(cnt, np.float32)
        w[rng.random(cnt) < 0.1] = 0.0
        rows.append(p)
        weight.append(w)
    # planted points of frame 3 (yaw -160 deg, origin (30, 25) = the corner of cell (68, 56)) and frame 2
    def local(f, wx, wy):  # the sensor coordinates of a world point
        cx, cy = centres[f]
        c, s = math.cos(yaws[f]), math.sin(yaws[f])
        d0, d1 = wx - cx, wy - cy
        return c * d0 + s * d1, -s * d0 + c * d1
    p3, w3 = rows[3], weight[3]
    plant = [(30.4, 25.4),                # the origin cell, 0.57 m away: L = 0
             (36.2, 25.2), (30.2, 31.2), (34.2, 29.2), (26.2, 29.2),   # horizontal, vertical, both diagonals
             (x0 + 47.75, 30.0), (31.0, y0 + 39.75),                   # last column, last row
             (34.2, 29.2), (34.3, 29.3)]                               # several points in one cell
    for i, (wx, wy) in enumerate(plant):
        p3[i, 3], p3[i, 4] = local(3, wx, wy)
        p3[i, 5], w3[i] = 0.0, 1.0
    p3[20, 3] = np.nan
    p3[21, 4] = np.inf
    w3[22], w3[23], w3[24] = 0.0, -1.0, np.nan
    for i in (22, 23, 24, 25):  # otherwise acceptable points: only the weight or the power rejects them
        p3[i, 3], p3[i, 4] = local(3, 33.0 + i * 0.1, 27.0)
        p3[i, 5] = 0.0
    p3[25, 5], w3[25] = -25.0, 1.0
    p0, w0 = rows[0], weight[0]
    for i, (wx, wy) in enumerate([(x0 + 0.25, 8.0), (10.0, y0 + 0.25)]):  # column 0, row 0
        p0[i, 3], p0[i, 4] = local(0, wx, wy)
        p0[i, 5], w0[i] = 0.0, 1.0
    # frame 0 at (10, 8), 14 m from the map's left edge: its far points fall outside the map; frame 5 stands outside
    points, weight = np.concatenate(rows), np.concatenate(weight)
    seg = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    n = len(points)
    seg[-1] = n + 1000
    case = dict(points=points, seg=seg, poses=poses, weight=weight, n=n, grid=(x0, y0, cell), shape=(ny, nx),
                params=dict(r_min=g['r_min'], r_max=g['r_max'], min_db=g['min_db']))
    _check_gpu_case(case, centres, yaws)
    return case


def _check_gpu_case(case, centres, yaws):
    """Every situation the issue lists occurs in the case."""
    pts, seg, n = case['points'], case['seg'], case['n']
    x0, y0, cell = case['grid']
    ny, nx = case['shape']
    par = case['params']
    Rw = half_window(cell, par['r_max'])
    assert Rw == 41 and (2 * Rw + 1) % 32 and (2 * Rw + 1) ** 2 % 32
    hits, free, stats = map_update(pts, seg, case['poses'], case['grid'], case['shape'], weight=case['weight'], n=n, **par)
    assert stats[4].tolist() == [0, 0, 0, 1] and stats[1].tolist() == [0, 0, 0, 0]
    assert (stats[[0, 2, 3, 5], 1] > 0).all() and (stats[[0, 2, 3, 5], 3] == 0).all()
    assert (stats[:, 0] > stats[:, 1])[[2, 3]].all()                                  # several points in one cell
    assert hits[0].any() and hits[-1].any() and hits[:, 0].any() and hits[:, -1].any()  # rows, columns 0 and N - 1
    inv = 1.0 / cell
    seen = dict(out=0, far=0, near=0, nan=0, w0=0, wneg=0, wnan=0, db=0, L0=0, hor=0, ver=0, diag=0, col0=0, octants=set(),
                clipped=0)
    for f in range(len(seg) - 1):
        ok, rot, org = frame_pose(case['poses'][f], x0, y0, inv)
        if not ok:
            continue
        r00, r01, r10, r11, px, py = rot
        ox, oy = org
        if not (0 <= ox < nx and 0 <= oy < ny):
            seen['clipped'] += int(stats[f, 1] > 0)   # a hit from a sensor outside the map: its ray leaves the map
        for i in range(int(seg[f]), min(int(seg[f + 1]), n)):
            x, y, db, w = float(pts[i, 3]), float(pts[i, 4]), float(pts[i, 5]), case['weight'][i]
            if not (np.isfinite(x) and np.isfinite(y)):
                seen['nan'] += 1
                continue
            seen['w0'] += int(w == 0)
            seen['wneg'] += int(w < 0)
            seen['wnan'] += int(np.isnan(w))
            seen['db'] += int(db < par['min_db'])
            r2 = x * x + y * y
            seen['far'] += int(r2 > par['r_max'] ** 2)
            seen['near'] += int(r2 < par['r_min'] ** 2)
            if not (w > 0) or db < par['min_db'] or not (par['r_min'] ** 2 <= r2 <= par['r_max'] ** 2):
                continue
            hx = math.floor(((r00 * x + r01 * y) + px - x0) * inv)
            hy = math.floor(((r10 * x + r11 * y) + py - y0) * inv)
            if not (0 <= hx < nx and 0 <= hy < ny):
                seen['out'] += 1
                continue
            seen['col0'] += int(hx == 0)
            ddx, ddy = hx - ox, hy - oy
            if max(abs(ddx), abs(ddy)) > Rw:
                continue
            seen['L0'] += int(ddx == 0 and ddy == 0)
            seen['hor'] += int(ddy == 0 and ddx != 0)
            seen['ver'] += int(ddx == 0 and ddy != 0)
            seen['diag'] += int(abs(ddx) == abs(ddy) and ddx != 0)
            if ddx and ddy and abs(ddx) != abs(ddy):
                seen['octants'].add((ddx > 0, ddy > 0, abs(ddx) > abs(ddy)))
    assert len(seen.pop('octants')) == 8, 'every octant'
    assert all(v > 0 for v in seen.values()), seen
