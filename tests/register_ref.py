"""numpy restatement of rsl_scan_register's specification (include/rsl.h), a scene builder and the case list its GPU
test runs (helper, not collected).

register() follows the header step by step, dense over all pairs and without any culling, in the dtype it is given:
np.float64 is the reference, np.longdouble the same text in the wider type.  The difference between the two is the
reference's own error, from which tests/test_gpu_register.py takes its tolerance (tol()).

window_rows() / pair_sets() restate the culling rule of the header; tests/test_register_host.py shows that the rule
removes no pair of the kernel's support on the GPU case list.
"""
import numpy as np

from rsl import tables
from rsl.chain import ChainConfig

MAX_K, MAX_ITERS = 64, 100
DEFAULTS = dict(h=0.5, h_coarse=1.0, dtheta=np.radians(0.25), K=20, iters=10, shrink=0.7, tol=1e-9, w_min=3.0, dt=0.1)
WIDE = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else None

_CFG = ChainConfig()
S_, C_ = _CFG.S, _CFG.num_chirps
AXES = tables.point_axes(_CFG, S_, C_)  # (r0, r_step, d0, d_step) of the default chain: 0.1503 m per range row


def effective_weight(points, weight):
    """The weight the specification gives every point: 0 for a non-finite x or y, or a weight that is not > 0."""
    pts = np.asarray(points, np.float32).reshape(-1, 8)
    w = np.ones(len(pts), np.float32) if weight is None else np.asarray(weight, np.float32)
    with np.errstate(invalid='ignore'):
        ok = np.isfinite(pts[:, 3]) & np.isfinite(pts[:, 4]) & (w > 0)
    return np.where(ok, w, np.float32(0)).astype(np.float64)


def _rot(th, x, y):
    c, s = np.cos(th), np.sin(th)
    return c * x - s * y, s * x + c * y


def _kernel(px, py, w, qx, qy, u, th, tx, ty, h):
    """(a [nP, nQ], d2, wu) of the pairs with positive weights at T = (th, tx, ty) and radius h."""
    mx, my = _rot(th, px, py)
    dx = (mx + tx)[:, None] - qx[None, :]
    dy = (my + ty)[:, None] - qy[None, :]
    d2 = dx * dx + dy * dy
    one = d2.dtype.type(1)
    a = np.maximum(0, one - d2 * (one / (h * h)))
    return a, d2, w[:, None] * u[None, :]


def score(P, w, Q, u, T, h, dtype=np.float64):
    """sum w u a^3 at T: the objective the fine stage ascends at a fixed h."""
    px, py, qx, qy = (np.asarray(v, dtype) for v in (P[:, 0], P[:, 1], Q[:, 0], Q[:, 1]))
    a, _, wu = _kernel(px, py, np.asarray(w, dtype), qx, qy, np.asarray(u, dtype), dtype(T[0]), dtype(T[1]),
                       dtype(T[2]), dtype(h))
    return float(np.sum(wu * a ** 3))


def register_pair(P, w, Q, u, init=(0.0, 0.0, 0.0), *, h, h_coarse, dtheta, K, iters, shrink, tol, w_min,
                  dtype=np.float64, dt=None, trace=None):
    """One frame pair.  P [nP, 2], Q [nQ, 2] (any float), w, u the effective weights.  Returns the row of 8 in dtype.
    trace: optional dict that receives 'scores' (S_k), 'T' (the pose before every step and the final one) and 'h'."""
    D = dtype
    keep_p, keep_q = np.asarray(w) > 0, np.asarray(u) > 0  # a weight of 0 adds 0 to every sum
    px, py, w = (np.asarray(v, D)[keep_p] for v in (P[:, 0], P[:, 1], w))
    qx, qy, u = (np.asarray(v, D)[keep_q] for v in (Q[:, 0], Q[:, 1], u))
    th0, tx, ty = (D(v) if np.isfinite(v) else D(0) for v in init)
    h, h_coarse, dtheta, shrink = D(h), D(h_coarse), D(dtheta), D(shrink)
    scores = np.zeros(2 * K + 1, D)
    for k in range(-K, K + 1):
        a, _, wu = _kernel(px, py, w, qx, qy, u, th0 + D(k) * dtheta, tx, ty, h_coarse)
        scores[k + K] = np.sum(wu * (a * a * a))
    if trace is not None:
        trace.update(scores=scores.copy(), T=[], h=[])
    best = int(np.argmax(scores))  # the first maximum
    if not scores[best] > 0:
        return np.array([th0, tx, ty, 0, 0, 0, 0, 1], D)
    ratio = scores[best] / np.sum(scores)
    th = th0 + D(best - K) * dtheta
    W = E = D(0)
    done, flag = 0, 0
    hcur = h_coarse
    for it in range(iters):
        hi = max(h, hcur)
        hcur = hcur * shrink
        if trace is not None:
            trace['T'].append((th, tx, ty))
            trace['h'].append(hi)
        a, d2, wu = _kernel(px, py, w, qx, qy, u, th, tx, ty, hi)
        g = wu * (a * a)
        W = np.sum(g)
        E = np.sum(g * d2)
        if not W > w_min:
            flag = 1
            break
        gp, gq = np.sum(g, axis=1), np.sum(g, axis=0)
        spx, spy, sqx, sqy = np.sum(gp * px), np.sum(gp * py), np.sum(gq * qx), np.sum(gq * qy)
        Dm = np.sum(g * (px[:, None] * qx[None, :] + py[:, None] * qy[None, :]))
        Xm = np.sum(g * (px[:, None] * qy[None, :] - py[:, None] * qx[None, :]))
        Dc = Dm - (spx * sqx + spy * sqy) / W
        Xc = Xm - (spx * sqy - spy * sqx) / W
        nth = np.arctan2(Xc, Dc)
        rx, ry = _rot(nth, spx, spy)
        ntx, nty = sqx / W - rx / W, sqy / W - ry / W
        change = max(abs(nth - th), abs(ntx - tx), abs(nty - ty))
        th, tx, ty = nth, ntx, nty
        done = it + 1
        if hi == h and change < tol:
            break
    if trace is not None:
        trace['T'].append((th, tx, ty))
    rms = np.sqrt(E / W) if W > 0 else D(0)
    return np.array([th, tx, ty, W, rms, ratio, done, flag], D)


def register(points, seg, weight=None, prev=None, init=None, dtype=np.float64, traces=None, **params):
    """rsl_scan_register on host arrays: points f32 [n, 8], seg [F + 1], weight [n] or None, prev = None or
    dict(points, weight=None, n=None), init [F, 3] or None.  Returns (rows [F, 8], omega [F, 3]) in dtype.  traces:
    optional dict that receives register_pair's trace of every frame that has a pair, by frame."""
    par = {**DEFAULTS, **params}
    dt = par.pop('dt')
    pts = np.asarray(points, np.float32).reshape(-1, 8)
    n = len(pts)
    seg = np.clip(np.asarray(seg, np.int64), 0, n)
    F = len(seg) - 1
    w = effective_weight(pts, weight)
    rows = np.zeros((F, 8), dtype)
    omega = np.zeros((F, 3), dtype)
    for f in range(F):
        b, e = int(seg[f]), max(int(seg[f]), int(seg[f + 1]))
        if f == 0:
            if prev is None or prev.get('points') is None:
                rows[0, 7] = 2
                continue
            qp = np.asarray(prev['points'], np.float32).reshape(-1, 8)
            m = len(qp) if prev.get('n') is None else min(int(prev['n']), len(qp))
            Q, u = qp[:m, 3:5], effective_weight(qp, prev.get('weight'))[:m]
        else:
            qb = min(int(seg[f - 1]), b)
            Q, u = pts[qb:b, 3:5], w[qb:b]
        i0 = (0.0, 0.0, 0.0) if init is None else tuple(np.asarray(init, np.float64)[f])
        tr = None if traces is None else traces.setdefault(f, {})
        rows[f] = register_pair(pts[b:e, 3:5], w[b:e], Q, u, i0, dtype=dtype, trace=tr, **par)
        if f > 0:
            omega[f - 1, 2] = rows[f, 0] / dtype(dt)
    return rows, omega


# ---- the culling rule of the header ---------------------------------------------------------------------------------

def window_rows(rho, h, axes=AXES):
    """(first, last) range row whose label interval r0 + r_step (i -+ 0.5) meets [rho - h, rho + h], one more row on
    each side."""
    r0, step = axes[0], axes[1]
    lo = np.ceil((rho - h - r0) / step - 0.5) - 1
    hi = np.floor((rho + h - r0) / step + 0.5) + 1
    return lo, hi


def pair_sets(P, w, Q, u, q_rc, T, h, C=C_, axes=AXES):
    """(dense, culled): the pairs (i, j) with a_ij(T, h) > 0 and positive weights, over all pairs, and over the pairs
    the row windows of the header leave."""
    px, py, qx, qy = (np.asarray(v, np.float64) for v in (P[:, 0], P[:, 1], Q[:, 0], Q[:, 1]))
    a, _, wu = _kernel(px, py, np.asarray(w, np.float64), qx, qy, np.asarray(u, np.float64), *map(np.float64, T),
                       np.float64(h))
    live = (a > 0) & (wu > 0)
    mx, my = _rot(np.float64(T[0]), px, py)
    rho = np.hypot(mx + T[1], my + T[2])
    lo, hi = window_rows(rho, h, axes)
    row = np.asarray(q_rc, np.int64) // C
    inside = (row[None, :] >= lo[:, None]) & (row[None, :] <= hi[:, None])
    return set(zip(*np.nonzero(live))), set(zip(*np.nonzero(live & inside)))


# ---- scenes ---------------------------------------------------------------------------------------------------------

def rows_from_xy(x, y, rng=None, axes=AXES, S=S_, C=C_):
    """Point rows f32 [n, 8] and rc i32 [n] of reflectors at (x, y), quantised through the label axes as the chain's
    point cloud is: the range row is the nearest label, the row's offset the remainder, x and y are formed from the
    fp32 range and azimuth; sorted by rc, as the compaction leaves a frame.  Returns (rows, rc, order)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    rng = rng or np.random.default_rng(0)
    r0, step, d0, dstep = axes
    rho, az = np.hypot(x, y), np.arctan2(y, x)
    i = np.clip(np.rint((rho - r0) / step), 0, S - 1).astype(np.int64)
    j = rng.integers(0, C, len(x))
    dr = (rho - r0) / step - i
    rows = np.zeros((len(x), 8), np.float32)
    rows[:, 0], rows[:, 1], rows[:, 2] = rho, d0 + dstep * j, az
    rows[:, 3], rows[:, 4] = rho * np.cos(az), rho * np.sin(az)
    rows[:, 5], rows[:, 6] = 0.0, dr
    rc = (i * C + j).astype(np.int32)
    order = np.argsort(rc, kind='stable')
    return rows[order], rc[order], order


def transform_world(x, y, yaw, adv):
    """Coordinates in the frame of a sensor that yawed by `yaw` and then stands `adv` = (a_x, a_y) (previous body
    frame) from where it was, of points given in the previous frame: p = R(-yaw) (q - adv)."""
    return _rot(-yaw, x - adv[0], y - adv[1])


def scene(rng, n, yaw, adv, noise=0.0, movers=0.0, clutter=0.0, mover_shift=(1.2, -0.9)):
    """Two clouds of one world seen before and after the sensor moved.  n static reflectors at 5-60 m within +-57
    degrees; the fraction `movers` of them moves rigidly by mover_shift between the frames (coherent outliers);
    `clutter` * n unmatched points are added to each cloud; position noise of `noise` metres on every coordinate.
    Returns dict(prev=(rows, rc), cur=(rows, rc), static f32 weight of the current cloud, truth=(yaw, adv_x, adv_y))."""
    rho, az = rng.uniform(5, 60, n), np.radians(rng.uniform(-57, 57, n))
    qx, qy = rho * np.cos(az), rho * np.sin(az)
    nm = int(round(movers * n))
    moved_x, moved_y = qx.copy(), qy.copy()
    moved_x[:nm] += mover_shift[0]
    moved_y[:nm] += mover_shift[1]
    px, py = transform_world(moved_x, moved_y, yaw, adv)
    static = np.ones(n, np.float32)
    static[:nm] = 0
    nc = int(round(clutter * n))

    def with_clutter(x, y, s):
        rho, az = rng.uniform(5, 60, nc), np.radians(rng.uniform(-57, 57, nc))
        x = np.concatenate([x, rho * np.cos(az)]) + noise * rng.standard_normal(len(x) + nc)
        y = np.concatenate([y, rho * np.sin(az)]) + noise * rng.standard_normal(len(y) + nc)
        return x, y, np.concatenate([s, np.ones(nc, np.float32)])
    qx, qy, sq = with_clutter(qx, qy, static)
    px, py, sp = with_clutter(px, py, static)
    qrows, qrc, qo = rows_from_xy(qx, qy, rng)
    prows, prc, po = rows_from_xy(px, py, rng)
    return dict(prev=(qrows, qrc), cur=(prows, prc), static=sp[po], static_prev=sq[qo],
                truth=(float(yaw), float(adv[0]), float(adv[1])))


# ---- the GPU test's case list ---------------------------------------------------------------------------------------

GPU_SIZES = (40, 0, 300, 700)  # the empty frame in the middle; 700 is longer than one pass of 256 threads x 2
_case = None


def gpu_case():
    """The inputs of tests/test_gpu_register.py, built once: F = 4 frames of 40, 0, 300 and 700 points, and a previous
    cloud of 60.  Frame 0 is the previous cloud after yaw +1.5 deg, advance (0.30, 0.05); frame 1 is empty, so frame 2
    meets an empty reference; frame 3 shares 300 reflectors with frame 2 (yaw -2.0 deg, advance (0.40, -0.10), 0.02 m
    noise) and carries 400 unmatched points.  One point of frame 3 is NaN, ten have weight 0 or below.  Returns
    dict(points f32 [1040, 8], rc i32, seg i64 [5], weight f32, prev=dict(points, rc, weight), init f64 [4, 3],
    truth)."""
    global _case
    if _case is not None:
        return _case
    rng = np.random.default_rng(31017)
    a = scene(rng, 40, np.radians(1.5), (0.30, 0.05), noise=0.0, clutter=0.5)      # prev 60, frame 0: 60 -> cut to 40
    q0, q0rc = a['prev']
    f0, f0rc = a['cur'][0][:40], a['cur'][1][:40]
    b = scene(rng, 300, np.radians(-2.0), (0.40, -0.10), noise=0.02)
    f2, f2rc = b['prev']
    extra = scene(rng, 400, 0.0, (0.0, 0.0))['cur']
    x = np.concatenate([b['cur'][0][:, 3], extra[0][:, 3]]).astype(np.float64)
    y = np.concatenate([b['cur'][0][:, 4], extra[0][:, 4]]).astype(np.float64)
    f3, f3rc, _ = rows_from_xy(x, y, rng)
    points = np.concatenate([f0, f2, f3]).astype(np.float32)
    rc = np.concatenate([f0rc, f2rc, f3rc]).astype(np.int32)
    seg = np.cumsum([0, 40, 0, 300, 700]).astype(np.int64)
    weight = rng.uniform(0.5, 2.0, len(points)).astype(np.float32)
    bad = seg[3] + rng.permutation(700)[:11]
    weight[bad[:5]] = 0.0
    weight[bad[5:10]] = -1.0
    points[bad[10], 3] = np.nan
    prev_w = rng.uniform(0.5, 2.0, len(q0)).astype(np.float32)
    init = np.zeros((4, 3))
    init[0] = (0.0, 0.25, 0.0)      # a start translation 0.07 m off
    init[3] = (0.0, 0.30, 0.0)      # 0.14 m off
    _case = dict(points=points, rc=rc, seg=seg, weight=weight, prev=dict(points=q0, rc=q0rc, weight=prev_w),
                 init=init, truth={0: a['truth'], 3: b['truth']})
    return _case


def tol(pairs):
    """(tolerance [5], spread [5]) from [(rows64, rowsWide), ...], per column of theta, t_x, t_y, W and rms: 100 x the
    largest |fp64 - long double| difference of the reference on these very cases, with a floor of 1e-12."""
    assert WIDE is not None, 'no extended long double on this platform: the reference has nothing to measure itself by'
    spread = np.zeros(5)
    for a, b in pairs:
        spread = np.maximum(spread, np.max(np.abs(a[:, :5].astype(WIDE) - b[:, :5]), axis=0).astype(np.float64))
    return np.maximum(100.0 * spread, 1e-12), spread
