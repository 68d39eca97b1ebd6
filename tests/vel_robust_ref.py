"""numpy fp64 oracle of the robust velocity solve (rsl_velocity_robust; the estimator is the doc comment in
include/rsl.h), a generator of planted two-population frames, and the comparator the GPU tests share.  Not collected.

Tolerances, and where they come from:

XTOL = 1e-9, relative to max(|x|_inf, 1e-3), for fixed-iteration (tol = 0) runs.  The device and this oracle sum the
    same weighted moments in different orders: each moment carries a relative rounding error of at most N * 2^-53
    (2e-12 at N = 2e4).  The solution of the 2x2 system amplifies it by at most the condition number of the weighted
    normal matrix k^2 M + ridge I of the last solve, which is <= 1e2 (COND_MAX) for the generator's azimuth spread
    (short segments: for the ridge the tests use); every reference run records that number and the comparator asserts
    the bound.  It is the last solve that counts: the first Tukey iteration from a contaminated LS start keeps only a
    narrow band of azimuths and its matrix reaches 1e2 .. 1e3, but an error made in iteration j reaches the result
    multiplied by the contraction rate (0.2 .. 0.7 here) once per remaining iteration.  The iteration itself is well
    conditioned: perturbing y by 1e-13 moved x by less than 2e-15 in the prototype.  2e-10 in all; 1e-9 leaves a
    factor 5.
SIGMA_RTOL = 1e-6: the estimated scale is 1.4826 x one fp32 value selected exactly; a residual that rounds to the
    neighbouring fp32 value moves it by 2^-23 = 1.2e-7 relative.
COST_RTOL = 1e-8 on cost and rmse_w: sums of N non-negative terms (N * 2^-53) at an x within XTOL; the terms are
    stationary in x at the fixed point to first order, and rho changes by at most 2 |r| k dx per cell otherwise.
W_ATOL = 1e-5 on the weights: f32 storage (6e-8) plus |du/dr| k dx <= (2 / t) * 322.5 * 4e-12.
n_in may differ by at most the multiplicity of the cells with ||r| - t| <= NEAR_RTOL * t, and at most NEAR_MAX of
    those may exist per frame (asserted on the oracle alone: the generator's seeds are chosen for it).
Early-stop runs (tol > 0): |it| within 1 of the oracle's and x within 10 * tol + XTOL * scale: an iteration that stops
    at step <= tol is within tol * rate / (1 - rate) of the fixed point, 9 tol at a contraction rate of 0.9, and the
    comparator asserts on the oracle alone that the ratio of its last two steps is below 0.9.
"""
import numpy as np

K_CHAIN = 4 * np.pi * 0.1 / (3e8 / 77e9)  # the chain's k = 4 pi dt / lambda = 322.5
BOX = (-50.0, 50.0, -50.0, 50.0)
LOSS_HUBER, LOSS_TUKEY = 1, 2
LOSS_ID = {'huber': LOSS_HUBER, 'tukey': LOSS_TUKEY, LOSS_HUBER: LOSS_HUBER, LOSS_TUKEY: LOSS_TUKEY}
DEFAULT_C = {LOSS_HUBER: 1.345, LOSS_TUKEY: 4.685}

XTOL = 1e-9
SIGMA_RTOL = 1e-6
COST_RTOL = 1e-8
W_ATOL = 1e-5
NEAR_RTOL = 1e-8
NEAR_MAX = 2
COND_MAX = 1e2
RATE_MAX = 0.9


def weighted_median_f32(a, m):
    """Lower weighted median of float32(a) (a >= 0) with integer multiplicities m: the smallest value v such that the
    multiplicities of the entries <= v sum to at least half the total.  0.0 when the total is 0."""
    a32 = np.asarray(a, np.float64).astype(np.float32)
    m = np.asarray(m, np.int64)
    total = int(m.sum())
    if total == 0:
        return 0.0
    order = np.argsort(a32, kind='stable')
    cum = np.cumsum(m[order])
    j = int(np.searchsorted(2 * cum, total, side='left'))  # first index with 2 cum >= total
    return float(a32[order][j])


def moments(w, c, s, y):
    return np.array([w.sum(), (w * c * c).sum(), (w * c * s).sum(), (w * s * s).sum(), (w * c * y).sum(),
                     (w * s * y).sum(), (w * y * y).sum()])


def _qcost(vx, vy, k, ridge, m):
    kx, ky = k * vx, k * vy
    return (m[6] - 2.0 * (kx * m[4] + ky * m[5]) + kx * kx * m[1] + 2.0 * kx * ky * m[2] + ky * ky * m[3] +
            ridge * (vx * vx + vy * vy))


def box_solve(m, k, ridge, bounds):
    """k_velocity's rule on the moments m = [n, cc, cs, ss, cy, sy, yy]: the interior solution when feasible, else the
    best of the four edge minimisers (first wins a tie)."""
    lx, hx, ly, hy = bounds
    H00, H01, H11 = k * k * m[1] + ridge, k * k * m[2], k * k * m[3] + ridge
    b0, b1 = k * m[4], k * m[5]
    det = H00 * H11 - H01 * H01
    if det > 1e-300:
        vx, vy = (H11 * b0 - H01 * b1) / det, (H00 * b1 - H01 * b0) / det
        if lx <= vx <= hx and ly <= vy <= hy:
            return np.array([vx, vy])
    best, bc = np.zeros(2), np.inf
    for edge in range(4):
        fix = edge >> 1
        val = ((hx if edge & 1 else lx) if fix == 0 else (hy if edge & 1 else ly))
        if fix == 0:
            x = (b1 - H01 * val) / H11 if H11 > 0 else 0.0
            x = min(max(x, ly), hy)
            v = (val, x)
        else:
            x = (b0 - H01 * val) / H00 if H00 > 0 else 0.0
            x = min(max(x, lx), hx)
            v = (x, val)
        cst = _qcost(v[0], v[1], k, ridge, m)
        if cst < bc:
            bc, best = cst, np.array(v)
    return best


def cond_number(m, k, ridge):
    H = np.array([[k * k * m[1] + ridge, k * k * m[2]], [k * k * m[2], k * k * m[3] + ridge]])
    ev = np.linalg.eigvalsh(H)
    return np.inf if ev[0] <= 0 else float(ev[1] / ev[0])


def weights(loss, a, t):
    """u(|r| = a) at the cut-off t; t = 0: 1 where a = 0, else 0 (both losses)."""
    a = np.asarray(a, np.float64)
    if loss == LOSS_HUBER:
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(a <= t, 1.0, t / np.where(a > 0, a, 1.0))
    if t == 0.0:
        return (a == 0.0).astype(np.float64)
    q = a / t
    return np.where(a < t, (1.0 - q * q) ** 2, 0.0)


def rho(loss, a, t):
    a = np.asarray(a, np.float64)
    if loss == LOSS_HUBER:
        return np.where(a <= t, a * a, 2.0 * t * a - t * t)
    if t == 0.0:
        return np.zeros_like(a)
    w = 1.0 - (a / t) ** 2
    return np.where(a < t, (t * t / 3.0) * (1.0 - w * w * w), t * t / 3.0)


def inliers(loss, a, t):
    if loss == LOSS_HUBER:
        return a <= t
    return (a < t) | ((t == 0.0) & (a == 0.0))


def robust_frame(az, y, m=None, *, k, loss, c=None, scale=None, iters=30, tol=1e-9, ridge=0.0, bounds=BOX):
    """One frame.  Returns x, cost, rmse_w, n_in, n, sigma, it (negative: the stop rule was not met), weights,
    residuals, and diagnostics: ls (the start), steps (max |dx| per iteration), cond (condition number of the normal
    matrix of the last solve; cond_max: the largest of the run), near (cells, multiplicity) within NEAR_RTOL of the cut-off."""
    loss = LOSS_ID[loss]
    c = DEFAULT_C[loss] if c is None else float(c)
    az = np.asarray(az, np.float64)
    y = np.asarray(y, np.float64)
    m = np.ones(len(y), np.int64) if m is None else np.asarray(m, np.int64)
    cs, sn = np.cos(az), np.sin(az)
    mw = m.astype(np.float64)
    mom = moments(mw, cs, sn, y)
    x = box_solve(mom, k, ridge, bounds)
    ls = x.copy()
    W = int(m.sum())
    fixed = scale is not None and scale > 0
    sigma = float(scale) if fixed else 0.0
    it, conv, steps = 0, W == 0, []
    cond = cond_max = cond_number(mom, k, ridge) if W > 0 else 1.0
    j = 1
    while not conv and j <= iters:
        r = y - k * (x[0] * cs + x[1] * sn)
        if not fixed:
            sigma = 1.4826 * weighted_median_f32(np.abs(r), m)
        if sigma == 0.0:
            conv = True
            break
        t = c * sigma
        w = mw * weights(loss, np.abs(r), t)
        mom = moments(w, cs, sn, y)
        if mom[0] == 0.0:
            conv = True
            break
        cond = cond_number(mom, k, ridge)
        cond_max = max(cond_max, cond)
        xn = box_solve(mom, k, ridge, bounds)
        dx = float(np.abs(xn - x).max())
        steps.append(dx)
        x, it = xn, j
        if tol > 0 and dx <= tol:
            conv = True
        j += 1
    if tol == 0:
        conv = True
    t = c * sigma
    r = y - k * (x[0] * cs + x[1] * sn)
    a = np.abs(r)
    u = weights(loss, a, t)
    su = float((mw * u).sum())
    nearm = (np.abs(a - t) <= NEAR_RTOL * t) & (m > 0)
    return dict(x=x, cost=float((mw * rho(loss, a, t)).sum() + ridge * (x * x).sum()),
                rmse_w=float(np.sqrt((mw * u * r * r).sum() / su)) if su > 0 else 0.0,
                n_in=int(m[inliers(loss, a, t)].sum()), n=W, sigma=sigma, it=it if conv else -it,
                weights=u, residuals=r, ls=ls, steps=steps, cond=cond, cond_max=cond_max, near=(int(nearm.sum()), int(m[nearm].sum())))


def robust_batch(az, y, m, seg, n=None, **kw):
    """Frames seg[f] .. seg[f + 1] (clamped to n, default len(y)).  out f64 [F, 8] in the library's column order,
    weights / residuals [N] (NaN where no frame covers a cell), frames: the per-frame dictionaries."""
    N = len(y) if n is None else min(int(n), len(y))
    seg = np.minimum(np.asarray(seg, np.int64), N)
    F = len(seg) - 1
    out = np.zeros((F, 8))
    wt = np.full(len(y), np.nan)
    rs = np.full(len(y), np.nan)
    frames = []
    for f in range(F):
        sl = slice(seg[f], max(seg[f], seg[f + 1]))
        r = robust_frame(az[sl], y[sl], None if m is None else m[sl], **kw)
        out[f] = [r['x'][0], r['x'][1], r['cost'], r['rmse_w'], r['n_in'], r['n'], r['sigma'], r['it']]
        wt[sl], rs[sl] = r['weights'], r['residuals']
        frames.append(r)
    return dict(out=out, weights=wt, residuals=rs, frames=frames, seg=seg)


def popcount(amask):
    a = np.asarray(amask).astype(np.int64) & 0xffffffff
    return np.array([bin(int(v)).count('1') for v in a], np.int64)


def grid_rad(G=361):
    """The chain's 0.5 degree azimuth grid (G = 361), or G points over the same [-90, 90] degrees."""
    return np.radians(np.linspace(-90.0, 90.0, G))


def planted(N, share, noise=0.05, seed=0, *, G=361, mmax=8, v_in=(0.004, -0.002), v_out=(-0.006, 0.005), k=K_CHAIN):
    """A frame of N cells on the G-point grid: round(share N) cells follow the motion v_out, the rest v_in, phase noise
    of standard deviation `noise`, multiplicities uniform in 0 .. mmax (mmax = 0: all 1) given as antenna masks."""
    rng = np.random.default_rng(seed)
    gidx = rng.integers(0, G, N).astype(np.int32)
    az = grid_rad(G)[gidx]
    is_out = np.zeros(N, bool)
    is_out[rng.permutation(N)[:int(round(share * N))]] = True
    v = np.where(is_out[:, None], np.asarray(v_out)[None], np.asarray(v_in)[None])
    y = k * (v[:, 0] * np.cos(az) + v[:, 1] * np.sin(az)) + noise * rng.standard_normal(N)
    m = rng.integers(0, mmax + 1, N) if mmax > 0 else np.ones(N, np.int64)
    amask = ((1 << m.astype(np.int64)) - 1).astype(np.uint32).view(np.int32)
    return dict(gidx=gidx, az=az, y=y, m=m.astype(np.int64), amask=amask, outlier=is_out, v_in=np.asarray(v_in),
                v_out=np.asarray(v_out), k=k)


def concat(frames):
    """Frames of planted() back to back: the per-cell arrays and seg i64 [F + 1]."""
    seg = np.concatenate([[0], np.cumsum([len(f['y']) for f in frames])]).astype(np.int64)
    cat = lambda key, dt: (np.concatenate([f[key] for f in frames]).astype(dt) if len(frames) else np.zeros(0, dt))
    return dict(gidx=cat('gidx', np.int32), az=cat('az', np.float64), y=cat('y', np.float64), m=cat('m', np.int64),
                amask=cat('amask', np.int32), seg=seg)


def assert_oracle_fit(ref, tol):
    """What the tolerances presuppose, asserted on the oracle alone."""
    for f, r in enumerate(ref['frames']):
        assert r['cond'] <= COND_MAX, ('condition number', f, r['cond'])
        assert r['near'][0] <= NEAR_MAX, ('cells at the cut-off', f, r['near'])
        if tol > 0 and r['it'] > 0 and len(r['steps']) >= 2 and r['steps'][-2] > 0:
            assert r['steps'][-1] / r['steps'][-2] < RATE_MAX, ('contraction rate', f, r['steps'][-2:])


def compare(tag, got_out, got_w, got_r, ref, *, tol, scale_of_x=None):
    """GPU rows / weights / residuals against robust_batch's result with the tolerances of the module docstring.
    Prints every figure before it asserts."""
    assert_oracle_fit(ref, tol)
    out, seg = ref['out'], ref['seg']
    worst = dict(x=0.0, sigma=0.0, cost=0.0, rmse=0.0, w=0.0, r=0.0)
    for f, fr in enumerate(ref['frames']):
        g, o = got_out[f], out[f]
        assert np.isfinite(g).all(), (tag, f, g)
        xs = max(np.abs(o[:2]).max(), 1e-3)
        ex = np.abs(g[:2] - o[:2]).max() / xs
        bound = XTOL if tol == 0 else (10 * tol) / xs + XTOL
        worst['x'] = max(worst['x'], ex)
        es = abs(g[6] - o[6]) / o[6] if o[6] != 0 else abs(g[6])
        worst['sigma'] = max(worst['sigma'], es)
        ec = abs(g[2] - o[2]) / abs(o[2]) if o[2] != 0 else abs(g[2])
        er = abs(g[3] - o[3]) / abs(o[3]) if o[3] != 0 else abs(g[3])
        worst['cost'], worst['rmse'] = max(worst['cost'], ec), max(worst['rmse'], er)
        print(f'{tag} frame {f} (n {int(o[5])}): x err {ex:.2e} (bound {bound:.2e}), sigma {es:.2e}, cost {ec:.2e}, '
              f'rmse {er:.2e}, it {g[7]:.0f} / {o[7]:.0f}, n_in {g[4]:.0f} / {o[4]:.0f}, cond {fr["cond"]:.1f} (max {fr["cond_max"]:.1f})')
        assert ex <= bound, (tag, f, 'x', g[:2], o[:2])
        if tol == 0:
            assert es <= SIGMA_RTOL, (tag, f, 'sigma', g[6], o[6])
            assert ec <= COST_RTOL and er <= COST_RTOL, (tag, f, 'cost / rmse', g[2:4], o[2:4])
            assert abs(g[4] - o[4]) <= fr['near'][1], (tag, f, 'n_in', g[4], o[4], fr['near'])
        assert g[5] == o[5], (tag, f, 'n', g[5], o[5])
        if tol == 0:
            assert g[7] == o[7], (tag, f, 'it', g[7], o[7])
        else:
            assert abs(abs(g[7]) - abs(o[7])) <= 1, (tag, f, 'it', g[7], o[7])
        sl = slice(seg[f], max(seg[f], seg[f + 1]))
        if got_w is not None and sl.stop > sl.start:
            worst['w'] = max(worst['w'], np.abs(got_w[sl] - ref['weights'][sl]).max())
        if got_r is not None and sl.stop > sl.start:
            worst['r'] = max(worst['r'], np.abs(got_r[sl] - ref['residuals'][sl]).max())
    print(f'{tag}: worst x {worst["x"]:.2e}, sigma {worst["sigma"]:.2e}, cost {worst["cost"]:.2e}, '
          f'rmse {worst["rmse"]:.2e}, weight {worst["w"]:.2e}, resid {worst["r"]:.2e}')
    if tol == 0:  # early-stop runs are compared on x and it alone
        assert worst['w'] <= W_ATOL, (tag, 'weights', worst['w'])
        # residuals: k dx (322.5 * XTOL * |x|, below 1e-9) plus rounding
        assert worst['r'] <= 1e-9, (tag, 'residuals', worst['r'])
    return worst
