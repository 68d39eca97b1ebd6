"""fp64 numpy reference of the wrapped-phase ego-motion solver (rsl_wrap.hip: rsl_wrapped_solve, rsl_wrapped_search),
test side.  No device code.

The cost is c(x) = sum_i wrap(y_i - k J_i . x)^2 + R(x), J = aux_ref.jacobian, R the Improved (mode 0) or Advanced
(mode 1) regulariser; radar_oracle.improved_cost / advanced_cost stay the oracle for its value (test_wrap_host.py pins
cost() here to them).  Every function takes x of shape [6] or [S, 6] and works on all S rows at once.

  Problem            the inputs of one call
  cost, grad, hess   the cost, its exact gradient and exact Hessian away from the wrap discontinuities
  local_min          exact active-set Newton: what a descent from a start must reach (a KKT point of the box problem)
  global_min         dense multi-start of local_min over the (v_x, v_y) box: the global-minimum oracle
  grid_shape, grid_points, stage1_terms, block_min, top_blocks   stage 1 and the top-k of rsl_wrapped_search
  solve_sections, search_sections   where each kernel's output lies in the caller-owned scratch
  device_descent     a restatement of the device's own loop (k_wrapped_ms / k_wrapped_grid2), used only to choose
                     iteration counts and to state margins; no test takes it for the truth
"""
import math

import numpy as np

import aux_ref

TWO_PI = 2.0 * np.pi
EPS = 2.0 ** -52


class Problem:
    """One call's inputs.  lo, hi: the box [6]; nv = 3 holds x[3..5] at 0 (clamped to the box); prev: Advanced's
    previous motion [6] or None."""

    def __init__(self, pos, ang, y, k, mode=0, nv=3, lo=None, hi=None, w=0.01, vmax=50.0, wmax=10.0, prev=None):
        self.pos = np.ascontiguousarray(np.asarray(pos, np.float64).reshape(-1, 3))
        self.ang = np.ascontiguousarray(np.asarray(ang, np.float64).reshape(-1, 2))
        self.y = np.ascontiguousarray(np.asarray(y, np.float64).reshape(-1))
        self.J = aux_ref.jacobian(self.pos, self.ang)
        self.n = len(self.y)
        self.k, self.mode, self.nv = float(k), int(mode), int(nv)
        self.lo = np.full(6, -2.0) if lo is None else np.asarray(lo, np.float64).reshape(6).copy()
        self.hi = np.full(6, 2.0) if hi is None else np.asarray(hi, np.float64).reshape(6).copy()
        self.w, self.vmax, self.wmax = float(w), float(vmax), float(wmax)
        self.prev = None if prev is None else np.asarray(prev, np.float64).reshape(6).copy()


def _rows(x):
    x = np.asarray(x, np.float64)
    return x.reshape(-1, 6), x.ndim == 1


def wrap(r):
    """r reduced to [-pi, pi]."""
    return r - TWO_PI * np.rint(r / TWO_PI)


def residuals(P, x):
    """wrap(y - k J x) [S, n]."""
    X, _ = _rows(x)
    return wrap(P.y[None, :] - P.k * (X @ P.J.T))


def _norms(X):
    return np.sqrt((X[:, :3] ** 2).sum(axis=1)), np.sqrt((X[:, 3:] ** 2).sum(axis=1))


def branches(P, x):
    """Advanced mode's penalty branches at x: (vm > 0.8 vmax, wm > 0.8 wmax, vm > 20 and wm > 5), bool [S] each."""
    X, _ = _rows(x)
    vm, wm = _norms(X)
    return vm > 0.8 * P.vmax, wm > 0.8 * P.wmax, (vm > 20) & (wm > 5)


def reg(P, x):
    X, one = _rows(x)
    if P.mode == 0:
        r = 0.01 * (X[:, :3] ** 2).sum(axis=1) + 0.01 * (X[:, 3:] ** 2).sum(axis=1)
        return r[0] if one else r
    vm, wm = _norms(X)
    av, aw = 0.8 * P.vmax, 0.8 * P.wmax
    r = np.where(vm > av, P.w * (vm - av) ** 2, 0.0) + np.where(wm > aw, P.w * (wm - aw) ** 2, 0.0)
    if P.prev is not None:
        r = r + P.w * 0.1 * ((X - P.prev) ** 2).sum(axis=1)
    r = r + np.where((vm > 20) & (wm > 5), P.w * 0.01 * (vm - 20) * (wm - 5), 0.0)
    r = r + P.w * 10.0 * X[:, 2] ** 2
    return r[0] if one else r


def data_cost(P, x):
    r = residuals(P, x)
    c = (r * r).sum(axis=1)
    return c[0] if np.asarray(x).ndim == 1 else c


def cost(P, x):
    return data_cost(P, x) + reg(P, x)


def data_grad(P, x):
    """-2 k sum_i r_i J_i."""
    g = -2.0 * P.k * (residuals(P, x) @ P.J)
    return g[0] if np.asarray(x).ndim == 1 else g


def data_hess(P):
    """2 k^2 J'J [6, 6]: exact wherever no residual sits on a wrap discontinuity."""
    return 2.0 * P.k * P.k * (P.J.T @ P.J)


def data_hess_exact(J, k):
    """2 k^2 J'J with every one of the 36 sums taken exactly (math.fsum), for the comparison with k_wrapped_hess."""
    J = np.asarray(J, np.float64)
    H = np.empty((6, 6))
    for a in range(6):
        for b in range(6):
            H[a, b] = 2.0 * k * k * math.fsum((J[:, a] * J[:, b]).tolist())
    return H


def _unit(V, m):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(m[:, None] > 0, V / m[:, None], 0.0)


def reg_grad(P, x):
    X, one = _rows(x)
    if P.mode == 0:
        g = 0.02 * X
        return g[0] if one else g
    vm, wm = _norms(X)
    av, aw = 0.8 * P.vmax, 0.8 * P.wmax
    uv, uw = _unit(X[:, :3], vm), _unit(X[:, 3:], wm)
    g = np.zeros_like(X)
    g[:, :3] += np.where(vm > av, 2.0 * P.w * (vm - av), 0.0)[:, None] * uv
    g[:, 3:] += np.where(wm > aw, 2.0 * P.w * (wm - aw), 0.0)[:, None] * uw
    if P.prev is not None:
        g += 0.2 * P.w * (X - P.prev)
    both = (vm > 20) & (wm > 5)
    g[:, :3] += np.where(both, P.w * 0.01 * (wm - 5), 0.0)[:, None] * uv
    g[:, 3:] += np.where(both, P.w * 0.01 * (vm - 20), 0.0)[:, None] * uw
    g[:, 2] += 20.0 * P.w * X[:, 2]
    return g[0] if one else g


def reg_hess(P, x, gauss_newton=False):
    """The exact Hessian of R [S, 6, 6]; with gauss_newton the positive semi-definite one the device descends with
    (the norm penalties' u u' part only, nothing for the vm wm cross term)."""
    X, one = _rows(x)
    S = len(X)
    H = np.zeros((S, 6, 6))
    I3 = np.eye(3)
    if P.mode == 0:
        H[:] = 0.02 * np.eye(6)
        return H[0] if one else H
    vm, wm = _norms(X)
    av, aw = 0.8 * P.vmax, 0.8 * P.wmax
    uv, uw = _unit(X[:, :3], vm), _unit(X[:, 3:], wm)
    Pv, Pw = uv[:, :, None] * uv[:, None, :], uw[:, :, None] * uw[:, None, :]
    with np.errstate(divide='ignore', invalid='ignore'):
        iv, iw = np.where(vm > 0, 1.0 / vm, 0.0), np.where(wm > 0, 1.0 / wm, 0.0)
    on = (vm > av)[:, None, None]
    H[:, :3, :3] += np.where(on, 2.0 * P.w * Pv, 0.0)
    if not gauss_newton:
        H[:, :3, :3] += np.where(on, (2.0 * P.w * (vm - av) * iv)[:, None, None] * (I3 - Pv), 0.0)
    on = (wm > aw)[:, None, None]
    H[:, 3:, 3:] += np.where(on, 2.0 * P.w * Pw, 0.0)
    if not gauss_newton:
        H[:, 3:, 3:] += np.where(on, (2.0 * P.w * (wm - aw) * iw)[:, None, None] * (I3 - Pw), 0.0)
    if P.prev is not None:
        H += 0.2 * P.w * np.eye(6)
    if not gauss_newton:
        both = ((vm > 20) & (wm > 5))[:, None, None]
        c = P.w * 0.01
        H[:, :3, :3] += np.where(both, (c * (wm - 5) * iv)[:, None, None] * (I3 - Pv), 0.0)
        H[:, 3:, 3:] += np.where(both, (c * (vm - 20) * iw)[:, None, None] * (I3 - Pw), 0.0)
        cross = c * uv[:, :, None] * uw[:, None, :]
        H[:, :3, 3:] += np.where(both, cross, 0.0)
        H[:, 3:, :3] += np.where(both, np.swapaxes(cross, 1, 2), 0.0)
    H[:, 2, 2] += 20.0 * P.w
    return H[0] if one else H


def grad(P, x):
    return data_grad(P, x) + reg_grad(P, x)


def hess(P, x):
    return data_hess(P) + reg_hess(P, x)


def clamp_start(P, x0, nx=None):
    """A start as the solver takes it: coordinates from nx (default nv) on are 0, then everything is clipped to the
    box."""
    X, one = _rows(x0)
    X = X.copy()
    X[:, (P.nv if nx is None else nx):] = 0.0
    X = np.minimum(np.maximum(X, P.lo), P.hi)
    return X[0] if one else X


def kkt_residual(P, x, nx=None):
    """max_a |the part of -grad that can still move x_a inside the box|, a < nx: 0 at a box-constrained stationary
    point.  [S]."""
    X, one = _rows(x)
    nx = P.nv if nx is None else nx
    g = grad(P, X)
    pg = np.where(X <= P.lo, np.minimum(g, 0.0), np.where(X >= P.hi, np.maximum(g, 0.0), g))
    pg[:, P.lo == P.hi] = 0.0
    r = np.abs(pg[:, :nx]).max(axis=1)
    return r[0] if one else r


def grad_scale(P, x):
    """The magnitude the rounding error of grad scales with: 2 k sum_i |r_i| |J_i| (max over coordinates) [S]."""
    X, one = _rows(x)
    s = 2.0 * P.k * (np.abs(residuals(P, X)) @ np.abs(P.J)).max(axis=1) + np.abs(reg_grad(P, X)).max(axis=1)
    return s[0] if one else s


def _masked_newton(H, g, free):
    """d with H_ff d_f = -g_f and d = 0 off the free set, per row."""
    ff = free[:, :, None] & free[:, None, :]
    Hm = np.where(ff, H, np.eye(6)[None])
    return np.linalg.solve(Hm, -np.where(free, g, 0.0)[:, :, None])[:, :, 0]


def local_min(P, x0, nx=None, maxit=100):
    """The box-constrained local minimiser reached from x0: an active-set Newton with the exact Hessian.  Per
    iteration: hold the coordinates that sit on a bound with the gradient (or the Newton direction) pointing out of
    the box, take the Newton direction on the others, go along it up to the first bound met (ratio test, step <= 1),
    halving while the cost does not fall.  It ends when no step lowers the cost; kkt_residual states how stationary
    the end is.  Coordinates from nx (default nv) on are held at their clamped start.  Returns (x, cost)."""
    X, one = _rows(x0)
    nx = P.nv if nx is None else nx
    X = np.minimum(np.maximum(X.copy(), P.lo), P.hi)
    if nx == P.nv:
        X = clamp_start(P, X)
    S = len(X)
    act = np.arange(6) < nx
    f = cost(P, X)
    done = np.zeros(S, bool)
    for _ in range(maxit):
        g, H = grad(P, X), data_hess(P)[None] + reg_hess(P, X)
        free = act[None] & ~(((X <= P.lo) & (g > 0)) | ((X >= P.hi) & (g < 0)))
        for _ in range(6):
            d = _masked_newton(H, g, free)
            out = free & (((X <= P.lo) & (d < 0)) | ((X >= P.hi) & (d > 0)))
            if not out.any():
                break
            free &= ~out
        with np.errstate(divide='ignore', invalid='ignore'):
            tmax = np.where(d > 0, (P.hi - X) / d, np.where(d < 0, (P.lo - X) / d, np.inf))
        t = np.minimum(1.0, tmax.min(axis=1))
        hit = tmax <= t[:, None]
        improved = np.zeros(S, bool)
        for ls in range(30):
            Xn = X + t[:, None] * d
            if ls == 0:
                Xn = np.where(hit, np.where(d > 0, P.hi, P.lo), Xn)
            Xn = np.minimum(np.maximum(Xn, P.lo), P.hi)
            fn = cost(P, Xn)
            ok = (fn < f) & ~done & ~improved
            X[ok], f[ok] = Xn[ok], fn[ok]
            improved |= ok
            if (improved | done).all():
                break
            t = t * 0.5
        done |= ~improved
        if done.all():
            break
    return (X[0], float(f[0])) if one else (X, f)


def grid_shape(lo, hi, spacing):
    """Stage 1's points per axis: ceil(width / spacing) clipped to 1..32768, for (v_x, v_y)."""
    def pts(w):
        g = math.ceil(w / spacing) if spacing > 0 else 1
        return int(min(max(g, 1), 32768))
    return pts(float(hi[0]) - float(lo[0])), pts(float(hi[1]) - float(lo[1]))


def grid_points(lo, hi, gx, gy):
    """Start s = iy gx + ix at (lo + (i + 0.5) (hi - lo) / g) per axis, clipped to the box.  [gx gy, 2]."""
    s = np.arange(gx * gy)
    ix, iy = s % gx, s // gx
    px = lo[0] + (ix + 0.5) * ((hi[0] - lo[0]) / gx)
    py = lo[1] + (iy + 0.5) * ((hi[1] - lo[1]) / gy)
    return np.stack([np.clip(px, lo[0], hi[0]), np.clip(py, lo[1], hi[1])], axis=1)


def grid_starts(P, base, gx, gy):
    """The 6-D points of stage 1's grid: (grid v_x, grid v_y, base[2..5]).  [gx gy, 6]."""
    X = np.tile(np.asarray(base, np.float64).reshape(1, 6), (gx * gy, 1))
    X[:, :2] = grid_points(P.lo, P.hi, gx, gy)
    return X


def stage1_terms(P, base):
    """T [n, 3] = (J0, J1, y - k sum_{a >= 2} J_a base_a)."""
    base = np.asarray(base, np.float64)
    return np.stack([P.J[:, 0], P.J[:, 1], P.y - P.k * (P.J[:, 2:] @ base[2:])], axis=1)


def block_min(costs, block=256):
    """Per block of `block` consecutive starts: (lowest cost, its start index; the lowest index among equal costs),
    and the second-lowest cost of the block (inf where the block has one start).  Three arrays [nblk]."""
    costs = np.asarray(costs, np.float64)
    nblk = (len(costs) + block - 1) // block
    best, idx, second = np.empty(nblk), np.empty(nblk, np.int64), np.empty(nblk)
    for b in range(nblk):
        c = costs[b * block:(b + 1) * block]
        j = int(np.argmin(c))  # the first of equal minima
        best[b], idx[b] = c[j], b * block + j
        rest = np.delete(c, j)
        second[b] = rest.min() if len(rest) else np.inf
    return best, idx, second


def top_blocks(blk_cost, blk_idx, nbest):
    """The blocks taken by the top-k, in (cost, start index) order: at most nbest of them."""
    order = np.lexsort((np.asarray(blk_idx), np.asarray(blk_cost)))
    return order[:nbest]


def global_min(P, gx, gy, base=None):
    """The lowest local_min over a gx x gy grid of starts on the (v_x, v_y) box (the other coordinates start at base,
    default 0).  Returns (x, cost)."""
    X0 = grid_starts(P, np.zeros(6) if base is None else base, gx, gy)
    X, f = local_min(P, X0)
    j = int(np.argmin(f))
    return X[j], float(f[j])


def solve_sections(lib, n, grid_n, nextra):
    """rsl_wrapped_solve's scratch in doubles (rsl_internal.h): J [6n] | Hd [36] | res [8 nstart]."""
    nstart = grid_n * grid_n + nextra
    return _carve(lib.rsl_wrapped_scratch_bytes(n, grid_n, nextra),
                  (('J', 6 * n), ('Hd', 36), ('res', 8 * nstart)))


def search_sections(lib, n, lo6, hi6, spacing, nbest, nextra):
    """rsl_wrapped_search's scratch in doubles (rsl_internal.h): J [6n] | Hd [36] | T [3n] | base [6] | blk [4 nblk] |
    starts [6 nstart] | res [8 nstart], nblk = ceil(gx gy / 256), nstart = nbest + nextra."""
    import ctypes
    six = ctypes.c_double * 6
    gx, gy = grid_shape(lo6, hi6, spacing)
    nblk, nstart = (gx * gy + 255) // 256, nbest + nextra
    total = lib.rsl_wrapped_search_scratch_bytes(n, six(*[float(v) for v in lo6]), six(*[float(v) for v in hi6]),
                                                 float(spacing), nbest, nextra)
    return _carve(total, (('J', 6 * n), ('Hd', 36), ('T', 3 * n), ('base', 6), ('blk', 4 * nblk),
                          ('starts', 6 * nstart), ('res', 8 * nstart)))


def _carve(total_bytes, parts):
    out, at = {}, 0
    for name, size in parts:
        out[name] = slice(at, at + size)
        at += size
    assert total_bytes == 8 * at, f'scratch layout changed: the library wants {total_bytes} bytes, the layout {8 * at}'
    return out


def device_descent(P, x0, iters, nx=None, free_set=True):
    """A restatement of the device's loop (k_wrapped_ms; with nx = 2 and x0 = grid_starts, k_wrapped_grid2's): the
    Gauss-Newton Hessian, the step solved on the free set (free_set False: on all nx coordinates, as before the
    free-set rule), x + step d clamped for step 1, 1/2, ..., 1/32, the first trial that lowers the cost taken, and the
    stop once a taken step gains no more than 1e-13 (1 + f).  Returns (x, cost)."""
    X, one = _rows(x0)
    nx = P.nv if nx is None else nx
    X = clamp_start(P, X) if nx == P.nv else np.minimum(np.maximum(X.copy(), P.lo), P.hi)
    f = cost(P, X)
    act = np.arange(6) < nx
    live = np.ones(len(X), bool)
    for _ in range(iters):
        g = grad(P, X)
        H = data_hess(P)[None] + reg_hess(P, X, gauss_newton=True)
        free = np.broadcast_to(act[None], X.shape).copy()
        if free_set:
            free &= ~(((X <= P.lo) & (g > 0)) | ((X >= P.hi) & (g < 0)))
        d = _masked_newton(H, g, free)
        took = np.zeros(len(X), bool)
        step = 1.0
        for _ in range(6):
            Xn = np.minimum(np.maximum(X + step * d, P.lo), P.hi)
            fn = cost(P, Xn)
            ok = (fn < f) & live & ~took
            gain = f - fn
            X[ok] = Xn[ok]
            stop = ok & (gain <= 1e-13 * (1.0 + fn))
            f[ok] = fn[ok]
            took |= ok
            live &= ~stop
            step *= 0.5
        live &= took
        if not live.any():
            break
    return (X[0], float(f[0])) if one else (X, f)
