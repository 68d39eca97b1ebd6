"""fp64 numpy / scipy references of the per-call kernels (rsl_aux.hip), test side.

The phase model is k (v + w x p).d = k J . [v; w] with J = [d, p x d], d = (cos el cos az, cos el sin az, sin el)
(velocity_solver.py:94-109).  Everything here is plain fp64 numpy; bvls_ref is scipy's own BVLS.
"""
import itertools

import numpy as np

EPS = 2.0 ** -52


def jacobian(pos, ang):
    """J f64 [n, 6] = [d, p x d] of pos [n, 3], ang [n, 2] = (az, el)."""
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    ang = np.asarray(ang, np.float64).reshape(-1, 2)
    ce = np.cos(ang[:, 1])
    d = np.stack([ce * np.cos(ang[:, 0]), ce * np.sin(ang[:, 0]), np.sin(ang[:, 1])], axis=1)
    return np.concatenate([d, np.cross(pos, d)], axis=1)


def pred_ref(J, x, k):
    """(k J x, sum_c |J_c x_c|: the magnitude the rounding error of one prediction scales with)."""
    x = np.asarray(x, np.float64)
    return k * (J[:, :len(x)] @ x), np.abs(J[:, :len(x)] * x).sum(axis=1)


def resid_ref(y, pred, wrap):
    r = np.asarray(y, np.float64) - pred
    return np.arctan2(np.sin(r), np.cos(r)) if wrap else r


def cost_ref(r, x, ridge):
    """sum r^2 + ridge |x|^2."""
    return float(np.sum(r * r) + ridge * np.sum(np.asarray(x, np.float64) ** 2))


def objective(Jk, y, x, ridge):
    """c(x) = sum (y - Jk x)^2 + ridge |x|^2 per target, Jk = k J[:, :nv]."""
    return cost_ref(y - Jk @ x, x, ridge)


def augmented(Jk, y, ridge):
    """(A, b) with |A x - b|^2 = c(x)."""
    nv = Jk.shape[1]
    return (np.concatenate([Jk, np.sqrt(ridge) * np.eye(nv)]), np.concatenate([y, np.zeros(nv)])) if ridge > 0 \
        else (Jk, y)


def bvls_ref(Jk, y, lo, hi, ridge):
    """scipy's lsq_linear(method='bvls', tol=1e-14) on J augmented with sqrt(ridge) I.  Returns (x, c(x), cond): cond
    is the condition number of the Hessian A'A.  Below 1e8 the problem is strictly convex, so the optimum is unique, and
    the Hessian over scipy's free set, a principal submatrix of it, is conditioned at least as well.  (The free set's
    condition alone does not make the optimum unique: with fewer targets than unknowns and no ridge, other active sets
    reach the same cost.)"""
    from scipy.optimize import lsq_linear
    A, b = augmented(Jk, y, ridge)
    res = lsq_linear(A, b, bounds=(np.asarray(lo, np.float64), np.asarray(hi, np.float64)), method='bvls', tol=1e-14)
    H = A.T @ A
    cond = np.linalg.cond(H) if np.abs(H).max() > 0 else np.inf
    return res.x, objective(Jk, y, res.x, ridge), cond


def bvls_brute(Jk, y, lo, hi, ridge):
    """The box-constrained minimum by enumeration of every active set (each variable free, at lo or at hi): the
    least-squares solution on the free variables (minimum norm where singular), kept when it lies inside the box;
    the best kept candidate is the optimum, since the optimum's own active set is one of them.  Returns (x, c(x))."""
    A, b = augmented(Jk, y, ridge)
    nv = A.shape[1]
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    best = (None, np.inf)
    for st in itertools.product((0, -1, 1), repeat=nv):
        st = np.array(st)
        x = np.where(st < 0, lo, hi).astype(np.float64)
        free = st == 0
        x[free] = 0.0
        if free.any():
            z = np.linalg.lstsq(A[:, free], b - A[:, ~free] @ x[~free], rcond=None)[0]
            if (z < lo[free]).any() or (z > hi[free]).any():
                continue
            x[free] = z
        c = objective(Jk, y, x, ridge)
        if c < best[1]:
            best = (x, c)
    return best


def preprocess_ref(rows, table, dc):
    """complex128(rows) * complex128(table), minus the row mean when dc."""
    out = np.asarray(rows).astype(np.complex128) * np.asarray(table).astype(np.complex128)
    return out - out.mean(axis=-1, keepdims=True) if dc else out


def cmul_f32_contracted(a, b):
    """The fp32 complex product of c64 a and b as the kernels' cmul forms it: re = fma(a.y, -b.y, a.x b.x),
    im = fma(a.y, b.x, a.x b.y).  Emulated in fp64, where a product of two f32 is exact (the sum's rounding to fp64
    before the one to fp32 can move the result by one f32 ulp, once in ~2^29 values)."""
    f32 = lambda v: v.astype(np.float32).astype(np.float64)
    ax, ay, bx, by = (np.asarray(v, np.float64) for v in (a.real, a.imag, b.real, b.imag))
    return f32(f32(ax * bx) - ay * by) + 1j * f32(f32(ax * by) + ay * bx)


K_PHASE = 4 * np.pi * 0.1 / (3e8 / 77e9)  # VelocitySolver's k at dt = 0.1 s, 77 GHz (~322 rad s / m)


def geometry(rs, n, degenerate, rmax=80.0):
    """(pos [n, 3], ang [n, 2]): general positions and elevations, or the reference's own targets (p = r d, elevation 0,
    r up to rmax: velocity_solver.py:334-339), for which columns 2..5 of J vanish."""
    az = rs.uniform(-1.5, 1.5, n)
    if degenerate:
        r = rs.uniform(1.0, rmax, n)
        return np.stack([r * np.cos(az), r * np.sin(az), np.zeros(n)], axis=1), np.stack([az, np.zeros(n)], axis=1)
    return rs.randn(n, 3) * 20, np.stack([az, rs.uniform(-0.3, 0.3, n)], axis=1)


def bvls_problems(seed, count):
    """Seeded box-constrained problems: nv in {3, 6}, n in {1, 2, 3, 5, 6, 7, 40, 300}, boxes of half-width 0.5-50 (three
    in ten not centred on 0, so some do not contain it), ridge in {0, 0.01}, every fifth degenerate, noise in
    {0, 0.01, 1} rad, the true motion up to two half-widths from the box centre (about half the components outside).
    Yields dicts: name, pos, ang, y, k, lo, hi, ridge."""
    rs = np.random.RandomState(seed)
    for q in range(count):
        nv = (3, 6)[rs.randint(2)]
        n = (1, 2, 3, 5, 6, 7, 40, 300)[rs.randint(8)]
        ridge = (0.0, 0.01)[rs.randint(2)]
        noise = (0.0, 0.01, 1.0)[rs.randint(3)]
        deg = q % 5 == 4
        pos, ang = geometry(rs, n, deg)
        hw = np.exp(rs.uniform(np.log(0.5), np.log(50.0), nv))
        ctr = rs.uniform(-20.0, 20.0, nv) if rs.rand() < 0.3 else np.zeros(nv)
        xt = ctr + hw * rs.uniform(-2.0, 2.0, nv)
        y = K_PHASE * (jacobian(pos, ang)[:, :nv] @ xt) + noise * rs.randn(n)
        yield dict(name=f'#{q} nv={nv} n={n} ridge={ridge} noise={noise} deg={int(deg)}', pos=pos, ang=ang, y=y,
                   k=K_PHASE, lo=ctr - hw, hi=ctr + hw, ridge=ridge)
