"""GPU: the per-call kernels (rsl_aux.hip) against the fp64 references of tests/aux_ref.py, at the sizes where a
256-thread strided loop and a one-workgroup reduction go wrong.  Every tolerance is derived from the rounding of the
number formats (EPS = 2^-52 for the fp64 kernels, 2^-24 for the fp32 one), not from what the kernels return.

rsl_phase_model      pred / resid / cost, wrap and ridge on and off, y absent, n = 0.
rsl_bvls             a seeded set of box-constrained problems and fixed edge cases against scipy's BVLS; the returned
                     cost against the per-target objective at the returned x, at exact fits too: it is a sum of
                     squares, so never negative.  (The moment form y'y - 2 b.x + x'Hx that k_bvls returned before
                     errs by ~1e-15 y'y there: see test_bvls_exact_fit_cost.)
rsl_preprocess_rows  rows * table and the fp64 mean removal at every S around the 64-lane and 256-thread boundaries.
"""
import numpy as np
import pytest

import aux_ref as R
from aux_ref import EPS

pytestmark = pytest.mark.gpu

X6 = np.array([3.0, -2.0, 0.5, 0.05, -0.02, 0.1])


# -- rsl_phase_model --------------------------------------------------------------------------------------------------
PM_N = [0, 1, 63, 64, 255, 256, 257, 1000]


def _pm_case(n, deg, wrap):
    """Geometry, and a y that lies at least k sum_c |J_c x_c| from the prediction: hundreds of radians, and the
    rounding of the prediction (bounded relative to that sum) then stays inside the residual's own bound.  With wrap
    the first targets' residuals are planted within 0, 1e-12 and 1e-6 rad of an odd multiple of pi, on either side."""
    rs = np.random.RandomState(1000 * n + 10 * deg + wrap)
    # the degenerate targets within 20 m: the column p x d is then rounding noise of size EPS r, which the bound on
    # pred (relative to the computed |J_c x_c|) does not cover beyond a few tens of metres
    pos, ang = R.geometry(rs, n, deg, rmax=20.0)
    J = R.jacobian(pos, ang)
    p, mag = R.pred_ref(J, X6, R.K_PHASE)
    far = R.K_PHASE * mag * rs.uniform(1.0, 2.0, n)
    y = np.where(p > 0, -far, far)
    if wrap:
        m = min(n, 12)
        odd = (2 * np.ceil(R.K_PHASE * mag[:m] / (2 * np.pi)) + 1) * np.pi
        dlt = np.array([0.0, 1e-12, -1e-12, 1e-6, -1e-6, 0.0] * 2)[:m]
        y[:m] = p[:m] + np.where(np.arange(m) % 2 == 0, odd, -odd) + dlt
    return pos, ang, J, y


@pytest.mark.parametrize('ridge', [0.0, 0.01])
@pytest.mark.parametrize('wrap', [0, 1])
@pytest.mark.parametrize('deg', [0, 1], ids=['general', 'degenerate'])
def test_phase_model(ctx, deg, wrap, ridge):
    from rsl import ops
    for n in PM_N:
        pos, ang, J, y = _pm_case(n, deg, wrap)
        p_ref, mag = R.pred_ref(J, X6, R.K_PHASE)
        only = ops.phase_model(pos, ang, X6, R.K_PHASE, ctx=ctx)  # y absent: the prediction alone
        assert set(only) == {'pred'} and only['pred'].shape == (n,)
        d_pred = 8 * EPS * R.K_PHASE * mag
        assert (np.abs(only['pred'] - p_ref) <= d_pred).all(), (n, np.abs(only['pred'] - p_ref).max())
        if n == 0:
            continue
        got = ops.phase_model(pos, ang, X6, R.K_PHASE, y=y, wrap=bool(wrap), ridge=ridge, ctx=ctx)
        assert np.array_equal(got['pred'], only['pred'])
        r_ref = R.resid_ref(y, p_ref, wrap)
        assert np.abs(y - p_ref).min() > 100.0
        if wrap:
            assert (np.abs(r_ref) <= np.pi).all() and (np.abs(got['resid']) <= np.pi + 4 * EPS).all()
            if n >= 12:
                assert (np.abs(np.abs(r_ref[:12]) - np.pi) < 2e-6).all()  # the planted residuals are at +-pi
        d_res = 16 * EPS * np.maximum(1.0, np.abs(y - p_ref))
        err = np.abs(np.angle(np.exp(1j * (got['resid'] - r_ref))))  # modulo 2 pi: either sign at +-pi
        assert (err <= d_res).all(), (n, (err / d_res).max())
        # the cost of the returned residuals, then those against the reference's: sum r^2 of n fp64 terms errs by
        # n EPS sum r^2, and an error d in r by 2 |r| d
        c_ref = R.cost_ref(r_ref, X6, ridge)
        tol = n * EPS * np.sum(r_ref ** 2) + 2 * np.sum(np.abs(r_ref) * d_res)
        assert abs(got['cost'] - c_ref) <= tol, (n, got['cost'], c_ref, tol)
        assert abs(got['cost'] - R.cost_ref(got['resid'], X6, ridge)) <= n * EPS * np.sum(r_ref ** 2)


# -- rsl_bvls ---------------------------------------------------------------------------------------------------------
def check_bvls(P, x, cost):
    """The four assertions on one problem P (aux_ref.bvls_problems' dict) and the solver's (x, cost)."""
    name, y, ridge = P['name'], P['y'], P['ridge']
    lo, hi = np.asarray(P['lo'], np.float64), np.asarray(P['hi'], np.float64)
    nv = len(lo)
    Jk = P['k'] * R.jacobian(P['pos'], P['ang'])[:, :nv]
    assert (lo <= x).all() and (x <= hi).all(), (name, x, lo, hi)
    x_ref, c_ref, cond = R.bvls_ref(Jk, y, lo, hi, ridge)
    yy = float(y @ y)
    cx = R.objective(Jk, y, x, ridge)
    print(f'{name}: c(x) {cx:.17g} scipy {c_ref:.17g} cost {cost:.17g} cond {cond:.3g} '
          f'dx {np.abs(x - x_ref).max():.3g}')
    assert cx <= c_ref * (1 + 1e-8) + 1e-10 * yy, (name, cx, c_ref)
    if cond < 1e8:
        assert np.abs(x - x_ref).max() <= 1e-6, (name, x, x_ref)
    H, b = Jk.T @ Jk + ridge * np.eye(nv), Jk.T @ y
    assert abs(cost - cx) <= 1e-12 * (yy + 2 * abs(b @ x) + x @ H @ x), (name, cost, cx)
    return x_ref


def _solve(ctx, P):
    from rsl import ops
    return ops.bvls(P['pos'], P['ang'], P['y'], P['k'], list(P['lo']), list(P['hi']), ridge=P['ridge'], ctx=ctx)


def test_bvls_seeded_problems(ctx):
    for P in R.bvls_problems(2024, 200):
        check_bvls(P, *_solve(ctx, P))


def _fixed(name, nv, n, deg, lo, hi, xt, ridge=0.0, noise=0.01, seed=5):
    rs = np.random.RandomState(seed)
    pos, ang = R.geometry(rs, n, deg)
    y = R.K_PHASE * (R.jacobian(pos, ang)[:, :len(xt)] @ np.asarray(xt, np.float64)) + noise * rs.randn(n)
    return dict(name=name, pos=pos, ang=ang, y=y, k=R.K_PHASE, lo=np.asarray(lo, np.float64)[:nv],
                hi=np.asarray(hi, np.float64)[:nv], ridge=ridge)


FAR = [400.0, -300.0, 40.0, 30.0, -30.0, 20.0]
BOX = [50.0, 50.0, 10.0, 10.0, 10.0, 10.0]


@pytest.mark.parametrize('nv', [3, 6])
def test_bvls_fixed_cases(ctx, nv):
    neg = [-b for b in BOX]
    # the optimum at a vertex: every bound active
    P = _fixed('vertex', nv, 40, 0, [-1.0] * 6, [1.0] * 6, FAR[:nv])
    x, cost = _solve(ctx, P)
    x_ref = check_bvls(P, x, cost)
    assert (np.abs(x) == 1.0).all() and np.abs(x - x_ref).max() <= 1e-12, (x, x_ref)
    # a box that does not contain 0, the true motion partly inside it
    P = _fixed('box without 0', nv, 40, 0, [5.0, -9.0, 1.0, 0.5, -3.0, 0.2], [10.0, -4.0, 3.0, 2.0, -1.0, 0.4],
               [7.0, -2.0, 0.0, 1.0, -2.0, 0.3][:nv])
    check_bvls(P, *_solve(ctx, P))
    # fewer targets than unknowns, and several strides of the 256-thread loops
    for n in (1, 2, 257, 1000):
        for ridge in (0.0, 0.01):
            P = _fixed(f'n={n} ridge={ridge}', nv, n, 0, neg, BOX, X6[:nv], ridge=ridge, seed=n)
            check_bvls(P, *_solve(ctx, P))
    # the reference's own geometry (p = r d, elevation 0): columns 2..5 of J vanish.  Without ridge the null components
    # come back as clamp(0, lo, hi) (solve_free's zero rule and the start point); with ridge they are the ridge solution
    lo = [-50.0, -50.0, 1.0, -10.0, -3.0, -10.0]
    hi = [50.0, 50.0, 3.0, 10.0, -1.0, 10.0]
    clamp0 = np.clip(0.0, lo, hi)[:nv]
    for ridge in (0.0, 0.01):
        P = _fixed(f'degenerate ridge={ridge}', nv, 40, 1, lo, hi, X6[:nv], ridge=ridge)
        x, cost = _solve(ctx, P)
        x_ref = check_bvls(P, x, cost)
        if ridge == 0.0:
            assert np.array_equal(x[2:], clamp0[2:]), (x, clamp0)
            Jk2 = P['k'] * R.jacobian(P['pos'], P['ang'])[:, :2]  # the two live columns: an unconstrained 2 x 2 fit
            assert np.abs(x[:2] - np.linalg.lstsq(Jk2, P['y'] - 0.0, rcond=None)[0]).max() <= 1e-6
        else:
            assert np.abs(x - x_ref).max() <= 1e-6 and np.abs(x[2:] - clamp0[2:]).max() <= 1e-6, (x, x_ref)


EXACT = [(nv, n, deg) for nv in (3, 6) for n in (3, 40, 300) for deg in (0, 1)]


def _exact(nv, n, deg):
    return _fixed(f'exact fit nv={nv} n={n} deg={deg}', nv, n, deg, [-b for b in BOX], BOX, X6[:nv], noise=0.0,
                  seed=100 * n + 10 * nv + deg)


@pytest.mark.parametrize('nv,n,deg', EXACT)
def test_bvls_exact_fit_cost(ctx, nv, n, deg):
    """y = k J x_t with x_t inside the box: the cost is a per-target sum of squares, so >= 0 and within the rounding of
    n residuals (each computed to a few EPS |y|) of the objective at the returned x.  The moment form
    y'y - 2 b.x + x'Hx cancels here: its error, ~1e-15 y'y ~ 1e-9, is ten orders above this bound, of either sign."""
    P = _exact(nv, n, deg)
    x, cost = _solve(ctx, P)
    check_bvls(P, x, cost)
    cx = R.objective(P['k'] * R.jacobian(P['pos'], P['ang'])[:, :nv], P['y'], x, 0.0)
    tol = 1e-9 * cx + n * (16 * EPS * np.abs(P['y']).max()) ** 2
    print(f"{P['name']}: cost {cost!r} c(x) {cx!r} tol {tol!r}")
    assert cost >= 0.0, (P['name'], cost)
    assert abs(cost - cx) <= tol, (P['name'], cost, cx, tol)


@pytest.mark.parametrize('n,deg', [(n, deg) for n in (3, 40, 300) for deg in (0, 1)])
def test_dropin_step1_cost_nonnegative(ctx, n, deg):
    """The same through the drop-in: step1_result.fun is the reference's sum of squares (velocity_solver.py:209-232)."""
    from src.velocity_solver.velocity_solver import VelocitySolver
    P = _exact(3, n, deg)
    vs = VelocitySolver()
    assert vs._k(0.1) == P['k']
    res = vs.two_step_optimization(P['pos'], P['ang'], P['y'], 0.1)
    print(f"{P['name']}: step1 fun {res['step1_result'].fun!r} step2 fun {res['step2_result'].fun!r}")
    assert res['success'] and res['step1_result'].fun >= 0.0, res['step1_result'].fun
    assert res['step2_result'].fun >= 0.0 and res['cost'] >= 0.0


# -- rsl_preprocess_rows ----------------------------------------------------------------------------------------------
PP_S = [1, 2, 63, 64, 255, 256, 257, 400, 1000]
E32 = 2.0 ** -24


def _c64(rs, *shape):
    return (rs.randn(*shape) + 1j * rs.randn(*shape)).astype(np.complex64)


@pytest.mark.parametrize('dc', [0, 1])
@pytest.mark.parametrize('rows', [1, 3, 257])
def test_preprocess_rows(ctx, rows, dc):
    """Inputs and table are complex64 already, so nothing is rounded on the way in.  Each output is within
    4 * 2^-24 * max |row * table| of the fp64 reference: the fp32 complex product is two roundings per component
    (below 3 * 2^-24 |in| |table| in modulus), the cast of the mean-free value one more; the mean is taken in fp64."""
    from rsl import ops
    rs = np.random.RandomState(rows)
    for S in PP_S:
        x, tab = _c64(rs, rows, S), _c64(rs, S)
        if rows > 1:
            x[1] += np.complex64(30 - 20j)  # a row with an offset
        got = ops.preprocess_rows(x, tab, bool(dc), ctx=ctx)
        assert got.shape == (rows, S)
        ref = R.preprocess_ref(x, tab, dc)
        prod = np.abs(x.astype(np.complex128) * tab.astype(np.complex128))
        tol = 4 * E32 * prod.max(axis=1, keepdims=True)
        err = np.abs(got - ref)
        assert (err <= tol).all(), (S, (err / tol).max())
        if not dc:
            # the fp32 product itself, in the kernel's FMA-contracted form.  (The uncontracted product that numpy may
            # or may not compute lies up to 2.1 * 2^-24 |in| |table| from the contracted one, one numpy form against
            # the other: not a reference for this bound.)
            f32 = R.cmul_f32_contracted(x, tab[None, :])
            assert (np.abs(got - f32) <= 2 * E32 * np.abs(x).astype(np.float64) * np.abs(tab)).all(), S


@pytest.mark.parametrize('S', [257, 1000])
def test_preprocess_rows_large_mean(ctx, S):
    """Rows whose product with the table has a common offset 100 times its spread: the mean is a sum of S values of
    ~100 and the output is ~1, so the mean has to be accumulated in fp64 to stay inside the same bound."""
    from rsl import ops
    rs = np.random.RandomState(S)
    tab = (np.complex64(0.8 - 0.6j) * (1 + 1e-3 * _c64(rs, S))).astype(np.complex64)
    x = (np.complex64(60 + 80j) + _c64(rs, 3, S) / np.float32(np.sqrt(2))).astype(np.complex64)
    ref = R.preprocess_ref(x, tab, True)
    full = R.preprocess_ref(x, tab, False)
    ratio = np.abs(full.mean(axis=1)) / np.sqrt((np.abs(ref) ** 2).mean(axis=1))
    assert (ratio > 90).all() and (ratio < 110).all(), ratio
    got = ops.preprocess_rows(x, tab, True, ctx=ctx)
    tol = 4 * E32 * np.abs(full).max(axis=1, keepdims=True)
    assert (np.abs(got - ref) <= tol).all(), (np.abs(got - ref) / tol).max()
