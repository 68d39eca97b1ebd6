"""GPU: the wrapped-phase solver's kernels (rsl_wrap.hip: k_wrapped_jac, k_wrapped_hess, k_wrapped_prep2,
k_wrapped_grid2, k_wrapped_topk, k_wrapped_ms, k_wrapped_best) stage by stage against the fp64 numpy reference in
tests/wrap_ref.py, through the public entry points rsl_wrapped_solve and rsl_wrapped_search: the caller owns the scratch,
and reading it after the call shows each kernel's own output (wrap_ref.solve_sections / search_sections).

tests/test_gpu_wrapped.py holds the solvers to a one-sided contract (cost <= the reference's differential evolution);
here every stage is held to its definition, and the descent to the box-constrained minimum itself.  The inputs are
tests/wrap_cases.py; tests/test_wrap_host.py asserts on the CPU every margin relied on here (which costs are distinct,
which boxes are one piece of the cost, which bounds are active).
"""
import ctypes

import numpy as np
import pytest

import radar_oracle as O
import wrap_cases as C
import wrap_ref as W

pytestmark = pytest.mark.gpu

TOL = 1e-9
SIX = ctypes.c_double * 6


def _call(ctx, P, name, own, sec, extra, iters):
    """One call of rsl_wrapped_solve / rsl_wrapped_search (name; own: its arguments between nv and extra) on a scratch
    filled with NaN.  Returns (out [8], {section: its doubles after the call})."""
    import torch
    from rsl.runtime import _ptr
    ex = np.zeros((0, 6)) if extra is None else np.asarray(extra, np.float64).reshape(-1, 6)
    total = max(s.stop for s in sec.values())
    scratch = torch.full((total,), float('nan'), dtype=torch.float64, device=ctx.device)
    dp, da, dy = ctx.to_dev(P.pos.reshape(-1)), ctx.to_dev(P.ang.reshape(-1)), ctx.to_dev(P.y)
    dprev = ctx.to_dev(P.prev) if P.prev is not None else None
    dex = ctx.to_dev(ex.reshape(-1)) if len(ex) else None
    out = torch.full((8,), float('nan'), dtype=torch.float64, device=ctx.device)
    ctx._bind()
    ctx.check(getattr(ctx.lib, name)(ctx.h, _ptr(dp), _ptr(da), P.n, _ptr(dy), P.k, P.mode, P.w, P.vmax, P.wmax,
                                     _ptr(dprev), SIX(*P.lo), SIX(*P.hi), P.nv, *own, _ptr(dex), len(ex), int(iters),
                                     _ptr(scratch), 8 * total, _ptr(out)), name)
    s = scratch.cpu().numpy()
    return out.cpu().numpy(), {k: s[v].copy() for k, v in sec.items()}


def _solve(ctx, P, extra=None, grid_n=0, iters=12):
    ne = 0 if extra is None else len(np.asarray(extra).reshape(-1, 6))
    sec = W.solve_sections(ctx.lib, P.n, grid_n, ne)
    return _call(ctx, P, 'rsl_wrapped_solve', (int(grid_n),), sec, extra, iters)


def _search(ctx, P, base, spacing, nbest, extra=None, iters=12):
    ne = 0 if extra is None else len(np.asarray(extra).reshape(-1, 6))
    sec = W.search_sections(ctx.lib, P.n, P.lo, P.hi, spacing, nbest, ne)
    return _call(ctx, P, 'rsl_wrapped_search', (SIX(*[float(v) for v in base]), float(spacing), int(nbest)), sec,
                 extra, iters)


def _oracle_cost(P, x):
    if P.mode == 0:
        return O.improved_cost(x, P.pos, P.ang, P.y, P.k)
    return O.advanced_cost(x, P.pos, P.ang, P.y, P.k, P.prev, w=P.w, vmax=P.vmax, wmax=P.wmax)


def _close(a, b, tol=TOL):
    return abs(a - b) <= tol * abs(b)


# ----------------------------------------------------------------------------------------------------------------------
# Jacobian and data Hessian
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 3, 255, 256, 257, 600])
def test_jacobian_and_hessian(ctx, n):
    """k_wrapped_jac and k_wrapped_hess: J against aux_ref.jacobian at 1e-15 absolute (|p| <~ 1, so one ulp of an entry
    is ~1e-16), Hd against 2 k^2 J'J with every sum exact (math.fsum) at 1e-13 of |Hd|, and Hd exactly symmetric.
    Elevations are off 0 and p is off d: all six columns and all 21 products are live."""
    P = C.jac_case(n)
    _, s = _solve(ctx, P, extra=np.zeros(6), iters=0)
    J = s['J'].reshape(n, 6)
    assert (np.abs(P.J) > 0).all() and (n < 3 or (np.abs(P.J).max(axis=0) > 0.05).all()) and np.abs(P.J).max() < 2.0
    print(f'n={n}: max |J - ref| = {np.abs(J - P.J).max():.3e}')
    assert np.abs(J - P.J).max() <= 1e-15
    Hd = s['Hd'].reshape(6, 6)
    ref = W.data_hess_exact(P.J, P.k)
    print(f'n={n}: |Hd - ref| / |Hd| = {np.linalg.norm(Hd - ref) / np.linalg.norm(ref):.3e}')
    assert np.abs(Hd - ref).max() <= 1e-13 * np.linalg.norm(ref)
    assert np.array_equal(Hd, Hd.T)


# ----------------------------------------------------------------------------------------------------------------------
# Cost only: iters = 0, one extra start
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,nv,prev', [(0, 3, None), (0, 6, None), (1, 3, None), (1, 6, None), (1, 3, C.PREV),
                                          (1, 6, C.PREV)])
def test_cost_only(ctx, mode, nv, prev):
    """iters = 0 from one extra start: out is the clamped start (x[3..5] = 0 with nv = 3), its cost by the oracle at
    1e-9 relative, and start index 0.  The points sit in every reachable combination of Advanced's penalty branches
    (vm > 0.8 vmax, wm > 0.8 wmax, vm > 20 and wm > 5; with nv = 3, wm = 0 and only the first can be on), at the
    pipeline's small k in the +-50 box, and one of them outside the box."""
    P = C.cost_problem(mode, nv, prev)
    pts = C.cost_points() + [('outside', np.array([70.0, -60.0, 12.0, -11.0, 3.0, 14.0]))]
    seen = set()
    for name, x in pts:
        out, _ = _solve(ctx, P, extra=x, iters=0)
        xs = W.clamp_start(P, x)
        assert np.array_equal(out[:6], xs), (name, out[:6], xs)
        if nv == 3:
            assert (out[3:6] == 0).all()
        want = _oracle_cost(P, xs)
        assert _close(out[6], want), (name, out[6], want)
        assert out[7] == 0
        seen.add(tuple(bool(b[0]) for b in W.branches(P, xs)))
    if mode == 1:
        assert len(seen) == (7 if nv == 6 else 2), seen


# ----------------------------------------------------------------------------------------------------------------------
# One Newton step is exact on a quadratic
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,nv', [(0, 3), (0, 6), (1, 3), (1, 6)])
def test_one_step_is_the_least_squares_minimiser(ctx, mode, nv):
    """No wrap, no bound active, iters = 1 from a start off 0: the result is the least-squares minimiser
    (np.linalg.lstsq on the rows k J and the square roots of the quadratic penalties) to 1e-12 absolute -- only if the
    gradient, Hd (k = 2: k and k^2 differ), the regulariser's gradient and Hessian and the solve are all right.  Mode 1
    has only its quadratic terms live (the previous motion and v_z)."""
    P = C.one_step_problem(mode, nv)
    out, _ = _solve(ctx, P, extra=C.ONE_STEP_START, iters=1)
    xe = C.one_step_exact(P)
    print(f'mode {mode} nv {nv}: max |x - lstsq| = {np.abs(out[:6] - xe).max():.3e}')
    assert np.abs(out[:6] - xe).max() <= 1e-12
    assert _close(out[6], _oracle_cost(P, out[:6]))


# ----------------------------------------------------------------------------------------------------------------------
# Active bounds: the descent ends at the box-constrained minimum
# ----------------------------------------------------------------------------------------------------------------------
ACTIVE = C.active_cases()


@pytest.mark.parametrize('entry', ['solve', 'search'])
@pytest.mark.parametrize('case', ACTIVE, ids=[c['name'] for c in ACTIVE])
def test_active_bounds_reach_the_box_minimum(ctx, case, entry):
    """A minimiser with one or two coordinates on a bound (and a collapsed axis): rsl_wrapped_solve from one start and
    rsl_wrapped_search from its grid both return the box-constrained minimum of the reference solver (which scipy's
    BVLS confirms on the CPU), cost within 1e-9 relative and x within 1e-9.

    Before the step was solved on the free coordinates only, the clamped full Newton step stalled at the clipped
    unconstrained minimiser: every case here then failed through both entry points, with costs 1.06 to 2.05 times the
    minimum from one start and 1.003 to 2.05 times through the search."""
    P = case['P']
    x, f = W.local_min(P, case['start'])
    if entry == 'solve':
        out, _ = _solve(ctx, P, extra=case['start'], iters=12)
    else:
        out, _ = _search(ctx, P, np.zeros(6), case['spacing'], case['nbest'], iters=12)
    print(f'{case["name"]} {entry}: cost / min - 1 = {out[6] / f - 1:.3e}, max |x - x*| = {np.abs(out[:6] - x).max():.3e}')
    assert _close(out[6], f), (out[6], f)
    assert np.abs(out[:6] - x).max() <= 1e-9, (out[:6], x)
    assert (out[:6] >= P.lo).all() and (out[:6] <= P.hi).all()


def test_advanced_descent_converges(ctx):
    """Advanced mode with every norm penalty on at the minimiser (vm > 0.8 vmax, wm > 0.8 wmax, vm > 20 and wm > 5) and
    nothing wrapping: the cost after the descent is within 1e-9 relative of the exact solver's minimum.

    iters = 20: the regulariser's Gauss-Newton Hessian drops the norm penalties' curvature across the motion, so the
    descent converges linearly; the restated loop on the CPU is 2e-11 relative above the minimum after 5 iterations
    and stops by its own gain rule before 10, 5e-15 above it.  20 is twice that; 3 iterations are not enough
    (test_wrap_host.py)."""
    P, xt = C.advanced_descent_problem()
    x, f = W.local_min(P, xt)
    out, _ = _solve(ctx, P, extra=xt, iters=C.ADV_ITERS)
    print(f'advanced descent: cost / min - 1 = {out[6] / f - 1:.3e}, max |x - x*| = {np.abs(out[:6] - x).max():.3e}')
    assert _close(out[6], f), (out[6], f)
    assert _close(out[6], _oracle_cost(P, out[:6]))


# ----------------------------------------------------------------------------------------------------------------------
# Stage 1 (k_wrapped_prep2, k_wrapped_grid2) with iters = 0
# ----------------------------------------------------------------------------------------------------------------------
def _check_stage1(P, base, spacing, nbest, s, out):
    """blk, starts, res and out of a search with iters = 0 against the reference; returns (block minima, their start
    indices, the blocks taken)."""
    gx, gy = W.grid_shape(P.lo, P.hi, spacing)
    b6 = np.clip(base, P.lo, P.hi)
    assert np.array_equal(s['base'], b6)
    X = W.grid_starts(P, b6, gx, gy)
    best, idx, _ = W.block_min(W.cost(P, X))
    nblk = len(best)
    blk = s['blk'].reshape(nblk, 4)
    take = W.top_blocks(best, idx, nbest)
    taken = np.zeros(nblk, bool)
    taken[take] = True
    ulp = 4 * W.EPS * max(np.abs(P.lo[:2]).max(), np.abs(P.hi[:2]).max())
    assert np.array_equal(blk[:, 3], idx.astype(np.float64)), (blk[:, 3], idx)
    assert np.abs(blk[:, 1:3] - X[idx, :2]).max() <= ulp
    assert (blk[:, 1:3] >= P.lo[:2]).all() and (blk[:, 1:3] <= P.hi[:2]).all()
    assert np.isposinf(blk[taken, 0]).all(), 'a taken block is marked +inf'
    assert (np.abs(blk[~taken, 0] - best[~taken]) <= TOL * best[~taken]).all()
    # the stage-2 starts: the taken blocks in (cost, index) order, then base for the surplus
    nstart = len(s['starts']) // 6
    starts = s['starts'].reshape(nstart, 6)
    want = np.tile(b6, (nbest, 1))
    want[:len(take), :2] = blk[take, 1:3]
    assert np.array_equal(starts[:nbest], want), (starts[:nbest], want)
    res = s['res'].reshape(nstart, 8)
    xs = W.clamp_start(P, starts)
    assert np.array_equal(res[:, :6], xs)
    assert np.array_equal(res[:, 7], np.arange(nstart))
    ref = W.cost(P, xs)
    assert (np.abs(res[:, 6] - ref) <= TOL * ref).all()
    if P.nv == 6:  # with nv = 3 stage 2 zeroes x[3..5], which stage 1 held at base
        assert (np.abs(res[:len(take), 6] - best[take]) <= TOL * best[take]).all()
    j = np.lexsort((res[:, 7], res[:, 6]))[0]
    assert np.array_equal(out, res[j]), (out, res[j])
    return best, idx, take


STAGE1 = C.stage1_cases()


@pytest.mark.parametrize('case', STAGE1, ids=[c[0] for c in STAGE1])
def test_stage1_blocks(ctx, case):
    """iters = 0: T is (J0, J1, y - k sum_{a >= 2} J_a base_a); blk[b] is the minimum over block b's 256 starts of
    the reference cost at the grid points lo + (i + 0.5) (hi - lo) / g, s = iy gx + ix, with that start's coordinates
    and its index (exact: the host test shows every block's runner-up is 1e-6 relative away).  Grids 1 x 1, 19 x 23
    (a partial last block), 64 x 64, and a collapsed v_y axis, which gets one point."""
    name, P, base, spacing, shape = case
    out, s = _search(ctx, P, base, spacing, 1, iters=0)
    T = s['T'].reshape(P.n, 3)
    assert np.abs(T - W.stage1_terms(P, np.clip(base, P.lo, P.hi))).max() <= 8 * W.EPS * (1 + np.abs(P.y).max())
    assert np.abs(s['J'].reshape(P.n, 6) - P.J).max() <= 1e-14 * np.abs(P.J).max()
    best, idx, take = _check_stage1(P, base, spacing, 1, s, out)
    assert len(best) == (shape[0] * shape[1] + 255) // 256
    if name == 'collapsed':
        assert (s['blk'].reshape(-1, 4)[:, 2] == P.lo[1]).all()


@pytest.mark.parametrize('gy', [64, 4100])
def test_stage1_exact_ties(ctx, gy):
    """y = 0, targets at azimuth 0, box +-2^-5 with spacing 2^-10: the grid points are exact, whole rows and mirror
    columns are bit-equal in cost.  The lowest index wins inside each block (the lower of the two mirror columns, in
    the block's first row) and across blocks (the top-k takes blocks 0, 1, 2, 3; out is stage-2 start 0).  gy = 4100
    makes 1025 blocks: the top-k's first thread then meets blocks 0 and 1024, equal, in its own stripe."""
    P, base, spacing = C.tie_case(gy)
    out, s = _search(ctx, P, base, spacing, 4, iters=0)
    best, idx, take = _check_stage1(P, base, spacing, 4, s, out)
    assert take.tolist() == [0, 1, 2, 3]
    assert np.array_equal(s['blk'].reshape(-1, 4)[:, 3], 256.0 * np.arange(len(best)) + idx[0])
    assert len(set(s['blk'].reshape(-1, 4)[4:, 0].tolist())) == 1  # the device's block minima tie bit for bit too
    assert out[7] == 0


# ----------------------------------------------------------------------------------------------------------------------
# Top-k and stage 2 with iters = 0
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nbest', [1, 4, 16, 19])
def test_topk_and_stage2_starts(ctx, nbest):
    """16 blocks, nbest in {1, 4, nblk, nblk + 3}, two extra starts (one outside the box), a base outside the box:
    base is clipped; starts[0..nbest) are the nbest lowest block results in (cost, index) order with the surplus
    slots equal to base; the taken blk entries are +inf and the others untouched; the extra starts follow unchanged;
    res[q] is (clamped starts[q], its cost, q); out is the lowest of res, the lowest index among equals (the surplus
    slots tie exactly)."""
    P, base, spacing, extra = C.topk_case()
    out, s = _search(ctx, P, base, spacing, nbest, extra=extra, iters=0)
    best, idx, take = _check_stage1(P, base, spacing, nbest, s, out)
    assert len(best) == 16 and len(take) == min(nbest, 16)
    starts = s['starts'].reshape(-1, 6)
    assert np.array_equal(starts[nbest:], extra)
    assert np.array_equal(starts[len(take):nbest], np.tile(np.clip(base, P.lo, P.hi), (nbest - len(take), 1)))


# ----------------------------------------------------------------------------------------------------------------------
# Best over many starts
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid_n', [17, 33])
def test_best_over_many_starts(ctx, grid_n):
    """rsl_wrapped_solve from a 33 x 33 grid (1089 starts, past k_wrapped_best's 1024-thread stripe) and a 17 x 17 one
    (a partial block): every res row's cost is the oracle's at its x, its x is inside the box, its cost is at most
    the cost at its clamped start, its index is its row; out is the argmin of res by (cost, index)."""
    P = C.many_starts_problem()
    extra = np.array([[0.7, -0.3, 0, 0, 0, 0.0], [5.0, 5.0, 0, 0, 0, 0]])
    out, s = _solve(ctx, P, extra=extra, grid_n=grid_n, iters=12)
    nstart = grid_n * grid_n + 2
    res = s['res'].reshape(nstart, 8)
    X0 = np.zeros((nstart, 6))
    X0[:-2, :2] = W.grid_points(P.lo, P.hi, grid_n, grid_n)
    X0[-2:] = extra
    f0 = W.cost(P, W.clamp_start(P, X0))
    assert np.array_equal(res[:, 7], np.arange(nstart))
    assert (res[:, :6] >= P.lo).all() and (res[:, :6] <= P.hi).all() and (res[:, 3:6] == 0).all()
    want = np.array([O.improved_cost(r[:6], P.pos, P.ang, P.y, P.k) for r in res])
    assert (np.abs(res[:, 6] - want) <= TOL * want).all()
    assert (res[:, 6] <= f0 * (1 + TOL)).all()
    assert (res[:, 6] < f0 * (1 - 1e-3)).sum() > nstart // 2  # the descents do descend
    j = np.lexsort((res[:, 7], res[:, 6]))[0]
    assert np.array_equal(out, res[j])


# ----------------------------------------------------------------------------------------------------------------------
# The global minimum, two-sided
# ----------------------------------------------------------------------------------------------------------------------
GLOBAL = C.global_cases()


@pytest.mark.parametrize('case', GLOBAL, ids=[c[0] for c in GLOBAL])
def test_global_minimum_two_sided(ctx, case):
    """k = 322.5, 8 targets, box +-0.03 m/s (three wrap periods), mode 0, nv = 3, through ops.wrapped_search: the
    device's cost is at most the global oracle's minimum (a dense multi-start of the exact local solver; doubling its
    density does not lower it, test_wrap_host.py) and the oracle's at most the device's, both within 1e-9 relative.
    The second case cuts the box 2 mm/s below the first one's minimiser: its global minimum sits on the box edge."""
    from rsl import ops
    name, P = case
    x, f = W.global_min(P, C.GLOBAL_GRID, C.GLOBAL_GRID)
    xd, fd = ops.wrapped_search(P.pos, P.ang, P.y, P.k, mode=0, lo=P.lo, hi=P.hi, nv=3, ctx=ctx)
    print(f'{name}: device {fd:.12g}, oracle {f:.12g}, max |x - x*| = {np.abs(xd - x).max():.3e}')
    assert fd <= f * (1 + TOL), (fd, f)
    assert f <= fd * (1 + TOL), 'the oracle grid is too coarse: a defect of the test'
    assert _close(fd, O.improved_cost(xd, P.pos, P.ang, P.y, P.k))
    assert (xd >= P.lo).all() and (xd <= P.hi).all()
