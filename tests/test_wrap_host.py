"""CPU: the numpy reference of the wrapped-phase solver (tests/wrap_ref.py) is pinned to the oracle's costs, to finite
differences and to scipy's BVLS, and every margin that tests/test_gpu_wrap_stages.py relies on is asserted on the very
inputs it uses (tests/wrap_cases.py)."""
import numpy as np
import pytest

import radar_oracle as O
import wrap_cases as C
import wrap_ref as W


def _oracle_cost(P, x):
    if P.mode == 0:
        return O.improved_cost(x, P.pos, P.ang, P.y, P.k)
    return O.advanced_cost(x, P.pos, P.ang, P.y, P.k, P.prev, w=P.w, vmax=P.vmax, wmax=P.wmax)


@pytest.mark.parametrize('mode,prev', [(0, None), (1, None), (1, C.PREV)])
def test_cost_equals_oracle(mode, prev):
    """cost() is the oracle's improved_cost / advanced_cost: on random x over the box and on one x in every
    reachable combination of Advanced's branches."""
    rs = np.random.RandomState(5)
    for k in (C.KPIPE, C.K77):
        P = C.cost_problem(mode, 6, prev)
        P.k = k
        X = rs.uniform(P.lo, P.hi, (200, 6))
        X = np.concatenate([X, np.stack([x for _, x in C.cost_points()])])
        got = W.cost(P, X)
        for x, c in zip(X, got):
            want = _oracle_cost(P, x)
            # the two form the prediction in different orders: each is within a few ulp of k sum_a |J_ia x_a| (1e5
            # rad at 77 GHz in the corner of the +-50 box), and the cost moves by 2 |r_i| times that
            dpred = 16 * W.EPS * P.k * (np.abs(P.J) @ np.abs(x))
            tol = 1e-13 * want + float(2 * np.abs(W.residuals(P, x)[0]) @ dpred)
            assert abs(c - want) <= tol, (mode, x, c, want, tol)
            assert abs(W.cost(P, x) - c) <= tol  # one row and many rows agree


def test_cost_points_cover_every_branch_combination():
    P = C.cost_problem(1, 6, None)
    seen = {tuple(bool(b[0]) for b in W.branches(P, x)) for _, x in C.cost_points()}
    # (vm > 40, wm > 8) on both forces the third; every other combination exists with the third on and off
    assert seen == {(False, False, False), (False, False, True), (True, False, False), (True, False, True),
                    (False, True, False), (False, True, True), (True, True, True)}
    for _, x in C.cost_points():
        assert (x >= P.lo).all() and (x <= P.hi).all()


@pytest.mark.parametrize('mode,prev', [(0, None), (1, None), (1, C.PREV)])
def test_gradient_and_hessian_against_finite_differences(mode, prev):
    """grad() and hess() are the derivatives of cost(): central differences at every branch combination."""
    P = C.cost_problem(mode, 6, prev)
    for name, x in C.cost_points():
        g, H = W.grad(P, x), W.hess(P, x)
        E = np.eye(6)
        gfd = np.array([(W.cost(P, x + 1e-5 * e) - W.cost(P, x - 1e-5 * e)) / 2e-5 for e in E])
        Hfd = np.stack([(W.grad(P, x + 1e-4 * e) - W.grad(P, x - 1e-4 * e)) / 2e-4 for e in E])
        assert np.abs(g - gfd).max() <= 1e-7 * max(1.0, np.abs(g).max()), (name, g, gfd)
        assert np.abs(H - Hfd).max() <= 1e-7 * np.abs(H).max(), (name, np.abs(H - Hfd).max())
        assert np.array_equal(H, H.T)
    # the device's Gauss-Newton Hessian of R is positive semi-definite everywhere
    for name, x in C.cost_points():
        assert np.linalg.eigvalsh(W.reg_hess(P, x, gauss_newton=True)).min() >= -1e-15


def test_data_hessian_exact_sum():
    P = C.jac_case(257)
    H = W.data_hess_exact(P.J, P.k)
    assert np.abs(H - W.data_hess(P)).max() <= 1e-13 * np.linalg.norm(H)
    assert np.array_equal(H, H.T)


ACTIVE = C.active_cases()


@pytest.mark.parametrize('case', ACTIVE, ids=[c['name'] for c in ACTIVE])
def test_local_min_equals_bvls_with_active_bounds(case):
    """The exact local solver against scipy's lsq_linear (bvls) on the unwrapped problem, with 1 and 2 coordinates on
    a bound; and the margins of the GPU test: the whole box is one piece of the cost, the bounds expected are active,
    the end is a KKT point, the restated device loop with the free-set rule reaches it from the start and through the
    two stages of the search, and without the rule (the clamped full Newton step) it does not."""
    P, start = case['P'], case['start']
    assert C.one_piece_margin(P) > 0.5
    x, f = W.local_min(P, start)
    xb, fb = C.bvls_of(P)
    assert np.abs(x[:P.nv] - xb).max() <= 1e-12 * max(1.0, np.abs(xb).max())
    assert abs(f - fb) <= 1e-12 * fb
    on = (x[:P.nv] <= P.lo[:P.nv]) | (x[:P.nv] >= P.hi[:P.nv])
    assert int(on.sum()) == case['active']
    assert W.kkt_residual(P, x) <= 1e-12 * W.grad_scale(P, x)
    assert f > 1e-3  # the 1e-9 relative bound on the cost is not a bound on rounding noise about 0
    xd, fd = W.device_descent(P, start, 12)
    assert np.abs(xd - x).max() <= 1e-12 and abs(fd - f) <= 1e-12 * f
    xp, fp = W.device_descent(P, start, 12, free_set=False)
    assert fp > f * (1 + 1e-3), 'the case does not tell the clamped Newton step from the box minimum'
    # the search: stage 1 over (v_x, v_y) from its grid, stage 2 from the nbest block winners
    gx, gy = W.grid_shape(P.lo, P.hi, case['spacing'])
    assert gx * gy <= 256 and max(gx, gy) == 8 and (gy == 1) == (P.lo[1] == P.hi[1])
    for free_set, ok in ((True, True), (False, False)):
        X1, f1 = W.device_descent(P, W.grid_starts(P, W.clamp_start(P, np.zeros(6), nx=6), gx, gy), 12, nx=2,
                                  free_set=free_set)
        _, f2 = W.device_descent(P, X1[np.argsort(f1, kind='stable')[:1]], 12, free_set=free_set)
        assert (abs(f2[0] - f) <= 1e-12 * f) == ok, (free_set, f2[0], f)


@pytest.mark.parametrize('mode,nv', [(0, 3), (0, 6), (1, 3), (1, 6)])
def test_local_min_no_active_bound_and_one_step_margins(mode, nv):
    """0 active bounds: local_min is the least-squares minimiser.  The margins of the one-step GPU test: no residual
    near a wrap between the start and the minimiser, the minimiser strictly inside the box, Advanced's branches
    off, a well-conditioned Hessian, every term of the gradient live at the start (k != k^2, v_z != 0, x != prev),
    and one restated device iteration lands on the minimiser."""
    P = C.one_step_problem(mode, nv)
    xe = C.one_step_exact(P)
    x0 = W.clamp_start(P, C.ONE_STEP_START)
    x, f = W.local_min(P, x0)
    assert np.abs(x - xe).max() <= 1e-13
    assert (xe > P.lo + 0.5).all() and (xe < P.hi - 0.5).all()
    for t in np.linspace(0, 1, 11):
        assert np.abs(P.y - P.k * (P.J @ (x0 + t * (xe - x0)))).max() < np.pi - 1.0
    assert not any(b[0] for b in W.branches(P, xe)) and not any(b[0] for b in W.branches(P, x0))
    assert np.linalg.cond(W.hess(P, xe)[:nv, :nv]) < 200
    assert P.k * P.k != P.k and (np.abs(W.reg_grad(P, x0)[:nv]) > 1e-4).all() and np.abs(x0 - xe).max() > 0.05
    x1, _ = W.device_descent(P, x0, 1)
    assert np.abs(x1 - xe).max() <= 1e-14


def test_advanced_descent_margins():
    """The converged Advanced descent's inputs: every norm penalty is on at the minimiser, no bound is active, nothing
    wraps, the exact solver ends at a stationary point, and the restated device loop is within 1e-10 relative of its
    cost (a tenth of the GPU test's bound) at ADV_ITERS and at half of it."""
    P, xt = C.advanced_descent_problem()
    x, f = W.local_min(P, xt)
    assert all(b[0] for b in W.branches(P, x))
    assert (x > P.lo).all() and (x < P.hi).all()
    assert W.kkt_residual(P, x) <= 1e-12 * W.grad_scale(P, x)
    assert np.abs(P.y - P.k * (P.J @ x)).max() < 1.0 and np.abs(P.y - P.k * (P.J @ xt)).max() < 1.0
    for it in (C.ADV_ITERS // 2, C.ADV_ITERS):
        _, fd = W.device_descent(P, xt, it)
        assert abs(fd - f) <= 1e-10 * f, (it, fd, f)
    _, f3 = W.device_descent(P, xt, 3)
    assert f3 - f > 1e-9 * f  # three iterations are not enough: the descent is what the test checks


STAGE1 = C.stage1_cases()


@pytest.mark.parametrize('case', STAGE1, ids=[c[0] for c in STAGE1])
def test_stage1_margins(case):
    """The grid is the one the case names, and in every block the best and the second-best reference costs differ by
    far more than 1e-9 relative, so the winner's index is determined."""
    name, P, base, spacing, shape = case
    assert W.grid_shape(P.lo, P.hi, spacing) == shape
    cs = W.cost(P, W.grid_starts(P, np.clip(base, P.lo, P.hi), *shape))
    best, idx, second = W.block_min(cs)
    assert len(best) == (shape[0] * shape[1] + 255) // 256
    assert ((second - best) > 1e-6 * best).all()
    assert (best > 1e-3).all()
    if name == '19x23':
        assert shape[0] * shape[1] % 256 != 0


@pytest.mark.parametrize('gy', [64, 4100])
def test_tie_case_margins(gy):
    """The exact-tie grids: every grid point is exact, mirror columns and whole rows are bit-equal in cost, every block
    has its minimum at least twice, and all blocks (16; 1025, more than the top-k has threads) have the same
    minimum."""
    P, base, spacing = C.tie_case(gy)
    assert W.grid_shape(P.lo, P.hi, spacing) == (64, gy)
    X = W.grid_starts(P, base, 64, gy)
    assert np.array_equal(X[:, :2] * 2 ** 11, np.rint(X[:, :2] * 2 ** 11))
    cs = W.cost(P, X)
    assert np.array_equal(cs, cs[::-1])
    assert np.array_equal(cs.reshape(gy, 64), np.tile(cs[:64], (gy, 1)))
    best, idx, second = W.block_min(cs)
    assert len(best) == gy // 4 and (gy == 64 or len(best) > 1024)
    assert np.array_equal(best, second) and len(set(best.tolist())) == 1
    assert np.array_equal(idx, 256 * np.arange(len(best)) + idx[0]) and idx[0] < 32
    assert not any(b.any() for b in W.branches(P, X))


def test_topk_case_margins():
    """The 16 block minima are distinct by far more than 1e-9 relative, so the top-k order is determined; so is the
    lowest stage-2 cost for every nbest the GPU test uses."""
    P, base, spacing, extra = C.topk_case()
    b = np.clip(base, P.lo, P.hi)
    assert not np.array_equal(b, base)
    gx, gy = W.grid_shape(P.lo, P.hi, spacing)
    best, idx, _ = W.block_min(W.cost(P, W.grid_starts(P, b, gx, gy)))
    assert len(best) == 16
    s = np.sort(best)
    assert (np.diff(s) > 1e-6 * s[1:]).all()
    assert ((extra < P.lo) | (extra > P.hi)).any()
    for nbest in (1, 4, 16, 19):
        take = W.top_blocks(best, idx, nbest)
        starts = np.tile(b, (nbest, 1))
        starts[:len(take), :2] = W.grid_points(P.lo, P.hi, gx, gy)[idx[take]]
        c = np.sort(W.cost(P, W.clamp_start(P, np.concatenate([starts, extra]))))
        c = c[np.concatenate([[True], np.diff(c) != 0])]  # the surplus slots repeat base: an exact tie, by design
        assert c[1] - c[0] > 1e-6 * c[0]


GLOBAL = C.global_cases()


@pytest.mark.parametrize('case', GLOBAL, ids=[c[0] for c in GLOBAL])
def test_global_oracle_is_stable(case):
    """Doubling the oracle's grid density does not lower its minimum; the minimiser is a KKT point; the second case's
    sits on the box edge; the restated two-stage device search reaches the same minimum."""
    name, P = case
    g = C.GLOBAL_GRID
    x, f = W.global_min(P, g, g)
    x2, f2 = W.global_min(P, 2 * g, 2 * g)
    assert f2 >= f * (1 - 1e-12), (f, f2)
    assert W.kkt_residual(P, x) <= 1e-12 * W.grad_scale(P, x)
    assert f > 1e-3
    on_edge = bool(((x[:3] <= P.lo[:3]) | (x[:3] >= P.hi[:3])).any())
    assert on_edge == (name == 'edge')
    width = min(P.hi[0] - P.lo[0], P.hi[1] - P.lo[1])
    gx, gy = W.grid_shape(P.lo, P.hi, min(0.5 * W.TWO_PI / P.k, width / 64))
    X1, f1 = W.device_descent(P, W.grid_starts(P, np.zeros(6), gx, gy), 12, nx=2)
    bb, bi, _ = W.block_min(f1)
    _, fd = W.device_descent(P, X1[bi[W.top_blocks(bb, bi, 64)]], 12)
    assert abs(fd.min() - f) <= 1e-12 * f


def test_scratch_sections_match_the_library():
    """The section offsets add up to the library's own scratch sizes (a layout change fails here, not silently)."""
    import rsl
    lib = rsl.load()
    s = W.solve_sections(lib, 7, 3, 2)
    assert s['J'] == slice(0, 42) and s['Hd'] == slice(42, 78) and s['res'] == slice(78, 78 + 88)
    s = W.search_sections(lib, 7, [-1, -1, 0, 0, 0, 0], [1, 1.5, 0, 0, 0, 0], 0.1, 4, 1)
    nblk = (20 * 25 + 255) // 256
    assert [s[k].stop - s[k].start for k in ('J', 'Hd', 'T', 'base', 'blk', 'starts', 'res')] == \
        [42, 36, 21, 6, 4 * nblk, 30, 40]
    with pytest.raises(AssertionError):
        W._carve(8 * 10, (('a', 4), ('b', 5)))
