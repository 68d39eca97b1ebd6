"""The inputs the wrapped-solver tests share (test_wrap_host.py states every margin the GPU tests in
test_gpu_wrap_stages.py rely on, on these same inputs).  Plain numpy; everything is seeded."""
import numpy as np

import aux_ref
import wrap_ref as W

K77 = 4 * np.pi * 0.1 / (3e8 / 77e9)   # 77 GHz, dt 0.1 s: ~322.5 rad s / m, wrap period 2 pi / k = 19.5 mm/s
KPIPE = 4 * np.pi * 0.1 / (77e9 / 3e8)  # the pipeline's lambda = fc / c (run_ego_motion_pipeline.py:246): ~0.0049


def planar(rs, n, az_lo=-0.2, az_hi=1.2, rmax=80.0):
    """The reference's own targets: elevation 0, p = r d, so only J's columns 0 and 1 are live."""
    az = rs.uniform(az_lo, az_hi, n)
    r = rs.uniform(1.0, rmax, n)
    return np.stack([r * np.cos(az), r * np.sin(az), np.zeros(n)], axis=1), np.stack([az, np.zeros(n)], axis=1)


def general(rs, n, scale=1.0):
    """Positions off the line of sight and elevations up to 0.3 rad: all six columns of J are live."""
    pos = rs.randn(n, 3) * scale
    return pos, np.stack([rs.uniform(-1.2, 1.2, n), rs.uniform(-0.3, 0.3, n)], axis=1)


def _one_piece(pos, ang, k, xt, half, noise, rs, **kw):
    """A problem whose whole box xt +- half lies in one piece of the wrapped cost (one_piece_margin > 0 states it):
    y = wrap(k J xt + noise)."""
    J = aux_ref.jacobian(pos, ang)
    y = W.wrap(k * (J @ xt) + noise * rs.randn(len(pos)))
    return W.Problem(pos, ang, y, k, lo=xt - half, hi=xt + half, **kw)


def one_piece_margin(P):
    """pi - max_i (|r_i(c)| + k sum_a |J_ia| h_a), c and h the box's centre and half-widths over the first nv
    coordinates (the others are 0): positive when no residual reaches a wrap discontinuity anywhere in the box, so the
    cost is one convex quadratic (mode 0) over it."""
    c, h = 0.5 * (P.lo + P.hi), 0.5 * (P.hi - P.lo)
    c[P.nv:], h[P.nv:] = 0.0, 0.0
    c = np.minimum(np.maximum(c, P.lo), P.hi)
    return float(np.pi - (np.abs(W.residuals(P, c)[0]) + P.k * (np.abs(P.J) @ h)).max())


def active_cases():
    """Box-constrained problems whose minimiser has active bounds, each a dict: name, P, start [6], active (the number
    of bounds active at the minimiser), spacing and nbest for rsl_wrapped_search.  Mode 0.  Four are the
    cases the stall at a bound was first shown on (nv 3; 6 and 20 planar targets, azimuths uniform in [-0.2, 1.2]; k =
    1 and 77 GHz; hi[0] below the true v_x); then a lower-bound twin of each, a two-bound corner, an nv = 6 case and a collapsed axis."""
    out = []

    def add(name, P, active, start=None):
        c = 0.5 * (P.lo + P.hi)
        out.append(dict(name=name, P=P, start=c if start is None else start, active=active,
                        spacing=float((P.hi[:2] - P.lo[:2]).max()) / 7.5, nbest=4))

    for k, tag, xt, half, cut in ((1.0, 'k1', np.array([1.0, 0.5, 0, 0, 0, 0.0]), 1.0, 0.4),
                                  (K77, 'k77', np.array([0.012, 0.006, 0, 0, 0, 0.0]), 0.004, 0.003)):
        for n in (6, 20):
            for sign in (1, -1):  # -1: the lower-bound twin (the mirrored problem)
                rs = np.random.RandomState(100 + n)
                pos, ang = planar(rs, n)
                P = _one_piece(pos, ang, k, sign * xt, np.full(6, half), 0.01, rs)
                if sign > 0:
                    P.hi[0] = xt[0] - cut
                else:
                    P.lo[0] = -xt[0] + cut
                add(f'{tag}_n{n}_{"hi" if sign > 0 else "lo"}', P, 1, start=sign * xt)
    rs = np.random.RandomState(7)
    pos, ang = general(rs, 12)  # elevations off 0: v_z is coupled to the two coordinates on their bounds
    xt = np.array([0.6, 0.4, 0.3, 0, 0, 0.0])
    P = _one_piece(pos, ang, 1.0, xt, np.full(6, 0.6), 0.01, rs)
    P.hi[0], P.hi[1] = xt[0] - 0.3, xt[1] - 0.1
    add('corner', P, 2, start=xt)
    rs = np.random.RandomState(8)
    pos, ang = general(rs, 20)
    xt = np.array([0.4, -0.3, 0.2, 0.1, -0.15, 0.2])
    P = _one_piece(pos, ang, 1.0, xt, np.full(6, 0.25), 0.01, rs, nv=6)
    P.hi[0], P.lo[4] = xt[0] - 0.1, xt[4] + 0.08
    add('nv6', P, 2, start=xt)
    rs = np.random.RandomState(9)
    pos, ang = general(rs, 10)
    xt = np.array([0.6, 0.4, 0.3, 0, 0, 0.0])
    P = _one_piece(pos, ang, 1.0, xt, np.full(6, 0.6), 0.01, rs)
    P.hi[0] = xt[0] - 0.3
    P.lo[1] = P.hi[1] = xt[1] + 0.2  # collapsed: v_y is given
    add('collapsed', P, 2)
    return out


def bvls_of(P):
    """scipy's BVLS on the unwrapped problem of a one-piece mode-0 case: y unwrapped about the box centre.
    (x [nv], cost)."""
    c = 0.5 * (P.lo + P.hi)
    c[P.nv:] = 0.0
    yu = P.k * (P.J @ c) + W.residuals(P, c)[0]
    A = P.k * P.J[:, :P.nv]
    lo, hi = P.lo[:P.nv], P.hi[:P.nv]
    var = lo < hi  # scipy wants lo < hi: a collapsed coordinate goes to the right-hand side
    x = lo.copy()
    x[var], f, _ = aux_ref.bvls_ref(A[:, var], yu - A[:, ~var] @ lo[~var], lo[var], hi[var], 0.01)
    return x, f + 0.01 * float(np.sum(lo[~var] ** 2))


def jac_case(n):
    """n targets with all six Jacobian columns live; |p| <~ 1, so that every entry of J is below ~1 and one ulp of it
    ~1e-16."""
    rs = np.random.RandomState(1000 + n)
    pos, ang = general(rs, n, scale=0.3)
    y = rs.uniform(-3, 3, n)
    return W.Problem(pos, ang, y, K77, nv=6)


ADV_BOX = dict(lo=[-50, -50, -10, -10, -10, -10], hi=[50, 50, 10, 10, 10, 10])


def cost_points():
    """(name, x6) in every reachable combination of Advanced's branches (vm > 40, wm > 8, vm > 20 and wm > 5), for
    vmax 50, wmax 10 and the +-50 / +-10 box.  vm > 40 and wm > 8 together imply the third; the other six
    combinations of the first two with the third on or off are all here."""
    v = lambda m: np.array([0.8, 0.56, 0.2]) / np.linalg.norm([0.8, 0.56, 0.2]) * m
    w = lambda m: np.array([0.5, -0.6, 0.62]) / np.linalg.norm([0.5, -0.6, 0.62]) * m
    pts = [('none', 3, 1), ('cross', 30, 6), ('v', 45, 3), ('v_cross', 45, 6), ('w', 10, 9), ('w_cross', 30, 9),
           ('v_w_cross', 45, 9)]
    return [(name, np.concatenate([v(a), w(b)])) for name, a, b in pts]


def cost_problem(mode, nv, prev):
    rs = np.random.RandomState(31)
    pos, ang = general(rs, 9, scale=20.0)
    y = rs.uniform(-3, 3, 9)
    return W.Problem(pos, ang, y, KPIPE, mode=mode, nv=nv, prev=prev, **ADV_BOX)


PREV = np.array([12.0, -5.0, 1.0, 0.5, -0.25, 2.0])


def one_step_problem(mode, nv):
    """A no-wrap quadratic with no bound active: one Newton step from ONE_STEP_START reaches its minimiser.  Mode 1
    has only its quadratic terms live (prev and v_z): the norms stay far below every threshold.  k = 2, so that k and
    k^2 differ, and the start is off 0, so that every term of the regulariser's gradient is live."""
    rs = np.random.RandomState(40 + nv + mode)
    pos, ang = general(rs, 20)
    xt = np.array([0.25, -0.2, 0.15, 0.1, -0.15, 0.125])
    xt[nv:] = 0.0
    y = W.wrap(2.0 * (aux_ref.jacobian(pos, ang) @ xt) + 0.02 * rs.randn(20))
    prev = np.array([0.15, -0.1, 0.05, 0.05, -0.05, 0.1]) if mode else None
    return W.Problem(pos, ang, y, 2.0, mode=mode, nv=nv, lo=np.full(6, -2.0), hi=np.full(6, 2.0), prev=prev, w=0.5)


ONE_STEP_START = np.array([0.05, -0.03, 0.08, 0.03, -0.08, 0.02])


def one_step_exact(P):
    """The minimiser of one_step_problem by least squares: rows k J, plus sqrt of each quadratic penalty."""
    nv = P.nv
    rows, rhs = [P.k * P.J[:, :nv]], [P.y]
    if P.mode == 0:
        rows.append(np.sqrt(0.01) * np.eye(nv))
        rhs.append(np.zeros(nv))
    else:
        rows.append(np.sqrt(0.1 * P.w) * np.eye(nv))
        rhs.append(np.sqrt(0.1 * P.w) * P.prev[:nv])
        e = np.zeros((1, nv))
        e[0, 2] = np.sqrt(10.0 * P.w)
        rows.append(e)
        rhs.append(np.zeros(1))
    x = np.zeros(6)
    x[:nv] = np.linalg.lstsq(np.concatenate(rows), np.concatenate(rhs), rcond=None)[0]
    return x


ADV_ITERS = 20


def advanced_descent_problem():
    """No wrap (the pipeline's small k), every norm penalty of Advanced mode active at the minimiser."""
    rs = np.random.RandomState(51)
    pos, ang = general(rs, 20, scale=20.0)
    xt = np.array([42.0, 15.0, 0.5, 6.0, 5.0, 3.0])
    y = KPIPE * (aux_ref.jacobian(pos, ang) @ xt) + 0.01 * rs.randn(20)
    P = W.Problem(pos, ang, y, KPIPE, mode=1, nv=6, prev=xt + np.array([1.0, -1.0, 0.2, 0.3, -0.2, 0.1]), **ADV_BOX)
    return P, xt


def stage1_cases():
    """(name, P, base6, spacing, (gx, gy)) for stage 1 with iters = 0: grids 1 x 1, 19 x 23 (a partial last block),
    64 x 64, and a collapsed v_y axis (one point on it)."""
    rs = np.random.RandomState(61)
    pos, ang = general(rs, 7, scale=5.0)
    y = rs.uniform(-3, 3, 7)
    base = np.array([9.0, 9.0, 0.3, 0.02, -0.03, 0.05])  # [0], [1] are overwritten by the grid
    out = []
    for name, lo, hi, mode, shape in (('1x1', (-0.4, 0.1), (0.3, 0.9), 0, (1, 1)),
                                      ('19x23', (-9.0, -11.5), (9.5, 11.0), 1, (19, 23)),
                                      ('64x64', (-32.0, -31.0), (31.5, 32.5), 0, (64, 64)),
                                      ('collapsed', (-9.0, 0.25), (9.5, 0.25), 1, (19, 1))):
        P = W.Problem(pos, ang, y, 1.0, mode=mode, nv=6, lo=[lo[0], lo[1], -1, -1, -1, -1],
                      hi=[hi[0], hi[1], 1, 1, 1, 1], prev=PREV * 0.1 if mode else None)
        out.append((name, P, base, 1.0, shape))
    return out


def tie_case(gy=64):
    """Exact ties (gy = 64; gy = 4100 makes 1025 blocks, so that the top-k's first thread meets two equal blocks, 0
    and 1024, in its own stripe; the v_y box is then [-2^-5, -2^-5 + gy 2^-10]): y = 0, every target at azimuth 0 (the cost does not depend on v_y: mode 1 without prev has no v_y
    term below its thresholds), box +-2^-5 on both axes, spacing 2^-10: a 64 x 64 grid whose points are exact, whose
    rows are bit-equal to each other and whose columns ix and 63 - ix are bit-equal.  The minimum is at one ix < 32
    and its mirror in every row (where k v_x is nearest a multiple of 2 pi): the lower ix of the first row of a block
    must win the block, and the top-k must take the 16 equal blocks in their order."""
    n = 5
    r = np.array([3.0, 10.0, 22.0, 41.0, 77.0])
    pos = np.stack([r, np.zeros(n), np.zeros(n)], axis=1)
    P = W.Problem(pos, np.zeros((n, 2)), np.zeros(n), K77, mode=1, nv=3, lo=[-2.0 ** -5, -2.0 ** -5, -1, -1, -1, -1],
                  hi=[2.0 ** -5, -2.0 ** -5 + gy * 2.0 ** -10, 1, 1, 1, 1])
    return P, np.zeros(6), 2.0 ** -10


def topk_case():
    """The 64 x 64 stage-1 case (16 blocks) with two extra starts, one outside the box, and a base outside the box."""
    name, P, base, spacing, shape = stage1_cases()[2]
    base = base.copy()
    base[2], base[5] = 1.5, -3.0  # clipped to 1 and -1
    extra = np.array([[1.0, -2.0, 0.1, 0.0, 0.1, 0.0], [40.0, 0.5, -2.0, 0.3, 0.0, 0.0]])
    return P, base, spacing, extra


def many_starts_problem():
    """77 GHz, 8 planar targets, the +-2 m/s box of the Improved solver: a glassy landscape for the descents of a
    33 x 33 or 17 x 17 grid."""
    rs = np.random.RandomState(71)
    pos, ang = planar(rs, 8, -1.2, 1.2)
    xt = np.array([0.7, -0.3, 0.0])
    y = W.wrap(K77 * (aux_ref.jacobian(pos, ang)[:, :3] @ xt) + 0.05 * rs.randn(8))
    return W.Problem(pos, ang, y, K77, lo=np.full(6, -2.0), hi=np.full(6, 2.0))


GLOBAL_GRID = 48  # the oracle's starts per axis over the +-0.03 box (2.4 wrap periods wide)


def global_cases():
    """(name, P): k = 322.5, n = 8, box +-0.03 m/s, mode 0, nv = 3; and the same data with hi[0] cut to 2 mm/s below the
    first case's minimiser, so that the global minimum of the second sits on the box edge."""
    rs = np.random.RandomState(81)
    pos, ang = planar(rs, 8, -1.2, 1.2)
    xt = np.array([0.011, -0.007, 0.0])
    y = W.wrap(K77 * (aux_ref.jacobian(pos, ang)[:, :3] @ xt) + 0.1 * rs.randn(8))
    P = W.Problem(pos, ang, y, K77, lo=np.full(6, -0.03), hi=np.full(6, 0.03))
    x, _ = W.global_min(P, GLOBAL_GRID, GLOBAL_GRID)
    Q = W.Problem(pos, ang, y, K77, lo=np.full(6, -0.03), hi=np.full(6, 0.03))
    Q.hi[0] = x[0] - 0.002
    return [('inside', P), ('edge', Q)]
