"""The fp64 reference of rsl_scan_register (tests/register_ref.py) is sound: CPU only.

What the reference reaches on the committed scene (test_accuracy_on_the_committed_scene; 600 reflectors, 0.03 m noise,
20 % coherent movers given weight 0, 25 % clutter, start translation off by 0.15 m, the defaults K = 20,
dtheta = 0.25 deg, h_coarse = 1 m, h = 0.5 m, 10 steps, shrink 0.7): yaw within 0.03 deg and translation within
0.02 m of the truth (measured: 8.7e-4 deg and 1.9e-3 m).  The bounds are four standard deviations of the noise's own
effect: a matched pair is off by 0.03 m * sqrt(2) = 0.042 m per coordinate, and about 480 static reflectors match.  The yaw is that over
the rms lever about the centroid (about 17 m) and sqrt(480): 1.1e-4 rad = 6.5e-3 deg.  The translation is
0.042 / sqrt(480) = 2e-3 m plus the yaw error times the centroid's lever (32 m): 4e-3 m together.
"""
import numpy as np
import pytest

import register_ref as R

PAR = {k: v for k, v in R.DEFAULTS.items() if k != 'dt'}


def clouds(sc):
    (q, _), (p, _) = sc['prev'], sc['cur']
    return p[:, 3:5], q[:, 3:5]


@pytest.mark.parametrize('yaw_deg, adv',
                         [(4.5, (1.5, 0.0)), (-3.0, (0.7, -1.2)), (0.0, (0.0, 0.0)), (2.0, (-1.0, 0.9))])
def test_exact_recovery(yaw_deg, adv):
    """A noise-free cloud and its rigidly moved copy are recovered within 1e-9 (fp64 coordinates: the fp32 rounding
    of the point rows is position noise of its own, 4e-6 m at 60 m)."""
    rng = np.random.default_rng(5)
    rho, az = rng.uniform(5, 60, 400), np.radians(rng.uniform(-57, 57, 400))
    Q = np.stack([rho * np.cos(az), rho * np.sin(az)], 1)
    yaw = np.radians(yaw_deg)
    P = np.stack(R.transform_world(Q[:, 0], Q[:, 1], yaw, adv), 1)
    one = np.ones(400)
    # the start translation within 0.2 m of the truth, as the Doppler displacement is
    row = R.register_pair(P, one, Q, one, (0.0, adv[0] - 0.15, adv[1] + 0.1), **{**PAR, 'iters': 40, 'tol': 1e-13})
    assert row[7] == 0
    assert abs(row[0] - yaw) < 1e-9 and abs(row[1] - adv[0]) < 1e-9 and abs(row[2] - adv[1]) < 1e-9


def test_monotone_score():
    """At h_coarse == h no step decreases sum w u a^3 (15 steps, slack 1e-9 relative)."""
    sc = R.scene(np.random.default_rng(11), 500, np.radians(1.3), (0.5, -0.2), noise=0.03, movers=0.2, clutter=0.25)
    P, Q = clouds(sc)
    w, u = sc['static'].astype(float), sc['static_prev'].astype(float)
    tr = {}
    par = {**PAR, 'h': 1.0, 'h_coarse': 1.0, 'iters': 15, 'tol': 0.0}
    R.register_pair(P, w, Q, u, (0.0, 0.4, 0.0), **par, trace=tr)
    s = [R.score(P, w, Q, u, T, 1.0) for T in tr['T']]
    assert len(s) == 16
    for a, b in zip(s, s[1:]):
        assert b >= a * (1 - 1e-9), s
    assert s[-1] > s[0]


def test_convention():
    """A sensor that yawed +2 deg and advanced 0.8 m along its previous x axis: theta = +2 deg, t = (0.8, 0), and the
    yaw rate goes into the previous row of omega."""
    rng = np.random.default_rng(3)
    sc = R.scene(rng, 300, np.radians(2.0), (0.8, 0.0))
    (q, _), (p, _) = sc['prev'], sc['cur']
    pts = np.concatenate([q, p])
    seg = np.array([0, len(q), len(q) + len(p)])
    rows, omega = R.register(pts, seg, init=np.array([[0, 0, 0], [0, 0.7, 0.0]]), dt=0.05)
    assert rows[0, 7] == 2 and not rows[0, :7].any()
    assert rows[1, 7] == 0
    assert abs(np.degrees(rows[1, 0]) - 2.0) < 1e-4          # the fp32 rows: 4e-6 m at up to 60 m
    assert abs(rows[1, 1] - 0.8) < 1e-5 and abs(rows[1, 2]) < 1e-5
    assert omega[0, 2] == rows[1, 0] / 0.05 and not omega[1].any() and not omega[:, :2].any()
    # a static point straight ahead comes closer by the advance
    i = np.argmin(np.abs(q[:, 4]))
    back = R._rot(rows[1, 0], *R.transform_world(q[i, 3], q[i, 4], np.radians(2.0), (0.8, 0.0)))
    assert abs(back[0] + rows[1, 1] - q[i, 3]) < 1e-4 and abs(back[1] + rows[1, 2] - q[i, 4]) < 1e-4


def _errors(row, truth):
    return abs(np.degrees(row[0] - truth[0])), float(np.hypot(row[1] - truth[1], row[2] - truth[2]))


@pytest.mark.parametrize('seed', [17, 18, 19])
def test_weights_matter(seed):
    """25 % coherent movers (all displaced by (0.2, -0.15) m, inside the kernel's radius, so they pull), once with
    weight 0 and once with weight 1: the first run is closer to the truth, in translation (what a common displacement
    corrupts: by about a quarter of 0.25 m times the movers' kernel weight) and in the pose error at the scene's mean
    lever of 30 m."""
    sc = R.scene(np.random.default_rng(seed), 600, np.radians(1.0), (0.6, 0.1), noise=0.03, movers=0.25,
                 mover_shift=(0.2, -0.15))
    P, Q = clouds(sc)
    init = (0.0, 0.5, 0.0)
    masked = R.register_pair(P, sc['static'].astype(float), Q, sc['static_prev'].astype(float), init, **PAR)
    blind = R.register_pair(P, np.ones(len(P)), Q, np.ones(len(Q)), init, **PAR)
    (a0, t0), (a1, t1) = _errors(masked, sc['truth']), _errors(blind, sc['truth'])
    assert masked[7] == 0 and blind[7] == 0
    assert t0 < t1 and t0 + 30 * np.radians(a0) < t1 + 30 * np.radians(a1), (a0, t0, a1, t1)
    assert t1 > 0.02 > t0


def test_accuracy_on_the_committed_scene():
    """See the module docstring for the figures and where the bounds come from."""
    sc = R.scene(np.random.default_rng(23), 600, np.radians(2.6), (0.9, -0.15), noise=0.03, movers=0.2, clutter=0.25)
    P, Q = clouds(sc)
    row = R.register_pair(P, sc['static'].astype(float), Q, sc['static_prev'].astype(float), (0.0, 0.75, -0.15), **PAR)
    a, t = _errors(row, sc['truth'])
    print(f'yaw error {a:.2e} deg, translation error {t:.2e} m, W {row[3]:.1f}, rms {row[4]:.3f}, steps {row[6]:.0f}')
    assert row[7] == 0
    assert a < 0.03 and t < 0.02


def test_degenerate_inputs():
    sc = R.scene(np.random.default_rng(2), 50, 0.01, (0.1, 0.0))
    (q, _), (p, _) = sc['prev'], sc['cur']
    far = p.copy()
    far[:, 3] += 500.0  # no overlap with q
    pts = np.concatenate([q, p[:0], p, far])
    seg = np.cumsum([0, len(q), 0, len(p), len(far)])
    init = np.array([[0, 0, 0], [0.01, 0.2, 0.3], [0.02, 0.1, 0.0], [0.03, 0.4, -0.5]])
    rows, omega = R.register(pts, seg, init=init)
    assert rows[0, 7] == 2 and not rows[0, :7].any()                  # no prev
    for f in (1, 2, 3):  # an empty frame, an empty reference, no overlap: flag 1, the start values kept
        assert rows[f, 7] == 1 and (rows[f, :3] == init[f]).all() and not rows[f, 3:7].any()
    assert (omega[:3, 2] == init[1:, 0] / R.DEFAULTS['dt']).all() and not omega[3].any()
    # too little support in the fine stage: flag 1 as well, theta at the coarse winner
    rows, _ = R.register(np.concatenate([q, p]), np.array([0, len(q), len(q) + len(p)]), w_min=1e6)
    assert rows[1, 7] == 1 and rows[1, 6] == 0 and rows[1, 3] > 0
    # a segment end past n is clamped, a NaN point and a weight <= 0 count as absent
    both = np.concatenate([q, p])
    ref, _ = R.register(both, np.array([0, len(q), len(both)]))
    got, _ = R.register(both, np.array([0, len(q), len(both) + 1000]))
    assert (got == ref).all()
    w = np.ones(len(both), np.float32)
    w[len(q) + 3], w[len(q) + 4] = 0.0, -2.0
    bad = both.copy()
    bad[len(q) + 5, 4] = np.nan
    keep = np.ones(len(both), bool)
    keep[len(q) + 3:len(q) + 6] = False
    got, _ = R.register(bad, np.array([0, len(q), len(both)]), weight=w)
    ref, _ = R.register(both[keep], np.array([0, len(q), len(both) - 3]))
    assert (got == ref).all()


def test_culling_keeps_the_support():
    """The row windows of the header leave every pair of the kernel's support, at every pose and radius the reference
    visits on the GPU case list: equality of the pair sets, and the windows do cut (fewer pairs are tested)."""
    c = R.gpu_case()
    pts, rc, seg = c['points'], c['rc'], c['seg']
    w = R.effective_weight(pts, c['weight'])
    pw = R.effective_weight(c['prev']['points'], c['prev']['weight'])
    pairs = {0: (pts[seg[0]:seg[1]], w[seg[0]:seg[1]], c['prev']['points'], pw, c['prev']['rc']),
             3: (pts[seg[3]:seg[4]], w[seg[3]:seg[4]], pts[seg[2]:seg[3]], w[seg[2]:seg[3]], rc[seg[2]:seg[3]])}
    for f, (P, wp, Q, uq, qrc) in pairs.items():
        assert (np.diff(qrc) >= 0).all()
        tr = {}
        R.register_pair(P[:, 3:5], wp, Q[:, 3:5], uq, tuple(c['init'][f]), **PAR, trace=tr)
        poses = list(zip(tr['T'][:-1], tr['h']))
        th0, tx, ty = c['init'][f]
        poses += [((th0 + k * PAR['dtheta'], tx, ty), PAR['h_coarse']) for k in (-20, -7, 0, 6, 20)]
        assert len(poses) >= 7
        for T, h in poses:
            dense, culled = R.pair_sets(P[:, 3:5], wp, Q[:, 3:5], uq, qrc, T, float(h))
            assert dense == culled
        assert len(dense) > 0
    # the windows do cut: 2 h / r_step rows, the two the interval touches at its ends and the two extra ones
    lo, hi = R.window_rows(np.array([30.0]), 0.5)
    assert 1.0 / R.AXES[1] + 2 <= hi[0] - lo[0] + 1 <= 1.0 / R.AXES[1] + 4
