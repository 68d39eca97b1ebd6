"""CPU: the numpy oracle of the robust velocity solve (tests/vel_robust_ref.py) against its own definition, and the
host-side surface of the feature (ChainConfig fields, the ctypes row).  The GPU parity is tests/test_gpu_vel_robust.py."""
import numpy as np
import pytest

import vel_robust_ref as R


@pytest.mark.parametrize('share', [0.25, 0.35, 0.45])
def test_oracle_recovers_planted_velocity(share):
    """Tukey with the noise scale given lands within 1e-4 of the planted velocity where plain LS misses it by more than
    1e-3 (the prototype measured 4e-5 or better against 2.5e-3 or worse)."""
    d = R.planted(600, share, noise=0.05, seed=11)
    r = R.robust_frame(d['az'], d['y'], d['m'], k=d['k'], loss='tukey', scale=0.05, iters=30, tol=1e-9)
    err = np.abs(r['x'] - d['v_in']).max()
    err_ls = np.abs(r['ls'] - d['v_in']).max()
    print(f'\nshare {share}: tukey error {err:.2e} after {r["it"]} iterations, LS error {err_ls:.2e}')
    assert r['it'] > 0  # converged
    assert err < 1e-4
    assert err_ls > 1e-3


def test_huber_fixed_point_is_stationary():
    """Huber with a fixed scale is convex: at the oracle's fixed point the gradient of sum m rho(r) vanishes (below
    1e-9 of its value at the LS start), which checks the iteration against the definition of the loss."""
    d = R.planted(600, 0.25, noise=0.05, seed=3)
    c, sigma = 1.345, 0.05
    cs, sn = np.cos(d['az']), np.sin(d['az'])

    def grad(x):  # d/dx sum m rho(r), rho' = 2 r u
        r = d['y'] - d['k'] * (x[0] * cs + x[1] * sn)
        u = R.weights(R.LOSS_HUBER, np.abs(r), c * sigma)
        g = -2.0 * d['k'] * d['m'] * u * r
        return np.array([(g * cs).sum(), (g * sn).sum()])

    r = R.robust_frame(d['az'], d['y'], d['m'], k=d['k'], loss='huber', c=c, scale=sigma, iters=1000, tol=1e-15)
    g0, g1 = np.abs(grad(r['ls'])).max(), np.abs(grad(r['x'])).max()
    print(f'\nhuber: |grad| {g0:.3e} at the LS start, {g1:.3e} after {abs(r["it"])} iterations')
    assert g0 > 0
    assert g1 < 1e-9 * g0
    # and rho' = 2 r u: the numerical derivative of the cost agrees
    x, h = r['ls'], 1e-7
    cost = lambda x: (d['m'] * R.rho(R.LOSS_HUBER, np.abs(d['y'] - d['k'] * (x[0] * cs + x[1] * sn)), c * sigma)).sum()
    num = (cost(x + [h, 0]) - cost(x - [h, 0])) / (2 * h)
    assert abs(num - grad(x)[0]) < 1e-5 * abs(grad(x)[0])


@pytest.mark.parametrize('seed', range(6))
def test_weighted_median_against_expansion(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 40))
    a = np.abs(rng.standard_normal(n)) * 10.0 ** rng.integers(-3, 3)
    a[rng.integers(0, n, 3)] = a[0]  # ties
    m = rng.integers(0, 9, n)
    got = R.weighted_median_f32(a, m)
    full = np.sort(np.repeat(a.astype(np.float32), m))
    if len(full) == 0:
        assert got == 0.0
        return
    want = full[(len(full) + 1) // 2 - 1]  # the smallest value with at least half of the entries at or below it
    assert (full <= want).sum() * 2 >= len(full) and (full < want).sum() * 2 < len(full)
    assert got == float(want)


def test_tukey_rho_and_weight_agree():
    """rho' = 2 r u for both losses, and both rho equal r^2 for small r."""
    t = 0.3
    r = np.linspace(-0.5, 0.5, 2001)
    for loss in (R.LOSS_HUBER, R.LOSS_TUKEY):
        h = 1e-6
        num = (R.rho(loss, np.abs(r + h), t) - R.rho(loss, np.abs(r - h), t)) / (2 * h)
        ana = 2 * r * R.weights(loss, np.abs(r), t)
        assert np.abs(num - ana).max() < 1e-5
        small = np.array([1e-4, -2e-4])
        assert np.allclose(R.rho(loss, np.abs(small), t), small ** 2, rtol=1e-5)


def test_chain_config_velocity_loss():
    import rsl
    assert rsl.ChainConfig().velocity_loss == 'ls'
    cfg = rsl.ChainConfig(velocity_loss='tukey', velocity_scale=0.05)
    assert (cfg.velocity_c, cfg.velocity_iters, cfg.velocity_tol) == (None, 30, 1e-9)
    with pytest.raises(ValueError):
        rsl.ChainConfig(velocity_loss='ransac')


def test_ctypes_row():
    from rsl import _lib
    res, args = _lib.SIGNATURES['rsl_velocity_robust']
    assert len(args) == 21
    assert (_lib.LOSS_HUBER, _lib.LOSS_TUKEY) == (1, 2)
    assert hasattr(_lib.load(), 'rsl_velocity_robust')
