"""fp64 numpy oracle of non-coherent integration (rsl_power_integrate) and of the three detection rules on a power map
(rsl_detect_power) (helper, not collected).

integrate() is the exact sum of the per-antenna fp64 powers.  reference_power() is the body of cfar_ref.reference on a
given fp64 power map instead of the power of a complex map -- the same training sums, order statistic, 3x3 rule, gate,
floor and tolerance bands, taken from cfar_ref and parity; test_nci_host.py pins it to cfar_ref.reference.  The GPU tests
hand it the fp64 cast of the very power map the detector read, so only the detector is under test.

method 'threshold' is rsl_detect's rule: no level (level = -inf, nothing is near it), the floor p > thr_power is the
threshold.
"""
import numpy as np

import cfar_cases as K
import cfar_ref as R
import parity as P

diff = R.diff
near_cap = R.near_cap
mask_bool = R.mask_bool


def integrate(rds):
    """rds c64 [..., A, S, C] -> the fp64 sum of cfar_ref.power over the antenna axis [..., S, C]."""
    return R.power(rds).sum(axis=-3)


def reference_power(p, window, alpha, *, method='ca', rank=0.75, thr_power=-1.0, gate=(0, 1 << 30)):
    """Returns dict(mask bool, p, level, nbmax, near bool[, n][, k]) for the power map p f64 [..., S, C]; method 'ca',
    'os' (rank) or 'threshold' (window, alpha and rank ignored)."""
    p = np.asarray(p, dtype=np.float64)
    S = p.shape[-2]
    extra = {}
    if method == 'os':
        xk, extra['n'], extra['k'] = R.order_statistic(p, window, rank)
        level = alpha * xk
    elif method == 'ca':
        s, extra['n'] = R.training_sum(p, window)
        level = alpha * s / extra['n'][:, None]
    elif method == 'threshold':
        level = np.full_like(p, -np.inf)
    else:
        raise ValueError(method)
    nb = R.neighbour_max(p)
    g = np.zeros(S, bool)
    g[max(gate[0], 0):min(gate[1], S - 1) + 1] = True
    mask = (p > level) & (p >= nb) & g[:, None]
    if thr_power >= 0:
        mask &= p > thr_power
    if method == 'threshold':
        near_lvl = np.zeros(p.shape, bool)
    else:
        near_lvl = np.abs(p - level) <= R.LEVEL_RTOL[method] * level
    near_max = np.abs(p - nb) <= P.PEAK_RTOL * np.maximum(p, nb)
    could_max = (p >= nb) | near_max
    could_lvl = (p > level) | near_lvl
    near = (near_lvl | near_max) & could_max & could_lvl & g[:, None]
    if thr_power >= 0:
        near &= p > thr_power
    return dict(mask=mask, p=p, level=level, nbmax=nb, near=near, **extra)


def motivating_scene():
    """[1, 8, 128, 64] unit noise with 54 reflectors of amplitude 2.0 (6 dB per antenna) and their cells."""
    z = K.noise((1, 8, 128, 64), 7)
    rng = np.random.default_rng(8)
    cells = [(i, j) for i in range(16, 120, 12) for j in range(6, 60, 9)]
    for i, j in cells:
        th = rng.uniform(-1, 1)
        ph = rng.uniform(0, 2 * np.pi)
        z[0, :, i, j] += (2.0 * np.exp(1j * (ph + np.pi * np.arange(8) * th))).astype(np.complex64)
    return z, cells
