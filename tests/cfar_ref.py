"""fp64 numpy CA-CFAR oracle and comparator for rsl_detect_cfar (helper, not collected).

The rule is the one documented in include/rsl.h.  With guard (gr, gd) and training (tr, td) half-sizes, hr = gr + tr,
hd = gd + td, the training cells of (i, j) are the offsets |di| <= hr, |dj| <= hd without the guard box |di| <= gr,
|dj| <= gd; Doppler wraps, range truncates, the mean divides by the cells that exist.  A cell is a peak iff
p > alpha * mean (strict), p >= every existing 3x3 neighbour (no wrap), i_lo <= i <= i_hi and p > thr_power
(thr_power < 0: no floor).

The oracle takes the fp64 power of the complex64 RDS it is handed -- always the RDS the GPU produced or was given --
so only the detector is under test.

Tolerances:
* CFAR_RTOL = 1e-4 on |p - alpha mean| relative to alpha mean: the kernel's training sum is at most 33 * 33 - 1 = 1088
  fp32 additions of non-negative terms, worst-case relative error 1088 * 2^-24 = 6.5e-5, plus a few roundings of the
  comparison itself.
* parity.PEAK_RTOL on |p - max_neighbour| relative to the larger of the two (the 3x3 test, as parity.peak_diff).
* near_cap: the tolerance may explain at most max(2, 1e-4 * cells) reference cells; asserted on the reference alone.
"""
import numpy as np

import parity as P

CFAR_RTOL = 1e-4


def power(rds):
    z = np.asarray(rds)
    return z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2


def training_sum(p, window):
    """p f64 [..., S, C] -> (sum over the training cells [..., S, C], n f64 [S]); double loop over the offsets,
    np.roll on Doppler, index mask on range."""
    gr, gd, tr, td = window
    hr, hd = gr + tr, gd + td
    S = p.shape[-2]
    rows = np.arange(S)
    s = np.zeros_like(p)
    n = np.zeros(S)
    for di in range(-hr, hr + 1):
        src = rows + di
        ok = (src >= 0) & (src < S)
        for dj in range(-hd, hd + 1):
            if abs(di) <= gr and abs(dj) <= gd:
                continue
            sh = np.roll(p, -dj, axis=-1)  # sh[..., j] = p[..., (j + dj) mod C]
            s[..., rows[ok], :] += sh[..., src[ok], :]
            n += ok
    return s, n


def neighbour_max(p):
    """Largest existing 3x3 neighbour (no wrap), per map; p [..., S, C]."""
    q = p.reshape((-1,) + p.shape[-2:])
    return P._neighbour_max(q).reshape(p.shape)


def cfar_reference(rds, window, alpha, *, thr_power=-1.0, gate=(0, 1 << 30)):
    """Returns dict(mask bool, p, level = alpha * mean, nbmax, near bool) for rds c64 [..., S, C]."""
    p = power(rds)
    S = p.shape[-2]
    s, n = training_sum(p, window)
    level = alpha * s / n[:, None]
    nb = neighbour_max(p)
    g = np.zeros(S, bool)
    g[max(gate[0], 0):min(gate[1], S - 1) + 1] = True
    mask = (p > level) & (p >= nb) & g[:, None]
    if thr_power >= 0:
        mask &= p > thr_power
    near_lvl = np.abs(p - level) <= CFAR_RTOL * level
    near_max = np.abs(p - nb) <= P.PEAK_RTOL * np.maximum(p, nb)
    # a band decides something only where the other test passes or is itself inside its band (an all-zero row, e.g.
    # the DC range bin, ties with its neighbours everywhere but never reaches its level)
    could_max = (p >= nb) | near_max
    could_lvl = (p > level) | near_lvl
    near = (near_lvl | near_max) & could_max & could_lvl & g[:, None]
    if thr_power >= 0:
        near &= p > thr_power
    return dict(mask=mask, p=p, level=level, nbmax=nb, near=near)


def near_cap(cells):
    return max(2, int(1e-4 * cells))


def cfar_diff(gpu_mask, ref):
    """gpu_mask bool like ref['mask'].  Returns (n_gpu, n_ref, n_diff, n_unexplained): a differing cell is explained
    only inside the CFAR_RTOL band of its level or the PEAK_RTOL band of its largest neighbour."""
    diff = gpu_mask ^ ref['mask']
    unexpl = diff & ~ref['near']
    return int(gpu_mask.sum()), int(ref['mask'].sum()), int(diff.sum()), int(unexpl.sum())


def mask_bool(words, C):
    """u64 / i64 mask words [..., W] -> bool [..., C]."""
    w = np.ascontiguousarray(words)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape + (8,)), axis=-1, bitorder='little')
    return bits.reshape(w.shape[:-1] + (w.shape[-1] * 64,))[..., :C].astype(bool)


def brute_force(p, window, alpha):
    """Per-cell loop of the same rule on one map p f64 [S, C] (no gate, no floor): the check of the oracle itself."""
    gr, gd, tr, td = window
    hr, hd = gr + tr, gd + td
    S, C = p.shape
    out = np.zeros((S, C), bool)
    for i in range(S):
        for j in range(C):
            tot, n = 0.0, 0
            for di in range(-hr, hr + 1):
                if not 0 <= i + di < S:
                    continue
                for dj in range(-hd, hd + 1):
                    if abs(di) <= gr and abs(dj) <= gd:
                        continue
                    tot += p[i + di, (j + dj) % C]
                    n += 1
            ok = p[i, j] > alpha * tot / n
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (di or dj) and 0 <= i + di < S and 0 <= j + dj < C:
                        ok = ok and p[i, j] >= p[i + di, j + dj]
            out[i, j] = ok
    return out
