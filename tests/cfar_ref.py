"""fp64 numpy oracle and comparator of the CFAR detectors rsl_detect_cfar ('ca') and rsl_detect_oscfar ('os') (helper,
not collected).

The rules are the ones documented in include/rsl.h.  With guard (gr, gd) and training (tr, td) half-sizes, hr = gr + tr,
hd = gd + td, the training cells of (i, j) are the offsets |di| <= hr, |dj| <= hd without the guard box |di| <= gr,
|dj| <= gd; Doppler wraps, range truncates, n(i) cells exist for range row i.  A cell is a peak iff p > level (strict),
p >= every existing 3x3 neighbour (no wrap), i_lo <= i <= i_hi and p > thr_power (thr_power < 0: no floor), where
* 'ca': level = alpha * mean of the training cells (the mean divides by the cells that exist);
* 'os': level = alpha * x_(k(i)), the k-th smallest training power, k(i) = min(n(i), max(1, ceil(rank * n(i)))).  The
  oracle gathers the training cells of a block of range rows, orders them and takes x_(k) -- the kernel never orders
  anything, it counts the cells below p / alpha.

The oracle takes the fp64 power of the complex64 RDS it is handed -- always the RDS the GPU produced or was given --
so only the detector is under test.

Tolerances:
* CFAR_RTOL = 1e-4 on |p - alpha mean| relative to alpha mean: the kernel's training sum is at most 33 * 33 - 1 = 1088
  fp32 additions of non-negative terms, worst-case relative error 1088 * 2^-24 = 6.5e-5, plus a few roundings of the
  comparison itself.
* OS_RTOL = 1e-6 on |p - level| relative to level = alpha x_(k): both sides carry the rounding of the kernel's fp32
  power, at most 3 * 2^-24 each (two squares and a sum); an order statistic moves by no more than its inputs do;
  (float)alpha and the fp32 product add 2^-24 each.  The sum, 8 * 2^-24, is below 5e-7.
* parity.PEAK_RTOL on |p - max_neighbour| relative to the larger of the two (the 3x3 test, as parity.peak_diff).
* near_cap: the tolerance may explain at most max(2, 1e-4 * cells) reference cells; asserted on the reference alone.
"""
import math

import numpy as np

import parity as P

CFAR_RTOL = 1e-4
OS_RTOL = 1e-6
LEVEL_RTOL = {'ca': CFAR_RTOL, 'os': OS_RTOL}


def power(rds):
    z = np.asarray(rds)
    return z.real.astype(np.float64) ** 2 + z.imag.astype(np.float64) ** 2


def training_offsets(window):
    gr, gd, tr, td = window
    hr, hd = gr + tr, gd + td
    return [(di, dj) for di in range(-hr, hr + 1) for dj in range(-hd, hd + 1)
            if not (abs(di) <= gr and abs(dj) <= gd)]


# -- the two levels ---------------------------------------------------------------------------------------
def training_sum(p, window):
    """p f64 [..., S, C] -> (sum over the training cells [..., S, C], n f64 [S]); loop over the offsets, np.roll on
    Doppler, index mask on range."""
    S = p.shape[-2]
    rows = np.arange(S)
    s = np.zeros_like(p)
    n = np.zeros(S)
    for di, dj in training_offsets(window):
        src = rows + di
        ok = (src >= 0) & (src < S)
        sh = np.roll(p, -dj, axis=-1)  # sh[..., j] = p[..., (j + dj) mod C]
        s[..., rows[ok], :] += sh[..., src[ok], :]
        n += ok
    return s, n


def rank_of(n, rank):
    """k(i) of the header, in fp64."""
    return min(int(n), max(1, int(math.ceil(rank * float(n)))))


def order_statistic(p, window, rank, block_bytes=64 << 20):
    """p f64 [..., S, C] -> (x_(k(i)) of every cell's training cells [..., S, C], n i64 [S], k i64 [S]); range rows
    in blocks of at most block_bytes of gathered training cells."""
    offs = training_offsets(window)
    S, Cn = p.shape[-2:]
    q = p.reshape((-1, S, Cn))
    rows = np.arange(S)
    n = np.zeros(S, np.int64)
    for di, _ in offs:
        n += (rows + di >= 0) & (rows + di < S)
    k = np.array([rank_of(v, rank) for v in n])
    out = np.empty_like(q)
    nb = max(1, int(block_bytes // (8 * q.shape[0] * Cn * len(offs))))
    cols = np.arange(Cn)
    for r0 in range(0, S, nb):
        r1 = min(S, r0 + nb)
        g = np.full((q.shape[0], r1 - r0, Cn, len(offs)), np.inf)  # a cell that does not exist is never the k-th
        for t, (di, dj) in enumerate(offs):
            src = np.arange(r0, r1) + di
            ok = (src >= 0) & (src < S)
            g[..., t][:, ok] = q[:, src[ok]][:, :, (cols + dj) % Cn]
        kk = k[r0:r1] - 1
        g = np.partition(g, np.unique(kk).tolist(), axis=-1)  # the k-th smallest in place for every k of the block
        out[:, r0:r1] = np.take_along_axis(g, kk[None, :, None, None], axis=-1)[..., 0]
    return out.reshape(p.shape), n, k


# -- the rule ---------------------------------------------------------------------------------------------
def neighbour_max(p):
    """Largest existing 3x3 neighbour (no wrap), per map; p [..., S, C]."""
    q = p.reshape((-1,) + p.shape[-2:])
    return P._neighbour_max(q).reshape(p.shape)


def reference(rds, window, alpha, *, method='ca', rank=0.75, thr_power=-1.0, gate=(0, 1 << 30)):
    """Returns dict(mask bool, p, level, nbmax, near bool, n[, k]) for rds c64 [..., S, C]; rank: 'os' only."""
    p = power(rds)
    S = p.shape[-2]
    extra = {}
    if method == 'os':
        xk, n, extra['k'] = order_statistic(p, window, rank)
        level = alpha * xk
    else:
        s, n = training_sum(p, window)
        level = alpha * s / n[:, None]
    nb = neighbour_max(p)
    g = np.zeros(S, bool)
    g[max(gate[0], 0):min(gate[1], S - 1) + 1] = True
    mask = (p > level) & (p >= nb) & g[:, None]
    if thr_power >= 0:
        mask &= p > thr_power
    near_lvl = np.abs(p - level) <= LEVEL_RTOL[method] * level
    near_max = np.abs(p - nb) <= P.PEAK_RTOL * np.maximum(p, nb)
    # a band decides something only where the other test passes or is itself inside its band (an all-zero row, e.g.
    # the DC range bin, ties with its neighbours everywhere but never reaches its level)
    could_max = (p >= nb) | near_max
    could_lvl = (p > level) | near_lvl
    near = (near_lvl | near_max) & could_max & could_lvl & g[:, None]
    if thr_power >= 0:
        near &= p > thr_power
    return dict(mask=mask, p=p, level=level, nbmax=nb, near=near, n=n, **extra)


def near_cap(cells):
    return max(2, int(1e-4 * cells))


def diff(gpu_mask, ref):
    """gpu_mask bool like ref['mask'].  Returns (n_gpu, n_ref, n_diff, n_unexplained): a differing cell is explained
    only inside the level band of its method or the PEAK_RTOL band of its largest neighbour."""
    d = gpu_mask ^ ref['mask']
    unexpl = d & ~ref['near']
    return int(gpu_mask.sum()), int(ref['mask'].sum()), int(d.sum()), int(unexpl.sum())


def mask_bool(words, C):
    """u64 / i64 mask words [..., W] -> bool [..., C]."""
    w = np.ascontiguousarray(words)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape + (8,)), axis=-1, bitorder='little')
    return bits.reshape(w.shape[:-1] + (w.shape[-1] * 64,))[..., :C].astype(bool)


# -- the checks of the oracle itself: per-cell loops on one map (no gate, no floor) ---------------------------
def _is_local_max(p, i, j):
    S, C = p.shape
    return all(p[i, j] >= p[i + di, j + dj] for di in (-1, 0, 1) for dj in (-1, 0, 1)
               if (di or dj) and 0 <= i + di < S and 0 <= j + dj < C)


def brute_force(p, window, alpha):
    """'ca' on p f64 [S, C]: the mean of the existing training cells, cell by cell."""
    offs = training_offsets(window)
    S, C = p.shape
    out = np.zeros((S, C), bool)
    for i in range(S):
        cells = [(i + di, dj) for di, dj in offs if 0 <= i + di < S]
        for j in range(C):
            tot = 0.0
            for r, dj in cells:
                tot += p[r, (j + dj) % C]
            out[i, j] = p[i, j] > alpha * tot / len(cells) and _is_local_max(p, i, j)
    return out


def brute_force_count(p32, window, rank, alpha):
    """'os' in the COUNTING form of the rule in fp32 on p32 f32 [S, C]: a peak iff at least k(i) existing training
    cells q have fl32(alpha_f * q) < p, and p >= every existing 3x3 neighbour."""
    offs = training_offsets(window)
    S, C = p32.shape
    af = np.float32(alpha)
    out = np.zeros((S, C), bool)
    for i in range(S):
        cells = [(i + di, dj) for di, dj in offs if 0 <= i + di < S]
        k = rank_of(len(cells), rank)
        for j in range(C):
            below = sum(1 for r, dj in cells if af * p32[r, (j + dj) % C] < p32[i, j])
            out[i, j] = below >= k and _is_local_max(p32, i, j)
    return out
