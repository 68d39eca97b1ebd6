"""fp64 numpy OS-CFAR oracle and comparator for rsl_detect_oscfar (helper, not collected).

The rule is the one documented in include/rsl.h.  The training cells are those of the CA-CFAR oracle (cfar_ref.py):
offsets |di| <= hr, |dj| <= hd without the guard box, Doppler wraps, range truncates, n(i) cells exist for range row i.
With k(i) = min(n(i), max(1, ceil(rank * n(i)))) and x_(k) the k-th smallest training power, a cell is a peak iff
p > alpha * x_(k(i)) (strict), p >= every existing 3x3 neighbour (no wrap), i_lo <= i <= i_hi and p > thr_power
(thr_power < 0: no floor).  The oracle gathers the training cells of a block of range rows, orders them and takes
x_(k) -- the kernel never orders anything, it counts the cells below p / alpha.

The oracle takes the fp64 power of the complex64 RDS it is handed, so only the detector is under test.

Tolerances:
* OS_RTOL = 1e-6 on |p - level| relative to level = alpha x_(k): both sides carry the rounding of the kernel's fp32
  power, at most 3 * 2^-24 each (two squares and a sum); an order statistic moves by no more than its inputs do;
  (float)alpha and the fp32 product add 2^-24 each.  The sum, 8 * 2^-24, is below 5e-7.
* parity.PEAK_RTOL on the 3x3 test and cfar_ref.near_cap on the cells the two bands may explain, as for CA-CFAR.
"""
import math

import numpy as np

import cfar_ref as C
import parity as P

OS_RTOL = 1e-6

power, neighbour_max, mask_bool, near_cap = C.power, C.neighbour_max, C.mask_bool, C.near_cap


def training_offsets(window):
    gr, gd, tr, td = window
    hr, hd = gr + tr, gd + td
    return [(di, dj) for di in range(-hr, hr + 1) for dj in range(-hd, hd + 1)
            if not (abs(di) <= gr and abs(dj) <= gd)]


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


def oscfar_reference(rds, window, rank, alpha, *, thr_power=-1.0, gate=(0, 1 << 30)):
    """Returns dict(mask bool, p, level = alpha * x_(k), nbmax, near bool, n, k) for rds c64 [..., S, C]."""
    p = power(rds)
    S = p.shape[-2]
    xk, n, k = order_statistic(p, window, rank)
    level = alpha * xk
    nb = neighbour_max(p)
    g = np.zeros(S, bool)
    g[max(gate[0], 0):min(gate[1], S - 1) + 1] = True
    mask = (p > level) & (p >= nb) & g[:, None]
    if thr_power >= 0:
        mask &= p > thr_power
    near_lvl = np.abs(p - level) <= OS_RTOL * level
    near_max = np.abs(p - nb) <= P.PEAK_RTOL * np.maximum(p, nb)
    # a band decides something only where the other test passes or is itself inside its band (cfar_ref.cfar_reference)
    could_max = (p >= nb) | near_max
    could_lvl = (p > level) | near_lvl
    near = (near_lvl | near_max) & could_max & could_lvl & g[:, None]
    if thr_power >= 0:
        near &= p > thr_power
    return dict(mask=mask, p=p, level=level, nbmax=nb, near=near, n=n, k=k)


oscfar_diff = C.cfar_diff  # (n_gpu, n_ref, n_diff, n_unexplained) of a GPU mask against the reference dict


def brute_force_count(p32, window, rank, alpha):
    """Per-cell loop of the COUNTING form of the rule in fp32 on one map p32 f32 [S, C] (no gate, no floor): a peak
    iff at least k(i) existing training cells q have fl32(alpha_f * q) < p, and p >= every existing 3x3 neighbour."""
    offs = training_offsets(window)
    S, Cn = p32.shape
    af = np.float32(alpha)
    out = np.zeros((S, Cn), bool)
    for i in range(S):
        cells = [(i + di, dj) for di, dj in offs if 0 <= i + di < S]
        k = rank_of(len(cells), rank)
        for j in range(Cn):
            below = sum(1 for r, dj in cells if af * p32[r, (j + dj) % Cn] < p32[i, j])
            ok = below >= k
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (di or dj) and 0 <= i + di < S and 0 <= j + dj < Cn:
                        ok = ok and p32[i, j] >= p32[i + di, j + dj]
            out[i, j] = ok
    return out
