"""fp64 / pure-Python references of the scene kernels (rsl_scene.hip), test side.

topk_ref        robust_angle_estimation.py:362-369: the peaks with power_db > thr, sorted by power descending with
                Python's own stable list.sort (so the order among ties is the reference's, not a re-derivation), the
                first kmax.
nearest_ref     radarscenes_complete_analysis.py:274-305 for a batch of frames: the oracle's associate_analyzer per
                frame pair, the same with IEEE products for the squares (associate_ieee), and the temporal phase of
                the matched pairs.
"""
import numpy as np

import radar_oracle as O


def topk_ref(pdb_f32, thr_db, kmax):
    """Indices (into pdb_f32) of the selected entries, in the reference's order."""
    peaks = [{'entry': i, 'power_db': float(p)} for i, p in enumerate(np.asarray(pdb_f32, np.float32))]
    kept = [p for p in peaks if p['power_db'] > thr_db]
    kept.sort(key=lambda x: x['power_db'], reverse=True)
    return [p['entry'] for p in kept[:kmax]]


def pair_phase(c, p):
    """angle(c * conj(p)) with the four products rounded separately, as k_associate_nearest forms them."""
    cr, ci, pr, pi = np.real(c), np.imag(c), np.real(p), np.imag(p)
    re = cr * pr + ci * pi
    im = ci * pr - cr * pi
    return np.arctan2(im, re)


def associate_ieee(cur_r, cur_az, prev_r, prev_az, thr):
    """associate_analyzer with the squares as IEEE products: sqrt(dr * dr + da * da), every operation rounded to
    nearest on its own, which is what k_associate_nearest computes.  The oracle, like the reference, writes dr ** 2:
    on a Python or numpy scalar that is libm's pow(x, 2.0), which is not correctly rounded (it differs from x * x in the
    last bit about once in 2000 values), so its distances are reproducible to an ulp, not to the bit."""
    match = np.full(len(cur_r), -1, np.int64)
    dist = np.full(len(cur_r), np.inf)
    for i in range(len(cur_r) if len(prev_r) else 0):
        dr, da = cur_r[i] - prev_r, cur_az[i] - prev_az
        d = np.sqrt(dr * dr + da * da)
        j = int(np.argmin(d))  # the first minimum: the strict '<' against the running minimum
        if d[j] < thr:
            match[i], dist[i] = j, d[j]
    return match, dist


def nearest_ref(range_m, az_rad, s0, off, thr):
    """The concatenated targets of the frames [off[f], off[f + 1]): (match i64 [N], dist f64 [N]) of the oracle's
    associate_analyzer, (match, dist) of associate_ieee, and phase f64 [N] of the oracle's matches."""
    N = int(off[-1])
    match, match_i = np.full(N, -1, np.int64), np.full(N, -1, np.int64)
    dist, dist_i = np.full(N, np.inf), np.full(N, np.inf)
    phase = np.zeros(N)
    for f in range(1, len(off) - 1):
        c, p = slice(off[f], off[f + 1]), slice(off[f - 1], off[f])
        m, d = O.associate_analyzer(range_m[c], az_rad[c], range_m[p], az_rad[p], thr=thr)
        match[c], dist[c] = m, d
        match_i[c], dist_i[c] = associate_ieee(range_m[c], az_rad[c], range_m[p], az_rad[p], thr)
        hit = np.nonzero(m >= 0)[0]
        phase[off[f] + hit] = pair_phase(s0[c][hit], s0[p][m[hit]])
    return match, dist, match_i, dist_i, phase
