"""numpy fp64 oracle of the consensus velocity solve (rsl_velocity_consensus; the estimator is the doc comment in
include/rsl.h), a generator of frames with several moving populations, and the comparator the GPU tests share.
Not collected.

What is exact, and what it presupposes.  The device and this oracle draw the same pairs (Philox is integer
arithmetic), but solve the 2x2 system and evaluate the residuals with differently rounded operations (fused
multiply-adds, another cos / sin).  A two-cell solve with |det| >= 0.1 has a condition number <= 20, so x_h carries a
relative error of about 1e-14 and a residual an absolute one of about 3e-14 for |y| <= 3, against a cut-off t >= 0.05.
So every decision of the definition is the same on both sides as long as none of them is closer than MARGIN = 1e-9
(three orders above that error) to its boundary; the comparator asserts on the oracle alone (assert_oracle_fit, the
seeds are chosen so that it holds):
  * for every valid hypothesis, and for the x of every refinement pass and the returned x, no cell has
    ||r| - t| <= MARGIN t;
  * no drawn pair has ||det| - min_det| <= MARGIN;
  * no hypothesis lies within MARGIN (relative to the box width) of a box edge;
  * the normal matrix of the last refinement has a condition number <= vel_robust_ref.COND_MAX (1e2).
Given those, best_h, n_valid, n_in, n and the weights are compared exactly; x within vel_robust_ref.XTOL (1e-9
relative to max(|x|_inf, 1e-3): the same weighted moments summed in another order, that module's derivation; with
refine = 0 the raw two-cell solve, far inside it); cost and rmse_in within COST_RTOL (1e-8); residuals within 1e-9.
"""
import numpy as np

import philox_ref as P
import vel_robust_ref as R

K_CHAIN, BOX, XTOL, COST_RTOL, COND_MAX = R.K_CHAIN, R.BOX, R.XTOL, R.COST_RTOL, R.COND_MAX
MARGIN = 1e-9
DEFAULT_C = 3.0
MAX_H = 4096
CHUNK = 1024  # kCvChunk of rsl_vel_consensus.hip: the cells staged into LDS per trip of the scoring loop
MOTIONS = ((0.004, -0.002), (-0.006, 0.005), (0.009, 0.004), (-0.003, -0.008))
SHARES = (0.4, 0.2, 0.2, 0.2)
_M32 = 0xFFFFFFFF


def pair_from_draw(x0, x1, nf):
    """The index rule on one pair of 32-bit draws (Python integers: exact for every n_f)."""
    i = (int(x0) * int(nf)) >> 32
    j = (int(x1) * (int(nf) - 1)) >> 32
    return i, j + (j >= i)


def draw_pairs(nf, hyps, seed, frame):
    """Local indices (i, j) int64 [hyps] of the hypotheses of global frame `frame` with n_f = nf >= 2 cells."""
    h = np.arange(hyps, dtype=np.uint32)
    fr = int(frame)
    x0, x1, _, _ = P.philox4x32_10(h, np.full(hyps, fr & _M32, np.uint32), np.full(hyps, (fr >> 32) & _M32, np.uint32),
                                   np.zeros(hyps, np.uint32), seed & _M32, (seed >> 32) & _M32)
    lo, hi = np.uint64(nf & _M32), np.uint64(nf >> 32)
    l1, h1 = np.uint64((nf - 1) & _M32), np.uint64((nf - 1) >> 32)
    x0, x1 = x0.astype(np.uint64), x1.astype(np.uint64)
    s32 = np.uint64(32)
    i = (x0 * hi + ((x0 * lo) >> s32)).astype(np.int64)  # (x0 nf) >> 32 without a 96-bit product
    j = (x1 * h1 + ((x1 * l1) >> s32)).astype(np.int64)
    return i, j + (j >= i)


def _near(a, t):
    return int((np.abs(a - t) <= MARGIN * t).sum())


def consensus_frame(az, y, m=None, *, k, scale, c=None, hyps=256, min_det=0.1, refine=3, seed=0, frame=0, ridge=0.0,
                    bounds=BOX):
    """One frame (global index `frame`).  Returns x, cost, rmse_in, n_in, n, best_h, n_valid, weights, residuals and
    diagnostics: ls (rsl_velocity's solution), scores, valid, x_h, cond (condition number of the normal matrix of the
    last refinement solve, 1.0 when none ran), passes (refinement solves run), near_cut / near_det / near_box (the
    decisions within MARGIN of their boundary)."""
    c = DEFAULT_C if c is None else float(c)
    az, y = np.asarray(az, np.float64), np.asarray(y, np.float64)
    nf = len(y)
    m = np.ones(nf, np.int64) if m is None else np.asarray(m, np.int64)
    cs, sn, mw = np.cos(az), np.sin(az), m.astype(np.float64)
    lx, hx, ly, hy = bounds
    t = c * float(scale)
    ls = R.box_solve(R.moments(mw, cs, sn, y), k, ridge, bounds)
    valid = np.zeros(hyps, bool)
    scores = np.zeros(hyps, np.int64)
    xh = np.zeros((hyps, 2))
    near_cut = near_det = near_box = 0
    if nf >= 2:
        i, j = draw_pairs(nf, hyps, seed, frame)
        assert ((i != j) & (i >= 0) & (j >= 0) & (i < nf) & (j < nf)).all()
        det = cs[i] * sn[j] - cs[j] * sn[i]
        with np.errstate(divide='ignore', invalid='ignore'):
            vx = (y[i] * sn[j] - y[j] * sn[i]) / (k * det)
            vy = (cs[i] * y[j] - cs[j] * y[i]) / (k * det)
            inbox = (vx >= lx) & (vx <= hx) & (vy >= ly) & (vy <= hy)
            edge = np.minimum(np.minimum(np.abs(vx - lx), np.abs(vx - hx)) / max(hx - lx, 1e-300),
                              np.minimum(np.abs(vy - ly), np.abs(vy - hy)) / max(hy - ly, 1e-300))
        ok_pair = (m[i] > 0) & (m[j] > 0)
        valid = ok_pair & (np.abs(det) >= min_det) & inbox
        near_det = int((np.abs(np.abs(det) - min_det) <= MARGIN).sum())
        near_box = int((ok_pair & (np.abs(det) >= min_det) & (edge <= MARGIN)).sum())
        xh[valid, 0], xh[valid, 1] = vx[valid], vy[valid]
        idx = np.flatnonzero(valid)
        for q in range(0, len(idx), 128):
            hh = idx[q:q + 128]
            a = np.abs(y[None] - k * (xh[hh, 0, None] * cs[None] + xh[hh, 1, None] * sn[None]))
            scores[hh] = (m[None] * (a <= t)).sum(1)
            near_cut += _near(a, t)
    n_valid = int(valid.sum())
    if n_valid:
        best_h = int(np.flatnonzero(valid)[np.argmax(scores[valid])])  # the first of the largest: the lowest h
        x = xh[best_h].copy()
    else:
        best_h, x = -1, ls.copy()
    cond, passes = 1.0, 0
    for _ in range(refine):
        a = np.abs(y - k * (x[0] * cs + x[1] * sn))
        near_cut += _near(a, t)
        mom = R.moments(mw * (a <= t), cs, sn, y)
        if mom[0] == 0.0:
            break
        cond = R.cond_number(mom, k, ridge)
        x = R.box_solve(mom, k, ridge, bounds)
        passes += 1
    r = y - k * (x[0] * cs + x[1] * sn)
    a = np.abs(r)
    near_cut += _near(a, t)
    inl = a <= t
    n_in = int(m[inl].sum())
    return dict(x=x, cost=float((mw * np.where(inl, r * r, t * t)).sum() + ridge * (x * x).sum()),
                rmse_in=float(np.sqrt((mw * inl * r * r).sum() / n_in)) if n_in > 0 else 0.0, n_in=n_in,
                n=int(m.sum()), best_h=best_h, n_valid=n_valid, weights=inl.astype(np.float64), residuals=r, ls=ls,
                scores=scores, valid=valid, x_h=xh, cond=cond, passes=passes, near_cut=near_cut, near_det=near_det,
                near_box=near_box)


def consensus_batch(az, y, m, seg, n=None, *, frame0=0, **kw):
    """Frames seg[f] .. seg[f + 1] (clamped to n, default len(y)), frame f drawing as global frame frame0 + f.
    out f64 [F, 8] in the library's column order, weights / residuals [N] (NaN where no frame covers a cell),
    frames: the per-frame dictionaries."""
    N = len(y) if n is None else min(int(n), len(y))
    seg = np.minimum(np.asarray(seg, np.int64), N)
    F = len(seg) - 1
    out = np.zeros((F, 8))
    wt, rs = np.full(len(y), np.nan), np.full(len(y), np.nan)
    frames = []
    for f in range(F):
        sl = slice(seg[f], max(seg[f], seg[f + 1]))
        r = consensus_frame(az[sl], y[sl], None if m is None else m[sl], frame=frame0 + f, **kw)
        out[f] = [r['x'][0], r['x'][1], r['cost'], r['rmse_in'], r['n_in'], r['n'], r['best_h'], r['n_valid']]
        wt[sl], rs[sl] = r['weights'], r['residuals']
        frames.append(r)
    return dict(out=out, weights=wt, residuals=rs, frames=frames, seg=seg)


def scene(N, seed, *, shares=SHARES, motions=MOTIONS, noise=0.05, G=361, mmax=8, k=K_CHAIN):
    """A frame of N cells on the G-point grid with len(shares) populations, population p following motions[p]: the
    draws are, in this order, the grid indices, the labels, the phase noise (standard deviation `noise`) and the
    multiplicities (uniform in 0 .. mmax, given as antenna masks; mmax = 0: all 1, nothing drawn)."""
    rng = np.random.default_rng(seed)
    gidx = rng.integers(0, G, N).astype(np.int32)
    lab = rng.choice(len(shares), N, p=list(shares))
    az = R.grid_rad(G)[gidx]
    v = np.asarray(motions, np.float64)[lab]
    y = k * (v[:, 0] * np.cos(az) + v[:, 1] * np.sin(az)) + noise * rng.standard_normal(N)
    m = rng.integers(0, mmax + 1, N) if mmax > 0 else np.ones(N, np.int64)
    amask = ((1 << m.astype(np.int64)) - 1).astype(np.uint32).view(np.int32)
    return dict(gidx=gidx, az=az, y=y, m=m.astype(np.int64), amask=amask, label=lab,
                motions=np.asarray(motions, np.float64), k=k)


concat = R.concat


def assert_oracle_fit(ref):
    """What exactness presupposes, asserted on the oracle alone."""
    for f, r in enumerate(ref['frames']):
        assert r['near_cut'] == 0, ('cells at the cut-off', f, r['near_cut'])
        assert r['near_det'] == 0, ('pairs at min_det', f, r['near_det'])
        assert r['near_box'] == 0, ('hypotheses at a box edge', f, r['near_box'])
        assert r['cond'] <= COND_MAX, ('condition number', f, r['cond'])


def compare(tag, got_out, got_w, got_r, ref):
    """GPU rows / weights / residuals against consensus_batch's result.  Prints every figure before it asserts."""
    assert_oracle_fit(ref)
    out, seg = ref['out'], ref['seg']
    worst = dict(x=0.0, cost=0.0, rmse=0.0, r=0.0)
    for f, fr in enumerate(ref['frames']):
        g, o = got_out[f], out[f]
        assert np.isfinite(g).all(), (tag, f, g)
        ex = np.abs(g[:2] - o[:2]).max() / max(np.abs(o[:2]).max(), 1e-3)
        ec = abs(g[2] - o[2]) / abs(o[2]) if o[2] != 0 else abs(g[2])
        er = abs(g[3] - o[3]) / abs(o[3]) if o[3] != 0 else abs(g[3])
        worst.update(x=max(worst['x'], ex), cost=max(worst['cost'], ec), rmse=max(worst['rmse'], er))
        print(f'{tag} frame {f} (n {int(o[5])}): x err {ex:.2e}, cost {ec:.2e}, rmse {er:.2e}, n_in {g[4]:.0f} / '
              f'{o[4]:.0f}, best_h {g[6]:.0f} / {o[6]:.0f}, n_valid {g[7]:.0f} / {o[7]:.0f}, passes {fr["passes"]}, '
              f'cond {fr["cond"]:.1f}')
        assert g[6] == o[6] and g[7] == o[7], (tag, f, 'best_h / n_valid', g[6:], o[6:])
        assert g[4] == o[4] and g[5] == o[5], (tag, f, 'n_in / n', g[4:6], o[4:6])
        assert ex <= XTOL, (tag, f, 'x', g[:2], o[:2])
        assert ec <= COST_RTOL and er <= COST_RTOL, (tag, f, 'cost / rmse', g[2:4], o[2:4])
        sl = slice(seg[f], max(seg[f], seg[f + 1]))
        if got_w is not None and sl.stop > sl.start:
            assert (got_w[sl] == ref['weights'][sl]).all(), (tag, f, 'weights')
        if got_r is not None and sl.stop > sl.start:
            worst['r'] = max(worst['r'], np.abs(got_r[sl] - ref['residuals'][sl]).max())
    print(f'{tag}: worst x {worst["x"]:.2e}, cost {worst["cost"]:.2e}, rmse {worst["rmse"]:.2e}, '
          f'resid {worst["r"]:.2e}')
    assert worst['r'] <= 1e-9, (tag, 'residuals', worst['r'])
    return worst
