"""fp64 numpy oracle of the spatially smoothed MUSIC estimator (rsl_doa_smoothed; the definition is the doc comment in
include/rsl.h), the two-source input generator and the parity rules the host and GPU tests share.  A helper module,
not collected.

The oracle works on the very c64 values the kernel reads (signatures and sub-array steering vectors are rounded to c64
first, then everything is fp64, eigendecomposition by np.linalg.eigh).  Eigenvectors are not unique, so parity is on
the invariants: eigenvalues, the null spectrum den, the model order and the picks.

Tolerances on every cell that is not `near` (near_cells):
  nsrc   equal
  eig    |eig - ref| <= EIG_TOL * lambda_1, EIG_TOL = 1e-5 (fp32 Jacobi: about L * sweeps * 2^-24 = 5e-6)
  den    |den - ref| <= DEN_TOL * L / gap on the whole row, gap = (lambda_k - lambda_{k+1}) / lambda_1 (the error of
         the noise-space projector scales as eps / gap)
  picks  equal (the oracle counts fp64 den values within TIE = 1e-12 as a tie, lower index first: the -90 and +90
         degree points of a half-wavelength array share one steering vector); a pick may sit at g +- 1 where the reference's den at the two indices differs by less than the den
         tolerance (counted and held to the cap of near cells)

DEN_TOL: measured on an MI355X as max(err * gap / L) of the kernel against this oracle over the named inputs of
tests/test_gpu_ssmusic.py (two_sources at (M, L, sep) = (8, 6, 8 / 12 / 20), (8, 5, 10), (16, 8, 5), (4, 3, 25), 30 dB,
1536 cells each, fixed k = 2 and estimate mode with rel 0.05 and 0.01; 1024 unit-norm Gaussian-noise signatures with
rel 0.05 and with k = 3, G = 361): 4.59e-7 (per set 1.6e-7 to 4.6e-7; the eigenvalue error on the same sets was at most
5.3e-7 lambda_1).  DEN_TOL = 4 x that value = 1.836e-6 (the margin covers other seeds and shapes).
"""
import numpy as np

EIG_TOL = 1e-5
MEASURED_DEN = 4.59e-7  # max(err * gap / L) measured on the device, see above
DEN_TOL = 4 * MEASURED_DEN
NEAR_GAP = 1e-3
NEAR_REL = 1e-5
TIE = 1e-12        # fp64 den values this close are a tie (den <= L <= 8: rounding is about 1e-15)


def near_cap(cells):
    return max(2, cells // 500)


def steering(grid_deg, M, d_over_lambda=0.5):
    """Steering matrix c128 [G, M] of a uniform linear array with element 0 at the origin."""
    psi = 2 * np.pi * d_over_lambda * np.sin(np.radians(np.asarray(grid_deg, np.float64)))
    return np.exp(1j * psi[:, None] * np.arange(M)[None, :])


def two_sources(n, M, sep_deg, snr_db, seed):
    """n unit-norm c64 signatures [n, M] of two coherent sources sep_deg apart on a half-wavelength array: theta_0
    uniform in [-50, 50 - sep], the second source at theta_0 + sep with amplitude uniform in [0.7, 1] and phase uniform
    in [0, 2 pi), complex Gaussian noise of power 10^(-snr / 10) per element.  Returns (sigs, theta_deg [n, 2])."""
    rng = np.random.default_rng(seed)
    t0 = rng.uniform(-50.0, 50.0 - sep_deg, n)
    th = np.stack([t0, t0 + sep_deg], axis=1)
    amp = rng.uniform(0.7, 1.0, n)
    ph = rng.uniform(0.0, 2 * np.pi, n)
    m = np.arange(M)[None, :]
    a0 = np.exp(1j * np.pi * np.sin(np.radians(th[:, :1])) * m)
    a1 = np.exp(1j * np.pi * np.sin(np.radians(th[:, 1:])) * m)
    sigma = np.sqrt(10.0 ** (-snr_db / 10.0) / 2.0)
    x = a0 + (amp * np.exp(1j * ph))[:, None] * a1 + sigma * (rng.standard_normal((n, M)) +
                                                               1j * rng.standard_normal((n, M)))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.complex64), th


def noise_sigs(n, M, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, M)) + 1j * rng.standard_normal((n, M))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.complex64)


def covariance(s, L):
    """Forward-backward smoothed covariance [n, L, L] of unit-norm signatures s [n, M]."""
    n, M = s.shape
    K = M - L + 1
    Rf = np.zeros((n, L, L), np.complex128)
    for k in range(K):
        sub = s[:, k:k + L]
        Rf += sub[:, :, None] * sub[:, None, :].conj()
    Rf /= K
    return 0.5 * (Rf + Rf[:, ::-1, ::-1].conj())


def local_minima(den):
    """The rule of the specification on rows of den [n, G]."""
    m = np.zeros(den.shape, bool)
    m[:, 1:-1] = (den[:, 1:-1] < den[:, :-2]) & (den[:, 1:-1] <= den[:, 2:])
    m[:, 0] = den[:, 0] < den[:, 1]
    m[:, -1] = den[:, -1] < den[:, -2]
    return m


def reference(sigs, steer_sub, L, nmax, num_sources=0, rel=0.05, signal_side=False):
    """The estimator in fp64.  sigs [n, M] (rounded to c64), steer_sub [G, L] (rounded to c64).  Returns a dict of
    nsrc i32 [n], idx i32 [n, nmax], den f64 [n, nmax], eig f64 [n, L], spec f64 [n, G], gap f64 [n] and sorted_min
    f64 [n, L] (the L deepest local minima of each row, inf where absent)."""
    x = np.asarray(sigs).astype(np.complex64).astype(np.complex128)
    a = np.asarray(steer_sub).astype(np.complex64).astype(np.complex128)
    n, M = x.shape
    G = a.shape[0]
    pw = (np.abs(x) ** 2).sum(axis=1)
    ok = pw > 0
    s = np.zeros_like(x)
    s[ok] = x[ok] / np.sqrt(pw[ok])[:, None]
    R = covariance(s, L)
    w, v = np.linalg.eigh(R)          # ascending
    w, v = w[:, ::-1], v[:, :, ::-1]  # descending
    if num_sources > 0:
        k = np.full(n, num_sources, np.int64)
    else:
        k = np.clip((w >= rel * w[:, :1]).sum(axis=1), 1, nmax)
    k = np.where(ok, k, 0)
    proj = np.abs(np.einsum('nlc,gl->ngc', v.conj(), a)) ** 2  # |v_c^H a_g|^2  [n, G, L]
    sel = np.arange(L)[None, :] >= k[:, None]                  # noise columns
    if signal_side:
        # ||a_g||^2 is L up to the c64 rounding of the steering values; the projector identity needs the exact norm
        spec = (np.abs(a) ** 2).sum(axis=1)[None, :] - (proj * ~sel[:, None, :]).sum(axis=2)
    else:
        spec = (proj * sel[:, None, :]).sum(axis=2)
    masked = np.where(local_minima(spec), spec, np.inf)
    order = np.argsort(masked, axis=1, kind='stable')
    smin = np.take_along_axis(masked, order[:, :L], axis=1)
    order = order[:, :smin.shape[1]].copy()
    # ties go to the lower index; fp64 values within TIE of each other are a tie (the -90 and +90 degree points of a
    # half-wavelength array have the same steering vector, and their den differs by rounding only)
    for _ in range(smin.shape[1]):
        for r in range(smin.shape[1] - 1):
            with np.errstate(invalid='ignore'):
                sw = (smin[:, r + 1] - smin[:, r] <= TIE) & (order[:, r + 1] < order[:, r]) & np.isfinite(smin[:, r + 1])
            order[sw, r], order[sw, r + 1] = order[sw, r + 1], order[sw, r]
    if smin.shape[1] < L:
        smin = np.pad(smin, ((0, 0), (0, L - smin.shape[1])), constant_values=np.inf)
    slot = np.arange(nmax)[None, :]
    have = (slot < k[:, None]) & np.isfinite(smin[:, :nmax])
    idx = np.where(have, order[:, :nmax], -1).astype(np.int32)
    den = np.where(have, smin[:, :nmax], np.nan)
    kk = np.clip(k, 1, L - 1)
    rows = np.arange(n)
    with np.errstate(invalid='ignore', divide='ignore'):
        gap = np.where(ok, (w[rows, kk - 1] - w[rows, kk]) / w[:, 0], np.nan)
    eig = np.where(ok[:, None], w, np.nan)
    spec = np.where(ok[:, None], spec, np.nan)
    return dict(nsrc=k.astype(np.int32), idx=idx, den=den, eig=eig, spec=spec, gap=gap, sorted_min=smin, ok=ok)


def den_tolerance(ref, L, den_tol):
    """Per-cell bound on |den - ref|: den_tol * L / gap."""
    with np.errstate(invalid='ignore', divide='ignore'):
        return den_tol * L / ref['gap']


def near_cells(ref, L, rel, estimate, den_tol):
    """Cells whose outcome the definition leaves to rounding: a small eigenvalue gap, an eigenvalue on the order
    threshold (estimate mode), or the k-th and (k+1)-th deepest minima closer than the den tolerance."""
    ok = ref['ok']
    near = ok & (ref['gap'] < NEAR_GAP)
    if estimate:
        lam = ref['eig']
        with np.errstate(invalid='ignore'):
            near |= ok & (np.abs(lam - rel * lam[:, :1]) <= NEAR_REL * lam[:, :1]).any(axis=1)
    k = ref['nsrc'].astype(np.int64)
    rows = np.arange(len(k))
    sm = ref['sorted_min']
    a, b = sm[rows, np.clip(k - 1, 0, L - 1)], sm[rows, np.clip(k, 0, L - 1)]
    with np.errstate(invalid='ignore'):
        close = np.isfinite(a) & np.isfinite(b) & (b - a < den_tolerance(ref, L, den_tol))
    return near | (ok & close)


def compare(out, ref, L, rel, estimate, den_tol):
    """Kernel outputs (dict of nsrc, idx, den, eig, spec as host arrays) against the oracle.  Returns the figures the
    tests assert on: near (count), nsrc_bad, eig_err (max over non-near cells of |eig - ref| / lambda_1), den_scaled
    (max of err * gap / L over the spec rows), den_bad (cells above the tolerance), pick_shift (cells with an explained
    g +- 1 pick), pick_bad (cells with an unexplained pick difference), pick_den_bad."""
    n = len(ref['nsrc'])
    near = near_cells(ref, L, rel, estimate, den_tol)
    use = ~near
    live = use & ref['ok']
    res = dict(cells=n, near=int(near.sum()))
    res['nsrc_bad'] = int((np.asarray(out['nsrc'])[use] != ref['nsrc'][use]).sum())
    lam1 = ref['eig'][:, :1]
    with np.errstate(invalid='ignore'):
        e = np.abs(np.asarray(out['eig'], np.float64) - ref['eig']) / lam1
    res['eig_err'] = float(e[live].max()) if live.any() else 0.0
    derr = np.abs(np.asarray(out['spec'], np.float64) - ref['spec']).max(axis=1)
    tol = den_tolerance(ref, L, den_tol)
    res['den_scaled'] = float((derr * ref['gap'] / L)[live].max()) if live.any() else 0.0
    res['den_bad'] = int((derr[live] > tol[live]).sum())
    # the empty cells: NaN rows on both sides
    empty = use & ~ref['ok']
    res['empty_bad'] = int((~np.isnan(np.asarray(out['spec'])[empty])).sum() +
                           (~np.isnan(np.asarray(out['eig'])[empty])).sum())
    gi, ri = np.asarray(out['idx']).astype(np.int64), ref['idx'].astype(np.int64)
    shift = np.zeros(n, bool)
    bad = np.zeros(n, bool)
    for c in np.nonzero(use & (gi != ri).any(axis=1))[0]:
        for s in np.nonzero(gi[c] != ri[c])[0]:
            g, r = gi[c, s], ri[c, s]
            if g >= 0 and r >= 0 and abs(g - r) == 1 and abs(ref['spec'][c, g] - ref['spec'][c, r]) < tol[c]:
                shift[c] = True
            else:
                bad[c] = True
    res['pick_shift'] = int((shift & ~bad).sum())
    res['pick_bad'] = int(bad.sum())
    # den at the picks: the kernel's own spec row at its picks, bit for bit
    od, osp = np.asarray(out['den']), np.asarray(out['spec'])
    pd = np.where(gi >= 0, np.take_along_axis(osp, np.clip(gi, 0, None), axis=1), np.nan)
    res['pick_den_bad'] = int((~((od == pd) | (np.isnan(od) & np.isnan(pd))))[use].sum())
    return res


def resolved(picks_deg, theta_deg, within=2.0):
    """Share of cells in which every true angle has a pick within `within` degrees (picks NaN where absent)."""
    d = np.abs(np.asarray(picks_deg)[:, :, None] - np.asarray(theta_deg)[:, None, :])
    d = np.where(np.isnan(d), np.inf, d)
    return float((d.min(axis=1) <= within).all(axis=1).mean())


def beamforming_two_peaks(sigs, steer):
    """Grid indices [n, 2] of the two highest local maxima of |a^H s|^2 (-1 where a cell has fewer)."""
    p = np.abs(np.asarray(sigs, np.complex128) @ np.asarray(steer).conj().T) ** 2
    m = local_minima(-p)
    masked = np.where(m, -p, np.inf)
    order = np.argsort(masked, axis=1, kind='stable')[:, :2]
    return np.where(np.isfinite(np.take_along_axis(masked, order, axis=1)), order, -1)
