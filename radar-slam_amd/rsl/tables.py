"""Host-side fp64 table construction (setup, not per-element work).

Everything the kernels need that depends only on the radar configuration is computed here once, in
float64 exactly as the reference computes it, and uploaded (cast to fp32 / c64 where the kernel
computes in fp32):

* ``chirp_table``   conj(reference_chirp) * window            (dechirp.py:74-83, 99-108, 139)
* ``range_gate``    index interval of linspace(0, rr*S, S) in [min_range, max_range]  (dechirp.py:241, 263)
* ``power_threshold`` 10^(thr/10) - 1e-12                      (dechirp.py:238, 252)
* ``azimuth_grid`` / ``steering_matrix``                       (angle_estimation.py:59-60, 92-107)
"""
from __future__ import annotations

import math

import numpy as np

C_LIGHT = 3e8


def samples_per_chirp(chirp_duration: float, sampling_rate: float) -> int:
    return int(chirp_duration * sampling_rate)  # dechirp.py:63 (truncating)


def window_values(window_type: str, n: int) -> np.ndarray:
    from scipy.signal import windows  # dechirp.py:15, 99-106
    if window_type == 'hann':
        return windows.hann(n)
    if window_type == 'hamming':
        return windows.hamming(n)
    if window_type == 'blackman':
        return windows.blackman(n)
    raise ValueError(f"Unknown window type: {window_type}")


def reference_chirp(fc, bandwidth, chirp_duration, sampling_rate) -> np.ndarray:
    S = samples_per_chirp(chirp_duration, sampling_rate)
    t = np.linspace(0, chirp_duration, S)
    chirp_rate = bandwidth / chirp_duration
    return np.exp(1j * (2 * np.pi * (fc * t + 0.5 * chirp_rate * t ** 2)))


def chirp_table(fc, bandwidth, chirp_duration, sampling_rate, window_type, S) -> np.ndarray:
    """conj(ref) * window as complex128[S].  Raises the reference's broadcast ValueError when the frame's
    sample count differs from int(T_c * f_s) (dechirp.py:139)."""
    ref = reference_chirp(fc, bandwidth, chirp_duration, sampling_rate)
    if ref.shape[0] != S:
        raise ValueError(f"operands could not be broadcast together with shapes ({S},) ({ref.shape[0]},) ")
    return np.conj(ref) * window_values(window_type, S)


def range_axis(bandwidth, S):
    return np.linspace(0, (C_LIGHT / (2 * bandwidth)) * S, S)


def doppler_axis(sampling_rate, C):
    return np.linspace(-sampling_rate / 2, sampling_rate / 2, C)


def range_gate(bandwidth, S, min_range, max_range):
    r = range_axis(bandwidth, S)
    ok = np.nonzero((r >= min_range) & (r <= max_range))[0]
    if ok.size == 0:
        return 1, 0
    return int(ok[0]), int(ok[-1])


def refine_mode_for_window(window_type: str) -> str:
    """The range-axis offset estimator of rsl_cell_refine that suits a fast-time window: the amplitude ratio for
    'hann' (its main lobe has the closed form), the log-parabola for 'hamming' and 'blackman'.  The Doppler axis is
    unwindowed (dechirp.py:143-166 windows fast time only) and takes 'rect'."""
    if window_type == 'hann':
        return 'hann'
    if window_type in ('hamming', 'blackman'):
        return 'log'
    raise ValueError(f"Unknown window type: {window_type}")


def point_axes(cfg, S: int, C: int, velocity: bool = False):
    """(r0, r_step, d0, d_step) of rsl_cell_refine for a configuration with ``bandwidth`` and ``sampling_rate`` (a
    ChainConfig, or anything with these attributes).  The default reproduces the reference's labels at integer bins
    (dechirp.py:241-242: linspace(0, rr S, S) and linspace(-fs / 2, fs / 2, C)).  velocity=True labels the Doppler
    axis in metres per second instead, from ``fc`` and ``pri``: bin C // 2 is 0 and one bin is lambda / (2 C pri)."""
    S, C = int(S), int(C)
    rr = C_LIGHT / (2 * cfg.bandwidth)
    r_step = rr * S / (S - 1) if S > 1 else rr
    if velocity:
        d_step = (C_LIGHT / cfg.fc) / (2.0 * C * cfg.pri)
        d0 = -(C // 2) * d_step
    else:
        d_step = cfg.sampling_rate / (C - 1) if C > 1 else cfg.sampling_rate
        d0 = -cfg.sampling_rate / 2
    return (0.0, float(r_step), float(d0), float(d_step))


def power_threshold(threshold_db: float) -> float:
    return float(10.0 ** (threshold_db / 10.0) - 1e-12)


def cfar_training_cells(guard, train) -> int:
    """Full-window training-cell count N of a 2-D CFAR window with half-sizes guard (range, doppler) and train
    (range, doppler): the (2 hr + 1)(2 hd + 1) box without the (2 gr + 1)(2 gd + 1) guard box."""
    gr, gd = int(guard[0]), int(guard[1])
    tr, td = int(train[0]), int(train[1])
    return (2 * (gr + tr) + 1) * (2 * (gd + td) + 1) - (2 * gr + 1) * (2 * gd + 1)


def cfar_alpha(pfa: float, n_train: int) -> float:
    """CA-CFAR factor on the training MEAN for false-alarm rate pfa: a square-law detector in exponential noise with
    N training cells has Pfa = (1 + alpha / N)^-N, so alpha = N (pfa^(-1/N) - 1)."""
    n = int(n_train)
    if n < 1 or not (0.0 < pfa < 1.0):
        raise ValueError('cfar_alpha: pfa must lie in (0, 1) and n_train be >= 1')
    return float(n * (pfa ** (-1.0 / n) - 1.0))


def os_cfar_rank(n: int, rank: float) -> int:
    """Rank k of the OS-CFAR order statistic among n training cells: min(n, max(1, ceil(rank * n))), rank in (0, 1]
    (the rule rsl_detect_oscfar applies per range row, in fp64)."""
    n = int(n)
    if n < 1 or not (0.0 < rank <= 1.0):
        raise ValueError('os_cfar_rank: rank must lie in (0, 1] and n be >= 1')
    return min(n, max(1, int(math.ceil(float(rank) * n))))


def os_cfar_pfa(alpha: float, n_train: int, k: int) -> float:
    """False-alarm rate of OS-CFAR with factor alpha on the k-th smallest of N training cells (square-law detector,
    exponential noise; Rohling 1983): prod_{m=0}^{k-1} (N - m) / (N - m + alpha)."""
    m = np.arange(int(k), dtype=np.float64)
    return float(np.exp(-np.log1p(alpha / (int(n_train) - m)).sum()))


def os_cfar_alpha(pfa: float, n_train: int, k: int) -> float:
    """OS-CFAR factor on the k-th smallest training cell for false-alarm rate pfa: os_cfar_pfa (strictly decreasing
    in alpha) inverted by bisection to fp64 precision."""
    n, k = int(n_train), int(k)
    if not (0.0 < pfa < 1.0) or not 1 <= k <= n:
        raise ValueError('os_cfar_alpha: pfa must lie in (0, 1) and k in [1, n_train]')
    lo, hi = 0.0, 1.0
    while os_cfar_pfa(hi, n, k) > pfa:
        lo, hi = hi, 2.0 * hi
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            return mid
        if os_cfar_pfa(mid, n, k) > pfa:
            lo = mid
        else:
            hi = mid


CFAR_METHODS = ('ca', 'os')  # cell averaging (rsl_detect_cfar), ordered statistic (rsl_detect_oscfar)


# -- non-coherent integration: the cell under test and every training cell are sums of L looks ------------------
# In exponential (unit-mean) noise such a sum is Gamma(L, 1)-distributed: density x^(L-1) e^-x / (L-1)!, survival
# function Q_L(t) = e^-t sum_{m<L} t^m / m!.

def _bisect_decreasing(rate, pfa: float) -> float:
    """The alpha > 0 with rate(alpha) = pfa, rate strictly decreasing from 1, to fp64 precision."""
    lo, hi = 0.0, 1.0
    while rate(hi) > pfa:
        lo, hi = hi, 2.0 * hi
    while True:
        mid = 0.5 * (lo + hi)
        if not lo < mid < hi:
            return mid
        if rate(mid) > pfa:
            lo = mid
        else:
            hi = mid


def _check_looks(what: str, looks) -> int:
    if int(looks) != looks or not 1 <= int(looks) <= 32:
        raise ValueError(f'{what}: looks must be an integer in [1, 32], not {looks!r}')
    return int(looks)


def cfar_pfa_nci(alpha: float, n_train: int, looks: int) -> float:
    """False-alarm rate of CA-CFAR with factor alpha on the mean of n training cells when every cell is the sum of
    `looks` looks: with T = alpha / n,  Pfa = sum_{k<L} C(nL + k - 1, k) T^k / (1 + T)^(nL + k)  (the training sum is
    Gamma(nL); looks = 1: (1 + alpha / n)^-n, cfar_alpha's closed form).  Terms by their ratio, no large factorials."""
    n, L = int(n_train), _check_looks('cfar_pfa_nci', looks)
    if n < 1 or not alpha >= 0.0:
        raise ValueError('cfar_pfa_nci: n_train must be >= 1 and alpha >= 0')
    T = float(alpha) / n
    term = math.exp(-n * L * math.log1p(T))
    total = term
    r = T / (1.0 + T)
    for k in range(1, L):
        term *= (n * L + k - 1) / k * r
        total += term
    return total


def cfar_alpha_nci(pfa: float, n_train: int, looks: int) -> float:
    """CA-CFAR factor on the training mean of maps that sum `looks` looks, for false-alarm rate pfa: cfar_pfa_nci
    (strictly decreasing in alpha) inverted by bisection."""
    n, L = int(n_train), _check_looks('cfar_alpha_nci', looks)
    if n < 1 or not (0.0 < pfa < 1.0):
        raise ValueError('cfar_alpha_nci: pfa must lie in (0, 1) and n_train be >= 1')
    return _bisect_decreasing(lambda a: cfar_pfa_nci(a, n, L), pfa)


def _gamma_sf(t, L: int):
    """Q_L(t) = e^-t sum_{m<L} t^m / m! for an array t >= 0."""
    t = np.asarray(t, dtype=np.float64)
    s = np.ones_like(t)
    term = np.ones_like(t)
    for m in range(1, L):
        term = term * t / m
        s += term
    return np.exp(-t) * s


def _gamma_cdf(x, L: int):
    """1 - Q_L(x); below x = 1 by its own series e^-x sum_{m>=L} x^m / m! (1 - Q cancels there)."""
    x = np.asarray(x, dtype=np.float64)
    xs = np.minimum(x, 1.0)
    term = xs ** L / math.factorial(L)
    s = term.copy()
    for m in range(L + 1, L + 40):
        term = term * xs / m
        s += term
    return np.where(x < 1.0, np.exp(-xs) * s, 1.0 - _gamma_sf(x, L))


_GL_X, _GL_W = np.polynomial.legendre.leggauss(16)


def _os_nci_nodes(n: int, k: int, L: int):
    """Quadrature nodes x and weights w (density of x_(k) included) of  E[g(x_(k))] ~ sum w g(x), x_(k) the k-th
    smallest of n Gamma(L, 1) variables, density k C(n, k) F^(k-1) (1 - F)^(n-k) f.  Composite 16-point Gauss-Legendre
    in s = log x (the order statistic's relative width is bounded below over every n, k, L admitted, its absolute
    width is not), panels of 0.002, only those that hold more than e^-60 of the largest panel's density."""
    logc = math.log(k) + math.lgamma(n + 1) - math.lgamma(k + 1) - math.lgamma(n - k + 1)

    def logdens_s(s):  # log of the density of s = log x_(k)
        x = np.exp(s)
        with np.errstate(divide='ignore'):
            lf = np.log(_gamma_cdf(x, L)) if k > 1 else 0.0
            lq = np.log(_gamma_sf(x, L)) if n > k else 0.0
        return logc + (k - 1) * lf + (n - k) * lq + (L - 1) * s - x - math.lgamma(L) + s

    h = 0.002
    s_lo = (math.log(1e-30) + math.lgamma(L + 1) - math.log(n)) / L  # n F(x) < 1e-30 below
    s_hi = math.log(L + 80.0 + 8.0 * math.sqrt(L) + math.log(n))      # n Q_L(x) < 1e-30 above
    edges = np.arange(s_lo, s_hi + h, h)
    mid = edges[:-1] + 0.5 * h
    with np.errstate(invalid='ignore'):
        ld = logdens_s(mid)
    ld = np.where(np.isnan(ld), -np.inf, ld)
    keep = ld > ld.max() - 60.0
    keep = keep | np.roll(keep, 1) | np.roll(keep, -1)
    s = (mid[keep, None] + 0.5 * h * _GL_X[None, :]).ravel()
    w = np.exp(logdens_s(s)) * np.tile(0.5 * h * _GL_W, int(keep.sum()))
    return np.exp(s), w


def os_cfar_pfa_nci(alpha: float, n_train: int, k: int, looks: int) -> float:
    """False-alarm rate of OS-CFAR with factor alpha on the k-th smallest of n training cells when every cell is the
    sum of `looks` looks:  Pfa = E[Q_L(alpha x_(k))]  by one-dimensional quadrature (looks = 1: os_cfar_pfa's
    product)."""
    n, k, L = int(n_train), int(k), _check_looks('os_cfar_pfa_nci', looks)
    if not 1 <= k <= n or not alpha >= 0.0:
        raise ValueError('os_cfar_pfa_nci: k must lie in [1, n_train] and alpha be >= 0')
    x, w = _os_nci_nodes(n, k, L)
    return float(np.dot(w, _gamma_sf(float(alpha) * x, L)))


def os_cfar_alpha_nci(pfa: float, n_train: int, k: int, looks: int) -> float:
    """OS-CFAR factor on the k-th smallest training cell of maps that sum `looks` looks, for false-alarm rate pfa:
    os_cfar_pfa_nci (strictly decreasing in alpha) inverted by bisection on one set of quadrature nodes."""
    n, k, L = int(n_train), int(k), _check_looks('os_cfar_alpha_nci', looks)
    if not (0.0 < pfa < 1.0) or not 1 <= k <= n:
        raise ValueError('os_cfar_alpha_nci: pfa must lie in (0, 1) and k in [1, n_train]')
    x, w = _os_nci_nodes(n, k, L)
    return _bisect_decreasing(lambda a: float(np.dot(w, _gamma_sf(a * x, L))), pfa)


def cfar_design_alpha(method: str, pfa: float, guard, train, rank: float = 0.75, looks: int = 1) -> float:
    """The factor of a CFAR design, from its false-alarm rate and the full-window training-cell count: 'ca' on the
    training mean (cfar_alpha), 'os' on the order statistic of rank ceil(rank * cells) (os_cfar_alpha).  looks > 1:
    the design for maps that sum that many looks (non-coherent integration: cfar_alpha_nci, os_cfar_alpha_nci)."""
    n = cfar_training_cells(guard, train)
    if looks == 1:
        return os_cfar_alpha(pfa, n, os_cfar_rank(n, rank)) if method == 'os' else cfar_alpha(pfa, n)
    if method == 'os':
        return os_cfar_alpha_nci(pfa, n, os_cfar_rank(n, rank), looks)
    return cfar_alpha_nci(pfa, n, looks)


def azimuth_grid(search_range=(-90, 90), search_resolution=0.5):
    return np.arange(search_range[0], search_range[1] + search_resolution, search_resolution)


def steering_matrix(grid_deg, antenna_positions, lambda_c) -> np.ndarray:
    az = np.radians(np.asarray(grid_deg, dtype=np.float64))
    ph = 2 * np.pi * antenna_positions[None, :] * np.sin(az)[:, None] / lambda_c
    return np.exp(1j * ph)


def default_sub_len(M: int) -> int:
    """Sub-array length of the smoothed MUSIC when none is given: min(8, M - M // 3) (6 of 8, 8 of 16 antennas)."""
    return min(8, int(M) - int(M) // 3)


def subarray_steering(steer_c128, L: int) -> np.ndarray:
    """Steering vectors c128 [G, L] of the first L elements of a uniform linear array, a_g[l] = exp(j l psi_g), from
    the array's steering matrix [G, M] (rsl_doa_smoothed).  Spatial smoothing needs equal element spacing: raises
    ValueError when the phase step between neighbouring elements is not the same along the array."""
    st = np.asarray(steer_c128, dtype=np.complex128)
    if st.ndim != 2 or st.shape[1] < 2:
        raise ValueError('subarray_steering: steering matrix [G, M] with M >= 2 expected')
    G, M = st.shape
    L = int(L)
    if not 2 <= L <= M:
        raise ValueError(f'subarray_steering: sub-array length {L} outside [2, {M}]')
    step = st[:, 1:] * st[:, :-1].conj()  # exp(j psi_g) between neighbours, for every neighbour pair
    if not np.allclose(step, step[:, :1], rtol=0.0, atol=1e-9) or not np.allclose(np.abs(st), 1.0, atol=1e-9):
        raise ValueError('subarray_steering: the element positions are not uniform (spatial smoothing needs a '
                         'uniform linear array)')
    return np.ascontiguousarray(st[:, :L] * st[:, :1].conj())  # element 0 as the phase reference
