"""CPU: the fp64 restatement of rsl_cell_refine (tests/refine_ref.py) is sound, and the accuracy the refinement is
documented with.  Every figure below is of the reference, noise-free, re-measured when the tests run (they print it);
the asserted bounds are the figures the estimators were chosen by, with 1.5x headroom.

Estimator bias, largest |error| in bins over 41 offsets in [-0.49, 0.49], a complex tone through an fp64 FFT:
    estimator on window                               N = 16     N = 128    N = 512    (bound / 1.5)
    amplitude ratio r / (1 + r), rectangular          6.2e-4     9.7e-6     6.0e-7     (6.2e-4, 9.7e-6, 6.0e-7)
    amplitude ratio (2r - 1) / (r + 1), Hann          6.1e-2     7.8e-3     2.0e-3     (6.1e-2, 7.8e-3, 2.0e-3)
    log-parabola, Hann                                1.4e-2     1.6e-2     1.6e-2     (1.4e-2, 1.6e-2, 1.6e-2)
    log-parabola, Hamming                             1.1e-2     1.5e-2     1.6e-2     (1.1e-2, 1.5e-2, 1.6e-2)
    log-parabola, Blackman                            5.8e-3     6.5e-3     6.6e-3     (5.8e-3, 6.5e-3, 6.6e-3)
    log-parabola, rectangular                         0.17       0.17       0.17       (0.17: useless there)
The Hann ratio's error is the difference between scipy's symmetric window (period N - 1) and the periodic one the
closed form belongs to; it falls as 1 / N.  The range axis of the chain is windowed and takes the Hann ratio or the
log-parabola; the Doppler axis is not and takes the rectangular ratio.

Azimuth vertex on the 0.5 degree grid, half-wavelength array, 2001 azimuths in [-75, 75] degrees, largest error:
    fp64 signature and table (the rule itself)    A = 2: 6.0e-6 deg    A = 8: 1.5e-4 deg    A = 32: 2.5e-3 deg
                                                  (these are the bounds / 1.5; the grid argmax alone: 0.24 deg, 0.144 rms)
    both rounded to c64, as the kernel reads them A = 2: 8.7e-4 deg    A = 8: 1.5e-4 deg    A = 32: 2.5e-3 deg
    At 2 antennas the beam is 60 degrees wide: over one grid step it varies by 7e-4 of its height, and fp32 inputs
    (6e-8) leave the vertex 1e-4 of a step.  That is the inputs' precision, not the rule's, and still 300 times closer
    than the grid.
    The same parabola over the angle instead of its sine, A = 8: 8.1e-3 deg over these azimuths.
Velocity: the LS solve over 500 noise-free cells (8 antennas, c64 signatures, azimuths in [-70, 70] degrees) misses
(3, -1) m/s by 7.3e-4 with grid azimuths, by 1.8e-7 with the refined ones and by 7e-16 with the true ones.
"""
import numpy as np
import pytest
from scipy.signal import windows

import radar_oracle as O
import refine_ref as R

HEADROOM = 1.5
OFFSETS = np.linspace(-0.49, 0.49, 41)
WINDOWS = {'rect': lambda n: np.ones(n), 'hann': windows.hann, 'hamming': windows.hamming,
           'blackman': windows.blackman}
# (window, estimator): the largest |error| in bins at N = 16, 128, 512
BIAS = {('rect', R.RECT): (6.2e-4, 9.7e-6, 6.0e-7),
        ('hann', R.HANN): (6.1e-2, 7.8e-3, 2.0e-3),
        ('hann', R.LOG): (1.4e-2, 1.6e-2, 1.6e-2),
        ('hamming', R.LOG): (1.1e-2, 1.5e-2, 1.6e-2),
        ('blackman', R.LOG): (5.8e-3, 6.5e-3, 6.6e-3),
        ('rect', R.LOG): (0.17, 0.17, 0.17)}
SIZES = (16, 128, 512)


def tones(N, window, axis):
    """One frame per offset: a 2-D complex tone at bin (k + d) of the axis under test (length N, windowed) and at an
    off-bin position of the other axis (length 8, unwindowed), through an fp64 FFT; 2 antennas.  Returns (rds c64
    [41, 2, S, C], the cells' rc)."""
    M = 8
    k, kb, db = N // 2 - 3, 5, 0.3
    n, m = np.arange(N), np.arange(M)
    w = WINDOWS[window](N)
    a = w[None, :] * np.exp(2j * np.pi * (k + OFFSETS)[:, None] * n[None, :] / N)  # [41, N]
    b = np.exp(2j * np.pi * (kb + db) * m / M)  # [M]
    x = a[:, :, None] * b[None, None, :] if axis == 0 else b[None, :, None] * a[:, None, :]
    X = np.fft.fft2(x, axes=(1, 2))
    rds = np.stack([X, X * np.exp(0.7j)], axis=1)
    S, C = X.shape[1:]
    rc = (k * C + kb) if axis == 0 else (kb * C + k)
    return rds, np.full(len(OFFSETS), rc)


def measured_bias(N, window, est, axis):
    """Largest |offset error| of the reference on the tones, in bins.  The reference consumes the fp64 powers rounded
    to fp32, as the kernel does."""
    rds, rc = tones(N, window, axis)
    P = (np.abs(rds) ** 2).sum(axis=1).astype(np.float32)
    F = len(OFFSETS)
    modes = (est, R.NONE) if axis == 0 else (R.NONE, est)
    out = R.refine(rds.astype(np.complex64), P, np.arange(F), rc, np.zeros(F, int), np.radians(R.grid_deg()),
                   R.steering_c64(2), *modes, (0, 1, 0, 1))
    got = out['points'][:, 6 if axis == 0 else 7]
    return float(np.abs(got - OFFSETS).max())


@pytest.mark.parametrize('window,est', list(BIAS))
def test_estimator_bias(window, est):
    name = {R.LOG: 'log', R.RECT: 'rect', R.HANN: 'hann'}[est]
    for N, bound in zip(SIZES, BIAS[(window, est)]):
        for axis in (0, 1):  # the estimators do not know the axis: the range axis and the wrapping Doppler axis
            e = measured_bias(N, window, est, axis)
            print(f'{name} estimator on {window} window, N = {N}, axis {axis}: largest |error| {e:.2e} bins '
                  f'(bound {HEADROOM * bound:.2e})')
            assert e <= HEADROOM * bound, (window, name, N, axis, e)
    if (window, est) == ('rect', R.LOG):  # why the Doppler axis does not take the log-parabola
        assert measured_bias(128, 'rect', R.LOG, 1) > 100 * measured_bias(128, 'rect', R.RECT, 1)


def vertex_error_deg(A, true_deg, mutate=None, dtype=np.complex128):
    """(vertex error, grid-argmax error) in degrees on the 0.5 degree grid for plane waves from true_deg; dtype: the
    precision the signatures and the steering table are rounded to (complex64: what the kernel is handed)."""
    grid = O.azimuth_grid()
    m = np.pi * np.arange(A)[None, :]
    steer = np.exp(1j * m * np.sin(np.radians(grid))[:, None]).astype(dtype)
    z = np.exp(1j * m * np.sin(np.radians(true_deg))[:, None]).astype(dtype)
    B = np.abs(z.astype(np.complex128) @ steer.astype(np.complex128).conj().T) ** 2
    g = np.argmax(B, axis=1)
    az = R.azimuth(z, g, np.radians(grid), steer, mutate=mutate)
    return np.abs(np.degrees(az.astype(np.float64)) - true_deg), np.abs(grid[g] - true_deg)


@pytest.mark.parametrize('A,bound', [(2, 6e-6), (8, 1.5e-4), (32, 2.5e-3)])
def test_azimuth_vertex_accuracy(A, bound):
    true = np.linspace(-75.0, 75.0, 2001) + 0.0137
    err, gerr = vertex_error_deg(A, true)
    print(f'A = {A}: vertex error max {err.max():.2e} deg, rms {np.sqrt((err ** 2).mean()):.2e}; grid argmax max '
          f'{gerr.max():.3f} deg, rms {np.sqrt((gerr ** 2).mean()):.3f} (bound {HEADROOM * bound:.2e})')
    assert err.max() <= HEADROOM * bound
    assert gerr.max() > 0.2  # the refinement had something to do
    e32, _ = vertex_error_deg(A, true, dtype=np.complex64)
    print(f'A = {A}: with the signature and the table rounded to c64, as the kernel reads them: {e32.max():.2e} deg')
    # What fp32 inputs may add.  Near its peak B(u) = B0 (1 - kappa (u - u*)^2) with kappa = pi^2 (A^2 - 1) / 12; the
    # vertex of the parabola through samples h apart is h (y0 - y2) / (2 (y0 - 2 y1 + y2)) with y0 - 2 y1 + y2 =
    # -2 kappa B0 h^2, so perturbing each sample by eps B0 moves it by at most eps / (2 kappa h) through the numerator
    # and eps / (kappa h) through the denominator (offset <= h / 2).  eps = 4 * 2^-24 (signature and table rounded,
    # squared); h = cos(theta) * 0.5 deg in u and the angle moves by 1 / cos(theta) of that: worst at 75 degrees.
    kappa, eps, step = np.pi ** 2 * (A * A - 1) / 12, 4 * 2.0 ** -24, np.radians(0.5)
    rounding = np.degrees(1.5 * eps / (kappa * step * np.cos(np.radians(75.1)) ** 2))
    print(f'    the rounding may add {rounding:.2e} deg')
    assert e32.max() <= HEADROOM * bound + rounding
    if A == 8:  # the parabola over the angle itself is an order of magnitude worse: the beam is symmetric in sin
        derr, _ = vertex_error_deg(A, true, mutate='degree_abscissa')
        print(f'A = 8: the same parabola over the angle: {derr.max():.2e} deg')
        assert derr.max() > 10 * err.max()


# -- the edge rules, one by one --------------------------------------------------------------------------------------
def small_case(seed=5, A=4, F=2, S=6, C=5):
    rng = np.random.default_rng(seed)
    rds = (rng.standard_normal((F, A, S, C)) + 1j * rng.standard_normal((F, A, S, C))).astype(np.complex64)
    return rds, R.power_f32(rds)


def run_small(rds, P, f, i, j, g, modes=(R.LOG, R.RECT), **kw):
    C = rds.shape[3]
    one = lambda v: np.atleast_1d(np.asarray(v))
    return R.refine(rds, P, one(f), one(i) * C + one(j), one(g), np.radians(R.grid_deg()),
                    R.steering_c64(rds.shape[1]), *modes, R.AXES, **kw)


def test_power_sum_is_the_fp32_sum_in_antenna_order():
    rds, P = small_case(A=7)
    p64 = (rds.real.astype(np.float64) ** 2 + rds.imag.astype(np.float64) ** 2).sum(axis=1)
    assert P.dtype == np.float32 and np.abs(P - p64).max() <= 7 * 2.0 ** -24 * p64.max()
    assert (P != R.power_f32(rds, reverse=True)).any()  # the order shows in the bits
    ints = (np.random.default_rng(1).integers(-8, 9, rds.shape) * (1 + 1j)).astype(np.complex64)
    exact = (ints.real.astype(np.int64) ** 2 + ints.imag.astype(np.int64) ** 2).sum(axis=1)
    assert np.array_equal(R.power_f32(ints), exact.astype(np.float32))  # small integers: every step is exact


def test_range_axis_truncates():
    rds, P = small_case()
    S = rds.shape[2]
    for i in (0, S - 1):
        out = run_small(rds, P, 1, i, 2, 18)
        assert out['points'][0, 6] == 0.0 and out['points'][0, 7] != 0.0
        assert out['points'][0, 0] == R.AXES[0] + R.AXES[1] * i
    assert run_small(rds, P, 1, 2, 2, 18)['points'][0, 6] != 0.0


def test_doppler_axis_wraps():
    rds, P = small_case()
    C = rds.shape[3]
    for j, (jm, jp) in ((0, (C - 1, 1)), (C - 1, (C - 2, 0))):
        out = run_small(rds, P, 0, 3, j, 18)
        want = R.offset(R.RECT, P[0, 3, jm], P[0, 3, j], P[0, 3, jp])
        assert out['points'][0, 7] == want and want != 0.0
        # no wrap of the label: it may pass the axis end
        assert out['points'][0, 1] == R.AXES[2] + R.AXES[3] * (j + want)


def test_grid_ends_and_out_of_range_index():
    rds, P = small_case()
    tab = np.radians(R.grid_deg())
    for g in (0, R.G_ - 1):
        out = run_small(rds, P, 0, 2, 2, g)
        assert out['az'][0] == tab[g] and out['points'][0, 2] == tab[g]
    ref = run_small(rds, P, 0, 2, 2, 18)['points'][0]
    for g in (-1, R.G_, 1 << 20):
        p = run_small(rds, P, 0, 2, 2, g)['points'][0]
        assert np.isnan(p[[2, 3, 4]]).all()
        assert np.array_equal(p[[0, 1, 5, 6, 7]], ref[[0, 1, 5, 6, 7]])  # the rest as usual


def test_vertex_needs_a_maximum():
    rds, P = small_case()
    z = rds[0, :, 2, 2].astype(np.complex128)
    B = np.abs(R.steering_c64(4).astype(np.complex128).conj() @ z) ** 2
    tab = np.radians(R.grid_deg())
    gmax = 1 + int(np.argmax(B[1:-1]))
    gmin = 1 + int(np.argmin(B[1:-1]))
    a = run_small(rds, P, 0, 2, 2, gmax)['az'][0]
    lo, hi = (np.arcsin((np.sin(tab[gmax + d]) + np.sin(tab[gmax])) / 2) for d in (-1, 1))
    assert a != tab[gmax] and lo <= a <= hi  # refined, inside the midpoints
    assert run_small(rds, P, 0, 2, 2, gmin)['az'][0] == tab[gmin]  # c >= 0: the table's value
    rds0 = rds.copy()
    rds0[0, :, 2, 2] = 0  # B = 0 at all three: c = 0
    assert run_small(rds0, R.power_f32(rds0), 0, 2, 2, 18)['az'][0] == tab[18]


def test_zero_power_and_equal_neighbours():
    rds, _ = small_case()
    rds[0, :, 2, 2] = 0
    P = R.power_f32(rds)
    for modes in ((R.LOG, R.LOG), (R.RECT, R.RECT), (R.HANN, R.HANN)):
        p = run_small(rds, P, 0, 2, 2, 18, modes)['points'][0]
        assert p[6] == 0.0 and p[7] == 0.0 and p[5] == pytest.approx(-120.0, abs=1e-9)
    # a zero neighbour: the log-parabola gives 0, the ratios go to the other side
    p = run_small(rds, P, 0, 2, 3, 18, (R.NONE, R.LOG))['points'][0]
    assert p[7] == 0.0
    assert run_small(rds, P, 0, 2, 3, 18, (R.NONE, R.RECT))['points'][0, 7] > 0.0
    rds[1, :, 3, 1] = rds[1, :, 3, 3]  # pm == pp bit for bit
    P = R.power_f32(rds)
    assert P[1, 3, 1] == P[1, 3, 3]
    for m in (R.LOG, R.RECT, R.HANN):
        assert run_small(rds, P, 1, 3, 2, 18, (R.NONE, m))['points'][0, 7] == 0.0
    assert (R.offset(R.NONE, P[0, 1], P[0, 2], P[0, 3]) == 0).all()


def test_offsets_stay_inside_half_a_bin():
    rng = np.random.default_rng(3)
    pm, p0, pp = (rng.exponential(1.0, 4000).astype(np.float32) for _ in range(3))
    for m in (R.LOG, R.RECT, R.HANN):
        d = R.offset(m, pm, p0, pp)
        assert np.isfinite(d).all() and np.abs(d).max() <= 0.5
    big = p0 >= np.maximum(pm, pp)  # a local maximum: the sign points at the larger neighbour
    for m in (R.LOG, R.RECT):
        d = R.offset(m, pm, p0, pp)[big]
        assert (np.sign(d) == np.sign(pp[big].astype(np.float64) - pm[big])).all()


# -- what the refined azimuths are for -------------------------------------------------------------------------------
def test_velocity_benefit():
    rng = np.random.default_rng(11)
    true = rng.uniform(-70, 70, 500)
    lam = 3e8 / 77e9
    k = 4 * np.pi * 0.1 / lam
    v = np.array([3.0, -1.0])
    y = k * (v[0] * np.cos(np.radians(true)) + v[1] * np.sin(np.radians(true)))
    grid = O.azimuth_grid()
    steer = R.steering_c64(8, grid)
    z = np.exp(1j * np.pi * np.arange(8)[None, :] * np.sin(np.radians(true))[:, None]).astype(np.complex64)
    g = np.argmax(np.abs(z.astype(np.complex128) @ steer.astype(np.complex128).conj().T) ** 2, axis=1)
    az = R.azimuth(z, g, np.radians(grid), steer).astype(np.float64)
    miss = {}
    for name, a in (('grid', np.radians(grid[g])), ('refined', az), ('true', np.radians(true))):
        vx, vy, _ = O.velocity_ls(a, y, lambda_c=lam)
        miss[name] = float(np.hypot(vx - v[0], vy - v[1]))
    print(f'LS velocity miss of (3, -1) m/s over 500 cells: grid {miss["grid"]:.2e}, refined {miss["refined"]:.2e}, '
          f'true azimuths {miss["true"]:.2e}')
    assert miss['refined'] * 100 <= miss['grid']


# -- mutations the GPU test's inputs must catch ------------------------------------------------------------------------
@pytest.fixture(scope='module')
def baseline():
    out = {}
    for A in (3, 8):
        c = R.gpu_case(A)
        args = (c['rds'], None, c['frame'], c['rc'], c['gidx'], c['az_table'], c['steer'])
        out[A] = (c, args, {m: R.refine(*args, *m, R.AXES) for m in ((R.HANN, R.RECT), (R.LOG, R.HANN))})
    return out


@pytest.mark.parametrize('mutation', R.MUTATIONS)
def test_gpu_case_catches_mutation(baseline, mutation):
    """A kernel with this mistake would hand back the mutated reference's values: on the GPU test's own cells some
    field is then further from the true reference than that test allows (2 ulp of fp32 per field, the azimuth's
    tolerance; for the antenna order: some power differs in its bits, which the null-power comparison sees)."""
    hit = 0
    for A, (c, args, base) in baseline.items():
        for modes, ref in base.items():
            mut = R.refine(*args, *modes, R.AXES, mutate=mutation)
            if mutation == 'reversed_antennas':
                f, rc = c['frame'], c['rc']
                used = ref['P'][f, rc // R.C_, rc % R.C_] != mut['P'][f, rc // R.C_, rc % R.C_]
                hit += int(used.sum())
                continue
            ulp = R.ulp_distance(mut['points32'], ref['points'])
            tol, _ = R.az_tol(c, *modes)
            with np.errstate(invalid='ignore'):
                daz = np.abs(mut['az'].astype(np.float64) - ref['az'].astype(np.float64))
            n = int((ulp > R.POINTS_TOL_ULP).any(axis=1).sum())
            print(f'{mutation}, A = {A}, modes {modes}: {n} of {R.N_} rows beyond 2 ulp, azimuth moved on '
                  f'{int((daz > tol).sum())} cells')
            assert n > 0, (mutation, A, modes)
            hit += n
    assert hit > 0


def test_gpu_case_has_what_it_promises():
    for A in R.GPU_A:
        c = R.gpu_case(A)
        f, rc, g, nm = c['frame'], c['rc'], c['gidx'], c['named']
        i, j = rc // R.C_, rc % R.C_
        assert len(rc) == R.N_ and len(np.unique(f * 1000 + rc)) < R.N_  # repeats; three 256-thread blocks
        for fr in range(R.F_):
            for ii in (0, R.S_ - 1):
                for jj in (0, R.C_ - 1):
                    assert ((f == fr) & (i == ii) & (j == jj)).any()
        assert g[nm['g0']] == 0 and g[nm['gend']] == R.G_ - 1 and g[nm['gover']] == R.G_ and g[nm['gunder']] == -1
        k = nm['zero']
        assert not c['rds'][f[k], :, i[k], j[k]].any()
        k = nm['equal']
        assert np.array_equal(c['rds'][f[k], :, i[k], j[k] - 1], c['rds'][f[k], :, i[k], j[k] + 1])
        out = R.refine(c['rds'], None, f, rc, g, c['az_table'], c['steer'], R.HANN, R.RECT, R.AXES)
        assert out['points'][nm['equal'], 7] == 0.0 and out['points'][nm['zero'], 5] == pytest.approx(-120.0)
        assert out['az'][nm['lowest']] == c['az_table'][g[nm['lowest']]]
        inner = (g > 0) & (g < R.G_ - 1)
        refined = inner & (out['az'].astype(np.float64) != c['az_table'][np.clip(g, 0, R.G_ - 1)])
        assert refined.sum() > 0.9 * inner.sum()  # nearly every cell takes the vertex
        assert np.isnan(out['points'][nm['gover'], 2:5]).all()
        # both signs and the clamp of each estimator occur
        for col in (6, 7):
            d = out['points'][:, col]
            assert (d > 0).any() and (d < 0).any()
