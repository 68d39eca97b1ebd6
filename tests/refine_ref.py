"""numpy restatement of rsl_cell_refine's specification (include/rsl.h) and the case list its GPU test runs (helper,
not collected).

refine() follows the header step by step in fp64: the five powers (read from an fp32 map, or formed from the RDS with
power_f32, which reproduces rsl_power_integrate's fp32 sum bit for bit), the offset estimators, the azimuth vertex and
the eight columns, which it returns both before and after the one rounding to fp32.  wide=True evaluates the azimuth
step (the three beamforming values, the sines, the vertex and the arcsine) in np.longdouble: the difference between
the two is the reference's own error, from which tests/test_gpu_refine.py takes its tolerance for out_az.

`mutate` swaps one rule for a plausible mistake (MUTATIONS); tests/test_refine_host.py shows that each of them moves
some output of gpu_case() beyond the GPU test's tolerance, so that test would catch the same mistake in the kernel.
"""
import numpy as np

NONE, LOG, RECT, HANN = 0, 1, 2, 3
MODES = {'none': NONE, 'log': LOG, 'rect': RECT, 'hann': HANN}
COLUMNS = ('range', 'doppler', 'az', 'x', 'y', 'power_db', 'range_offset', 'doppler_offset')
MUTATIONS = ('degree_abscissa', 'no_doppler_wrap', 'swapped_sign', 'q_min', 'reversed_antennas', 'no_frame_stride')

_WIDE = np.longdouble if np.finfo(np.longdouble).nmant >= 63 else None


def power_f32(rds, reverse=False):
    """rds c64 [F, A, S, C] -> f32 [F, S, C]: fmaf(re, re, im * im) per antenna, added in antenna order in fp32 (from
    the last antenna down with reverse).  The fused multiply-add is evaluated in the 64-bit significand of the x87
    long double (re * re is exact in 48 bits; the sum with the rounded im * im is then rounded once more to fp32, which
    differs from the single rounding only where the wide sum lands on an fp32 midpoint), or exactly in rationals where
    the platform has no such type."""
    z = np.asarray(rds)
    assert z.dtype == np.complex64 and z.ndim == 4
    re, im = z.real, z.imag
    t = im * im  # fp32 product, rounded
    if _WIDE is not None:
        p = (re.astype(_WIDE) * re.astype(_WIDE) + t.astype(_WIDE)).astype(np.float32)
    else:
        from fractions import Fraction
        p = np.array([np.float32(Fraction(float(a)) * Fraction(float(a)) + Fraction(float(b)))
                      for a, b in zip(re.ravel(), t.ravel())], dtype=np.float32).reshape(re.shape)
    acc = np.zeros(p[:, 0].shape, np.float32)
    order = range(z.shape[1] - 1, -1, -1) if reverse else range(z.shape[1])
    for a in order:
        acc = acc + p[:, a]  # fp32 add
    return acc


def offset(mode, pm, p0, pp, mutate=None):
    """The offset of one axis in fp64 from its fp32 powers, element-wise."""
    pm, p0, pp = (np.asarray(v, dtype=np.float32) for v in (pm, p0, pp))
    out = np.zeros(p0.shape, np.float64)
    if mode == NONE:
        return out
    m, c, p = pm.astype(np.float64), p0.astype(np.float64), pp.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        if mode == LOG:
            ok = (pm > 0) & (p0 > 0) & (pp > 0)
            lm, l0, lp = np.log(m), np.log(c), np.log(p)
            den = lm - 2.0 * l0 + lp
            ok &= den < 0
            v = np.clip(0.5 * (lm - lp) / den, -0.5, 0.5)
            return np.where(ok, v, 0.0)
        ok = (p0 > 0) & (pm != pp)
        q = np.minimum(pm, pp) if mutate == 'q_min' else np.maximum(pm, pp)
        r = np.sqrt(q.astype(np.float64) / c)
        s = np.where(pp > pm, 1.0, -1.0)
        if mutate == 'swapped_sign':
            s = -s
        v = r / (1.0 + r) if mode == RECT else np.maximum(0.0, (2.0 * r - 1.0) / (r + 1.0))
        return np.where(ok, s * np.minimum(0.5, v), 0.0)


def five_powers(P, f, i, j, mutate=None):
    """(p0, prm, prp, pdm, pdp, inner, dwrap) of the cells from the map P f32 [F, S, C]: the Doppler axis wraps, the
    range axis truncates (inner: the cells with both range neighbours)."""
    _, S, C = P.shape
    inner = (i > 0) & (i < S - 1)
    im, ip = np.clip(i - 1, 0, S - 1), np.clip(i + 1, 0, S - 1)
    p0 = P[f, i, j]
    if mutate == 'no_doppler_wrap':  # the Doppler axis truncated like the range axis
        dok = (j > 0) & (j < C - 1)
        pdm, pdp = P[f, i, np.clip(j - 1, 0, C - 1)], P[f, i, np.clip(j + 1, 0, C - 1)]
    else:
        dok = np.ones(j.shape, bool)
        pdm, pdp = P[f, i, (j - 1) % C], P[f, i, (j + 1) % C]
    return p0, P[f, im, j], P[f, ip, j], pdm, pdp, inner, dok


def azimuth(z, g, az_table, steer, wide=False, mutate=None):
    """Step 3 for the signatures z c64 [n, A] (unnormalised) and grid indices g: fp64, or long double with wide."""
    T = _WIDE if (wide and _WIDE is not None) else np.float64
    g = np.asarray(g, dtype=np.int64)
    G = az_table.shape[0]
    n = g.shape[0]
    az = np.full(n, np.nan, dtype=T)
    valid = (g >= 0) & (g < G)
    gc = np.clip(g, 0, G - 1)
    tab = az_table.astype(T)
    az[valid] = tab[gc[valid]]
    inner = valid & (g > 0) & (g < G - 1)
    if not inner.any():
        return az
    gi = g[inner]
    zr, zi = z[inner].real.astype(T), z[inner].imag.astype(T)
    B = []
    for k in (-1, 0, 1):
        a = steer[gi + k]
        ar, ai = a.real.astype(T), a.imag.astype(T)
        br = np.zeros(gi.shape, T)
        bi = np.zeros(gi.shape, T)
        for m in range(z.shape[1]):  # antenna order, as the kernel adds
            br = br + (ar[:, m] * zr[:, m] + ai[:, m] * zi[:, m])
            bi = bi + (ar[:, m] * zi[:, m] - ai[:, m] * zr[:, m])
        B.append(br * br + bi * bi)
    absc = tab if mutate == 'degree_abscissa' else np.sin(tab)
    u0, u1, u2 = absc[gi - 1], absc[gi], absc[gi + 1]
    with np.errstate(divide='ignore', invalid='ignore'):
        d01 = (B[1] - B[0]) / (u1 - u0)
        d12 = (B[2] - B[1]) / (u2 - u1)
        c = (d12 - d01) / (u2 - u0)
        use = (c < 0) & np.isfinite(c)
        lo, hi = (u0 + u1) / 2, (u1 + u2) / 2
        us = np.minimum(hi, np.maximum(lo, lo - d01 / c / 2))
        ref = us if mutate == 'degree_abscissa' else np.arcsin(us)
    res = az[inner]
    res[use] = ref[use]
    az[inner] = res
    return az


def refine(rds, power, frame, rc, gidx, az_table, steer_c64, range_mode, doppler_mode, axes, wide=False, mutate=None):
    """The specification on host arrays: rds c64 [F, A, S, C]; power f32 [F, S, C] or None; frame, rc, gidx [n];
    az_table f64 [G]; steer_c64 c64 [G, A]; modes as ids or names; axes (r0, r_step, d0, d_step).  Returns dict(points
    f64 [n, 8] before the rounding, points32 f32 [n, 8], az f64 [n] (long double with wide), P the power map used)."""
    rds = np.asarray(rds)
    F, A, S, C = rds.shape
    rm = MODES.get(range_mode, range_mode)
    dm = MODES.get(doppler_mode, doppler_mode)
    f = np.asarray(frame, dtype=np.int64)
    rc = np.asarray(rc, dtype=np.int64)
    if mutate == 'no_frame_stride':
        f = np.zeros_like(f)
    i, j = rc // C, rc % C
    P = np.asarray(power, dtype=np.float32) if power is not None else power_f32(rds, mutate == 'reversed_antennas')
    p0, prm, prp, pdm, pdp, inner, dok = five_powers(P, f, i, j, mutate)
    dr = np.where(inner, offset(rm, prm, p0, prp, mutate), 0.0)
    dd = np.where(dok, offset(dm, pdm, p0, pdp, mutate), 0.0)
    z = rds[f, :, i, j]  # [n, A]
    az = azimuth(z, gidx, np.asarray(az_table, np.float64), np.asarray(steer_c64), wide, mutate)
    a64 = az.astype(np.float64)
    r0, r_step, d0, d_step = (float(v) for v in axes)
    rng = r0 + r_step * (i + dr)
    dop = d0 + d_step * (j + dd)
    pts = np.stack([rng, dop, a64, rng * np.cos(a64), rng * np.sin(a64),
                    10.0 * np.log10(p0.astype(np.float64) + 1e-12), dr, dd], axis=1)
    return dict(points=pts, points32=pts.astype(np.float32), az=az, P=P)


def ulp_distance(got32, want64):
    """|got - round(want)| in units of the fp32 spacing at the reference value (0 where both are NaN; +-0 are equal)."""
    got32 = np.asarray(got32, dtype=np.float32)
    want32 = np.asarray(want64).astype(np.float32)
    both_nan = np.isnan(got32) & np.isnan(want32)
    sp = np.spacing(np.maximum(np.abs(want32), np.abs(got32)))
    with np.errstate(invalid='ignore'):
        d = np.abs(got32.astype(np.float64) - want32.astype(np.float64)) / sp.astype(np.float64)
    d = np.where(both_nan, 0.0, d)
    return np.where(np.isnan(d), np.inf, d)


# -- the GPU test's case list ------------------------------------------------------------------------------------------
F_, S_, C_, G_, N_ = 3, 16, 8, 37, 700
GPU_A = (2, 3, 4, 8, 16, 32)
AXES = (1.5, 0.16, -4.0e3, 1.1e3)  # no axis starts at 0 or has a unit step


def grid_deg():
    return np.linspace(-90.0, 90.0, G_)  # 5 degrees


def steering_c64(A, deg=None):
    """Half-wavelength uniform linear array over the grid, rounded to c64 as Context.steering_c64 uploads it."""
    az = np.radians(grid_deg() if deg is None else np.asarray(deg, np.float64))
    return np.exp(1j * np.pi * np.arange(A)[None, :] * np.sin(az)[:, None]).astype(np.complex64)


_cases = {}


def gpu_case(A):
    """The inputs of tests/test_gpu_refine.py at A antennas, built once: dict(rds c64 [3, A, 16, 8], frame, rc i32
    [700], gidx i32 [700], az_table f64 [37], steer c64 [37, A], named: the list positions of the forced cells).

    700 cells drawn with repeats over 384; half the RDS cells are unit noise, half carry a tone of 6 to 20 dB from an
    off-grid azimuth that leaks into its four neighbours.  gidx is the fp64 argmax of |a^H z|^2 over the grid.  Forced
    into the list: the four corners (i in {0, S-1}) x (j in {0, C-1}) of every frame, g = 0 and g = G - 1, an all-zero
    cell, a cell whose Doppler neighbours are equal bit for bit (pm == pp), gidx = G and gidx = -1, and a cell whose
    gidx is the grid's least beamforming value (c >= 0)."""
    if A in _cases:
        return _cases[A]
    rng = np.random.default_rng(9100 + A)
    z = (rng.standard_normal((F_, A, S_, C_)) + 1j * rng.standard_normal((F_, A, S_, C_))) / np.sqrt(2)
    tone = rng.random((F_, S_, C_)) < 0.5
    for f, i, j in zip(*np.nonzero(tone)):
        th = np.radians(rng.uniform(-80, 80))
        a = np.exp(1j * (np.pi * np.arange(A) * np.sin(th) + rng.uniform(0, 2 * np.pi)))
        amp = 10 ** (rng.uniform(6, 20) / 20)
        z[f, :, i, j] += amp * a
        for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
            if 0 <= i + di < S_:
                z[f, :, i + di, (j + dj) % C_] += amp * rng.uniform(0.2, 0.9) * a
    zero, equal, lowest = (1, 7, 3), (2, 5, 4), (0, 9, 5)
    z[zero[0], :, zero[1], zero[2]] = 0
    rds = z.astype(np.complex64)
    rds[equal[0], :, equal[1], equal[2] - 1] = rds[equal[0], :, equal[1], equal[2] + 1]
    frame = rng.integers(0, F_, N_)
    rc = rng.integers(0, S_ * C_, N_)
    named = {}
    pos = iter(rng.permutation(N_)[:32].tolist())

    def force(name, f, i, j):
        k = next(pos)
        frame[k], rc[k] = f, i * C_ + j
        named[name] = k
    for f in range(F_):
        for i in (0, S_ - 1):
            for j in (0, C_ - 1):
                force(f'corner{f}_{i}_{j}', f, i, j)
    force('zero', *zero)
    force('equal', *equal)
    force('lowest', *lowest)
    for name in ('g0', 'gend', 'gover', 'gunder'):
        force(name, int(rng.integers(0, F_)), int(rng.integers(1, S_ - 1)), int(rng.integers(1, C_ - 1)))
    steer = steering_c64(A)
    sig = rds[frame, :, rc // C_, rc % C_].astype(np.complex128)
    B = np.abs(sig @ steer.astype(np.complex128).conj().T) ** 2
    gidx = np.argmax(B, axis=1)
    gidx[named['g0']], gidx[named['gend']], gidx[named['gover']], gidx[named['gunder']] = 0, G_ - 1, G_, -1
    gidx[named['lowest']] = 1 + int(np.argmin(B[named['lowest'], 1:G_ - 1]))
    case = dict(rds=rds, frame=frame.astype(np.int32), rc=rc.astype(np.int32), gidx=gidx.astype(np.int32),
                az_table=np.radians(grid_deg()), steer=steer, named=named)
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    _cases[A] = case
    return case


# out_points: 2 ulp of fp32 per field: one for the final rounding falling either way (the device's fp64 value and the
# reference's differ in their last bits), one spare
POINTS_TOL_ULP = 2.0


def az_tol(case, range_mode=HANN, doppler_mode=RECT):
    """(tolerance, spread): 100 x the largest |fp64 - long double| difference of the reference's azimuth on the case's
    own cells, and that difference."""
    assert _WIDE is not None, 'no extended long double on this platform: the reference has nothing to measure itself by'
    a = refine(case['rds'], None, case['frame'], case['rc'], case['gidx'], case['az_table'], case['steer'],
               range_mode, doppler_mode, AXES)['az']
    b = refine(case['rds'], None, case['frame'], case['rc'], case['gidx'], case['az_table'], case['steer'],
               range_mode, doppler_mode, AXES, wide=True)['az']
    ok = ~np.isnan(a)
    spread = float(np.max(np.abs(a[ok].astype(b.dtype) - b[ok])))
    return 100.0 * spread, spread
