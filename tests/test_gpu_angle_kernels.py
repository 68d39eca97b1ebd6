"""GPU: the per-signature angle kernels against the fp64 references of tests/angle_ref.py, at every array size that
picks another branch: k_music_subspace and k_esprit_subspace (rsl_subspace.hip), k_confidence and k_cell_extras
(rsl_doa.hip).  tests/test_angle_host.py shows on a CPU that the references and the inputs are sound.

ESPRIT values are compared as eigenvalue phases, sin(radians(deg)) / scale against angle(lambda), wrapped.
    reference spread (Gram-Schmidt basis against LAPACK's QR of the same columns, test_angle_host.py):
        reference-determined inputs (kk <= 2)        8.9e-15 rad
        3 <= kk < M - 1, by (M, K)                   4e-15 (kk = 3) .. 1.6e-6 rad (kk = 10 .. 14 at M = 12, 16): the two
                                                     non-zero eigenvalues sit next to a Jordan block of size kk - 2
    tolerance used = 100 x spread, computed from the references when the tests run:
        kk <= 2 and k_cell_extras                    8.9e-13 rad   (angle_ref.esprit_tol)
        3 <= kk < M - 1                              that, or 100 x the (M, K)'s own spread where larger: 8.9e-13 ..
                                                     1.6e-4 rad    (angle_ref.cluster_tol)
    measured on an MI355X:
        largest error of a reference-determined value        4.9e-15 rad (k_esprit_subspace), 1.8e-15 (k_cell_extras)
        K = 2 outputs equal to numpy's eigvals(Phi)[0] on O.esprit_svd's path (recorded, not asserted: the order is
        LAPACK's)                                            720 of 720 (and 720 of 720 at K = -(M-3))
        3 <= kk < M - 1: cells whose value is not the angle of one of the two non-zero eigenvalues (cap: 3 % per (M, K)):
            none of 1267.  Until the kernel took the first Schur diagonal entry among the two of largest modulus it took
            the first entry as it was, which on 11 of these 1267 cells (0.9 %) is a numerically zero eigenvalue whose
            argument is round-off; by (M, kk), of 127 (126): (5, 3) 2  (8, 3) 0  (8, 5) 1  (8, 6) 4  (12, 3) 0
            (12, 9) 0  (12, 10) 2  (16, 3) 0  (16, 13) 1  (16, 14) 1, the 4 at (8, 6) being over the cap; a host build of
            the same source landed on the same cells, and on 600 other signatures per case on 1.7-1.8 % at kk = M - 2.

The steering table of k_confidence at A > 16 is uploaded by hand (its fp64 copy and np.angle copy, the two members the
kernel reads): ctx.steering also builds the MFMA operand table, which stops at 16 antennas."""
import numpy as np
import pytest

import angle_ref as R
import radar_oracle as O

pytestmark = pytest.mark.gpu

P = R.PLANTED


# -- k_music_subspace -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M', [1, 2, 3, 5, 8, 15, 16])
def test_music_every_size(ctx, M):
    """Every K in [-M-1, M+1] at n = 25, G = 37 (925 threads: four blocks, the last one partly filled) against the
    Householder-basis den through the explicit reflector, on a steering table with an amplitude taper.  1e-11 on den is the figure of test_music_num_sources_general;
    where den_ref <= 1e-9 the kernel may have cut the spectrum to 0 (den <= 1e-12) instead."""
    from rsl import ops
    steer = R.music_steering(M)
    sigs = R.music_signatures(M, steer, 400 + M)
    den = R.music_den_all(sigs, steer)
    worst = 0.0
    for K in range(-M - 1, M + 2):
        lo = R.music_lo(M, K)
        got = ops.subspace_music(sigs, steer, K, ctx=ctx)
        assert got.shape == (25, 37)
        want = den[:, :, lo]
        with np.errstate(divide='ignore'):
            err = np.abs(1 / got - want)      # inf where the spectrum is 0, nan where it is nan
        live = want > 1e-9
        if live.any():
            worst = max(worst, float(np.nanmax(err[live])))
        assert (err[live] <= 1e-11).all(), (K, np.nanmax(err[live]))
        assert ((got == 0) | (err <= 1e-11))[~live].all(), K
        # the zero signature: eigh(0) is the identity in reversed order, den = sum_{j >= lo} |a_{M-1-j}|^2
        zden = np.sum(np.abs(steer[:, ::-1][:, lo:]) ** 2, axis=1)
        assert (got[21] == 0).all() if lo == M else np.abs(1 / got[21] - zden).max() <= 1e-11, K
        assert np.array_equal(got[24], got[0]) and np.array_equal(got[23], got[1]), K   # no dependence on the index
    print(f'MUSIC M = {M}: largest |1/spec - den_ref| {worst:.2e}')


# -- k_esprit_subspace ------------------------------------------------------------------------------------------------
def _nearest(got, ph):
    """Wrapped phase distance of each output (deg) to the nearest of its candidates ph [n, k]."""
    return np.abs(R.wrap(R.deg_to_phase(got)[:, None] - ph)).min(axis=1)


def _svd_path_first(sigs):
    """angle(eigvals(Phi)[0]) on O.esprit_svd's own path with num_sources = 2 (LAPACK's order)."""
    from scipy.linalg import svd
    out = []
    for s in sigs:
        U, _, _ = svd(np.column_stack([s[:-1], s[1:]]))
        out.append(np.angle(np.linalg.eigvals(np.linalg.pinv(U[:-1, :2]) @ U[1:, :2])[0]))
    return np.array(out)


@pytest.mark.parametrize('M', R.ESPRIT_M)
def test_esprit_determined(ctx, M):
    """n = 130 (three 64-thread blocks).  K = 1 and K = -(M-2) (kk = 1) against O.esprit_closed on all 130; K = 2 and
    K = -(M-3) (kk = 2, M >= 4): the value is one of the reference's two candidates on the 120 signatures of rank 2;
    the 10 noiseless exponentials (rank 1: the second eigenvalue is not reference-determined) are finite and in range."""
    from rsl import ops
    sigs, per = R.determined_case(M)
    tol = R.esprit_tol()
    assert tol <= 2e-12
    closed = R.deg_to_phase(O.esprit_closed(sigs))
    for K, r in per.items():
        got = ops.subspace_esprit(sigs, K, R.ESPRIT_SCALE, ctx=ctx)
        assert got.shape == (130,)
        assert np.isfinite(got).all() and (np.abs(got) <= 90.0).all(), K
        if r['kk'] == 1:
            err = np.abs(R.wrap(R.deg_to_phase(got) - closed))
        else:
            assert r['kk'] == 2 and r['sound'][:120].all() and r['rank1'][120:].all()   # no rank-2 cell is left out
            err = _nearest(got[:120], r['ph'][:120])
            first = int((np.abs(R.wrap(R.deg_to_phase(got[:120]) - _svd_path_first(sigs[:120]))) <= tol).sum())
            print(f'ESPRIT M = {M} K = {K}: {first} of 120 equal eigvals(Phi)[0] of the svd path')
        print(f'ESPRIT M = {M} K = {K} kk = {r["kk"]}: largest phase error {err.max():.2e} rad (tolerance {tol:.2e})')
        assert (err <= tol).all(), (K, err.max(), int(np.argmax(err)))


@pytest.mark.parametrize('M', [3, 4, 8, 16])
def test_esprit_zero_by_construction(ctx, M):
    """kk = M - 1 (K = M-1, M, M+3): Phi = U^H shift U is nilpotent, every eigenvalue is 0 and the value is exactly
    0.0; an empty Phi (K = 0, K = -(M-1)) is 0.0 as well.  The zero signature is finite at every other K."""
    from rsl import ops
    sigs = R.esprit_signatures(M, 300 + M)
    sigs[7] = 0
    for K in (M - 1, M, M + 3, 0, -(M - 1)):
        got = ops.subspace_esprit(sigs, K, R.ESPRIT_SCALE, ctx=ctx)
        assert got.shape == (130,) and (got == 0.0).all(), (K, np.flatnonzero(got != 0.0)[:5])
    for K in range(-M, M + 2):
        assert np.isfinite(ops.subspace_esprit(sigs[5:9], K, R.ESPRIT_SCALE, ctx=ctx)[2]), K


def test_esprit_short_arrays(ctx):
    """M <= 2: X has fewer than two rows, Phi is empty at any K."""
    from rsl import ops
    for M in (1, 2):
        sigs = R.cluster_signatures(M, 700 + M)
        for K in range(-3, 5):
            assert (ops.subspace_esprit(sigs, K, R.ESPRIT_SCALE, ctx=ctx) == 0.0).all(), (M, K)


@pytest.mark.parametrize('M', R.CLUSTER_M)
def test_esprit_zero_cluster(ctx, M):
    """3 <= kk < M - 1 (K = 3, M-3, M-2 and -1): Phi has two non-zero eigenvalues and a Jordan block at 0, and the value
    is the first Schur diagonal entry among the two of largest modulus: finite, in range, the same on a second call and at any index, and on all but 3 %
    of the cells of each (M, K) the angle of one of the two non-zero eigenvalues (measured: on all; module docstring)."""
    from rsl import ops
    sigs, per = R.cluster_case(M)
    distinct = np.setdiff1d(np.arange(130), R.REPEATS)
    over = []
    for K, r in per.items():
        got = ops.subspace_esprit(sigs, K, R.ESPRIT_SCALE, ctx=ctx)
        assert np.isfinite(got).all() and (np.abs(got) <= 90.0).all(), K
        assert np.array_equal(got, ops.subspace_esprit(sigs, K, R.ESPRIT_SCALE, ctx=ctx)), K
        assert (got[list(R.REPEATS)] == got[0]).all(), K
        tol = R.cluster_tol(M, K)
        ok = r['sound'][distinct]
        miss = (_nearest(got[distinct], r['ph'][distinct]) > tol) & ok
        print(f'ESPRIT M = {M} K = {K} kk = {r["kk"]}: {int(miss.sum())} of {int(ok.sum())} cells on the zero cluster '
              f'(tolerance {tol:.2e} rad): {distinct[miss].tolist()}')
        if miss.sum() > 0.03 * ok.sum():
            over.append((K, int(miss.sum()), int(ok.sum())))
    assert not over, over


# -- k_confidence and k_cell_extras on a real layout ------------------------------------------------------------------
def _steer_dev(ctx, steer):
    if steer.shape[1] <= 16:
        return ctx.steering(steer)
    flat = np.ascontiguousarray(steer.astype(np.complex128)).view(np.float64)
    return dict(c128=ctx.to_dev(flat.copy()), phase=ctx.to_dev(np.angle(steer).astype(np.float64)))


@pytest.mark.parametrize('A', R.CONF_A)
def test_confidence(ctx, A):
    """300 cells of a c64 RDS [4, A, 8, 16] against angle_ref.confidence on the fp64-normalised fp32 signature.  1e-12
    absolute: every term is O(1), A <= 32 summands carry a few ulp of libm each, and log10 is clipped at 1 long before
    the percentile gets small enough to matter.  The antenna counts cover the three forms of the percentile's
    interpolation (test_angle_host.py), and 0.4 sqrt(A) > 1 from A = 7 makes the clip at 1.0 live."""
    _, steer = R.steering_table(A)
    rds, frame, rc, gidx, sig32 = R.layout_case(A, 500 + A, R.plant_confidence)
    n = len(rc)
    conf = ctx.confidence(ctx.to_dev(rds), ctx.to_dev(frame), ctx.to_dev(rc), ctx.to_dev(gidx), _steer_dev(ctx, steer), n)
    got = conf.cpu().numpy()
    s = R.normalise32(sig32)
    want = np.array([R.confidence(s[c], steer[gidx[c]]) for c in range(n)])
    err = np.abs(got - want)
    print(f'confidence A = {A}: largest error {err.max():.2e}; planted '
          + ', '.join(f'{k} {got[P[k]]:.6f}' for k in ('zero', 'one_zero', 'pct_zero', 'matched', 'wrap', 'snr_clip')))
    assert got.shape == (n,) and (err <= 1e-12).all(), (err.max(), int(np.argmax(err)))
    assert ((got >= 0) & (got <= 1)).all()
    if A >= 7:
        assert got[P['matched']] == 1.0


@pytest.mark.parametrize('A', R.EXTRAS_A)
def test_cell_extras(ctx, A):
    """The <4>, <8>, <16> instances and run-time A on both sides of 16, 300 cells of a c64 RDS [4, A, 8, 16].
    sig_out: fp32 rounding of a value <= 1 is 2^-25 per component, 2^-23 asked.  phase: each of the two sums of two
    products errs by <= 2e-16, divided by a modulus >= 1e-3 that is <= 2e-13 rad, 1e-12 asked; a product that is exactly
    0 gives exactly 0.0.  esprit: the closed form, and (up to its 16 antennas) k_esprit_subspace with K = 1 on the same
    values, as phases."""
    from rsl import ops
    grid, _ = R.steering_table(A)
    az_table = np.radians(grid)
    rds, frame, rc, gidx, sig32 = R.layout_case(A, 600 + A, R.plant_extras)
    n = len(rc)
    d, fr, rcd, gd, azd = (ctx.to_dev(x) for x in (rds, frame, rc, gidx, az_table))
    want = dict(want_sig=True, want_esprit=True, want_phase=True, gidx=gd, az_table=azd)
    sig, esp, ph, az = (t.cpu().numpy() for t in ctx.cell_extras(d, fr, rcd, n=n, **want))
    s, phase, closed = R.cell_extras(sig32)
    assert sig.shape == (n, A) and sig.dtype == np.complex64
    assert np.abs(sig - s).max() <= 2.0 ** -23
    live = np.abs(s[:, 0]) * np.abs(s[:, 1]) >= 1e-3
    assert live.sum() >= 200
    perr = np.abs(R.wrap(ph - phase))
    assert (perr[live] <= 1e-12).all(), perr[live].max()
    planted = [P['zero'], *P['s0_zero'], *P['s1_zero']]
    assert (ph[planted] == 0.0).all(), ph[planted]
    assert np.isfinite(ph).all() and np.isfinite(esp).all()
    if A == 2:     # no row to regress on: dd = 0 -> exactly 0.0 (the numpy closed form has nothing to return here)
        assert (esp == 0.0).all()
    else:
        tol = R.esprit_tol()
        eerr = np.abs(R.wrap(R.deg_to_phase(esp) - R.deg_to_phase(closed)))
        serr = np.zeros(n)
        if A <= 16:   # rsl_esprit_subspace takes up to 16 antennas
            sub = ops.subspace_esprit(s, 1, R.ESPRIT_SCALE, ctx=ctx)
            serr = np.abs(R.wrap(R.deg_to_phase(esp) - R.deg_to_phase(sub)))
        print(f'cell_extras A = {A}: phase {perr[live].max():.2e}, esprit vs closed {eerr.max():.2e}, vs subspace '
              f'{serr.max():.2e} rad (tolerance {tol:.2e})')
        assert (eerr <= tol).all(), (eerr.max(), int(np.argmax(eerr)))
        assert (serr <= tol).all(), (serr.max(), int(np.argmax(serr)))
        assert esp[P['zero']] == 0.0
    assert np.array_equal(az, az_table[gidx])
    # the device-side count bounds the cells: rows from n_dev on keep what the buffers held
    torch = ctx.torch
    bufs = {k: torch.full((n,), -77.0, dtype=torch.float64, device=ctx.device) for k in ('esprit', 'phase', 'az')}
    n_dev = ctx.to_dev(np.array([200], dtype=np.int64))
    _, e2, p2, a2 = ctx.cell_extras(d, fr, rcd, n=n, n_dev=n_dev, want_esprit=True, want_phase=True, gidx=gd,
                                    az_table=azd, bufs=bufs)
    for t, full in ((e2, esp), (p2, ph), (a2, az)):
        t = t.cpu().numpy()
        assert np.array_equal(t[:200], full[:200]) and (t[200:] == -77.0).all()


def test_cell_extras_one_antenna(ctx):
    """A = 1 has no s1: an invalid argument (ValueError), not a launch error."""
    d = ctx.to_dev(np.ones((1, 1, 2, 2), np.complex64))
    z = ctx.to_dev(np.zeros(1, np.int32))
    with pytest.raises(ValueError, match='at least 2 antennas'):
        ctx.cell_extras(d, z, z, n=1, want_phase=True)
