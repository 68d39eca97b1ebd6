"""CPU: the references of tests/angle_ref.py and the inputs of tests/test_gpu_angle_kernels.py are sound before any GPU
is involved.  Every test is a property of the references alone.

Reference spread (the largest phase difference between the ESPRIT candidates from the Gram-Schmidt basis and from
LAPACK's QR of the same columns, over the sound inputs; printed by test_span_invariance), measured with numpy 2.2 /
OpenBLAS:
    determined inputs (kk <= 2, M = 3 .. 16):   8.9e-15 rad
    3 <= kk < M - 1, by (M, K):                 4e-15 (kk = 3) .. 1.6e-6 rad (M = 12, kk = 10; M = 16, kk = 13)
The second figure is not an error of either construction: the two non-zero eigenvalues of Phi sit next to a Jordan
block of size kk - 2 at 0, and their condition number grows with it.  So the GPU tests use 100 x the first figure
for every reference-determined value and, at a (M, K) with 3 <= kk < M - 1, 100 x that case's own spread where it is
larger (angle_ref.esprit_tol / cluster_tol)."""
import numpy as np
import pytest

import angle_ref as R
import radar_oracle as O


def _cases():
    for kind, Ms in (('determined', R.ESPRIT_M), ('cluster', R.CLUSTER_M)):
        for M in Ms:
            for K, r in R._case(kind, M)[1].items():
                yield kind, M, K, r


def test_span_invariance():
    """The candidate sets of the two basis constructions agree: the determined inputs to 2e-14 rad (so the tolerance of
    the GPU tests is at most 2e-12), the 3 <= kk < M - 1 inputs to a hundredth of the 1e-3 rad that separates their
    candidates."""
    for kind, M, K, r in _cases():
        print(f'{kind:10s} M = {M:2d}  K = {K:3d}  kk = {r["kk"]:2d}  spread {R.case_spread(kind, M, K):.2e} rad')
    det, clu = R.reference_spread('determined'), R.reference_spread('cluster')
    print(f'reference spread: determined {det:.2e} rad, 3 <= kk < M - 1 {clu:.2e} rad; tolerance {R.esprit_tol():.2e}')
    assert 0 < det <= 2e-14
    assert clu <= 1e-5
    for M in R.CLUSTER_M:
        for K in R.cluster_K(M):
            assert R.esprit_tol() <= R.cluster_tol(M, K) <= 1e-3


def test_nilpotent_at_full_rank():
    """kk = M - 1: Us is a full unitary U and Phi = U^H shift U, so Phi^L = 0 and every eigenvalue is 0: the kernel
    writes 0.0 there, where numpy's eigvals returns a ring of modulus eps^(1/L)."""
    for M in range(3, 17):
        L = M - 1
        for s in R.esprit_signatures(M, 300 + M)[[0, 50, 110, 125]]:
            for basis in (R.basis_gs, R.basis_qr):
                Phi = R.esprit_phi(s, L, basis)
                assert Phi.shape == (L, L)
                assert np.linalg.norm(np.linalg.matrix_power(Phi, L)) <= 1e-12, M
        assert R.esprit_kk(M, M - 1) == R.esprit_kk(M, M) == R.esprit_kk(M, M + 3) == L


def test_inputs_sound():
    """K = 2 at M >= 4: both eigenvalues have modulus > 1e-3 and their phases are more than 1e-3 rad apart.
    3 <= kk < M - 1: the third-largest modulus is at most half the second, and the two largest are more than 1e-3 rad
    apart.  An input that fails is dropped (by the reference); at most 5 % per (M, K)."""
    worst3 = 0.0
    for kind, M, K, r in _cases():
        live = ~r['rank1']
        ok = r['sound']
        assert not (ok & r['rank1']).any()
        dropped = int((live & ~ok).sum())
        print(f'{kind:10s} M = {M:2d}  K = {K:3d}  dropped {dropped} of {int(live.sum())}')
        assert dropped <= 0.05 * live.sum(), (M, K, dropped)
        if r['kk'] == 1:
            assert ok.all()
        elif r['kk'] == 2:
            assert (r['mod'][ok, 1] > 1e-3).all()
            assert (np.abs(R.wrap(r['ph'][ok, 0] - r['ph'][ok, 1])) > 1e-3).all()
            assert int(r['rank1'].sum()) == 10
        else:
            assert (r['mod'][ok, 2] <= 0.5 * r['mod'][ok, 1]).all()
            assert (np.abs(R.wrap(r['ph'][ok, 0] - r['ph'][ok, 1])) > 1e-3).all()
            worst3 = max(worst3, float((r['mod'][ok, 2] / r['mod'][ok, 1]).max()))
    print(f'largest third / second modulus among the kept inputs: {worst3:.2f}')


def test_rank_one_inputs():
    """The 10 noiseless exponentials make X rank 1: the span takes e_0 in place of the second singular vector, and at
    kk = 1 the candidate is the exponential's own phase."""
    for M in R.ESPRIT_M:
        sigs, per = R.determined_case(M)
        for s in sigs[120:]:
            sv = np.linalg.svd(np.column_stack([s[:-1], s[1:]]), compute_uv=False)
            assert sv[1] <= 1e-14 * sv[0]
            cols, _ = R.span_columns(s, 2)
            assert np.array_equal(cols[:, 1], np.eye(M - 1)[:, 0])
        om = np.angle(sigs[120:, 1] / sigs[120:, 0])
        assert np.abs(R.wrap(per[1]['ph'][120:, 0] - om)).max() <= 1e-13


def test_music_reference_consistency():
    for M in (1, 2, 3, 5, 8, 15, 16):
        _, steer = R.steering_table(M)
        sigs = R.music_signatures(M, steer, 400 + M)
        den = R.music_den_all(sigs, steer)
        for c in (0, 7, 20, 21, 22):
            for g in (0, 12, 36):
                for K in range(-M - 1, M + 2):
                    assert abs(R.music_den(sigs[c], steer[g], K) - den[c, g, R.music_lo(M, K)]) <= 1e-13
        assert np.abs(den[:, :, 0] - M).max() <= 1e-12 * M            # K = 0: |a|^2
        assert (den[:, :, M] == 0).all()                                # K >= M: no noise subspace
        for K in (M, M + 1):
            assert R.music_den(sigs[3], steer[5], K) == 0.0
        if M >= 2:   # K = 1: the closed form den = M - |a^H s|^2 (zero signature: M - 1)
            closed = O.music_spectrum_closed(sigs, steer)
            dc = 1 / np.where(closed > 0, closed, np.inf)
            live = dc > 1e-9
            assert np.abs(den[:, :, 1] - dc)[live].max() <= 1e-12 * M
            assert (den[:, :, 1][~live] <= 1e-9).all()
            assert abs(den[22, len(steer) // 3, 1]) <= 1e-12 * M        # the steering row: den -> 0 at its own angle
        assert np.array_equal(sigs[24], sigs[0]) and np.array_equal(sigs[23], sigs[1]) and not sigs[21].any()
        assert sigs[20, 0] == 0
        # the tapered table of the GPU test: a zero signature's den depends on the column order (reversed identity)
        tap = R.music_steering(M)
        zden = R.music_den_all(sigs[21:22], tap)[0]
        for lo in range(M + 1):
            assert np.abs(zden[:, lo] - np.sum(np.abs(tap[:, :M - lo]) ** 2, axis=1)).max() <= 1e-12 * M
            if 0 < lo < M:
                assert np.abs(zden[:, lo] - np.sum(np.abs(tap[:, lo:]) ** 2, axis=1)).min() > 0.01


def test_esprit_reference_consistency():
    """kk = 1 equals O.esprit_closed; Phi is empty exactly where kk = 0 or M <= 2; Python slicing for kk."""
    for M in R.ESPRIT_M:
        sigs, per = R.determined_case(M)
        closed = R.deg_to_phase(O.esprit_closed(sigs))
        for K in (1, -(M - 2)):
            assert per[K]['kk'] == 1
            assert np.abs(R.wrap(per[K]['ph'][:, 0] - closed)).max() <= 1e-13, (M, K)
            deg = np.array([R.esprit_candidates(s, K)[2][0] for s in sigs[:5]])
            assert R.phase_err(deg, closed[:5]).max() <= 1e-13
    s = R.esprit_signatures(8, 1)[0]
    assert R.esprit_candidates(s, 0) is None and R.esprit_candidates(s, -7) is None and R.esprit_candidates(s, -9) is None
    assert R.esprit_candidates(s[:2], 1) is None and R.esprit_candidates(s[:2], 5) is None
    assert [R.esprit_kk(8, K) for K in (-9, -7, -6, -1, 0, 1, 6, 7, 8, 11)] == [0, 0, 1, 6, 0, 1, 6, 7, 7, 7]
    assert R.cluster_K(5) == [3, -1] and R.cluster_K(8) == [3, 5, 6, -1] and R.cluster_K(16) == [3, 13, 14, -1]
    # the phase comparison wraps: +-90 degrees are one phase
    assert R.phase_err(90.0, -np.pi) <= 1e-15 and R.phase_err(-90.0, np.pi) <= 1e-15
    assert R.wrap(np.pi) == np.pi and R.wrap(-np.pi) == np.pi and R.wrap(3 * np.pi / 2) == -np.pi / 2


@pytest.mark.parametrize('A', [2, 3, 8, 32])
def test_confidence_reference(A):
    """confidence equals O.angle_confidence on the oracle's own steering vector (any A it accepts), and the planted
    cells of the GPU test do what they are planted for."""
    grid, steer = R.steering_table(A)
    rds, frame, rc, gidx, sig32 = R.layout_case(A, 500 + A, R.plant_confidence)
    s = R.normalise32(sig32)
    for c in list(range(12)) + [150, 299]:
        assert R.confidence(s[c], steer[gidx[c]]) == O.angle_confidence(s[c], grid[gidx[c]], num_antennas=A)
    F, S, C, n = (R.LAYOUT[k] for k in ('F', 'S', 'C', 'n'))
    assert len(set(zip(frame.tolist(), rc.tolist()))) == n and set(frame.tolist()) == set(range(F))
    assert (frame[0], rc[0]) == (0, 0) and (frame[1], rc[1]) == (F - 1, S * C - 1)
    P = R.PLANTED
    assert not s[P['zero']].any() and R.confidence(s[P['zero']], steer[gidx[P['zero']]]) == 0.3 * np.exp(
        -np.mean(np.abs(np.angle(steer[gidx[P['zero']]]))))
    assert s[P['one_zero'], A // 2] == 0 and s[P['one_zero']].any()
    assert np.percentile(np.abs(s[P['pct_zero']]) ** 2, 20) == 0
    m, am = s[P['matched']], steer[gidx[P['matched']]]
    assert abs(np.abs(np.vdot(am, m)) - np.sqrt(A)) <= 1e-6
    if A >= 7:   # 0.4 sqrt(A) > 1: the clip
        assert R.confidence(m, am) == 1.0
    w = s[P['wrap']]
    assert np.abs(np.abs(np.angle(w)) - np.pi).max() <= 1e-6 and (np.angle(w[1:]) < 0).all()


def test_confidence_percentile_forms():
    """The antenna counts of the GPU test reach all three forms of numpy's linear interpolation at index 0.2 (A - 1):
    an integer index, a fraction below 0.5 and a fraction of at least 0.5."""
    forms = {}
    for A in R.CONF_A:
        vi = 0.2 * (A - 1)
        f = vi - np.floor(vi)
        forms.setdefault('integer' if f == 0 else 'low' if f < 0.5 else 'high', []).append(A)
    print(forms)
    assert set(forms) == {'integer', 'low', 'high'}
    assert 32 in R.CONF_A and {4, 8, 16} <= set(R.CONF_A) and {4, 8, 16, 17, 32} <= set(R.EXTRAS_A)


def test_cell_extras_reference():
    rds, frame, rc, gidx, sig32 = R.layout_case(5, 600, R.plant_extras)
    s, phase, esp = R.cell_extras(sig32)
    n2 = np.sum(np.abs(s) ** 2, axis=1)
    assert np.abs(n2[n2 > 0] - 1).max() <= 1e-15 and (n2 == 0).sum() == 1
    assert np.array_equal(sig32, rds[frame, :, rc // R.LAYOUT['C'], rc % R.LAYOUT['C']])
    assert np.abs(R.wrap(phase - np.angle(sig32[:, 1].astype(complex) * np.conj(sig32[:, 0].astype(complex))))
                  ).max() <= 1e-15
    P = R.PLANTED
    assert not s[list(P['s0_zero']), 0].any() and not s[list(P['s1_zero']), 1].any()
    assert s[list(P['s0_zero']), 1].all() and s[list(P['s1_zero']), 0].all()
    assert R.cell_extras(sig32[:, :2])[2] is None
    e1 = np.array([R.esprit_candidates(x, 1)[1][0] for x in s[8:40]])
    assert np.abs(R.wrap(R.deg_to_phase(esp[8:40]) - e1)).max() <= 1e-13
