"""CPU: the two restatements the GPU tests of the scene and per-call kernels lean on (tests/scene_ref.py,
tests/aux_ref.py), pinned to something more literal than themselves."""
import numpy as np

import aux_ref as A
import scene_ref as S


def test_topk_ref_is_the_reference_selection():
    """topk_ref against the three reference lines (robust_angle_estimation.py:363-365) run on a list of peak dicts as
    extract_range_doppler_peaks builds them, on a tie-heavy input with signed zeros, a NaN and values at the threshold."""
    rs = np.random.RandomState(0)
    pdb = (np.round(rs.uniform(-30.0, -20.0, 400)) / 1.0).astype(np.float32)  # 11 levels: ties everywhere
    pdb[[3, 50, 51, 300]] = [0.0, -0.0, 0.0, -0.0]
    pdb[7] = np.nan
    pdb[[8, 9]] = [-25.0, np.nextafter(np.float32(-25.0), np.float32(0.0))]
    peaks = [{'range_bin': i // 20, 'doppler_bin': i % 20, 'power_db': float(p)} for i, p in enumerate(pdb)]
    for max_targets in (1, 4, 50, 256, 1000):
        filtered_peaks = [p for p in peaks if p['power_db'] > -25.0]
        filtered_peaks.sort(key=lambda x: x['power_db'], reverse=True)
        filtered_peaks = filtered_peaks[:max_targets]
        want = [p['range_bin'] * 20 + p['doppler_bin'] for p in filtered_peaks]
        assert S.topk_ref(pdb, -25.0, max_targets) == want
    sel = S.topk_ref(pdb, -25.0, 1000)
    assert sel[:4] == [3, 50, 51, 300]  # +0 and -0 compare equal: entry order
    assert 7 not in sel and 8 not in sel and 9 in sel
    assert all(pdb[a] > pdb[b] or (pdb[a] == pdb[b] and a < b) for a, b in zip(sel, sel[1:]))


def test_pair_phase_is_the_angle_of_the_product():
    rs = np.random.RandomState(1)
    c, p = rs.randn(200) + 1j * rs.randn(200), rs.randn(200) + 1j * rs.randn(200)
    np.testing.assert_allclose(S.pair_phase(c, p), np.angle(c * np.conj(p)), rtol=0, atol=1e-15)


def test_associate_ieee_is_the_oracle_rule():
    """associate_ieee (x * x for the squares) against the oracle's associate_analyzer (x ** 2: libm's pow) on lattice and
    continuous targets: the same matches, the first of tied previous targets included; distances equal to the bit on
    the lattice (its squares are exact either way) and within an ulp elsewhere."""
    import radar_oracle as O
    rs = np.random.RandomState(3)
    for lattice in (True, False):
        pr = rs.randint(0, 40, 60) * 0.5 if lattice else rs.uniform(0, 20, 60)
        pa = rs.randint(-4, 5, 60) * 0.25 if lattice else rs.uniform(-1, 1, 60)
        cr = rs.randint(0, 60, 90) * 0.5 if lattice else rs.uniform(0, 30, 90)
        ca = rs.randint(-4, 5, 90) * 0.25 if lattice else rs.uniform(-1, 1, 90)
        pr[7], pa[7] = pr[3], pa[3]  # a duplicate previous target
        for thr in (5.0, 1.0, 0.0):
            m, d = O.associate_analyzer(cr, ca, pr, pa, thr=thr)
            mi, di = S.associate_ieee(cr, ca, pr, pa, thr)
            assert np.array_equal(m, mi), (lattice, thr)
            assert 7 not in mi
            hit = m >= 0
            assert np.array_equal(np.isinf(d), np.isinf(di))
            if lattice:
                assert np.array_equal(d[hit], di[hit])
            else:
                assert (np.abs(d[hit] - di[hit]) <= np.spacing(di[hit])).all()
    assert S.associate_ieee(cr, ca, pr[:0], pa[:0], 5.0)[0].tolist() == [-1] * 90


def test_bvls_ref_against_active_set_enumeration():
    """scipy's BVLS (bvls_ref) against the minimum over all 27 active sets for nv = 3: the same cost, and the same x
    where the optimum is unique."""
    seen = 0
    for P in A.bvls_problems(7, 120):
        if len(P['lo']) != 3:
            continue
        Jk = P['k'] * A.jacobian(P['pos'], P['ang'])[:, :3]
        x, c, cond = A.bvls_ref(Jk, P['y'], P['lo'], P['hi'], P['ridge'])
        xb, cb = A.bvls_brute(Jk, P['y'], P['lo'], P['hi'], P['ridge'])
        assert xb is not None, P['name']
        yy = float(P['y'] @ P['y'])
        assert abs(c - cb) <= 1e-9 * cb + 1e-12 * yy, (P['name'], c, cb)
        if cond < 1e8:
            assert np.abs(x - xb).max() <= 1e-7, (P['name'], x, xb)
            seen += 1
    assert seen >= 20


def test_preprocess_ref_mean_free():
    rs = np.random.RandomState(2)
    x = (rs.randn(3, 50) + 1j * rs.randn(3, 50) + 100).astype(np.complex64)
    t = (rs.randn(50) + 1j * rs.randn(50)).astype(np.complex64)
    out = A.preprocess_ref(x, t, True)
    assert out.dtype == np.complex128 and np.abs(out.mean(axis=1)).max() < 1e-12
    assert np.array_equal(A.preprocess_ref(x, t, False), x.astype(np.complex128) * t.astype(np.complex128))
