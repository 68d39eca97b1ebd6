"""CPU tests of the range-azimuth maps: the resolution statement on the fp64 oracle alone (tests/ra_ref.py), the
ChainConfig and rsl.ops argument checks (raised before any device is touched), and the identity that ties the Doppler-bin
covariance to the chirp-domain one."""
import numpy as np
import pytest

import ra_ref as R
import radar_oracle as O


def test_oracle_resolution_statement():
    """Two 20 dB sources 10 degrees apart, each in its own 4 of 32 Doppler bins, 8 antennas, loading 1e-2: Capon shows
    two local maxima within 2 degrees of the truth in every one of 200 range bins, Bartlett in none."""
    z, truth, g, st = R.resolution_scene()
    st64 = st.astype(np.complex64)
    cov = R.cov_ref(z[None])[0]
    assert cov.shape == (200, 8, 8) and len(g) == 181
    cap = R.map_ref(cov, st64, 'capon', R.RES['loading'])
    assert R.count_resolved(cap['map'], g, truth) == 200
    assert R.count_resolved(R.map_ref(cov, st64, 'bartlett')['map'], g, truth) == 0
    assert cap['kappa'].max() <= 8 / R.RES['loading'] + 1  # cond(R_l) <= A / loading + 1


def test_oracle_single_source_level():
    """Both estimators return the source power + noise / A for one source in white noise (exact covariance)."""
    A, P, s2 = 8, 7.0, 0.5
    sv = R.steering([12.0], R.ula(A))
    cov = (P * np.outer(sv[0], sv[0].conj()) + s2 * np.eye(A))[None]
    for method in ('bartlett', 'capon'):
        got = R.map_ref(cov, sv, method, 1e-4)['map'][0, 0]
        want = P + s2 / A
        assert abs(got - want) <= (1e-12 if method == 'bartlett' else 2e-4 * want), (method, got, want)


def test_doppler_covariance_is_the_chirp_covariance():
    """Parseval along slow time: over the full window the Doppler-bin covariance (1/C) sum_c x_c x_c^H of a range bin
    equals the sum over the chirps of y y^H of that bin's range spectra, i.e. C times the chirp-domain covariance
    Y Y^H / C (the Doppler FFT is unnormalised).  Checked in fp64 on the oracle's RDS, DC removal off; the window acts
    along fast time only and does not enter."""
    A, C, Tc = 4, 16, 3.2e-6
    np.random.seed(5)
    frame = O.synthesize_frame(O.TEST_SCENE, chirp_duration=Tc, num_chirps=C, num_antennas=A)
    rds = O.range_doppler_spectrum(frame, chirp_duration=Tc, dc_removal=False)  # [A, S, C]
    bb = frame * np.conj(O.reference_chirp(77e9, 1e9, Tc, 10e6)) * O.window('hann', frame.shape[-1])
    y = np.fft.fftshift(np.fft.fft(bb, axis=-1), axes=-1)  # range spectra [A, C, S]
    want = np.einsum('pcr,qcr->rpq', y, y.conj())  # sum over the chirps = C (Y Y^H / C)
    got = R.cov_ref(rds[None])[0]
    assert got.shape == want.shape == (frame.shape[-1], A, A)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_chain_config_validation():
    import rsl
    assert rsl.ChainConfig().ra_map is None and rsl.ChainConfig().ra_doppler is None
    assert rsl.ChainConfig().ra_loading == 1e-2
    rsl.ChainConfig(ra_map='capon', ra_doppler=(0, 128), ra_loading=1e-4)
    rsl.ChainConfig(ra_map='bartlett', num_antennas=16, ra_doppler=(127, 128), ra_loading=1.0)
    for kw, msg in ((dict(ra_map='music'), "ra_map must be None, 'bartlett' or 'capon'"),
                    (dict(ra_map='capon', ra_doppler=(5, 5)), r'ra_doppler must be \(c0, c1\)'),
                    (dict(ra_map='capon', ra_doppler=(-1, 5)), 'ra_doppler must be'),
                    (dict(ra_map='capon', ra_doppler=(0, 129)), 'c1 <= 128'),
                    (dict(ra_map='capon', ra_doppler=(0, 17), num_chirps=16), 'c1 <= 16'),
                    (dict(ra_map='capon', ra_doppler=(1, 2, 3)), 'ra_doppler must be'),
                    (dict(ra_map='capon', ra_loading=9e-5), r'ra_loading must lie in \[0.0001, 1\]'),
                    (dict(ra_loading=1.5), 'ra_loading must lie in'),
                    (dict(ra_loading=float('nan')), 'ra_loading must lie in'),
                    (dict(ra_map='capon', num_antennas=1), 'ra_map needs 2 to 16 antennas'),
                    (dict(ra_map='bartlett', num_antennas=17), 'ra_map needs 2 to 16 antennas')):
        with pytest.raises(ValueError, match=msg):
            rsl.ChainConfig(**kw)
    rsl.ChainConfig(num_antennas=32)  # without ra_map the antenna count is not its business


def test_ops_value_errors_come_before_any_launch():
    """Every check below raises before a context is made: the test passes without a device."""
    from rsl import ops
    st = R.steering(R.grid(37), R.ula(8))
    z = np.zeros((8, 4, 16), np.complex64)
    cov = np.zeros((4, 8, 8), np.complex64)
    for bad, msg in ((np.zeros((4, 16), np.complex64), 'rds must be'),
                     (np.zeros((1, 4, 16), np.complex64), 'antennas outside'),
                     (np.zeros((17, 4, 16), np.complex64), 'antennas outside'),
                     (np.zeros((8, 0, 16), np.complex64), 'empty range or Doppler axis')):
        with pytest.raises(ValueError, match=msg):
            ops.range_covariance(bad)
    for win in ((-1, 4), (4, 4), (5, 4), (0, 17)):
        with pytest.raises(ValueError, match='Doppler window'):
            ops.range_covariance(z, doppler=win)
        with pytest.raises(ValueError, match='Doppler window'):
            ops.range_azimuth_map(st, rds=z, doppler=win)
    with pytest.raises(ValueError, match="method must be 'bartlett' or 'capon'"):
        ops.range_azimuth_map(st, rds=z, method='music')
    for loading in (0.0, 9.9e-5, 1.01, float('nan')):
        with pytest.raises(ValueError, match='loading'):
            ops.range_azimuth_map(st, rds=z, loading=loading)
    with pytest.raises(ValueError, match='exactly one of rds and cov'):
        ops.range_azimuth_map(st)
    with pytest.raises(ValueError, match='exactly one of rds and cov'):
        ops.range_azimuth_map(st, rds=z, cov=cov)
    with pytest.raises(ValueError, match='RDS of 4 antennas, steering matrix of 8'):
        ops.range_azimuth_map(st, rds=np.zeros((4, 4, 16), np.complex64))
    with pytest.raises(ValueError, match='covariances of 4 antennas'):
        ops.range_azimuth_map(st, cov=np.zeros((3, 4, 4), np.complex64))
    with pytest.raises(ValueError, match=r'cov must be \[.., A, A\]'):
        ops.range_azimuth_map(st, cov=np.zeros((3, 8, 7), np.complex64))
    with pytest.raises(ValueError, match='steer_c128 must be'):
        ops.range_azimuth_map(st[0], rds=z)
    with pytest.raises(ValueError, match='antennas outside'):
        ops.range_azimuth_map(R.steering(R.grid(37), R.ula(17)), cov=np.zeros((3, 17, 17), np.complex64))


def test_binding_constants_match_the_header():
    import os
    import re
    from rsl import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rsl.h')).read()
    vals = dict(re.findall(r'^#define (RSL_RA_[A-Z_]+) (\S+)', src, flags=re.M))
    assert vals == {'RSL_RA_BARTLETT': '0', 'RSL_RA_CAPON': '1', 'RSL_RA_MAX_A': '16', 'RSL_RA_MIN_LOADING': '1e-4'}
    assert (_lib.RA_BARTLETT, _lib.RA_CAPON, _lib.RA_MAX_A, _lib.RA_MIN_LOADING) == (0, 1, 16, 1e-4)
    assert _lib.RA_IDS == {'bartlett': 0, 'capon': 1}
