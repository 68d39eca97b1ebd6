"""GPU tests of the range-azimuth maps: rsl_range_cov / k_range_cov (the per-range spatial covariance as one fp32 MFMA
Gram tile), rsl_range_azimuth / k_range_azimuth (Bartlett and Capon over a steering table), the chain option ra_map and
the drop-in method, against the fp64 oracle of tests/ra_ref.py.

Each parity test prints its largest error in units of its bound's scale before it asserts.  Measured on one MI355X:
covariance 0.7-6.9 u sqrt(R_pp R_qq) against bounds of 10-264 u; Bartlett 2.3-4.3 u t / A against 16-520; Capon 1.7-3.6
u kappa ref against 16-128."""
import ctypes

import numpy as np
import pytest

import ra_ref as R

pytestmark = pytest.mark.gpu

MARGIN = 4096  # sentinel elements on each side of a tested output
_cache = {}


def ident(v):
    return '-'.join('full' if x is None else ('%d_%d' % x if isinstance(x, tuple) else str(x)) for x in v)


def sentinel_out(ctx, shape, dtype, fill):
    """(flat buffer, its view of `shape` MARGIN elements in) filled with `fill`."""
    torch = ctx.torch
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * MARGIN,), fill, dtype=dtype, device=ctx.device)
    return buf, buf[MARGIN:MARGIN + n].view(shape)


def margins_untouched(buf, n, fill):
    head, tail = buf[:MARGIN].cpu().numpy(), buf[MARGIN + n:].cpu().numpy()
    want = np.full(MARGIN, fill, dtype=head.dtype)
    return head.tobytes() == want.tobytes() and tail.tobytes() == want.tobytes()


# -- 1. the covariance ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', R.COV_CASES, ids=ident)
def test_cov_against_fp64(ctx, case):
    """|cov - ref| <= 2 (Cw + 4) u sqrt(ref_pp ref_qq); exactly Hermitian; the zero bin exactly 0; margins untouched;
    a batch equals its frames run alone, bitwise."""
    F, A, S, C, win = case
    c0, c1 = win or (0, C)
    z, zero = R.cov_input(F, A, S, C, 100 * A + C)
    dev = ctx.to_dev(z)
    fill = complex(-7.5, 3.25)
    buf, out = sentinel_out(ctx, (F, S, A, A), ctx.torch.complex64, fill)
    got = ctx.range_cov(dev, win, out=out)
    ctx.torch.cuda.synchronize()
    assert got is out
    g = out.cpu().numpy()
    assert margins_untouched(buf, F * S * A * A, fill)
    ref = R.cov_ref(z, c0, c1)
    bound = R.cov_bound(ref, c1 - c0)
    err = np.abs(g.astype(np.complex128) - ref)
    scale = np.sqrt(np.abs(np.einsum('...pp->...p', ref).real))
    scale = scale[..., :, None] * scale[..., None, :]
    rel = float((err[scale > 0] / scale[scale > 0]).max())
    print(f'\ncov {case}: max |cov - ref| / sqrt(ref_pp ref_qq) = {rel:.3e} = {rel / R.U:.2f} u, '
          f'bound {2 * (c1 - c0 + 4)} u')
    assert (err <= bound).all(), (case, float((err - bound).max()))
    gt = np.swapaxes(g, -1, -2)
    assert (g.real.view(np.int32) == gt.real.view(np.int32)).all()  # bitwise conjugate pairs
    assert (g.imag == -gt.imag).all() and (np.einsum('...pp->...p', g).imag == 0).all()
    assert (np.einsum('...pp->...p', g).real >= 0).all()
    if zero is not None:
        assert not g[:, zero].any()
    else:  # a single range bin: the same launch on the zeroed input
        assert not ctx.range_cov(ctx.to_dev(np.zeros_like(z)), win).cpu().numpy().any()
    if F > 1:
        for f in range(F):
            alone = ctx.range_cov(dev[f:f + 1].contiguous(), win).cpu().numpy()
            assert alone.tobytes() == g[f:f + 1].tobytes(), (case, f)


def test_cov_unaligned_input_takes_the_one_bin_steps(ctx):
    """An RDS 8 bytes into an allocation has no 16-B aligned rows: the same tile by one c64 per lane.  The sum over k
    is then formed in another order, so the two agree within the bound, not bitwise."""
    torch = ctx.torch
    shape = (2, 8, 9, 64)
    z, _ = R.cov_input(*shape, 77)
    buf = torch.empty((z.size + 1,), dtype=torch.complex64, device=ctx.device)
    view = buf[1:].view(shape)
    view.copy_(ctx.to_dev(z))
    assert view.data_ptr() % 16 == 8
    g = ctx.range_cov(view).cpu().numpy()
    ref = R.cov_ref(z)
    assert (np.abs(g.astype(np.complex128) - ref) <= R.cov_bound(ref, 64)).all()
    assert (g == np.conj(np.swapaxes(g, -1, -2))).all()


def test_cov_small_integers_are_exact(ctx):
    """Integer parts up to 8 and a power-of-two window: every product, sum and the scaling is exact in fp32, so any
    wrong lane, row or quadrant shows as a whole-number error (both tile sizes, pad rows, asymmetric data)."""
    for A, C in ((5, 16), (8, 64), (11, 8), (16, 32)):
        rng = np.random.default_rng(A)
        z = (rng.integers(-8, 9, (2, A, 3, C)) + 1j * rng.integers(-8, 9, (2, A, 3, C))).astype(np.complex64)
        g = ctx.range_cov(ctx.to_dev(z)).cpu().numpy()
        assert (g.astype(np.complex128) == R.cov_ref(z)).all(), (A, C)


# -- 2. the spectrum ----------------------------------------------------------------------------------------------------
NS = (1, 15, 17, 1003)
GS = (1, 37, 361)
LOADINGS = (1e-4, 1e-2, 1.0)


def covs(A):
    if A not in _cache:
        _cache[A] = R.psd_covs(A, max(NS), 10 + A)
    return _cache[A]


def check_rows(tag, m, arg, ref, method, A, worst):
    """Device map [n, G] and arg [n] against the oracle's rows; updates worst[method] (error / bound scale)."""
    bound = R.map_bound(ref, method, A)
    err = np.abs(m.astype(np.float64) - ref['map'])
    live = ref['t'] > 0
    if live.any():
        if method == 'bartlett':
            s = float((err[live] / (R.U * ref['t'][live] / A)[:, None]).max())  # in units of u t / A
        else:
            s = float((err[live] / (R.U * ref['kappa'][live, None] * ref['map'][live])).max())  # in units of u kappa ref
        worst[method] = max(worst.get(method, 0.0), s)
    assert (err <= bound).all(), (tag, float((err - bound).max()))
    assert not m[~live].any() and not arg[~live].any(), tag
    assert (arg == np.argmax(m, axis=1)).all(), tag  # the device row's first maximum
    n = np.arange(len(arg))
    assert (ref['map'][n, arg] >= ref['map'].max(axis=1) - bound.max(axis=1)).all(), tag


@pytest.mark.parametrize('array', ['ula', 'perturbed'])
@pytest.mark.parametrize('A', [2, 3, 8, 9, 16])
def test_spectrum_against_fp64(ctx, A, array):
    """Bartlett: |map - ref| <= (2 A^2 + 8) u t / A.  Capon: |map - ref| <= 8 A u kappa(R_l) ref.  Every G, n and
    loading of the issue; the lower triangle and the diagonal's imaginary part of the device input are NaN (not
    read)."""
    torch = ctx.torch
    c = covs(A)
    dirty = c.copy()
    lo = np.tril_indices(A, -1)
    dirty[:, lo[0], lo[1]] = np.nan
    diag = c[:, np.arange(A), np.arange(A)].copy()
    diag.imag = np.nan
    dirty[:, np.arange(A), np.arange(A)] = diag
    assert np.isfinite(dirty.real[:, np.arange(A), np.arange(A)]).all()
    dev = ctx.to_dev(dirty)
    pos = R.ula(A) if array == 'ula' else R.perturbed(A)
    worst = {}
    kmax = 0.0
    for G in GS:
        st = R.steering(R.grid(G), pos).astype(np.complex64)
        d_st = ctx.steering_c64(st)
        for method, loads in (('bartlett', (1e-2,)), ('capon', LOADINGS)):
            for loading in loads:
                ref = R.map_ref(c, st, method, loading)
                kmax = max(kmax, float(ref['kappa'].max()))
                full = None
                for n in sorted(NS, reverse=True):
                    bm, m = sentinel_out(ctx, (n, G), torch.float32, -3.0)
                    ba, a = sentinel_out(ctx, (n,), torch.int32, -9)
                    ctx.range_azimuth(dev[:n], d_st, method, loading=loading, out=dict(map=m, arg=a))
                    torch.cuda.synchronize()
                    assert margins_untouched(bm, n * G, -3.0) and margins_untouched(ba, n, -9)
                    mh, ah = m.cpu().numpy(), a.cpu().numpy()
                    sub = {k: v[:n] for k, v in ref.items()}
                    check_rows((A, array, G, method, loading, n), mh, ah, sub, method, A, worst)
                    if full is None:
                        full = (mh, ah)
                    else:  # a row depends on its own covariance only
                        assert mh.tobytes() == full[0][:n].tobytes() and (ah == full[1][:n]).all()
    print(f'\nspectrum A={A} {array}: largest error Bartlett {worst["bartlett"]:.2f} u t/A (bound {2 * A * A + 8}), '
          f'Capon {worst["capon"]:.3f} u kappa ref (bound {8 * A}); largest kappa {kmax:.3g}')


def test_spectrum_without_arg_and_method_ids(ctx):
    from rsl import _lib
    c = ctx.to_dev(covs(8)[:17])
    st = ctx.steering_c64(R.steering(R.grid(37), R.ula(8)))
    m0, a0 = ctx.range_azimuth(c, st, 'capon', want_arg=True)
    m1, a1 = ctx.range_azimuth(c, st, _lib.RA_CAPON)
    assert a1 is None and ctx.torch.equal(m0, m1) and a0.dtype == ctx.torch.int32
    with pytest.raises(ValueError):
        ctx.range_azimuth(c, st, 'music')
    with pytest.raises(ValueError):
        ctx.range_azimuth(c, ctx.steering_c64(R.steering(R.grid(37), R.ula(7))), 'capon')


# -- 3. resolution ------------------------------------------------------------------------------------------------------
def test_resolution_capon_separates_what_bartlett_merges(ctx):
    """8 antennas, 32 snapshots, 181 grid points, two 20 dB sources 10 degrees apart in every one of 200 range bins:
    on the oracle alone Capon resolves both in every bin and Bartlett in none; the device maps satisfy the same."""
    from rsl import ops
    z, truth, g, st = R.resolution_scene()
    st64 = st.astype(np.complex64)
    cov = R.cov_ref(z[None])[0]
    S = R.RES['S']
    assert R.count_resolved(R.map_ref(cov, st64, 'capon', R.RES['loading'])['map'], g, truth) == S
    assert R.count_resolved(R.map_ref(cov, st64, 'bartlett')['map'], g, truth) == 0
    cap = ops.range_azimuth_map(st, rds=z, method='capon', loading=R.RES['loading'], want_arg=True, ctx=ctx)
    bar = ops.range_azimuth_map(st, rds=z, method='bartlett', ctx=ctx)
    assert cap['map'].shape == (S, R.RES['G']) and cap['cov'].shape == (S, 8, 8) and cap['arg'].shape == (S,)
    nc, nb = R.count_resolved(cap['map'], g, truth), R.count_resolved(bar['map'], g, truth)
    print(f'\nresolved on the device: Capon {nc} of {S}, Bartlett {nb} of {S}')
    assert nc == S and nb == 0
    assert (np.abs(g[cap['arg']]) <= R.RES['sep'] / 2 + R.RES['tol']).all()


# -- 4. the per-call layer and the drop-in --------------------------------------------------------------------------------
def test_ops_layers(ctx):
    from rsl import ops
    from src.angle_estimation.angle_estimation import AngleEstimator
    z, _ = R.cov_input(2, 8, 6, 32, 3)
    cov = ops.range_covariance(z, ctx=ctx)
    assert cov.shape == (2, 6, 8, 8) and cov.dtype == np.complex128
    one = ops.range_covariance(z[0], doppler=(3, 20), ctx=ctx)
    assert one.shape == (6, 8, 8)
    ref = R.cov_ref(z[:1], 3, 20)[0]
    assert (np.abs(one - ref) <= R.cov_bound(ref, 17)).all()
    kept = ops.range_covariance(z, ctx=ctx, keep_on_device=True)
    assert kept.is_cuda and (kept.cpu().numpy() == cov.astype(np.complex64)).all()
    est = AngleEstimator(num_antennas=8)
    out = est.range_azimuth_map(z[0], method='bartlett', doppler=(3, 20))
    assert set(out) == {'map', 'angles_deg', 'arg'} and out['map'].shape == (6, len(est.azimuth_grid))
    want = ops.range_azimuth_map(est._steer, cov=one.astype(np.complex64), method='bartlett', want_arg=True, ctx=ctx)
    assert np.array_equal(out['map'], want['map']) and np.array_equal(out['arg'], want['arg'])
    assert 'cov' not in want and out['arg'].dtype == np.int64
    single = ops.range_azimuth_map(est._steer, cov=one[1].astype(np.complex64), ctx=ctx)
    assert single['map'].shape == (len(est.azimuth_grid),)
    assert np.array_equal(single['map'], ops.range_azimuth_map(est._steer, cov=one.astype(np.complex64),
                                                               ctx=ctx)['map'][1])


# -- 5. the chain -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def chains(ctx):
    """The two-frame batch of tests/test_gpu_chain.py's first shape through the default chain, the Capon chain and a
    guarded Bartlett chain with a Doppler window."""
    import radar_oracle as O
    import rsl
    A, C, Tc = 8, 16, 3.2e-6
    frames = []
    for f in range(2):
        np.random.seed(1000 + f)
        frames.append(O.synthesize_frame(O.TEST_SCENE, chirp_duration=Tc, num_chirps=C, num_antennas=A))
    cube = ctx.to_dev(np.stack(frames).astype(np.complex64))
    out = {}
    for name, kw in (('plain', {}), ('capon', dict(ra_map='capon')),
                     ('bartlett', dict(ra_map='bartlett', ra_doppler=(3, 12)))):
        ch = rsl.RadarChain(rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=Tc, **kw), 2, ctx,
                            guard=(name == 'bartlett'))
        ch.run(cube)
        out[name] = (ch, ch.results())
    return out


@pytest.mark.parametrize('name', ['capon', 'bartlett'])
def test_chain_map_equals_the_per_call_map(ctx, chains, name):
    from rsl import ops, tables
    ch, res = chains[name]
    cfg = ch.cfg
    steer = tables.steering_matrix(ch.grid, np.arange(ch.A) * (cfg.lambda_c / 2), cfg.lambda_c)
    want = ops.range_azimuth_map(steer, rds=ch.rds, method=name, doppler=cfg.ra_doppler, loading=cfg.ra_loading,
                                 want_arg=True, ctx=ctx)
    assert res['ra_map'].shape == (2, ch.S, len(ch.grid)) and res['ra_map'].dtype == np.float32
    assert res['ra_map'].astype(np.float64).tobytes() == want['map'].tobytes()
    assert np.array_equal(res['ra_arg'], want['arg']) and res['ra_arg'].shape == (2, ch.S)
    assert res['ra_map'].max() > 0
    assert ch.guard_violations() == []


@pytest.mark.parametrize('name', ['capon', 'bartlett'])
def test_chain_other_results_unchanged(chains, name):
    plain_ch, plain = chains['plain']
    assert plain_ch.ra is None and 'ra_map' not in plain and 'ra_arg' not in plain
    _, res = chains[name]
    assert set(res) == set(plain) | {'ra_map', 'ra_arg'}
    for k, v in plain.items():
        assert np.asarray(res[k]).tobytes() == np.asarray(v).tobytes(), k


# -- 6. arguments -------------------------------------------------------------------------------------------------------
def test_empty_batches_launch_nothing_and_timing_id(ctx):
    torch = ctx.torch
    st = ctx.steering_c64(R.steering(R.grid(37), R.ula(8)))
    ctx.timing(True)
    try:
        ctx.timing_reset()
        cov = ctx.range_cov(torch.zeros((0, 8, 4, 16), dtype=torch.complex64, device=ctx.device))
        assert tuple(cov.shape) == (0, 4, 8, 8)
        m, a = ctx.range_azimuth(cov, st, 'capon', want_arg=True)
        assert tuple(m.shape) == (0, 4, 37) and tuple(a.shape) == (0, 4)
        assert ctx.timing_read()['doa_scan'][1] == 0
        cov = ctx.range_cov(torch.zeros((1, 8, 4, 16), dtype=torch.complex64, device=ctx.device))
        m, a = ctx.range_azimuth(cov, st, 'capon', want_arg=True)
        assert ctx.timing_read()['doa_scan'][1] == 2  # both timed under RSL_K_DOA_SCAN
        assert not m.any() and not a.any()  # t = 0: all 0, arg 0
    finally:
        ctx.timing_reset()
        ctx.timing(False)


def test_invalid_arguments_return_the_code_and_write_nothing(ctx):
    torch = ctx.torch
    lib = ctx.lib
    ctx._bind()
    F, A, S, C, G = 1, 8, 4, 16, 37
    rds = torch.ones((F, A, S, C), dtype=torch.complex64, device=ctx.device)
    cov = torch.full((F, S, A, A), complex(5.0, 5.0), dtype=torch.complex64, device=ctx.device)
    bad_cov = [dict(A=1), dict(A=17), dict(c0=-1), dict(c0=5, c1=5), dict(c0=6, c1=5), dict(c1=C + 1), dict(rds=None),
               dict(cov=None)]
    for kw in bad_cov:
        a = dict(rds=rds.data_ptr(), F=F, A=A, S=S, C=C, c0=0, c1=C, cov=cov.data_ptr())
        a.update(kw)
        rc = lib.rsl_range_cov(ctx.h, a['rds'], a['F'], a['A'], a['S'], a['C'], a['c0'], a['c1'], a['cov'])
        assert rc == 1, kw
        assert lib.rsl_last_error(ctx.h).startswith(b'rsl_range_cov'), kw
    torch.cuda.synchronize()
    assert (cov == complex(5.0, 5.0)).all()
    # bad antenna counts and windows are errors for an empty batch too; null pointers are not
    assert lib.rsl_range_cov(ctx.h, None, 0, 1, S, C, 0, C, None) == 1
    assert lib.rsl_range_cov(ctx.h, None, 0, A, S, C, 0, C, None) == 0
    st = ctx.steering_c64(R.steering(R.grid(G), R.ula(A)))
    good = ctx.to_dev(R.psd_covs(A, 4, 1))
    m = torch.full((4, G), -2.0, dtype=torch.float32, device=ctx.device)
    arg = torch.full((4,), -5, dtype=torch.int32, device=ctx.device)
    bad_map = [dict(method=2), dict(method=-1), dict(A=1), dict(A=17), dict(G=0), dict(loading=9e-5),
               dict(loading=1.0001), dict(loading=float('nan')), dict(loading=-1.0), dict(cov=None), dict(steer=None),
               dict(map=None), dict(n=-1)]
    for kw in bad_map:
        a = dict(cov=good.data_ptr(), n=4, A=A, steer=st.data_ptr(), G=G, method=1, loading=1e-2, map=m.data_ptr())
        a.update(kw)
        rc = lib.rsl_range_azimuth(ctx.h, a['cov'], a['n'], a['A'], a['steer'], a['G'], a['method'],
                                   ctypes.c_double(a['loading']), a['map'], arg.data_ptr())
        assert rc == 1, kw
        assert lib.rsl_last_error(ctx.h).startswith(b'rsl_range_azimuth'), kw
    torch.cuda.synchronize()
    assert (m == -2.0).all() and (arg == -5).all()
    assert lib.rsl_range_azimuth(ctx.h, None, 0, A, None, G, 0, ctypes.c_double(1e-2), None, None) == 0
    assert lib.rsl_range_azimuth(ctx.h, None, 0, A, None, G, 7, ctypes.c_double(1e-2), None, None) == 1
    # the boundary values are valid, Bartlett checks the loading's range too
    for method, loading in ((1, 1e-4), (1, 1.0), (0, 1e-4)):
        assert lib.rsl_range_azimuth(ctx.h, good.data_ptr(), 4, A, st.data_ptr(), G, method, ctypes.c_double(loading),
                                     m.data_ptr(), None) == 0
    assert lib.rsl_range_azimuth(ctx.h, good.data_ptr(), 4, A, st.data_ptr(), G, 0, ctypes.c_double(2.0),
                                 m.data_ptr(), None) == 1
    torch.cuda.synchronize()
