"""GPU tests of the spatially smoothed MUSIC (rsl_doa_smoothed / k_doa_smoothed) against the fp64 numpy oracle in
tests/ssmusic_ref.py, which runs on the very c64 signatures and steering values the kernel reads.

Eigenvectors are not unique, so parity is on the invariants (model order, eigenvalues, the null spectrum, the picks).
Every parity test first asserts, on the reference alone, that the cells whose outcome the definition leaves to
rounding (ssmusic_ref.near_cells) number at most ssmusic_ref.near_cap(cells), then holds every other cell to the
tolerances stated in ssmusic_ref's docstring.
"""
from ctypes import c_void_p

import numpy as np
import pytest

import ssmusic_ref as R

pytestmark = pytest.mark.gpu

LAM = 3e8 / 77e9
REL = 0.05


def grid_for(G):
    return np.linspace(-90.0, 90.0, G)


def steer_for(G, M):
    from rsl import tables
    return tables.steering_matrix(grid_for(G), np.arange(M) * LAM / 2, LAM)


def run_op(ctx, st, sigs, L, k, nmax, rel=REL):
    from rsl import ops
    r = ops.doa_smoothed(st, sigs=sigs, sub_len=L, num_sources=k, rel=rel, nmax=nmax, want_eig=True, want_spec=True,
                         ctx=ctx)
    return dict(nsrc=r['nsrc'], idx=r['gidx'], den=r['den'], eig=r['eig'], spec=r['spec'], deg=r['deg'])


def head(ref, n):
    return {k: v[:n] for k, v in ref.items()}


def check(tag, out, ref, L, rel, estimate):
    """The cap on the reference alone, then every figure of ssmusic_ref.compare; each is printed before it is asserted."""
    c = R.compare(out, ref, L, rel, estimate, R.DEN_TOL)
    print(f'{tag}: cells {c["cells"]}, near {c["near"]}, nsrc_bad {c["nsrc_bad"]}, eig_err {c["eig_err"]:.2e}, '
          f'den_scaled {c["den_scaled"]:.2e} (DEN_TOL {R.DEN_TOL:.2e}), den_bad {c["den_bad"]}, '
          f'pick_shift {c["pick_shift"]}, pick_bad {c["pick_bad"]}')
    cap = R.near_cap(c['cells'])
    assert c['near'] <= cap, (tag, c)
    assert c['nsrc_bad'] == 0, (tag, c)
    assert c['eig_err'] <= R.EIG_TOL, (tag, c)
    assert c['den_bad'] == 0, (tag, c)
    assert c['empty_bad'] == 0, (tag, c)
    assert c['pick_bad'] == 0, (tag, c)
    assert c['pick_shift'] <= cap, (tag, c)
    assert c['pick_den_bad'] == 0, (tag, c)
    return c


# -- 1. signature parity -------------------------------------------------------------------------------------------
# inputs chosen so that the reference alone leaves at most near_cap cells to rounding on all three grids (two sources
# at least two steps of the coarsest grid apart; L = M has a single sub-array, whose forward-backward covariance of two
# coherent sources is close to rank 1 for many relative phases, so that case takes Gaussian-noise signatures)
SHAPES = [(8, 6, ('two', 12, 7)), (8, 5, ('two', 12, 7)), (4, 3, ('two', 25, 7)), (16, 8, ('two', 12, 7)),
          (8, 8, ('noise', 4)), (3, 2, ('two', 30, 7))]
NCELL = 1003


def make_sigs(M, gen, n=NCELL):
    if gen[0] == 'two':
        return R.two_sources(n, M, gen[1], 30, gen[2])[0]
    return R.noise_sigs(n, M, gen[1])


@pytest.mark.parametrize('estimate', [False, True], ids=['fixed', 'estimate'])
@pytest.mark.parametrize('M,L,gen', SHAPES, ids=[f'M{m}L{l}' for m, l, _ in SHAPES])
def test_signature_parity(ctx, M, L, gen, estimate):
    sigs = make_sigs(M, gen)
    nmax = min(3, L - 1)
    k = 0 if estimate else min(2, L - 1)  # two sources; one where a sub-array of 2 resolves no more
    print()
    for G in (361, 91, 37):
        st = steer_for(G, M)
        from rsl import tables
        ref = R.reference(sigs, tables.subarray_steering(st, L), L, nmax, k, REL)
        for n in (1, 15, 17, NCELL):  # one group, a partial wave, one cell into the fifth group, many workgroups
            out = run_op(ctx, st, sigs[:n], L, k, nmax)
            assert out['idx'].shape == (n, nmax) and out['spec'].shape == (n, G) and out['eig'].shape == (n, L)
            check(f'M={M} L={L} G={G} n={n} k={k}', out, head(ref, n), L, REL, estimate)


#    the inputs DEN_TOL was measured on (ssmusic_ref's docstring); den_scaled is printed for each
NAMED = [(8, 6, ('two', 8, 1)), (8, 6, ('two', 12, 1)), (8, 6, ('two', 20, 1)), (8, 5, ('two', 10, 1)),
         (16, 8, ('two', 5, 1)), (4, 3, ('two', 25, 1)), (8, 6, ('noise', 5))]


@pytest.mark.parametrize('M,L,gen', NAMED, ids=[f'M{m}L{l}{g[0]}{g[1]}' for m, l, g in NAMED])
def test_named_inputs_parity(ctx, M, L, gen):
    from rsl import tables
    two = gen[0] == 'two'
    sigs = make_sigs(M, gen, 1536 if two else 1024)
    nmax = min(3, L - 1)
    st = steer_for(361, M)
    sub = tables.subarray_steering(st, L)
    print()
    for k, rel in ((2 if two else 3, 0.05), (0, 0.05), (0, 0.01)):
        ref = R.reference(sigs, sub, L, nmax, k, rel)
        out = run_op(ctx, st, sigs, L, k, nmax, rel)
        check(f'M={M} L={L} {gen} k={k} rel={rel}', out, ref, L, rel, k == 0)


# -- 2. the RDS path, lists shorter than their capacity ---------------------------------------------------------
def test_rds_path_and_untouched_slots(ctx):
    torch = ctx.torch
    rng = np.random.default_rng(21)
    F, A, S, C, L, nmax, G = 2, 8, 16, 8, 6, 3, 361
    rds = (rng.standard_normal((F, A, S, C)) + 1j * rng.standard_normal((F, A, S, C))).astype(np.complex64)
    rds[1, :, 3, 2] = 0  # an empty cell in the list
    cap, n = 40, 29
    fr = rng.integers(0, F, cap).astype(np.int32)
    rc = rng.integers(0, S * C, cap).astype(np.int32)
    fr[5], rc[5] = 1, 3 * C + 2
    st = steer_for(G, A)
    sub = ctx.steering_sub(st, L)
    d = ctx.to_dev(rds)
    sigs = rds[fr, :, rc // C, rc % C]

    def prefilled(rows):
        full = lambda shape, v, dt: torch.full(shape, v, dtype=dt, device=ctx.device)
        return dict(nsrc=full((rows,), -7, torch.int32), idx=full((rows, nmax), -7, torch.int32),
                    den=full((rows, nmax), float('nan'), torch.float32),
                    eig=full((rows, L), float('nan'), torch.float32),
                    spec=full((rows, G), float('nan'), torch.float32))
    from rsl import tables
    ref = R.reference(sigs, tables.subarray_steering(st, L), L, nmax, 2, REL)
    for n_dev, rows in ((n, n), (1000, cap)):  # a count below the capacity; an overflowed count clamps to it
        o = prefilled(cap + 8)
        ctx.doa_smoothed(d, ctx.to_dev(fr), ctx.to_dev(rc), sub, n=cap,
                         n_dev=ctx.to_dev(np.array([n_dev], np.int64)), nmax=nmax, num_sources=2, out=o)
        h = {k: v.cpu().numpy() for k, v in o.items()}
        assert (h['nsrc'][rows:] == -7).all() and (h['idx'][rows:] == -7).all()
        assert np.isnan(h['den'][rows:]).all() and np.isnan(h['eig'][rows:]).all() and np.isnan(h['spec'][rows:]).all()
        out = {k: v[:rows] for k, v in h.items()}
        print()
        check(f'rds path n_dev={n_dev}', out, head(ref, rows), L, REL, False)
        assert out['nsrc'][5] == 0 and (out['idx'][5] == -1).all() and np.isnan(out['den'][5]).all()
    # the op's RDS form (frame 0) equals its signature form
    from rsl import ops
    rb, db = rc[fr == 0] // C, rc[fr == 0] % C
    a = ops.doa_smoothed(st, rds=rds[0], rbins=rb, dbins=db, sub_len=L, num_sources=2, ctx=ctx)
    b = ops.doa_smoothed(st, sigs=sigs[fr == 0], sub_len=L, num_sources=2, ctx=ctx)
    for k in ('nsrc', 'gidx', 'den', 'deg'):
        assert a[k].tobytes() == b[k].tobytes(), k


# -- 3. resolution on the device ----------------------------------------------------------------------------------
@pytest.mark.parametrize('L', [5, 6])
def test_resolution_on_device(ctx, L):
    sigs, theta = R.two_sources(2000, 8, 10, 30, 11)
    out = run_op(ctx, steer_for(361, 8), sigs, L, 2, 3)
    rate = R.resolved(out['deg'], theta)
    print(f'\nL={L}: both sources within 2 degrees in {rate:.3f} of the cells')
    assert rate >= 0.95
    assert (out['nsrc'] == 2).all()


# -- 4. degenerate cells ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('M,L', [(8, 6), (16, 8), (4, 3)])
def test_degenerate_cells(ctx, M, L):
    G = 361
    st = steer_for(G, M)
    on_grid = [40, 180, 251]
    sigs = np.zeros((5, M), np.complex64)
    for row, g in zip((1, 2, 4), on_grid):
        sigs[row] = (st[g] * (0.3 + 0.4j)).astype(np.complex64)
    for nmax in (1, L - 1):
        out = run_op(ctx, st, sigs, L, 0, nmax)
        assert out['idx'].shape == (5, nmax)
        for row in (0, 3):  # zero signature: empty cell
            assert out['nsrc'][row] == 0 and (out['idx'][row] == -1).all() and np.isnan(out['den'][row]).all()
            assert np.isnan(out['eig'][row]).all() and np.isnan(out['spec'][row]).all()
        for row, g in zip((1, 2, 4), on_grid):  # one noise-free source on the grid: rank 1, gap 1
            assert out['nsrc'][row] == 1
            assert out['idx'][row, 0] == g and (out['idx'][row, 1:] == -1).all()
            print(f'M={M} L={L} nmax={nmax} g={g}: den at the pick {out["den"][row, 0]:.2e}')
            assert 0 <= out['den'][row, 0] <= R.DEN_TOL * L
            assert np.isnan(out['den'][row, 1:]).all()
            assert abs(out['eig'][row, 0] - out['eig'][row].sum()) <= R.EIG_TOL * out['eig'][row, 0]


# -- 5. bad arguments ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bad', [dict(M=2), dict(M=17), dict(L=1), dict(L=9), dict(M=4, L=5), dict(nmax=0), dict(nmax=6),
                                 dict(k=-1), dict(k=4), dict(rel=0.0), dict(rel=1.0), dict(rel=float('nan')),
                                 dict(G=2)], ids=lambda b: '-'.join(f'{k}={v}' for k, v in b.items()))
def test_bad_arguments(ctx, bad):
    """The library's own checks (Context.doa_smoothed passes everything through)."""
    torch = ctx.torch
    a = {**dict(M=8, L=6, nmax=3, k=0, rel=0.05, G=361), **bad}
    rds = torch.zeros((4, a['M'], 1, 1), dtype=torch.complex64, device=ctx.device)
    fr = ctx.to_dev(np.arange(4, dtype=np.int32))
    rc = ctx.to_dev(np.zeros(4, np.int32))
    sub = torch.ones((a['G'], a['L']), dtype=torch.complex64, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.doa_smoothed(rds, fr, rc, sub, n=4, nmax=a['nmax'], num_sources=a['k'], rel=a['rel'])


def test_bad_pointers_and_op_arguments(ctx):
    from rsl import ops
    torch = ctx.torch
    rds = torch.zeros((4, 8, 1, 1), dtype=torch.complex64, device=ctx.device)
    fr = ctx.to_dev(np.arange(4, dtype=np.int32))
    rc = ctx.to_dev(np.zeros(4, np.int32))
    sub = torch.ones((361, 6), dtype=torch.complex64, device=ctx.device)
    nsrc = torch.zeros((4,), dtype=torch.int32, device=ctx.device)
    idx = torch.zeros((4, 3), dtype=torch.int32, device=ctx.device)
    p = lambda t: c_void_p(t.data_ptr())
    base = dict(rds=p(rds), fr=p(fr), rc=p(rc), sub=p(sub), nsrc=p(nsrc), idx=p(idx))
    for null in base:
        a = {**base, null: None}
        rcode = ctx.lib.rsl_doa_smoothed(ctx.h, a['rds'], 8, 1, 1, a['fr'], a['rc'], None, 4, a['sub'], 361, 6, 3, 0,
                                         0.05, a['nsrc'], a['idx'], None, None, None)
        assert rcode == 1, (null, rcode)  # RSL_ERR_INVALID
        with pytest.raises(ValueError):
            ctx.check(rcode, 'rsl_doa_smoothed')
    st = steer_for(91, 8)
    sigs = R.noise_sigs(3, 8, 1)
    for kw in (dict(sub_len=1), dict(sub_len=9), dict(nmax=0), dict(num_sources=4), dict(num_sources=-1),
               dict(rel=0.0), dict(rel=1.5)):
        with pytest.raises(ValueError):
            ops.doa_smoothed(st, sigs=sigs, ctx=ctx, **kw)
    with pytest.raises(ValueError):  # signatures of another antenna count
        ops.doa_smoothed(st, sigs=R.noise_sigs(3, 6, 1), ctx=ctx)
    pos = np.arange(8) * LAM / 2
    pos[2] += 0.2 * LAM
    from rsl import tables
    with pytest.raises(ValueError):  # not a uniform array
        ops.doa_smoothed(tables.steering_matrix(grid_for(91), pos, LAM), sigs=sigs, ctx=ctx)


# -- 6. empty batch, timing id ---------------------------------------------------------------------------------------
def test_empty_batch_launches_nothing(ctx):
    torch = ctx.torch
    st = steer_for(91, 8)
    sub = ctx.steering_sub(st, 6)
    sigs = R.noise_sigs(9, 8, 3)
    rds = ctx.to_dev(sigs.reshape(9, 8, 1, 1))
    fr = ctx.to_dev(np.arange(9, dtype=np.int32))
    rc = ctx.to_dev(np.zeros(9, np.int32))
    ctx.timing(True)
    try:
        ctx.timing_reset()
        ctx.doa_smoothed(rds, fr, rc, sub, n=0)
        assert ctx.timing_read()['doa_scan'][1] == 0
        nsrc, idx, den, _, _ = ctx.doa_smoothed(rds, fr, rc, sub, n=9)
        assert ctx.timing_read()['doa_scan'][1] == 1  # timed under RSL_K_DOA_SCAN
        assert (nsrc.cpu().numpy() >= 1).all()
    finally:
        ctx.timing_reset()
        ctx.timing(False)
    # a device count of 0: nothing is written
    o = dict(nsrc=torch.full((9,), -7, dtype=torch.int32, device=ctx.device),
             idx=torch.full((9, 3), -7, dtype=torch.int32, device=ctx.device))
    ctx.doa_smoothed(rds, fr, rc, sub, n=9, n_dev=ctx.to_dev(np.zeros(1, np.int64)), out=o, want_den=False)
    assert (o['nsrc'].cpu().numpy() == -7).all() and (o['idx'].cpu().numpy() == -7).all()
    from rsl import ops
    e = ops.doa_smoothed(st, sigs=np.zeros((0, 8), np.complex64), want_eig=True, want_spec=True, ctx=ctx)
    assert e['gidx'].shape == (0, 3) and e['spec'].shape == (0, 91) and e['eig'].shape == (0, 6)


# -- 7. chain ----------------------------------------------------------------------------------------------------------
CH = dict(num_antennas=8, num_chirps=64, chirp_duration=25.6e-6)


@pytest.fixture(scope='module')
def chains(ctx):
    import radar_oracle as O
    import rsl
    frames = []
    for s in (1000, 1001):
        np.random.seed(s)
        frames.append(O.synthesize_frame(O.TEST_SCENE, chirp_duration=25.6e-6, num_chirps=64, num_antennas=8))
    cube = ctx.to_dev(np.stack(frames).astype(np.complex64))
    out = {}
    for name, kw in (('plain', {}), ('multi', dict(multi_source=True)),
                     ('multi2', dict(multi_source=True, ss_len=5, ss_sources=2, ss_max=2))):
        ch = rsl.RadarChain(rsl.ChainConfig(**CH, **kw), 2, ctx)
        ch.run(cube)
        res = ch.results()
        res['chain'] = ch
        out[name] = res
    return out


@pytest.mark.parametrize('name', ['multi', 'multi2'])
def test_chain_multi_source(ctx, chains, name):
    from rsl import ops
    a, b = chains['plain'], chains[name]
    assert a['chain'].S == 256 and a['chain'].ss is None and not any(k.startswith('ss_') for k in a)
    for k in a:  # every existing result is byte-identical
        if k == 'chain':
            continue
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    ch = b['chain']
    cfg = ch.cfg
    nc = int(b['cell_base'][-1])
    assert nc >= 6
    C = ch.C
    rds = ch.rds.cpu().numpy()
    sigs = rds[b['c_frame'], :, b['c_rc'] // C, b['c_rc'] % C]
    lam = cfg.lambda_c
    from rsl import tables
    st = tables.steering_matrix(ch.grid, np.arange(8) * lam / 2, lam)
    r = ops.doa_smoothed(st, sigs=sigs, sub_len=cfg.ss_len, num_sources=cfg.ss_sources, rel=cfg.ss_rel,
                         nmax=cfg.ss_max, ctx=ctx)
    assert b['ss_gidx'].shape == (nc, ch.ss.nmax)
    for k, kk in (('ss_nsrc', 'nsrc'), ('ss_gidx', 'gidx'), ('ss_den', 'den')):
        x, y = np.ascontiguousarray(b[k]), np.ascontiguousarray(r[kk])
        assert x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes(), k
    assert (b['ss_nsrc'] >= 1).all() and (b['ss_gidx'][:, 0] >= 0).all()


# -- 8. drop-in ------------------------------------------------------------------------------------------------------
def test_process_targets_smoothed(ctx):
    from rsl import ops
    from src.angle_estimation.angle_estimation import AngleEstimator
    rng = np.random.default_rng(5)
    A, S, C = 8, 16, 8
    rds = (0.01 * (rng.standard_normal((A, S, C)) + 1j * rng.standard_normal((A, S, C)))).astype(np.complex64)
    sigs, theta = R.two_sources(3, A, 14, 30, 9)
    cells = [(2, 1), (7, 5), (15, 7)]
    for (r, d), s in zip(cells, sigs):
        rds[:, r, d] = 5.0 * s
    peaks = [{'antenna': 0, 'range_bin': r, 'doppler_bin': d, 'range_m': 1.5 * r, 'doppler_hz': 10.0 * d,
              'power_db': 3.0} for r, d in cells]
    est = AngleEstimator(fc=77e9, num_antennas=A)
    plain = est.process_targets(rds, {'peaks': peaks}, 'music')
    tg = est.process_targets_smoothed(rds, {'peaks': peaks}, num_sources=2)
    assert len(tg) == 3
    assert set(tg[0]) == set(plain[0]) | {'angles_deg', 'num_sources', 'eigenvalues'}
    ref = ops.doa_smoothed(est._steer, rds=rds, rbins=[c[0] for c in cells], dbins=[c[1] for c in cells],
                           num_sources=2, want_eig=True, want_spec=True, grid_deg=est.azimuth_grid, ctx=ctx)
    for n, t in enumerate(tg):
        assert t['num_sources'] == 2 == ref['nsrc'][n]
        assert t['angles_deg'] == [a for a in ref['deg'][n] if not np.isnan(a)] and len(t['angles_deg']) == 2
        assert t['azimuth_deg'] == t['angles_deg'][0]
        assert np.array_equal(t['eigenvalues'], ref['eig'][n]) and t['eigenvalues'].shape == (6,)
        assert np.array_equal(t['spectrum'] > 0, ref['spec'][n] > 1e-12)
        assert np.allclose(t['spectrum'][ref['spec'][n] > 1e-12], 1.0 / ref['spec'][n][ref['spec'][n] > 1e-12])
        assert np.abs(np.sort(t['angles_deg']) - theta[n]).max() <= 2.0
        assert np.array_equal(t['spatial_signature'], plain[n]['spatial_signature'])
        for k in ('range_m', 'doppler_hz', 'power_db', 'antenna', 'range_bin', 'doppler_bin'):
            assert t[k] == plain[n][k]
    # estimate mode with a cap of one source, and another sub-array length
    t1 = est.process_targets_smoothed(rds, {'peaks': peaks}, sub_len=5, max_sources=1)
    assert all(t['num_sources'] == 1 and len(t['angles_deg']) == 1 and t['eigenvalues'].shape == (5,) for t in t1)
