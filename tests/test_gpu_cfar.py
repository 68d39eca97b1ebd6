"""GPU tests of the CA-CFAR detector (rsl_detect_cfar / k_detect_cfar) against the fp64 numpy oracle in
tests/cfar_ref.py, which runs on the very complex64 RDS the kernel read, so only the detector is under test.

Every parity test first asserts, on the reference alone, that the tolerance bands (cfar_ref.CFAR_RTOL on the level,
parity.PEAK_RTOL on the 3x3 test) hold at most cfar_ref.near_cap(cells) cells, then asserts zero unexplained
differences.
"""
import math

import numpy as np
import pytest

import cfar_ref as R
import parity as P
import radar_oracle as O

pytestmark = pytest.mark.gpu

WINDOWS = [(1, 1, 4, 4), (2, 2, 8, 8), (0, 1, 0, 6), (1, 0, 5, 0)]  # (gr, gd, tr, td); Doppler-only, range-only
NO_GATE = (0, 1 << 30)


def alpha_for(window, pfa):
    from rsl import tables
    return tables.cfar_alpha(pfa, tables.cfar_training_cells(window[:2], window[2:]))


def make_frames(A, C, Tc, seeds):
    frames = []
    for s in seeds:
        np.random.seed(s)
        frames.append(O.synthesize_frame(O.TEST_SCENE, chirp_duration=Tc, num_chirps=C, num_antennas=A))
    return np.stack(frames)


def run_cfar(ctx, rds_dev, window, alpha, thr_power=-1.0, gate=NO_GATE, want_db=False):
    torch = ctx.torch
    pk = torch.full(tuple(rds_dev.shape), float('nan'), dtype=torch.float32, device=rds_dev.device)
    mask, rc, db = ctx.detect_cfar(rds_dev, window[:2], window[2:], alpha, thr_power, gate[0], gate[1],
                                   want_db=want_db, out=dict(peak_pow=pk))
    torch.cuda.synchronize()
    return dict(mask=mask.cpu().numpy(), row_count=rc.cpu().numpy(), peak_pow=pk.cpu().numpy(),
                db=db.cpu().numpy() if db is not None else None)


def check_against_oracle(tag, rds_np, window, alpha, got, thr_power=-1.0, gate=NO_GATE):
    """Cap on the reference alone, then mask / row_count / peak_pow (/ db_map) against it.  Returns the GPU mask."""
    C = rds_np.shape[-1]
    ref = R.cfar_reference(rds_np, window, alpha, thr_power=thr_power, gate=gate)
    cells = ref['mask'].size
    n_near = int(ref['near'].sum())
    print(f'\n{tag}: reference peaks {int(ref["mask"].sum())} of {cells} cells, near-threshold {n_near}')
    assert n_near <= R.near_cap(cells), (tag, n_near, cells)
    gm = R.mask_bool(got['mask'], C)
    ng, nr, nd, nu = R.cfar_diff(gm, ref)
    print(f'{tag}: gpu peaks {ng}, differing {nd}, unexplained {nu}')
    assert nu == 0, (tag, ng, nr, nd, nu)
    cnt = gm.sum(-1)
    assert (got['row_count'] == cnt).all(), tag
    # row-compact peak powers: slot k of a row = the power of its k-th peak in Doppler order; the rest untouched
    rows = gm.reshape(-1, C)
    pkf = got['peak_pow'].reshape(-1, C)
    rank = np.cumsum(rows, axis=1) - 1
    ri = np.nonzero(rows)[0]
    want = ref['p'].reshape(-1, C)[rows]
    have = pkf[ri, rank[rows]].astype(np.float64)
    assert np.allclose(have, want, rtol=1e-6, atol=0), tag
    assert (np.isnan(pkf) == (np.arange(C)[None, :] >= cnt.reshape(-1, 1))).all(), tag
    if got['db'] is not None:  # 10 log10f(p + 1e-12) evaluated in fp32 on the fp32 power
        p32 = ref['p'].astype(np.float32)
        want_db = np.float32(10.0) * np.log10(p32 + np.float32(1e-12))
        err = float(np.abs(got['db'].astype(np.float64) - want_db.astype(np.float64)).max())
        print(f'{tag}: db_map max error {err:.3e} dB')
        assert err <= 1e-5, (tag, err)
    return gm


# -- 1. oracle parity ----------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_rds(ctx):
    from rsl import ops, tables
    frames = make_frames(4, 32, 6.4e-6, (7, 8))  # S = 64
    table = tables.chirp_table(77e9, 1e9, 6.4e-6, 10e6, 'hann', 64)
    dev = ops.range_doppler(frames, table, ctx=ctx, keep_on_device=True).contiguous()
    assert tuple(dev.shape) == (2, 4, 64, 32)
    return dev, dev.cpu().numpy()


@pytest.mark.parametrize('pfa', [1e-2, 1e-4])
@pytest.mark.parametrize('window', WINDOWS)
def test_oracle_parity(ctx, small_rds, window, pfa):
    dev, host = small_rds
    alpha = alpha_for(window, pfa)
    got = run_cfar(ctx, dev, window, alpha, want_db=True)
    gm = check_against_oracle(f'parity {window} pfa {pfa}', host, window, alpha, got)
    if pfa == 1e-2:
        assert gm.any()  # the scene's targets stand above any of these levels


# -- 2. strong cells: the add-only training sum -----------------------------------------------------------
def spiked_maps():
    rng = np.random.default_rng(5)

    def noise():
        return ((rng.standard_normal((64, 32)) + 1j * rng.standard_normal((64, 32))) / math.sqrt(2)).astype(
            np.complex64)
    z = noise()
    z[0, 0] = 3e4
    z[31, 16] = 1e5
    z[63, 31] = 3e4
    z[20, 5] = z[20, 7] = 40
    a, b = noise(), noise()
    # [F = 2, A = 2]: the spiked map at (0, 1) and (1, 0), so that its range row 0 and row S-1 both border a quiet map
    return np.stack([np.stack([a, z]), np.stack([z, b])])


@pytest.mark.parametrize('window', WINDOWS)
def test_strong_cells(ctx, window):
    host = spiked_maps()
    dev = ctx.to_dev(host)
    alpha = alpha_for(window, 1e-2)
    got = run_cfar(ctx, dev, window, alpha)
    gm = check_against_oracle(f'strong {window}', host, window, alpha, got)
    for f, a in ((0, 1), (1, 0)):
        assert gm[f, a, 0, 0] and gm[f, a, 31, 16] and gm[f, a, 63, 31]


# -- 3. shapes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,C', [(50, 100), (21, 21), (200, 64), (130, 128), (40, 512)])
def test_shapes(ctx, S, C):
    rng = np.random.default_rng(S * 1000 + C)
    host = ((rng.standard_normal((1, 2, S, C)) + 1j * rng.standard_normal((1, 2, S, C))) / math.sqrt(2)).astype(
        np.complex64)
    window = (2, 2, 8, 8)
    alpha = alpha_for(window, 1e-2)
    got = run_cfar(ctx, ctx.to_dev(host), window, alpha, want_db=False)
    check_against_oracle(f'shape S{S} C{C}', host, window, alpha, got)
    # with a range gate and a power floor
    gate, floor = (5, S - 7), 3.0
    got = run_cfar(ctx, ctx.to_dev(host), window, 2.0, thr_power=floor, gate=gate)
    gm = check_against_oracle(f'shape S{S} C{C} gated', host, window, 2.0, got, thr_power=floor, gate=gate)
    assert gm.any() and not gm[:, :, :gate[0]].any() and not gm[:, :, gate[1] + 1:].any()


# -- 4. degenerate maps -----------------------------------------------------------------------------------
def test_degenerate_maps(ctx):
    S, C = 48, 64
    window = (2, 2, 8, 8)
    zero = ctx.to_dev(np.zeros((1, 2, S, C), np.complex64))
    got = run_cfar(ctx, zero, window, 0.5)
    assert not got['mask'].any() and not got['row_count'].any() and np.isnan(got['peak_pow']).all()
    const = ctx.to_dev(np.full((1, 2, S, C), 1.5 + 0.5j, np.complex64))  # p = 2.5, every window sum exact in fp32
    got = run_cfar(ctx, const, window, 2.0)
    assert not got['mask'].any() and not got['row_count'].any()
    got = run_cfar(ctx, const, window, 0.5, gate=(3, 40))
    want_rows = np.zeros(S, np.int32)
    want_rows[3:41] = C
    assert (got['row_count'] == want_rows[None, None, :]).all()
    assert R.mask_bool(got['mask'], C)[:, :, 3:41].all()
    assert (got['peak_pow'][:, :, 3:41] == np.float32(2.5)).all()
    assert np.isnan(got['peak_pow'][:, :, :3]).all() and np.isnan(got['peak_pow'][:, :, 41:]).all()


# -- 5. arguments -----------------------------------------------------------------------------------------
BAD = [  # (S, C), guard, train, alpha
    ((64, 64), (-1, 2), (8, 8), 5.0),
    ((64, 64), (2, -1), (8, 8), 5.0),
    ((64, 64), (2, 2), (-1, 8), 5.0),
    ((64, 64), (2, 2), (8, -1), 5.0),
    ((64, 64), (2, 2), (0, 0), 5.0),      # no training cell
    ((64, 64), (9, 2), (8, 8), 5.0),      # hr = 17
    ((64, 64), (2, 9), (8, 8), 5.0),      # hd = 17
    ((64, 20), (2, 2), (8, 8), 5.0),      # 2 hd + 1 > C
    ((16, 64), (2, 2), (8, 8), 5.0),      # 2 hr + 1 > S
    ((64, 64), (2, 2), (8, 8), 0.0),
    ((64, 64), (2, 2), (8, 8), -3.0),
    ((64, 64), (2, 2), (8, 8), float('inf')),
    ((64, 64), (2, 2), (8, 8), float('nan')),
    ((8200, 64), (2, 2), (8, 8), 5.0),    # S > 8192
    ((64, 576), (2, 2), (8, 8), 5.0),     # C above RSL_CFAR_MAX_C (unsupported)
]


@pytest.mark.parametrize('shape,guard,train,alpha', BAD)
def test_bad_arguments(ctx, shape, guard, train, alpha):
    torch = ctx.torch
    rds = torch.zeros((1, 1) + shape, dtype=torch.complex64, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.detect_cfar(rds, guard, train, alpha, -1.0, 0, shape[0] - 1)


def test_empty_batch_launches_nothing(ctx):
    torch = ctx.torch
    ctx.timing(True)
    try:
        ctx.timing_reset()
        empty = torch.zeros((0, 2, 64, 64), dtype=torch.complex64, device=ctx.device)
        mask, rc, _ = ctx.detect_cfar(empty, (2, 2), (8, 8), 5.0, -1.0, 0, 63)
        assert tuple(mask.shape) == (0, 2, 64, 1) and tuple(rc.shape) == (0, 2, 64)
        assert ctx.timing_read()['detect'][1] == 0
        one = torch.zeros((1, 2, 64, 64), dtype=torch.complex64, device=ctx.device)
        ctx.detect_cfar(one, (2, 2), (8, 8), 5.0, -1.0, 0, 63)
        assert ctx.timing_read()['detect'][1] == 1  # timed under RSL_K_DETECT
    finally:
        ctx.timing_reset()
        ctx.timing(False)


# -- 6. chain ---------------------------------------------------------------------------------------------
CH = dict(num_antennas=8, num_chirps=64, chirp_duration=25.6e-6)


@pytest.fixture(scope='module')
def chains(ctx):
    import rsl
    frames = make_frames(8, 64, 25.6e-6, (1000, 1001))
    cube = ctx.to_dev(frames.astype(np.complex64))
    out = {}
    for name, kw in (('plain', {}), ('threshold', dict(detector='threshold')),
                     ('cfar', dict(detector='cfar', cfar_pfa=1e-2)),
                     ('none', dict(detector='cfar', cfar_alpha=1e9))):
        ch = rsl.RadarChain(rsl.ChainConfig(**CH, **kw), 2, ctx)
        ch.run(cube)
        res = ch.results()
        res['rds'] = ch.rds.cpu().numpy()
        res['mask'] = ch.mask.cpu().numpy()
        res['chain'] = ch
        out[name] = res
    return out


def test_chain_cfar_entries_and_cells(chains):
    from rsl import tables
    r = chains['cfar']
    ch = r['chain']
    C = 64
    window = (2, 2, 8, 8)
    alpha = alpha_for(window, 1e-2)
    assert ch.cfar_alpha == alpha
    thr = tables.power_threshold(-20.0)
    ref = R.cfar_reference(r['rds'], window, alpha, thr_power=thr, gate=(ch.i_lo, ch.i_hi))
    n_near = int(ref['near'].sum())
    print(f'\nchain: reference peaks {int(ref["mask"].sum())}, near-threshold {n_near} of {ref["mask"].size}')
    assert n_near <= R.near_cap(ref['mask'].size)
    gm = R.mask_bool(r['mask'], C)
    ng, nr, nd, nu = R.cfar_diff(gm, ref)
    print(f'chain: gpu peaks {ng}, differing {nd}, unexplained {nu}')
    assert nu == 0 and ng > 0
    eb, cb = r['entry_base'], r['cell_base']
    for f in range(2):
        a, i, j = np.nonzero(gm[f])  # antenna -> range -> doppler
        sl = slice(eb[f], eb[f + 1])
        assert (r['e_ant'][sl] == a).all() and (r['e_rbin'][sl] == i).all() and (r['e_dbin'][sl] == j).all()
        db = 10 * np.log10(ref['p'][f][a, i, j] + 1e-12)
        assert np.abs(r['e_pdb'][sl] - db).max() < 1e-4
        ci, cj = np.nonzero(gm[f].any(0))  # union cells, range-major
        cs = slice(cb[f], cb[f + 1])
        assert (r['c_frame'][cs] == f).all() and (r['c_rc'][cs] == ci * C + cj).all()
        am = sum(gm[f][k, ci, cj].astype(np.int64) << k for k in range(8))
        assert (r['c_amask'][cs].astype(np.int64) & 0xffffffff == am).all()
        assert (r['e_cell'][sl] == cb[f] + np.searchsorted(ci * C + cj, i * C + j)).all()


def test_chain_cfar_cells_match_default_chain(chains):
    """gidx / esprit / phase of every CFAR cell equal, bit for bit, the default detector's values for that cell (with
    the -20 dB floor in force the CFAR cells are a subset of its cells)."""
    r, d = chains['cfar'], chains['plain']
    key = lambda x: x['c_frame'].astype(np.int64) << 32 | x['c_rc'].astype(np.int64)
    kd, kr = key(d), key(r)
    assert (np.diff(kd) > 0).all()
    pos = np.searchsorted(kd, kr)
    assert (pos < len(kd)).all() and (kd[pos] == kr).all()
    assert len(kr) > 0 and len(kr) < len(kd)
    assert (r['gidx'] == d['gidx'][pos]).all()
    for name in ('esprit', 'phase'):
        assert (r[name].view(np.int64) == d[name][pos].view(np.int64)).all(), name


def test_chain_cfar_velocity(chains):
    r = chains['cfar']
    cb, grid = r['cell_base'], r['grid']
    for f in range(2):
        sl = slice(cb[f], cb[f + 1])
        w = np.array([bin(int(m) & 0xffffffff).count('1') for m in r['c_amask'][sl]])
        az = np.repeat(np.radians(grid[r['gidx'][sl]]), w)
        y = np.repeat(r['phase'][sl], w)
        assert len(y) >= 3
        vx, vy, cost = O.velocity_ls(az, y, lambda_c=3e8 / 77e9)
        v = r['velocity'][f]
        assert abs(v[2] - cost) <= P.VEL_COST_RTOL * cost
        assert abs(v[0] - vx) < P.VEL_ATOL and abs(v[1] - vy) < P.VEL_ATOL
        assert int(v[5]) == len(y)


def test_chain_threshold_detector_unchanged(chains):
    a, b = chains['plain'], chains['threshold']
    assert (a['mask'] == b['mask']).all()
    for k in ('entry_base', 'cell_base', 'e_ant', 'e_rbin', 'e_dbin', 'e_cell', 'e_pdb', 'c_frame', 'c_rc', 'c_amask',
              'gidx', 'esprit', 'phase', 'velocity'):
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def test_chain_cfar_no_detection(chains):
    r = chains['none']
    assert r['entry_base'][-1] == 0 and r['cell_base'][-1] == 0
    assert len(r['e_ant']) == 0 and len(r['c_rc']) == 0 and len(r['gidx']) == 0
    assert (r['velocity'][:, 5] == 0).all()
    assert not r['mask'].any()


def test_chain_rejects_unknown_detector():
    import rsl
    with pytest.raises(ValueError):
        rsl.ChainConfig(**CH, detector='os-cfar')


# -- 7. drop-in -------------------------------------------------------------------------------------------
def test_dropin_cfar(ctx):
    from rsl import ops
    from src.radar_signal.dechirp import SignalPreprocessor
    frame = make_frames(4, 32, 6.4e-6, (7,))[0]
    pre = SignalPreprocessor(chirp_duration=6.4e-6)
    rds = pre.generate_range_doppler_spectrum(frame)
    out = pre.extract_range_doppler_peaks_cfar(rds, pfa=1e-2, min_range=0.0, max_range=1e9)
    assert set(out) == {'peaks', 'range_bins_m', 'doppler_bins_hz', 'power_spectrum_db'}
    want = ops.detect_peaks_cfar(rds, pfa=1e-2, ctx=ctx)
    got = [(p['antenna'], int(p['range_bin']), int(p['doppler_bin'])) for p in out['peaks']]
    assert got == list(zip(want['antenna'].tolist(), want['range_bin'].tolist(), want['doppler_bin'].tolist()))
    assert len(got) > 0
    assert set(out['peaks'][0]) == {'antenna', 'range_bin', 'doppler_bin', 'range_m', 'doppler_hz', 'power_db'}
    assert out['power_spectrum_db'].shape == rds.shape
    assert np.allclose([p['power_db'] for p in out['peaks']], want['power_db'])
    # the default range gate (1 m .. 200 m) only removes rows
    gated = pre.extract_range_doppler_peaks_cfar(rds, pfa=1e-2)
    assert set((p['antenna'], int(p['range_bin']), int(p['doppler_bin'])) for p in gated['peaks']) <= set(got)
