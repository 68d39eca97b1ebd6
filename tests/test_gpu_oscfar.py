"""GPU tests of the OS-CFAR detector (rsl_detect_oscfar / k_detect_oscfar) against the fp64 numpy oracle in
tests/oscfar_ref.py, which runs on the very complex64 RDS the kernel read, so only the detector is under test.

The structure is that of test_gpu_cfar.py, whose inputs (make_frames, spiked_maps, WINDOWS, BAD) are reused.  Every
parity test first asserts, on the reference alone, that the tolerance bands (oscfar_ref.OS_RTOL on the level,
parity.PEAK_RTOL on the 3x3 test) hold at most near_cap(cells) cells, then asserts zero unexplained differences.
"""
import math

import numpy as np
import pytest

import cfar_ref as CA
import oscfar_ref as R
from test_gpu_cfar import BAD, CH, NO_GATE, WINDOWS, make_frames, run_cfar, spiked_maps

pytestmark = pytest.mark.gpu

RESULT_KEYS = ('entry_base', 'cell_base', 'e_ant', 'e_rbin', 'e_dbin', 'e_cell', 'e_pdb', 'c_frame', 'c_rc',
               'c_amask', 'gidx', 'esprit', 'phase', 'velocity')


def alpha_for(window, pfa, rank):
    from rsl import tables
    n = tables.cfar_training_cells(window[:2], window[2:])
    return tables.os_cfar_alpha(pfa, n, tables.os_cfar_rank(n, rank))


def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / math.sqrt(2)).astype(np.complex64)


def run_oscfar(ctx, rds_dev, window, rank, alpha, thr_power=-1.0, gate=NO_GATE, want_db=False):
    torch = ctx.torch
    pk = torch.full(tuple(rds_dev.shape), float('nan'), dtype=torch.float32, device=rds_dev.device)
    mask, rc, db = ctx.detect_oscfar(rds_dev, window[:2], window[2:], rank, alpha, thr_power, gate[0], gate[1],
                                     want_db=want_db, out=dict(peak_pow=pk))
    torch.cuda.synchronize()
    return dict(mask=mask.cpu().numpy(), row_count=rc.cpu().numpy(), peak_pow=pk.cpu().numpy(),
                db=db.cpu().numpy() if db is not None else None)


def check_against_oracle(tag, rds_np, window, rank, alpha, got, thr_power=-1.0, gate=NO_GATE, cap=None):
    """Cap on the reference alone, then mask / row_count / peak_pow (/ db_map) against it.  Returns the GPU mask."""
    C = rds_np.shape[-1]
    ref = R.oscfar_reference(rds_np, window, rank, alpha, thr_power=thr_power, gate=gate)
    cells = ref['mask'].size
    n_near = int(ref['near'].sum())
    print(f'\n{tag}: reference peaks {int(ref["mask"].sum())} of {cells} cells, near-threshold {n_near}')
    assert n_near <= (R.near_cap(cells) if cap is None else cap), (tag, n_near, cells)
    gm = R.mask_bool(got['mask'], C)
    ng, nr, nd, nu = R.oscfar_diff(gm, ref)
    print(f'{tag}: gpu peaks {ng}, differing {nd}, unexplained {nu}')
    assert nu == 0, (tag, ng, nr, nd, nu)
    cnt = gm.sum(-1)
    assert (got['row_count'] == cnt).all(), tag
    # row-compact peak powers: slot k of a row = the power of its k-th peak in Doppler order; the rest untouched
    rows = gm.reshape(-1, C)
    pkf = got['peak_pow'].reshape(-1, C)
    slot = np.cumsum(rows, axis=1) - 1
    ri = np.nonzero(rows)[0]
    want = ref['p'].reshape(-1, C)[rows]
    have = pkf[ri, slot[rows]].astype(np.float64)
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
@pytest.mark.parametrize('rank', [0.75, 0.5])
@pytest.mark.parametrize('window', WINDOWS)
def test_oracle_parity(ctx, small_rds, window, rank, pfa):
    """Rows 0 .. hr-1 and S-hr .. S-1 have a truncated window (k = 45 against 84 at (1, 1, 4, 4), rank 0.75)."""
    dev, host = small_rds
    alpha = alpha_for(window, pfa, rank)
    got = run_oscfar(ctx, dev, window, rank, alpha, want_db=True)
    gm = check_against_oracle(f'parity {window} rank {rank} pfa {pfa}', host, window, rank, alpha, got, cap=2)
    if pfa == 1e-2:
        assert gm.any()


# -- 2. strong cells --------------------------------------------------------------------------------------
@pytest.mark.parametrize('window', WINDOWS)
def test_strong_cells(ctx, window):
    host = spiked_maps()
    alpha = alpha_for(window, 1e-2, 0.75)
    got = run_oscfar(ctx, ctx.to_dev(host), window, 0.75, alpha)
    gm = check_against_oracle(f'strong {window}', host, window, 0.75, alpha, got)
    for f, a in ((0, 1), (1, 0)):
        assert gm[f, a, 0, 0] and gm[f, a, 31, 16] and gm[f, a, 63, 31]


# -- 3. masking: three equal reflectors inside each other's window ------------------------------------------
def test_masking_on_device(ctx):
    from rsl import tables
    from test_oscfar_host import masking_scene
    host = masking_scene()[None, None]
    dev = ctx.to_dev(host)
    window, targets = (0, 1, 0, 6), [(20, 10), (20, 13), (20, 16)]
    ca = run_cfar(ctx, dev, window, tables.cfar_alpha(1e-4, 12))
    cm = CA.mask_bool(ca['mask'], 32)[0, 0]
    assert not any(cm[t] for t in targets)
    alpha = alpha_for(window, 1e-4, 0.75)
    got = run_oscfar(ctx, dev, window, 0.75, alpha)
    gm = check_against_oracle('masking', host, window, 0.75, alpha, got)[0, 0]
    assert all(gm[t] for t in targets)


# -- 4. shapes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S,C,window', [(50, 100, (2, 2, 8, 8)), (21, 21, (2, 2, 8, 8)), (200, 64, (2, 2, 8, 8)),
                                        (130, 128, (2, 2, 8, 8)), (40, 512, (2, 2, 8, 8)),
                                        (40, 512, (4, 4, 12, 12))])
def test_shapes(ctx, S, C, window):
    A = 1 if window[2] == 12 else 2  # the largest window (hr = hd = RSL_CFAR_MAX_HALF) at [1, 1, 40, 512]
    host = noise((1, A, S, C), S * 1000 + C)
    alpha = alpha_for(window, 1e-2, 0.75)
    got = run_oscfar(ctx, ctx.to_dev(host), window, 0.75, alpha)
    check_against_oracle(f'shape S{S} C{C} {window}', host, window, 0.75, alpha, got)
    # with a range gate and a power floor
    gate, floor = (5, S - 7), 3.0
    got = run_oscfar(ctx, ctx.to_dev(host), window, 0.75, 2.0, thr_power=floor, gate=gate)
    gm = check_against_oracle(f'shape S{S} C{C} {window} gated', host, window, 0.75, 2.0, got, thr_power=floor,
                              gate=gate)
    assert gm.any() and not gm[:, :, :gate[0]].any() and not gm[:, :, gate[1] + 1:].any()


# -- 5. degenerate maps -----------------------------------------------------------------------------------
def test_degenerate_maps(ctx):
    S, C = 48, 64
    window = (2, 2, 8, 8)
    zero = ctx.to_dev(np.zeros((1, 2, S, C), np.complex64))
    got = run_oscfar(ctx, zero, window, 0.75, 0.5)
    assert not got['mask'].any() and not got['row_count'].any() and np.isnan(got['peak_pow']).all()
    const = ctx.to_dev(np.full((1, 2, S, C), 1.5 + 0.5j, np.complex64))  # p = 2.5, alpha p exact in fp32
    got = run_oscfar(ctx, const, window, 0.75, 2.0)
    assert not got['mask'].any() and not got['row_count'].any()
    got = run_oscfar(ctx, const, window, 0.75, 0.5, gate=(3, 40))
    want_rows = np.zeros(S, np.int32)
    want_rows[3:41] = C
    assert (got['row_count'] == want_rows[None, None, :]).all()
    assert R.mask_bool(got['mask'], C)[:, :, 3:41].all()
    assert (got['peak_pow'][:, :, 3:41] == np.float32(2.5)).all()
    assert np.isnan(got['peak_pow'][:, :, :3]).all() and np.isnan(got['peak_pow'][:, :, 41:]).all()


@pytest.mark.parametrize('rank,alpha', [(1.0, 0.6), (1e-6, 30.0)])
def test_extreme_ranks(ctx, rank, alpha):
    """rank 1: the window maximum (k = n(i)); a tiny rank: the minimum (k = 1)."""
    host = noise((1, 2, 48, 64), 77)
    window = (1, 1, 4, 4)
    got = run_oscfar(ctx, ctx.to_dev(host), window, rank, alpha)
    gm = check_against_oracle(f'rank {rank}', host, window, rank, alpha, got)
    assert gm.any() and not gm.all()


# -- 6. arguments -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape,guard,train,alpha', BAD)
def test_bad_arguments(ctx, shape, guard, train, alpha):
    torch = ctx.torch
    rds = torch.zeros((1, 1) + shape, dtype=torch.complex64, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.detect_oscfar(rds, guard, train, 0.75, alpha, -1.0, 0, shape[0] - 1)


@pytest.mark.parametrize('rank', [0.0, -0.1, 1.0001, float('nan')])
def test_bad_rank(ctx, rank):
    torch = ctx.torch
    rds = torch.zeros((1, 1, 64, 64), dtype=torch.complex64, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.detect_oscfar(rds, (2, 2), (8, 8), rank, 5.0, -1.0, 0, 63)


# -- 7. empty batch ---------------------------------------------------------------------------------------
def test_empty_batch_launches_nothing(ctx):
    torch = ctx.torch
    ctx.timing(True)
    try:
        ctx.timing_reset()
        empty = torch.zeros((0, 2, 64, 64), dtype=torch.complex64, device=ctx.device)
        mask, rc, _ = ctx.detect_oscfar(empty, (2, 2), (8, 8), 0.75, 5.0, -1.0, 0, 63)
        assert tuple(mask.shape) == (0, 2, 64, 1) and tuple(rc.shape) == (0, 2, 64)
        assert ctx.timing_read()['detect'][1] == 0
        one = torch.zeros((1, 2, 64, 64), dtype=torch.complex64, device=ctx.device)
        ctx.detect_oscfar(one, (2, 2), (8, 8), 0.75, 5.0, -1.0, 0, 63)
        assert ctx.timing_read()['detect'][1] == 1  # timed under RSL_K_DETECT
    finally:
        ctx.timing_reset()
        ctx.timing(False)


# -- 8. chain ---------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def chains(ctx):
    import rsl
    frames = make_frames(8, 64, 25.6e-6, (1000, 1001))
    cube = ctx.to_dev(frames.astype(np.complex64))
    out = {}
    for name, kw in (('plain', {}), ('cfar', dict(detector='cfar', cfar_pfa=1e-2)),
                     ('ca', dict(detector='cfar', cfar_pfa=1e-2, cfar_method='ca')),
                     ('os', dict(detector='cfar', cfar_method='os', cfar_pfa=1e-2)),
                     ('none', dict(detector='cfar', cfar_method='os', cfar_alpha=1e9))):
        ch = rsl.RadarChain(rsl.ChainConfig(**CH, **kw), 2, ctx)
        ch.run(cube)
        res = ch.results()
        res['rds'] = ch.rds.cpu().numpy()
        res['mask'] = ch.mask.cpu().numpy()
        res['chain'] = ch
        out[name] = res
    return out


def test_chain_oscfar_entries_and_cells(chains):
    from rsl import tables
    r = chains['os']
    ch = r['chain']
    C = 64
    window = (2, 2, 8, 8)
    assert ch.cfar_alpha == tables.os_cfar_alpha(1e-2, 416, 312)
    thr = tables.power_threshold(-20.0)
    ref = R.oscfar_reference(r['rds'], window, 0.75, ch.cfar_alpha, thr_power=thr, gate=(ch.i_lo, ch.i_hi))
    n_near = int(ref['near'].sum())
    print(f'\nchain: reference peaks {int(ref["mask"].sum())}, near-threshold {n_near} of {ref["mask"].size}')
    assert n_near <= R.near_cap(ref['mask'].size)
    gm = R.mask_bool(r['mask'], C)
    ng, nr, nd, nu = R.oscfar_diff(gm, ref)
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


def test_chain_oscfar_cells_match_default_chain(chains):
    """gidx / esprit / phase of every OS-CFAR cell equal, bit for bit, the default detector's values for that cell
    (with the -20 dB floor in force the OS-CFAR cells are a subset of its cells)."""
    r, d = chains['os'], chains['plain']
    key = lambda x: x['c_frame'].astype(np.int64) << 32 | x['c_rc'].astype(np.int64)
    kd, kr = key(d), key(r)
    assert (np.diff(kd) > 0).all()
    pos = np.searchsorted(kd, kr)
    assert (pos < len(kd)).all() and (kd[pos] == kr).all()
    assert len(kr) > 0 and len(kr) < len(kd)
    assert (r['gidx'] == d['gidx'][pos]).all()
    for name in ('esprit', 'phase'):
        assert (r[name].view(np.int64) == d[name][pos].view(np.int64)).all(), name


def test_chain_method_ca_is_the_cfar_chain(chains):
    a, b = chains['cfar'], chains['ca']
    assert a['chain'].cfar_alpha == b['chain'].cfar_alpha
    assert (a['mask'] == b['mask']).all()
    for k in RESULT_KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def test_chain_oscfar_no_detection(chains):
    r = chains['none']
    assert r['entry_base'][-1] == 0 and r['cell_base'][-1] == 0
    assert len(r['e_ant']) == 0 and len(r['c_rc']) == 0 and len(r['gidx']) == 0
    assert (r['velocity'][:, 5] == 0).all()
    assert not r['mask'].any()


# -- 9. drop-in -------------------------------------------------------------------------------------------
def test_dropin_oscfar(ctx):
    from rsl import ops
    from src.radar_signal.dechirp import SignalPreprocessor
    frame = make_frames(4, 32, 6.4e-6, (7,))[0]
    pre = SignalPreprocessor(chirp_duration=6.4e-6)
    rds = pre.generate_range_doppler_spectrum(frame)
    out = pre.extract_range_doppler_peaks_cfar(rds, pfa=1e-2, method='os', min_range=0.0, max_range=1e9)
    assert set(out) == {'peaks', 'range_bins_m', 'doppler_bins_hz', 'power_spectrum_db'}
    want = ops.detect_peaks_cfar(rds, pfa=1e-2, method='os', ctx=ctx)
    got = [(p['antenna'], int(p['range_bin']), int(p['doppler_bin'])) for p in out['peaks']]
    assert got == list(zip(want['antenna'].tolist(), want['range_bin'].tolist(), want['doppler_bin'].tolist()))
    assert len(got) > 0
    assert set(out['peaks'][0]) == {'antenna', 'range_bin', 'doppler_bin', 'range_m', 'doppler_hz', 'power_db'}
    assert np.allclose([p['power_db'] for p in out['peaks']], want['power_db'])
    ca = ops.detect_peaks_cfar(rds, pfa=1e-2, ctx=ctx)  # the default method is 'ca', as before
    assert ca['antenna'].tolist() == ops.detect_peaks_cfar(rds, pfa=1e-2, method='ca', ctx=ctx)['antenna'].tolist()
    with pytest.raises(ValueError):
        ops.detect_peaks_cfar(rds, pfa=1e-2, method='go', ctx=ctx)
