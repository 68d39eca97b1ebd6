"""The cases that tests/test_gpu_cfar.py (CA: rsl_detect_cfar / k_detect_cfar) and tests/test_gpu_oscfar.py (OS:
rsl_detect_oscfar / k_detect_oscfar) run, and the host checks that test_cfar_host.py and test_oscfar_host.py share
(helper, not collected).  A detector is det = (method, rank): CA = ('ca', None), or ('os', rank).  The two test files
keep their test names and parameters and call these bodies with their detector.

Every parity case first asserts, on the reference alone (tests/cfar_ref.py, run on the very complex64 RDS the kernel
read), that the tolerance bands (cfar_ref.CFAR_RTOL or OS_RTOL on the level, parity.PEAK_RTOL on the 3x3 test) hold at
most cfar_ref.near_cap(cells) cells, then asserts zero unexplained differences.
"""
import math
import os
import re

import numpy as np
import pytest

import cfar_ref as R
import radar_oracle as O

WINDOWS = [(1, 1, 4, 4), (2, 2, 8, 8), (0, 1, 0, 6), (1, 0, 5, 0)]  # (gr, gd, tr, td); Doppler-only, range-only
DEFAULT = (2, 2, 8, 8)
LARGEST = (4, 4, 12, 12)  # hr = hd = RSL_CFAR_MAX_HALF: at C = 512 the largest LDS request of either kernel
NO_GATE = (0, 1 << 30)
CA, OS = ('ca', None), ('os', 0.75)
RESULT_KEYS = ('entry_base', 'cell_base', 'e_ant', 'e_rbin', 'e_dbin', 'e_cell', 'e_pdb', 'c_frame', 'c_rc',
               'c_amask', 'gidx', 'esprit', 'phase', 'velocity')
CH = dict(num_antennas=8, num_chirps=64, chirp_duration=25.6e-6)
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


# -- inputs -----------------------------------------------------------------------------------------------
def alpha_for(det, window, pfa):
    from rsl import tables
    return tables.cfar_design_alpha(det[0], pfa, window[:2], window[2:], det[1])


def noise(shape, seed):
    rng = np.random.default_rng(seed)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / math.sqrt(2)).astype(np.complex64)


def make_frames(A, C, Tc, seeds):
    frames = []
    for s in seeds:
        np.random.seed(s)
        frames.append(O.synthesize_frame(O.TEST_SCENE, chirp_duration=Tc, num_chirps=C, num_antennas=A))
    return np.stack(frames)


def spiked_maps():
    rng = np.random.default_rng(5)

    def unit():
        return ((rng.standard_normal((64, 32)) + 1j * rng.standard_normal((64, 32))) / math.sqrt(2)).astype(
            np.complex64)
    z = unit()
    z[0, 0] = 3e4
    z[31, 16] = 1e5
    z[63, 31] = 3e4
    z[20, 5] = z[20, 7] = 40
    a, b = unit(), unit()
    # [F = 2, A = 2]: the spiked map at (0, 1) and (1, 0), so that its range row 0 and row S-1 both border a quiet map
    return np.stack([np.stack([a, z]), np.stack([z, b])])


def masking_scene():
    """Three equal reflectors inside each other's window."""
    rng = np.random.default_rng(11)
    z = ((rng.standard_normal((64, 32)) + 1j * rng.standard_normal((64, 32))) / math.sqrt(2)).astype(np.complex64)
    z[20, 10] = z[20, 13] = z[20, 16] = 30
    return z


_shared = {}  # what both test files use of one session's GPU context, built once


def small_rds(ctx):
    """(device, host) RDS [2, 4, 64, 32] of two frames of the test scene."""
    if 'small_rds' not in _shared:
        from rsl import ops, tables
        frames = make_frames(4, 32, 6.4e-6, (7, 8))  # S = 64
        table = tables.chirp_table(77e9, 1e9, 6.4e-6, 10e6, 'hann', 64)
        dev = ops.range_doppler(frames, table, ctx=ctx, keep_on_device=True).contiguous()
        assert tuple(dev.shape) == (2, 4, 64, 32)
        _shared['small_rds'] = (dev, dev.cpu().numpy())
    return _shared['small_rds']


def chains(ctx):
    """name -> results of one two-frame batch through a chain: the default, each detector at Pfa 1e-2 ('cfar' leaves
    cfar_method at its default) and each with a factor that detects nothing."""
    if 'chains' not in _shared:
        import rsl
        frames = make_frames(8, 64, 25.6e-6, (1000, 1001))
        cube = ctx.to_dev(frames.astype(np.complex64))
        out = {}
        for name, kw in (('plain', {}), ('threshold', dict(detector='threshold')),
                         ('cfar', dict(detector='cfar', cfar_pfa=1e-2)),
                         ('ca', dict(detector='cfar', cfar_pfa=1e-2, cfar_method='ca')),
                         ('os', dict(detector='cfar', cfar_method='os', cfar_pfa=1e-2)),
                         ('none-ca', dict(detector='cfar', cfar_alpha=1e9)),
                         ('none-os', dict(detector='cfar', cfar_method='os', cfar_alpha=1e9))):
            ch = rsl.RadarChain(rsl.ChainConfig(**CH, **kw), 2, ctx)
            ch.run(cube)
            res = ch.results()
            res['rds'] = ch.rds.cpu().numpy()
            res['mask'] = ch.mask.cpu().numpy()
            res['chain'] = ch
            out[name] = res
        _shared['chains'] = out
    return _shared['chains']


# -- running a detector and checking it ---------------------------------------------------------------------
def detect(ctx, det, rds, guard, train, alpha, thr_power, i_lo, i_hi, **kw):
    """The Context entry point of a detector, with its own positional signature."""
    if det[0] == 'os':
        return ctx.detect_oscfar(rds, guard, train, det[1], alpha, thr_power, i_lo, i_hi, **kw)
    return ctx.detect_cfar(rds, guard, train, alpha, thr_power, i_lo, i_hi, **kw)


def run(ctx, det, rds_dev, window, alpha, thr_power=-1.0, gate=NO_GATE, want_db=False):
    torch = ctx.torch
    pk = torch.full(tuple(rds_dev.shape), float('nan'), dtype=torch.float32, device=rds_dev.device)
    mask, rc, db = detect(ctx, det, rds_dev, window[:2], window[2:], alpha, thr_power, gate[0], gate[1],
                          want_db=want_db, out=dict(peak_pow=pk))
    torch.cuda.synchronize()
    return dict(mask=mask.cpu().numpy(), row_count=rc.cpu().numpy(), peak_pow=pk.cpu().numpy(),
                db=db.cpu().numpy() if db is not None else None)


def check_against_oracle(tag, det, rds_np, window, alpha, got, thr_power=-1.0, gate=NO_GATE, cap=None):
    """Cap on the reference alone, then mask / row_count / peak_pow (/ db_map) against it.  Returns the GPU mask."""
    C = rds_np.shape[-1]
    ref = R.reference(rds_np, window, alpha, method=det[0], rank=det[1], thr_power=thr_power, gate=gate)
    cells = ref['mask'].size
    n_near = int(ref['near'].sum())
    print(f'\n{tag}: reference peaks {int(ref["mask"].sum())} of {cells} cells, near-threshold {n_near}')
    assert n_near <= (R.near_cap(cells) if cap is None else cap), (tag, n_near, cells)
    gm = R.mask_bool(got['mask'], C)
    ng, nr, nd, nu = R.diff(gm, ref)
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


# -- the cases ----------------------------------------------------------------------------------------------
def oracle_parity(ctx, det, window, pfa, cap=None):
    dev, host = small_rds(ctx)
    alpha = alpha_for(det, window, pfa)
    got = run(ctx, det, dev, window, alpha, want_db=True)
    gm = check_against_oracle(f'parity {det} {window} pfa {pfa}', det, host, window, alpha, got, cap=cap)
    if pfa == 1e-2:
        assert gm.any()  # the scene's targets stand above any of these levels


def strong_cells(ctx, det, window):
    """CA: the add-only training sum; OS: the count that no outlier moves."""
    host = spiked_maps()
    alpha = alpha_for(det, window, 1e-2)
    got = run(ctx, det, ctx.to_dev(host), window, alpha)
    gm = check_against_oracle(f'strong {det} {window}', det, host, window, alpha, got)
    for f, a in ((0, 1), (1, 0)):
        assert gm[f, a, 0, 0] and gm[f, a, 31, 16] and gm[f, a, 63, 31]


def shapes(ctx, det, S, C, window=DEFAULT):
    A = 1 if window == LARGEST else 2  # the largest window at [1, 1, 40, 512]
    host = noise((1, A, S, C), S * 1000 + C)
    alpha = alpha_for(det, window, 1e-2)
    got = run(ctx, det, ctx.to_dev(host), window, alpha)
    check_against_oracle(f'shape {det} S{S} C{C} {window}', det, host, window, alpha, got)
    # with a range gate and a power floor
    gate, floor = (5, S - 7), 3.0
    got = run(ctx, det, ctx.to_dev(host), window, 2.0, thr_power=floor, gate=gate)
    gm = check_against_oracle(f'shape {det} S{S} C{C} {window} gated', det, host, window, 2.0, got, thr_power=floor,
                              gate=gate)
    assert gm.any() and not gm[:, :, :gate[0]].any() and not gm[:, :, gate[1] + 1:].any()


def degenerate_maps(ctx, det):
    S, C = 48, 64
    zero = ctx.to_dev(np.zeros((1, 2, S, C), np.complex64))
    got = run(ctx, det, zero, DEFAULT, 0.5)
    assert not got['mask'].any() and not got['row_count'].any() and np.isnan(got['peak_pow']).all()
    # p = 2.5: every window sum and every alpha p are exact in fp32
    const = ctx.to_dev(np.full((1, 2, S, C), 1.5 + 0.5j, np.complex64))
    got = run(ctx, det, const, DEFAULT, 2.0)
    assert not got['mask'].any() and not got['row_count'].any()
    got = run(ctx, det, const, DEFAULT, 0.5, gate=(3, 40))
    want_rows = np.zeros(S, np.int32)
    want_rows[3:41] = C
    assert (got['row_count'] == want_rows[None, None, :]).all()
    assert R.mask_bool(got['mask'], C)[:, :, 3:41].all()
    assert (got['peak_pow'][:, :, 3:41] == np.float32(2.5)).all()
    assert np.isnan(got['peak_pow'][:, :, :3]).all() and np.isnan(got['peak_pow'][:, :, 41:]).all()


def bad_arguments(ctx, det, shape, guard, train, alpha):
    torch = ctx.torch
    rds = torch.zeros((1, 1) + shape, dtype=torch.complex64, device=ctx.device)
    with pytest.raises(ValueError):
        detect(ctx, det, rds, guard, train, alpha, -1.0, 0, shape[0] - 1)


def empty_batch_launches_nothing(ctx, det):
    torch = ctx.torch
    ctx.timing(True)
    try:
        ctx.timing_reset()
        empty = torch.zeros((0, 2, 64, 64), dtype=torch.complex64, device=ctx.device)
        mask, rc, _ = detect(ctx, det, empty, (2, 2), (8, 8), 5.0, -1.0, 0, 63)
        assert tuple(mask.shape) == (0, 2, 64, 1) and tuple(rc.shape) == (0, 2, 64)
        assert ctx.timing_read()['detect'][1] == 0
        one = torch.zeros((1, 2, 64, 64), dtype=torch.complex64, device=ctx.device)
        detect(ctx, det, one, (2, 2), (8, 8), 5.0, -1.0, 0, 63)
        assert ctx.timing_read()['detect'][1] == 1  # timed under RSL_K_DETECT
    finally:
        ctx.timing_reset()
        ctx.timing(False)


def chain_entries_and_cells(r, det, alpha):
    """r: the results of the detector's chain at Pfa 1e-2; alpha: its factor from the tables."""
    from rsl import tables
    ch = r['chain']
    C = 64
    assert ch.cfar_alpha == alpha == alpha_for(det, DEFAULT, 1e-2)
    thr = tables.power_threshold(-20.0)
    ref = R.reference(r['rds'], DEFAULT, alpha, method=det[0], rank=det[1], thr_power=thr, gate=(ch.i_lo, ch.i_hi))
    n_near = int(ref['near'].sum())
    print(f'\nchain {det}: reference peaks {int(ref["mask"].sum())}, near-threshold {n_near} of {ref["mask"].size}')
    assert n_near <= R.near_cap(ref['mask'].size)
    gm = R.mask_bool(r['mask'], C)
    ng, nr, nd, nu = R.diff(gm, ref)
    print(f'chain {det}: gpu peaks {ng}, differing {nd}, unexplained {nu}')
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


def chain_cells_match_default_chain(r, d):
    """gidx / esprit / phase of every CFAR cell of r equal, bit for bit, the default detector's values (d) for that
    cell (with the -20 dB floor in force the CFAR cells are a subset of its cells)."""
    key = lambda x: x['c_frame'].astype(np.int64) << 32 | x['c_rc'].astype(np.int64)
    kd, kr = key(d), key(r)
    assert (np.diff(kd) > 0).all()
    pos = np.searchsorted(kd, kr)
    assert (pos < len(kd)).all() and (kd[pos] == kr).all()
    assert len(kr) > 0 and len(kr) < len(kd)
    assert (r['gidx'] == d['gidx'][pos]).all()
    for name in ('esprit', 'phase'):
        assert (r[name].view(np.int64) == d[name][pos].view(np.int64)).all(), name


def chain_same_results(a, b):
    assert (a['mask'] == b['mask']).all()
    for k in RESULT_KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k


def chain_no_detection(r):
    assert r['entry_base'][-1] == 0 and r['cell_base'][-1] == 0
    assert len(r['e_ant']) == 0 and len(r['c_rc']) == 0 and len(r['gidx']) == 0
    assert (r['velocity'][:, 5] == 0).all()
    assert not r['mask'].any()


def dropin_against_ops(ctx, **method):
    """extract_range_doppler_peaks_cfar against ops.detect_peaks_cfar on one frame's spectrum."""
    from rsl import ops
    from src.radar_signal.dechirp import SignalPreprocessor
    frame = make_frames(4, 32, 6.4e-6, (7,))[0]
    pre = SignalPreprocessor(chirp_duration=6.4e-6)
    rds = pre.generate_range_doppler_spectrum(frame)
    out = pre.extract_range_doppler_peaks_cfar(rds, pfa=1e-2, min_range=0.0, max_range=1e9, **method)
    assert set(out) == {'peaks', 'range_bins_m', 'doppler_bins_hz', 'power_spectrum_db'}
    want = ops.detect_peaks_cfar(rds, pfa=1e-2, ctx=ctx, **method)
    got = [(p['antenna'], int(p['range_bin']), int(p['doppler_bin'])) for p in out['peaks']]
    assert got == list(zip(want['antenna'].tolist(), want['range_bin'].tolist(), want['doppler_bin'].tolist()))
    assert len(got) > 0
    assert set(out['peaks'][0]) == {'antenna', 'range_bin', 'doppler_bin', 'range_m', 'doppler_hz', 'power_db'}
    assert np.allclose([p['power_db'] for p in out['peaks']], want['power_db'])
    return pre, rds, out, got


# -- host surface -------------------------------------------------------------------------------------------
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rsl.h')


def header_source():
    """include/rsl.h without its comments."""
    return re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)


def header_declares(fn, extra):
    """fn is declared with the family's argument names, `extra` between the window and alpha."""
    m = re.search(rf'int\s+{fn}\s*\(([^)]*)\)', header_source())
    assert m, f'{fn} not declared in include/rsl.h'
    names = [a.strip().split()[-1].lstrip('*') for a in m.group(1).split(',')]
    assert names == (['h', 'rds', 'F', 'A', 'S', 'C', 'guard_r', 'guard_d', 'train_r', 'train_d'] + extra +
                     ['alpha', 'thr_power', 'i_lo', 'i_hi', 'mask', 'row_count', 'db_map', 'peak_pow'])


def library_exports_and_rejects_null_handle(fn, extra):
    from rsl import _lib
    assert fn in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, fn)
    rc = getattr(lib, fn)(None, None, 1, 1, 64, 64, 2, 2, 8, 8, *extra, 9.0, -1.0, 0, 63, None, None, None, None)
    assert rc == _lib.RSL_ERR_INVALID == 1


def brute_force_map():
    rng = np.random.default_rng(3)
    z = (rng.standard_normal((12, 9)) + 1j * rng.standard_normal((12, 9))).astype(np.complex64)
    z[4, 4] = 30.0
    z[0, 8] = 20.0
    return z


def check_training_cells(n, window):
    """The count of training cells: full window in the middle rows, truncated at the range edges.  Returns the full
    count."""
    gr, gd, tr, td = window
    full = (2 * (gr + tr) + 1) * (2 * (gd + td) + 1) - (2 * gr + 1) * (2 * gd + 1)
    assert n[6] == full and n[11] == n[0]
    assert n[0] < full if tr else n[0] == full  # a Doppler-only window loses nothing at the range edges
    return full
