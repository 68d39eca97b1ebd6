"""GPU tests of detection on the antenna-summed power map (non-coherent integration): rsl_power_integrate /
k_power_integrate, rsl_detect_power (the three detection kernels instantiated for a real element), the chain option
detect_on='sum' and the drop-in method, against the fp64 oracle of tests/nci_ref.py.

The oracle of a detector runs on the fp64 cast of the very power map the GPU produced, so only the detector is under
test; every parity case first asserts, on the reference alone, that the tolerance bands hold at most near_cap(cells)
cells, then asserts zero unexplained differences (as tests/cfar_cases.py does).
"""
import functools
import math

import numpy as np
import pytest

import cfar_cases as K
import cfar_ref as R
import nci_ref as N
from cfar_cases import BAD, CH, DEFAULT, LARGEST, NO_GATE, WINDOWS

pytestmark = pytest.mark.gpu

SHAPES = [(2, 8, 64, 32), (1, 4, 50, 100), (1, 2, 21, 21), (1, 3, 200, 64), (1, 16, 40, 512), (1, 1, 48, 64)]
SUMMED = [s for s in SHAPES if s[1] > 1]
RULES = [('ca', None), ('os', 0.75)]
_cache = {}


def ident(v):
    return '-'.join(map(str, v)) if isinstance(v, tuple) else None


def noise_rds(shape):
    F, A, S, C = shape
    return K.noise(shape, 1000 * S + C + A)


def summed(ctx, shape):
    """(device power f32 [F, S, C], its fp64 host cast, host RDS) of the shape's noise map, integrated on the GPU once."""
    if shape not in _cache:
        z = noise_rds(shape)
        p = ctx.integrate_power(ctx.to_dev(z))
        _cache[shape] = (p, p.cpu().numpy().astype(np.float64), z)
    return _cache[shape]


@functools.lru_cache(maxsize=None)
def design(method, rank, window, pfa, looks):
    from rsl import tables
    return tables.cfar_design_alpha(method, pfa, window[:2], window[2:], 0.75 if rank is None else rank, looks=looks)


def run(ctx, power, rule, window, alpha, rank=None, thr_power=-1.0, gate=NO_GATE, want_db=False):
    """detect_power with NaN-prefilled peak powers -> host dict with the unit antenna axis."""
    torch = ctx.torch
    F, S, C = power.shape
    pk = torch.full((F, 1, S, C), float('nan'), dtype=torch.float32, device=power.device)
    window = window or DEFAULT
    mask, rc, db = ctx.detect_power(power, rule, window[:2], window[2:], 0.75 if rank is None else rank, alpha,
                                    thr_power, gate[0], gate[1], want_db=want_db, out=dict(peak_pow=pk))
    torch.cuda.synchronize()
    assert tuple(mask.shape) == (F, 1, S, (C + 63) // 64) and tuple(rc.shape) == (F, 1, S)
    return dict(mask=mask.cpu().numpy(), row_count=rc.cpu().numpy(), peak_pow=pk.cpu().numpy(),
                db=db.cpu().numpy() if db is not None else None)


def check(tag, got, p64, rule, window, alpha, rank=None, thr_power=-1.0, gate=NO_GATE):
    """Cap on the reference alone, then mask / row_count / peak_pow (/ dB map) of a run on the power map p64 [F, S, C]
    against it (the checks of cfar_cases.check_against_oracle).  Returns (GPU mask bool [F, S, C], reference)."""
    C = p64.shape[-1]
    ref = N.reference_power(p64, window, alpha, method=rule, rank=rank, thr_power=thr_power, gate=gate)
    cells = ref['mask'].size
    n_near = int(ref['near'].sum())
    print(f'\n{tag}: reference peaks {int(ref["mask"].sum())} of {cells} cells, near-threshold {n_near}')
    assert n_near <= N.near_cap(cells), (tag, n_near, cells)
    gm = N.mask_bool(got['mask'], C)[:, 0]
    ng, nr, nd, nu = N.diff(gm, ref)
    print(f'{tag}: gpu peaks {ng}, differing {nd}, unexplained {nu}')
    assert nu == 0, (tag, ng, nr, nd, nu)
    cnt = gm.sum(-1)
    assert (got['row_count'][:, 0] == cnt).all(), tag
    rows = gm.reshape(-1, C)
    pkf = got['peak_pow'].reshape(-1, C)
    slot = np.cumsum(rows, axis=1) - 1
    ri = np.nonzero(rows)[0]
    assert (pkf[ri, slot[rows]].astype(np.float64) == p64.reshape(-1, C)[rows]).all(), tag  # the map's own values
    assert (np.isnan(pkf) == (np.arange(C)[None, :] >= cnt.reshape(-1, 1))).all(), tag
    if got['db'] is not None:  # 10 log10f(P + 1e-12f) evaluated in fp32 on the fp32 power
        p32 = p64.astype(np.float32)
        want_db = np.float32(10.0) * np.log10(p32 + np.float32(1e-12))
        err = float(np.abs(got['db'][:, 0].astype(np.float64) - want_db.astype(np.float64)).max())
        print(f'{tag}: db_map max error {err:.3e} dB')
        assert err <= 1e-5, (tag, err)
    return gm, ref


# -- 1. the sum -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', SHAPES, ids=ident)
def test_sum_against_fp64(ctx, shape):
    """Two roundings per term and A - 1 additions of non-negative terms: relative error <= (A + 2) 2^-24."""
    A = shape[1]
    p, p64, z = summed(ctx, shape)
    assert tuple(p.shape) == (shape[0], shape[2], shape[3]) and p.dtype == ctx.torch.float32
    want = N.integrate(z)
    err = float((np.abs(p64 - want) / want).max())
    print(f'\nsum {shape}: max relative error {err:.3e}, bound {(A + 2) * 2.0 ** -24:.3e}')
    assert err <= (A + 2) * 2.0 ** -24


@pytest.mark.parametrize('shape', [(1, 4, 50, 100), (1, 2, 21, 21), (2, 16, 40, 512), (1, 11, 8, 24)], ids=ident)
def test_sum_of_small_integers_is_exact(ctx, shape):
    rng = np.random.default_rng(shape[1])
    z = (rng.integers(-8, 9, shape) + 1j * rng.integers(-8, 9, shape)).astype(np.complex64)
    got = ctx.integrate_power(ctx.to_dev(z)).cpu().numpy()
    assert (got.astype(np.float64) == N.integrate(z)).all()


def test_sum_unaligned_input_takes_the_scalar_path(ctx):
    """A view 8 bytes into an allocation is not 16-B aligned: the same values by the one-cell-per-lane form."""
    torch = ctx.torch
    shape = (1, 4, 50, 100)
    p, _, z = summed(ctx, shape)
    buf = torch.empty((z.size + 1,), dtype=torch.complex64, device=ctx.device)
    view = buf[1:].view(shape)
    view.copy_(ctx.to_dev(z))
    assert view.data_ptr() % 16 == 8
    assert torch.equal(ctx.integrate_power(view), p)
    out = torch.empty((z.size // 4 + 1,), dtype=torch.float32, device=ctx.device)[1:].view(1, 50, 100)
    assert torch.equal(ctx.integrate_power(ctx.to_dev(z), out=out), p)


def test_sum_empty_batch_launches_nothing_and_arguments(ctx):
    torch = ctx.torch
    ctx.timing(True)
    try:
        ctx.timing_reset()
        empty = torch.zeros((0, 8, 64, 64), dtype=torch.complex64, device=ctx.device)
        assert tuple(ctx.integrate_power(empty).shape) == (0, 64, 64)
        m, rc, _ = ctx.detect_power(torch.zeros((0, 64, 64), device=ctx.device), 'ca', (2, 2), (8, 8), 0.75, 5.0, -1.0,
                                    0, 63)
        assert tuple(m.shape) == (0, 1, 64, 1) and tuple(rc.shape) == (0, 1, 64)
        assert ctx.timing_read()['detect'][1] == 0
        one = torch.zeros((1, 8, 64, 64), dtype=torch.complex64, device=ctx.device)
        p = ctx.integrate_power(one)
        assert ctx.timing_read()['detect'][1] == 1  # timed under RSL_K_DETECT
        for rule in ('threshold', 'ca', 'os'):
            ctx.detect_power(p, rule, (2, 2), (8, 8), 0.75, 5.0, -1.0, 0, 63)
        assert ctx.timing_read()['detect'][1] == 4
    finally:
        ctx.timing_reset()
        ctx.timing(False)
    with pytest.raises(ValueError):
        ctx.integrate_power(torch.zeros((1, 33, 8, 8), dtype=torch.complex64, device=ctx.device))
    out = torch.zeros((1, 8, 8), device=ctx.device)
    rds = torch.zeros((1, 2, 8, 8), dtype=torch.complex64, device=ctx.device)
    ctx._bind()
    for r, o in ((None, out.data_ptr()), (rds.data_ptr(), None)):
        with pytest.raises(ValueError):
            ctx.check(ctx.lib.rsl_power_integrate(ctx.h, r, 1, 2, 8, 8, o), 'null pointer')
    with pytest.raises(ValueError):
        ctx.check(ctx.lib.rsl_power_integrate(ctx.h, rds.data_ptr(), 1, 0, 8, 8, out.data_ptr()), 'A = 0')
    with pytest.raises(ValueError):
        ctx.integrate_power(torch.zeros((1, 2, 8, 8), device=ctx.device))  # not complex64


# -- 2. one antenna: the new path is the old kernels, bit for bit ---------------------------------------------------
def one_antenna_maps(ctx):
    if 'one' not in _cache:
        dev, _ = K.small_rds(ctx)
        _cache['one'] = [ctx.to_dev(noise_rds((1, 1, 48, 64))), dev[:, 0:1].contiguous()]
    return _cache['one']


def same_outputs(ctx, old, new):
    torch = ctx.torch
    for a, b in zip(old, new):
        assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))  # bytes (NaN included)


@pytest.mark.parametrize('which', [0, 1], ids=['noise-48-64', 'scene-antenna-0'])
@pytest.mark.parametrize('window', WINDOWS, ids=ident)
def test_one_antenna_is_bit_identical_to_the_per_antenna_detectors(ctx, window, which):
    torch = ctx.torch
    rds = one_antenna_maps(ctx)[which]
    F, _, S, C = rds.shape
    power = ctx.integrate_power(rds)

    def nan():
        return torch.full((F, 1, S, C), float('nan'), dtype=torch.float32, device=ctx.device)
    for thr, gate in ((-1.0, NO_GATE), (float(power.median()), (5, S - 7))):
        for rule, rank, old in (('threshold', None, lambda o: ctx.detect(rds, thr, *gate, want_db=True, out=o)),
                                ('ca', None, lambda o: ctx.detect_cfar(rds, window[:2], window[2:], alpha, thr, *gate,
                                                                       want_db=True, out=o)),
                                ('os', 0.75, lambda o: ctx.detect_oscfar(rds, window[:2], window[2:], 0.75, alpha, thr,
                                                                         *gate, want_db=True, out=o))):
            alpha = 1.0 if rule == 'threshold' else design(rule, rank, window, 1e-2, 1)
            po, pn = nan(), nan()
            mo, ro, do = old(dict(peak_pow=po))
            mn, rn, dn = ctx.detect_power(power, rule, window[:2], window[2:], 0.75, alpha, thr, *gate, want_db=True,
                                          out=dict(peak_pow=pn))
            same_outputs(ctx, (mo, ro, do, po), (mn, rn, dn, pn))
            assert int(rn.sum()) > 0, (rule, window, thr)


# -- 3. parity of the three rules on summed maps --------------------------------------------------------------------
PARITY = [(s, w) for s in SUMMED for w in WINDOWS] + [((1, 16, 40, 512), LARGEST)]


@pytest.mark.parametrize('rule,rank', RULES, ids=['ca', 'os'])
@pytest.mark.parametrize('shape,window', PARITY, ids=[f'{ident(s)}-w{ident(w)}' for s, w in PARITY])
def test_parity_on_summed_maps(ctx, shape, window, rule, rank):
    A = shape[1]
    p, p64, _ = summed(ctx, shape)
    for pfa in (1e-2, 1e-4):
        alpha = design(rule, rank, window, pfa, A)
        got = run(ctx, p, rule, window, alpha, rank, want_db=(pfa == 1e-2))
        gm, ref = check(f'parity {rule} {shape} {window} pfa {pfa}', got, p64, rule, window, alpha, rank)
        # the design: the level alone is crossed by about pfa of the cells (a 3x3 maximum among them nearly always)
        crossed = int((ref['p'] > ref['level']).sum())
        print(f'level crossed by {crossed} cells, design {pfa * ref["p"].size:.1f}')


@pytest.mark.parametrize('rule,rank', RULES + [('threshold', None)], ids=['ca', 'os', 'threshold'])
@pytest.mark.parametrize('shape', SUMMED, ids=ident)
def test_gate_and_floor_on_summed_maps(ctx, shape, rule, rank):
    """The gated and floored run of each shape: the floor is the mean summed power A (threshold rule: two standard
    deviations above it), the factor the Pfa 1e-2 design; the result is the ungated, unfloored mask cut to the gate
    and the floor."""
    A, S = shape[1], shape[2]
    p, p64, _ = summed(ctx, shape)
    gate = (5, S - 7)
    floor = A * (1 + 2 / math.sqrt(A)) if rule == 'threshold' else float(A)
    alpha = 1.0 if rule == 'threshold' else design(rule, rank, DEFAULT, 1e-2, A)
    got = run(ctx, p, rule, DEFAULT, alpha, rank, thr_power=floor, gate=gate, want_db=True)
    gm, _ = check(f'gated {rule} {shape}', got, p64, rule, DEFAULT, alpha, rank, thr_power=floor, gate=gate)
    assert not gm[:, :gate[0]].any() and not gm[:, gate[1] + 1:].any()
    free = N.mask_bool(run(ctx, p, rule, DEFAULT, alpha, rank)['mask'], shape[3])[:, 0]
    g = np.zeros(S, bool)
    g[gate[0]:gate[1] + 1] = True
    assert (gm == (free & g[None, :, None] & (p64 > floor))).all()
    if gm.size >= 4096:
        assert gm.any()


@pytest.mark.parametrize('rule,rank', RULES, ids=['ca', 'os'])
def test_degenerate_maps(ctx, rule, rank):
    S, C = 48, 64
    zero = ctx.integrate_power(ctx.to_dev(np.zeros((1, 4, S, C), np.complex64)))
    assert not zero.any()
    got = run(ctx, zero, rule, DEFAULT, 0.5, rank)
    assert not got['mask'].any() and not got['row_count'].any() and np.isnan(got['peak_pow']).all()
    got = run(ctx, zero, 'threshold', None, 1.0, thr_power=0.0)  # p > 0 fails everywhere
    assert not got['mask'].any() and not got['row_count'].any()
    # 4 antennas of 1.5 + 0.5j: P = 10 exactly, and every window sum and every alpha P are exact in fp32
    const = ctx.integrate_power(ctx.to_dev(np.full((1, 4, S, C), 1.5 + 0.5j, np.complex64)))
    assert (const == 10.0).all()
    got = run(ctx, const, rule, DEFAULT, 2.0, rank)
    assert not got['mask'].any() and not got['row_count'].any()
    got = run(ctx, const, rule, DEFAULT, 0.5, rank, gate=(3, 40))
    want_rows = np.zeros(S, np.int32)
    want_rows[3:41] = C
    assert (got['row_count'] == want_rows[None, None, :]).all()
    assert N.mask_bool(got['mask'], C)[:, :, 3:41].all()
    assert (got['peak_pow'][:, :, 3:41] == np.float32(10.0)).all()
    assert np.isnan(got['peak_pow'][:, :, :3]).all() and np.isnan(got['peak_pow'][:, :, 41:]).all()


def over_antennas(maps, A, seed):
    """maps c64 [F, S, C] -> [F, A, S, C]: every antenna its own unit noise, the strong cells of the map (the
    reflectors, |z| > 10) repeated on every antenna; antenna 0 is the map itself."""
    F, S, C = maps.shape
    z = K.noise((F, A, S, C), seed)
    z[:, 0] = maps
    strong = np.abs(maps) > 10
    for a in range(1, A):
        z[:, a][strong] = maps[strong]
    return z


@pytest.mark.parametrize('rule,rank', RULES, ids=['ca', 'os'])
@pytest.mark.parametrize('window', WINDOWS, ids=ident)
def test_strong_cells_on_summed_maps(ctx, window, rule, rank):
    """cfar_cases.spiked_maps over 4 antennas: the add-only training sum of CA, the count of OS that no outlier
    moves."""
    z = over_antennas(K.spiked_maps().reshape(4, 64, 32), 4, 41)  # frames: quiet, spiked, spiked, quiet
    p = ctx.integrate_power(ctx.to_dev(z))
    alpha = design(rule, rank, window, 1e-2, 4)
    got = run(ctx, p, rule, window, alpha, rank)
    gm, _ = check(f'strong {rule} {window}', got, p.cpu().numpy().astype(np.float64), rule, window, alpha, rank)
    for f in (1, 2):
        assert gm[f, 0, 0] and gm[f, 31, 16] and gm[f, 63, 31]


def test_masking_on_summed_maps(ctx):
    """Three equal reflectors (amplitude 30 on each of 4 antennas) inside each other's window (0, 1, 0, 6).  Two of
    them among 12 training cells hold the CA level near alpha P / 6, so CA loses them once alpha > 6.  A sum of 4 looks
    needs Pfa 1e-6 for that (alpha = 6.48; at 1e-4 it is 4.56, where one look had 13.9): the case runs at 1e-6, where
    the CA reference keeps none and OS keeps all three."""
    z = over_antennas(K.masking_scene()[None], 4, 12)
    p = ctx.integrate_power(ctx.to_dev(z))
    p64 = p.cpu().numpy().astype(np.float64)
    window, targets, pfa = (0, 1, 0, 6), [(20, 10), (20, 13), (20, 16)], 1e-6
    a_ca = design('ca', None, window, pfa, 4)
    ref_ca = N.reference_power(p64, window, a_ca, method='ca')
    assert not any(ref_ca['mask'][0][t] for t in targets)  # on the reference first
    cm, _ = check('masking ca', run(ctx, p, 'ca', window, a_ca), p64, 'ca', window, a_ca)
    assert not any(cm[0][t] for t in targets)
    a_os = design('os', 0.75, window, pfa, 4)
    gm, _ = check('masking os', run(ctx, p, 'os', window, a_os, 0.75), p64, 'os', window, a_os, 0.75)
    assert all(gm[0][t] for t in targets)


# -- 4. the motivating scene on the device --------------------------------------------------------------------------
def test_motivating_scene_on_the_device(ctx):
    z, cells = N.motivating_scene()
    ii, jj = np.array(cells).T
    dev = ctx.to_dev(z)
    p = ctx.integrate_power(dev)
    alpha = design('ca', None, DEFAULT, 1e-4, 8)
    got = run(ctx, p, 'ca', DEFAULT, alpha)
    gm, ref = check('motivating scene', got, p.cpu().numpy().astype(np.float64), 'ca', DEFAULT, alpha)
    assert (gm == ref['mask']).all()
    assert gm[0][ii, jj].all() and int(gm.sum()) - 54 <= 5
    per = K.run(ctx, K.CA, dev, DEFAULT, K.alpha_for(K.CA, DEFAULT, 1e-4))
    union = R.mask_bool(per['mask'], 64)[0].any(axis=0)
    print(f'per-antenna union holds {int(union[ii, jj].sum())} of 54, integrated {int(gm[0][ii, jj].sum())}')
    assert int(union[ii, jj].sum()) < 40


# -- 5. arguments -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rule', ['ca', 'os'])
@pytest.mark.parametrize('shape,guard,train,alpha', BAD)
def test_bad_arguments(ctx, shape, guard, train, alpha, rule):
    power = ctx.torch.zeros((1,) + shape, dtype=ctx.torch.float32, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.detect_power(power, rule, guard, train, 0.75, alpha, -1.0, 0, shape[0] - 1)


@pytest.mark.parametrize('rank', [0.0, -0.1, 1.0001, float('nan')])
def test_bad_rank(ctx, rank):
    power = ctx.torch.zeros((1, 64, 64), dtype=ctx.torch.float32, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.detect_power(power, 'os', (2, 2), (8, 8), rank, 5.0, -1.0, 0, 63)
    ctx.detect_power(power, 'ca', (2, 2), (8, 8), rank, 5.0, -1.0, 0, 63)  # CA does not look at it


@pytest.mark.parametrize('rule', ['go', 3, -1])
def test_unknown_rule(ctx, rule):
    power = ctx.torch.zeros((1, 64, 64), dtype=ctx.torch.float32, device=ctx.device)
    with pytest.raises(ValueError):
        ctx.detect_power(power, rule, (2, 2), (8, 8), 0.75, 5.0, -1.0, 0, 63)


def test_power_of_wrong_dtype_or_rank(ctx):
    torch = ctx.torch
    for bad in (torch.zeros((1, 64, 64), dtype=torch.float64, device=ctx.device),
                torch.zeros((1, 64, 64), dtype=torch.complex64, device=ctx.device),
                torch.zeros((1, 1, 64, 64), dtype=torch.float32, device=ctx.device),
                torch.zeros((64, 64), dtype=torch.float32, device=ctx.device)):
        with pytest.raises(ValueError):
            ctx.detect_power(bad, 'ca', (2, 2), (8, 8), 0.75, 5.0, -1.0, 0, 63)
    # the threshold rule ignores window, rank and factor
    ok = torch.ones((1, 8, 8), dtype=torch.float32, device=ctx.device)
    _, rc, _ = ctx.detect_power(ok, 'threshold', (-1, -1), (0, 0), float('nan'), float('nan'), 0.5, 0, 7)
    assert int(rc.sum()) == 64


# -- 6. chain -----------------------------------------------------------------------------------------------------
SUM_CHAINS = {'ca': dict(detector='cfar', cfar_pfa=1e-2), 'os': dict(detector='cfar', cfar_method='os', cfar_pfa=1e-2),
              'threshold': dict(detector='threshold')}


@pytest.fixture(scope='module')
def chains(ctx):
    """name -> results of the two-frame batch of cfar_cases.chains through a chain with detect_on='sum' (+ 'plain',
    the default chain of cfar_cases; 'antenna', the default spelled out; 'none', a factor that detects nothing;
    'guarded', the CA chain with guard pads and the smoothed MUSIC)."""
    import rsl
    out = {'plain': K.chains(ctx)['plain']}
    cube = ctx.to_dev(K.make_frames(8, 64, 25.6e-6, (1000, 1001)).astype(np.complex64))
    variants = {name: dict(detect_on='sum', **kw) for name, kw in SUM_CHAINS.items()}
    variants['antenna'] = dict(detect_on='antenna')
    variants['none'] = dict(detect_on='sum', detector='cfar', cfar_alpha=1e9)
    variants['guarded'] = dict(detect_on='sum', multi_source=True, **SUM_CHAINS['ca'])
    for name, kw in variants.items():
        ch = rsl.RadarChain(rsl.ChainConfig(**CH, **kw), 2, ctx, guard=(name == 'guarded'))
        ch.run(cube)
        res = ch.results()
        res['rds'] = ch.rds.cpu().numpy()
        res['mask'] = ch.mask.cpu().numpy()
        res['chain'] = ch
        out[name] = res
    return out


@pytest.mark.parametrize('name', list(SUM_CHAINS))
def test_chain_power_mask_and_lists(ctx, chains, name):
    from rsl import tables
    torch = ctx.torch
    r = chains[name]
    ch, cfg = r['chain'], r['chain'].cfg
    C, S = 64, ch.S
    assert tuple(ch.power.shape) == (2, S, C) and tuple(ch.mask.shape) == (2, 1, S, 1)
    assert tuple(ch.row_count.shape) == (2, 1, S) and tuple(ch.peak_pow.shape) == (2, 1, S, C)
    assert ch.entry_cap == int(math.ceil(cfg.entry_frac * 2 * S * C)) + 64
    assert torch.equal(ch.power.view(torch.int32), ctx.integrate_power(ch.rds).view(torch.int32))
    rule = 'threshold' if name == 'threshold' else name
    rank = 0.75 if name == 'os' else None
    if name == 'threshold':
        assert ch.cfar_alpha is None
    else:
        assert ch.cfar_alpha == tables.cfar_design_alpha(name, 1e-2, (2, 2), (8, 8), 0.75, looks=8)
    p64 = ch.power.cpu().numpy().astype(np.float64)
    ref = N.reference_power(p64, DEFAULT, ch.cfar_alpha, method=rule, rank=rank,
                            thr_power=tables.power_threshold(-20.0), gate=(ch.i_lo, ch.i_hi))
    n_near = int(ref['near'].sum())
    print(f'\nchain sum {name}: reference peaks {int(ref["mask"].sum())}, near-threshold {n_near} of {ref["mask"].size}')
    assert n_near <= N.near_cap(ref['mask'].size)
    gm = N.mask_bool(r['mask'], C)[:, 0]
    ng, nr, nd, nu = N.diff(gm, ref)
    print(f'chain sum {name}: gpu peaks {ng}, differing {nd}, unexplained {nu}')
    assert nu == 0 and ng > 0
    assert not gm[:, :ch.i_lo].any() and not gm[:, ch.i_hi + 1:].any()
    # every cell is one entry
    eb, cb = r['entry_base'], r['cell_base']
    assert (eb == cb).all() and eb[-1] == ng == len(r['e_ant']) == len(r['c_rc'])
    assert (r['e_ant'] == 0).all() and (r['c_amask'] == 1).all()
    assert (r['e_cell'] == np.arange(ng)).all()  # its own position in the batch's cell list (cell_base included)
    for f in range(2):
        i, j = np.nonzero(gm[f])  # range -> doppler
        sl = slice(eb[f], eb[f + 1])
        assert (r['e_rbin'][sl] == i).all() and (r['e_dbin'][sl] == j).all()
        assert (r['e_cell'][sl] == cb[f] + np.arange(len(i))).all()
        assert (r['c_frame'][sl] == f).all() and (r['c_rc'][sl] == i * C + j).all()
        db = 10 * np.log10(p64[f][i, j] + 1e-12)
        assert np.abs(r['e_pdb'][sl] - db).max() < 1e-4


@pytest.mark.parametrize('name', list(SUM_CHAINS))
def test_chain_cells_match_default_chain(chains, name):
    """gidx / esprit / phase run unchanged on the full-A RDS: bit-identical for every cell the default chain lists too."""
    r, d = chains[name], chains['plain']
    assert r['rds'].tobytes() == d['rds'].tobytes()
    key = lambda x: x['c_frame'].astype(np.int64) << 32 | x['c_rc'].astype(np.int64)
    kd, kr = key(d), key(r)
    assert (np.diff(kd) > 0).all() and (np.diff(kr) > 0).all()
    both = np.isin(kr, kd)
    assert both.any()
    pos = np.searchsorted(kd, kr[both])
    print(f'\nchain sum {name}: {len(kr)} cells, {int(both.sum())} of them among the default chain\'s {len(kd)}')
    assert (r['gidx'][both] == d['gidx'][pos]).all()
    for k in ('esprit', 'phase'):
        assert (r[k][both].view(np.int64) == d[k][pos].view(np.int64)).all(), k


@pytest.mark.parametrize('name', list(SUM_CHAINS))
def test_chain_velocity_weighs_every_cell_once(ctx, chains, name):
    ch = chains[name]['chain']
    cfg = ch.cfg
    out, _, _ = ctx.velocity(None, ch.ext['phase'], ch.offs['cell_base'], k=ch.k, ridge=cfg.ridge, bounds=cfg.bounds,
                             amask=None, gidx=ch.gidx, az_table=ch.az_table, n=ch.cell_cap)
    got = chains[name]['velocity']
    want = out.cpu().numpy()
    assert got.shape == want.shape == (2, 8) and got.tobytes() == want.tobytes()
    cb = chains[name]['cell_base']
    assert (got[:, 5] == np.diff(cb)).all() and (np.diff(cb) >= 3).all()  # the solve's sample count: the cells


def test_chain_no_detection(chains):
    K.chain_no_detection(chains['none'])


def test_chain_detect_on_antenna_is_the_default(chains):
    assert chains['antenna']['chain'].power is None
    K.chain_same_results(chains['plain'], chains['antenna'])


def test_chain_guard_and_multi_source(chains):
    r = chains['guarded']
    ch = r['chain']
    assert ch.guard_violations() == []
    K.chain_same_results(chains['ca'], r)
    nc = int(r['cell_base'][-1])
    assert nc > 0 and r['ss_nsrc'].shape == (nc,) and r['ss_gidx'].shape == (nc, ch.ss.nmax)
    assert ((r['ss_nsrc'] >= 1) & (r['ss_nsrc'] <= ch.ss.nmax)).all()
    # ... of every cell: what a per-call smoothed MUSIC on the chain's own lists gives
    L = ch.lists
    nsrc, idx, den, _, _ = ch.ctx.doa_smoothed(ch.rds, L['c_frame'], L['c_rc'], ch.ss.steer, n=nc, nmax=ch.ss.nmax,
                                               num_sources=ch.cfg.ss_sources, rel=ch.cfg.ss_rel)
    assert (r['ss_nsrc'] == nsrc[:nc].cpu().numpy()).all() and (r['ss_gidx'] == idx[:nc].cpu().numpy()).all()
    assert np.array_equal(r['ss_den'], den[:nc].cpu().numpy().astype(np.float64), equal_nan=True)


# -- 7. drop-in -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(), dict(method='os'), dict(detector='threshold', threshold_db=-20.0)],
                         ids=['ca', 'os', 'threshold'])
def test_dropin_integrated(ctx, kw):
    from rsl import ops
    from src.angle_estimation.angle_estimation import AngleEstimator
    from src.radar_signal.dechirp import SignalPreprocessor
    frame = K.make_frames(4, 32, 6.4e-6, (7,))[0]
    pre = SignalPreprocessor(chirp_duration=6.4e-6)
    rds = pre.generate_range_doppler_spectrum(frame)
    out = pre.extract_range_doppler_peaks_integrated(rds, pfa=1e-2, min_range=0.0, max_range=1e9, **kw)
    assert set(out) == {'peaks', 'range_bins_m', 'doppler_bins_hz', 'power_spectrum_db'}
    okw = dict(kw)
    okw.setdefault('threshold_db', -math.inf)
    want = ops.detect_peaks_integrated(rds, pfa=1e-2, ctx=ctx, **okw)
    got = [(p['antenna'], int(p['range_bin']), int(p['doppler_bin'])) for p in out['peaks']]
    assert got == list(zip(want['antenna'].tolist(), want['range_bin'].tolist(), want['doppler_bin'].tolist()))
    assert len(got) > 0 and all(a == 0 for a, _, _ in got) and want['cells'] == len(got)
    assert set(out['peaks'][0]) == {'antenna', 'range_bin', 'doppler_bin', 'range_m', 'doppler_hz', 'power_db'}
    assert np.allclose([p['power_db'] for p in out['peaks']], want['power_db'])
    db = out['power_spectrum_db']
    assert db.shape == (1,) + rds.shape[1:]
    p64 = ops.integrate_power(rds, ctx=ctx)
    assert p64.shape == rds.shape[1:] and np.abs(db[0] - 10 * np.log10(p64 + 1e-12)).max() < 1e-4
    for p in out['peaks']:
        assert abs(db[p['antenna'], p['range_bin'], p['doppler_bin']] - p['power_db']) < 1e-4
    if kw.get('detector') == 'threshold':
        assert all(p['power_db'] > -20.0 for p in out['peaks'])
    targets = AngleEstimator(num_antennas=4).process_targets(rds, out)
    assert len(targets) == len(out['peaks'])
    with pytest.raises(ValueError):
        ops.detect_peaks_integrated(rds, detector='go', ctx=ctx)
