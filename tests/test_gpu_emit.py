"""rsl_peak_emit on random mask words against numpy, after rsl_peak_offsets on the same words: the compact path
(k_emit_cells + k_emit_entries) and the general one (k_emit).  The integer lists follow from the masks alone and must
match exactly; power_db is checked against fp64 10 log10(p + 1e-12) of the peak powers the case lays out as the
kernels read them (compact path) or of |rds|^2 (general path).  Every case is the smallest shape that reaches its
branch, and asserts in numpy that it does."""
import functools

import numpy as np
import pytest

from test_gpu_offsets import popcount

pytestmark = pytest.mark.gpu

K_EMIT_CAP = 2048   # items of one round of an entry block (256 mask words)
K_CELL_CAP = 4096   # items of a cell block (64 union words)
PDB_TOL = 1e-4      # dB, the project's tolerance for a power in dB (cfar_cases.py)

# name: (F, A, S, C), density ('quarter': word & word, 'full': every bit below C), peak_pow_group (None: no peak
# powers, the general path reads an RDS), what the case reaches
CASES = {
    'aligned_rounds': ((2, 3, 32, 128), 'quarter', 1),   # S*W = 64, W = 2; an entry block of more than one round
    'full': ((2, 3, 32, 128), 'full', 1),                # 8 rounds in an entry block, a cell block at its capacity
    'unaligned_w2': ((2, 2, 40, 100), 'quarter', 1),     # S*W = 80: a second cell block of 16 words; C % 64 != 0
    'unaligned_w1': ((3, 2, 24, 64), 'quarter', 1),      # one partly filled cell block per frame; frames in one block
    'a12_packed': ((1, 12, 32, 64), 'quarter', 1),       # MAXA = 16: antenna masks packed with the item codes
    'a32_bit31': ((1, 32, 16, 64), 'quarter', 1),        # MAXA = 32: the separate antenna-mask array, antenna bit 31
    'group4': ((2, 2, 32, 64), 'quarter', 4),            # grouped peak powers
    'general_w3': ((2, 2, 20, 130), 'quarter', None),    # W = 3: the general path
    'general_w2': ((2, 2, 32, 128), 'quarter', None),    # the general path at a power-of-two W
}


def exclusive(x):
    return np.cumsum(x) - x


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs and numpy oracle of one case (host arrays, built once)."""
    (F, A, S, C), density, group = CASES[name]
    W = (C + 63) // 64
    rng = np.random.default_rng(sum(name.encode()))
    word = lambda: rng.integers(0, 1 << 64, size=(F, A, S, W), dtype=np.uint64)
    if density == 'full':
        mask = np.full((F, A, S, W), ~np.uint64(0))
    else:
        mask = word() & word()
        mask[:, :, ::7] = 0  # some empty rows
    for w in range(W):  # no bits at or above C
        n = min(64, C - 64 * w)
        mask[..., w] &= np.uint64((1 << n) - 1)
    rows = popcount(mask).sum(-1)  # [F, A, S]

    bits = np.unpackbits(mask.view(np.uint8).reshape(F, A, S, W * 8), axis=-1, bitorder='little')[..., :C].astype(bool)
    assert bits.sum() == rows.sum()
    f, a, i, j = np.nonzero(bits)  # (f, a, i, j) order
    union = bits.any(axis=1)       # [F, S, C]
    cf, ci, cj = np.nonzero(union)  # (f, i, j) order
    cell_id = (np.cumsum(union.ravel()) - 1).reshape(F, S, C)
    amask = (bits.astype(np.uint32) << np.arange(A, dtype=np.uint32)[None, :, None, None]).sum(1, dtype=np.uint32)
    want = dict(e_coord=(a.astype(np.uint32) << 26) | (i.astype(np.uint32) << 13) | j.astype(np.uint32),
                e_cell=cell_id[f, i, j].astype(np.int32), c_frame=cf.astype(np.int32),
                c_rc=(ci * C + cj).astype(np.int32), c_amask=amask[cf, ci, cj])
    ne, nc = len(f), len(cf)
    assert ne > 0 and nc > 0

    # peak powers as the kernels read them: the entry of row (f, a, i) with rank r lies at (row - i % g) * C + (peaks
    # of the earlier rows of its group) + r; every other slot is NaN
    peak_pow = rds = None
    if group is not None:
        assert S % group == 0
        p = rng.uniform(np.log(1e-3), np.log(1e3), ne)
        p = np.exp(p).astype(np.float32)
        row = (f * A + a) * S + i
        start = exclusive(rows.ravel())  # a row's first entry
        slot = (row - i % group) * C + np.arange(ne) - start[row - i % group]
        assert len(np.unique(slot)) == ne and slot.max() < F * A * S * C
        peak_pow = np.full(F * A * S * C, np.nan, dtype=np.float32)
        peak_pow[slot] = p
        rds = np.zeros((F, A, S, C), dtype=np.complex64)  # its shape only: the compact path does not read it
    else:
        rds = (rng.standard_normal((F, A, S, C)) + 1j * rng.standard_normal((F, A, S, C))).astype(np.complex64)
        p = np.abs(rds.astype(np.complex128)[f, a, i, j]) ** 2
    want['e_pdb'] = 10.0 * np.log10(p.astype(np.float64) + 1e-12)

    # what the case is there for
    words = popcount(mask).ravel()
    uwords = popcount(np.bitwise_or.reduce(mask, axis=1)).reshape(F, -1)  # [F, S * W]
    pow2 = W & (W - 1) == 0
    if name == 'aligned_rounds':
        assert S * W == 64 and W == 2 and words[:256].sum() > K_EMIT_CAP
    elif name == 'full':
        assert words[:256].sum() == 8 * K_EMIT_CAP and uwords[0, :64].sum() == K_CELL_CAP
    elif name == 'unaligned_w2':
        assert S * W == 64 + 16 and C % 64 != 0 and uwords[:, 64:].sum(1).min() > 0
    elif name == 'unaligned_w1':
        assert W == 1 and S * W < 64 and F * A * S * W <= 256 and F > 1
    elif name == 'a12_packed':
        assert 8 < A <= 16 and (want['c_amask'] >> 8).any()
    elif name == 'a32_bit31':
        assert A == 32 and (want['c_amask'] >> 31).any()
    elif name == 'group4':
        assert group == 4 and (slot != row * C + np.arange(ne) - start[row]).any()
    elif name == 'general_w3':
        assert W == 3 and not pow2 and group is None
    elif name == 'general_w2':
        assert pow2 and group is None
    if group is not None:
        assert pow2 and W <= 64  # the compact path
    return dict(shape=(F, A, S, C), mask=mask, rows=rows.astype(np.int32), peak_pow=peak_pow, group=group or 1,
                rds=rds, want=want, ne=ne, nc=nc)


def run_emit(ctx, c, entry_cap, cell_cap, bufs=None):
    F, A, S, C = c['shape']
    mask = ctx.to_dev(c['mask'].view(np.int64))
    offs = ctx.offsets(mask, ctx.to_dev(c['rows']), C)
    assert int(offs['entry_base'][F].item()) == c['ne'] and int(offs['cell_base'][F].item()) == c['nc']
    pk = None if c['peak_pow'] is None else ctx.to_dev(c['peak_pow'])
    lists = ctx.emit(ctx.to_dev(c['rds']), mask, offs, entry_cap, cell_cap, want_pdb=True, bufs=bufs, peak_pow=pk,
                     peak_pow_group=c['group'])
    ctx.torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in lists.items()}
    for k in ('e_coord', 'c_amask'):
        got[k] = got[k].view(np.uint32)
    return got


def check_lists(got, want, ne, nc):
    for k, n in (('e_coord', ne), ('e_cell', ne), ('c_frame', nc), ('c_rc', nc), ('c_amask', nc)):
        bad = np.nonzero(got[k][:n] != want[k][:n])[0]
        assert bad.size == 0, (k, int(bad.size), int(bad[0]), got[k][bad[0]], want[k][bad[0]])
    err = np.abs(got['e_pdb'][:ne].astype(np.float64) - want['e_pdb'][:ne])
    print(f'power_db: max |error| {err.max() if ne else 0.0:.3g} dB over {ne} entries')
    assert not (err > PDB_TOL).any() and not np.isnan(err).any(), ('e_pdb', float(np.nanmax(err)))


@pytest.mark.parametrize('name', list(CASES))
def test_emit_against_numpy(ctx, name):
    c = case(name)
    check_lists(run_emit(ctx, c, c['ne'], c['nc']), c['want'], c['ne'], c['nc'])


def test_emit_capacity_cut(ctx):
    """Lists cut at half the true counts: the prefix is the oracle's, and no slot past the capacity is written."""
    c = case('aligned_rounds')
    torch = ctx.torch
    ecap, ccap = c['ne'] // 2, c['nc'] // 2
    assert 0 < ecap < c['ne'] and 0 < ccap < c['nc']
    pad, sent = 1024, -7
    bufs = {k: torch.full((cap + pad,), sent, dtype=dt, device=ctx.device)
            for k, cap, dt in (('e_coord', ecap, torch.int32), ('e_cell', ecap, torch.int32),
                               ('e_pdb', ecap, torch.float32), ('c_frame', ccap, torch.int32),
                               ('c_rc', ccap, torch.int32), ('c_amask', ccap, torch.int32))}
    got = run_emit(ctx, c, ecap, ccap, bufs=bufs)
    check_lists(got, c['want'], ecap, ccap)
    for k, v in got.items():
        cap = ecap if k.startswith('e_') else ccap
        tail = v[cap:]
        assert tail.size == pad and (tail == np.asarray(sent).astype(tail.dtype)).all(), k
