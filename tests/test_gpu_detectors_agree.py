"""The three detectors make the same decisions on the same RDS: the detection fused into the Doppler FFT
(rsl_rds_detect: general tile body, register body, the three packed kernels, and the unfused fall-back inside the
library), the standalone threshold detector (rsl_detect) and the CA-CFAR detector (rsl_detect_cfar) with its level
switched off.

Switching the CFAR level off: with guard (0, 0), train (1, 1) and alpha = 1e-20 the CFAR condition p n > alpha sum
holds for every cell the power floor thr_power > 0 lets through (sum <= 8 max p, and 1e-20 * 8 max p is far below
thr_power n), so the rule reduces to k_detect's: 3x3 'reflect' local maximum, range gate, p > thr_power.
test_cfar_rule_reduces_to_threshold_rule confirms that reduction on the CPU, cfar_ref.reference against the plain
rule on a random map.

The cube is complex noise of variance 0.02 per sample and the window table is random and complex (rds_ref.make_table:
an all-ones table hides a wrong table index), so the mean RDS power is S * C * 0.02 * mean |table|^2; with that as the
threshold nearly every 3x3 local maximum passes (the largest of nine exponential powers exceeds their mean 98 % of the
time), so roughly 11 % of the cells are peaks, edge rows and tile borders included.  The RDS the detectors agree on is
itself compared with the fp64 numpy reference (rds_ref.reference, parity.RDS_ATOL_REL).
"""
import numpy as np
import pytest

import cfar_ref as R
import parity as P
import rds_ref
from rds_ref import LISTS, lists_of

SHAPES = [  # (F, A, C, S): each the smallest that reaches its body
    (2, 2, 32, 128),    # fused, general tile body
    (2, 2, 64, 64),     # fused, register body on padded rows
    (2, 2, 64, 256),    # packed _r64
    (2, 2, 128, 512),   # packed _r128
    (1, 2, 256, 1024),  # packed _r256
    (2, 2, 48, 96),     # unfused: rsl_rds + rsl_detect inside the library
]
SEED = 20
CFAR_OFF = dict(guard=(0, 0), train=(1, 1), alpha=1e-20)


def test_cfar_rule_reduces_to_threshold_rule():
    rng = np.random.default_rng(3)
    S, C = 40, 24
    z = (rng.standard_normal((2, S, C)) + 1j * rng.standard_normal((2, S, C))).astype(np.complex64)
    p = R.power(z)
    thr = float(p.mean())
    for gate in ((0, S - 1), (3, S - 5)):
        g = np.zeros(S, bool)
        g[gate[0]:gate[1] + 1] = True
        plain = (p > thr) & (p >= R.neighbour_max(p)) & g[:, None]
        ref = R.reference(z, CFAR_OFF['guard'] + CFAR_OFF['train'], CFAR_OFF['alpha'], thr_power=thr, gate=gate)
        assert plain.any() and (ref['mask'] == plain).all()
        assert plain[:, gate[0]].any() or plain[:, gate[1]].any()


def make_cube(ctx, F, A, C, S):
    torch = ctx.torch
    g = torch.Generator().manual_seed(SEED)
    re = torch.randn((F, A, C, S), generator=g) * 0.1
    im = torch.randn((F, A, C, S), generator=g) * 0.1
    return torch.complex(re, im).to(ctx.device)


@pytest.mark.gpu
@pytest.mark.parametrize('C', [910, 911, 1639, 2731, 4096])
def test_detect_wide_maps(ctx, C):
    """rsl_detect at every rows-per-workgroup value of k_detect (16 up to C = 910, then 8, 4 and 2 up to C = 4096, the
    last with exactly 64 KiB of LDS), against the plain rule in numpy.  The map is real, so its fp32 power x * x is the
    same number in numpy as in the kernel and the comparison is exact; S = 19 leaves a partial last tile at each value."""
    torch = ctx.torch
    F, A, S = 1, 2, 19
    rng = np.random.default_rng([SEED, C])
    x = rng.standard_normal((F, A, S, C), dtype=np.float32)
    p = x * x
    thr = float(np.median(p))
    rds = ctx.to_dev(x.astype(np.complex64))
    nb = R.neighbour_max(p.astype(np.float64))
    for i_lo, i_hi in ((0, S - 1), (2, S - 3)):
        g = np.zeros(S, bool)
        g[i_lo:i_hi + 1] = True
        want = (p.astype(np.float64) > thr) & (p >= nb) & g[:, None]
        out = dict(peak_pow=torch.full((F, A, S, C), float('nan'), dtype=torch.float32, device=ctx.device))
        mask, rc, _ = ctx.detect(rds, thr, i_lo, i_hi, out=out)
        torch.cuda.synchronize()
        got = R.mask_bool(mask.cpu().numpy(), C)
        assert want.any() and (got == want).all(), int((got ^ want).sum())
        assert (rc.cpu().numpy() == want.sum(axis=-1)).all()
        pk = out['peak_pow'].cpu().numpy()
        for a in range(A):
            for i in range(S):
                n = int(want[0, a, i].sum())
                assert (pk[0, a, i, :n] == p[0, a, i][want[0, a, i]]).all() and np.isnan(pk[0, a, i, n:]).all()
    with pytest.raises(ValueError, match='C too large'):
        ctx.detect(ctx.empty((1, 1, 2, 4097), torch.complex64), thr, 0, 1)


@pytest.mark.gpu
@pytest.mark.parametrize('gate', ['full', 'inner'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'F%d_A%d_C%d_S%d' % s)
def test_detectors_agree(ctx, shape, gate):
    torch = ctx.torch
    F, A, C, S = shape
    i_lo, i_hi = (0, S - 1) if gate == 'full' else (3, S - 5)
    W = (C + 63) // 64
    tab = rds_ref.make_table(S, SEED)
    thr = rds_ref.mean_power(tab, S, C)
    cube = make_cube(ctx, F, A, C, S)
    table = ctx.to_dev(tab)

    def buffers():
        return dict(mask=ctx.empty((F, A, S, W), torch.int64), row_count=ctx.empty((F, A, S), torch.int32),
                    peak_pow=torch.full((F, A, S, C), float('nan'), dtype=torch.float32, device=ctx.device))

    rds = ctx.empty((F, A, S, C), torch.complex64)
    fused = buffers()
    fused['db'] = ctx.empty((F, A, S, C), torch.float32)
    fused['group'] = ctx.rds_detect(cube, table, thr, i_lo, i_hi, rds=rds, work=ctx.empty((F, A, C, S), torch.complex64),
                                    mask=fused['mask'], row_count=fused['row_count'], peak_pow=fused['peak_pow'],
                                    db_map=fused['db'], dc_removal=True)
    plain = buffers()
    _, _, plain['db'] = ctx.detect(rds, thr, i_lo, i_hi, want_db=True, out=plain)
    plain['group'] = 1
    cfar = buffers()
    _, _, cfar['db'] = ctx.detect_cfar(rds, CFAR_OFF['guard'], CFAR_OFF['train'], CFAR_OFF['alpha'], thr, i_lo, i_hi,
                                       want_db=True, out=cfar)
    cfar['group'] = 1
    torch.cuda.synchronize()

    host = lambda t: t.cpu().numpy()
    err = P.rds_error(host(rds), rds_ref.reference(host(cube), tab, 0, C, True))
    print(f'\n{shape}: rds error {err:.3e}')
    assert err <= P.RDS_ATOL_REL, err
    m0, r0, d0 = host(fused['mask']), host(fused['row_count']), host(fused['db'])
    frac = r0.sum() / (F * A * (i_hi - i_lo + 1) * C)
    print(f'\n{shape} gate {(i_lo, i_hi)}: group {fused["group"]}, peaks {int(r0.sum())} ({100 * frac:.2f} % of the gated '
          f'cells), rows 0 / S-1: {int(r0[:, :, 0].sum())} / {int(r0[:, :, S - 1].sum())}')
    assert r0.sum() > 0
    if gate == 'full':  # the 'reflect' edge rows decide something
        assert r0[:, :, 0].sum() + r0[:, :, S - 1].sum() > 0
    else:
        assert not r0[:, :, :i_lo].any() and not r0[:, :, i_hi + 1:].any()
    for name, det in (('detect', plain), ('detect_cfar', cfar)):
        assert host(det['mask']).tobytes() == m0.tobytes(), (name, 'mask')
        assert host(det['row_count']).tobytes() == r0.tobytes(), (name, 'row_count')
        assert host(det['db']).tobytes() == d0.tobytes(), (name, 'db_map')
    ne0, nc0, l0 = lists_of(ctx, rds, fused, C)
    assert ne0 == int(r0.sum()) and 0 < nc0 <= ne0
    for name, det in (('detect', plain), ('detect_cfar', cfar)):
        ne, nc, l = lists_of(ctx, rds, det, C)
        assert (ne, nc) == (ne0, nc0), name
        for k in LISTS:
            assert l[k] == l0[k], (name, k)
