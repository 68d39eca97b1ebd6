"""GPU: every FFT size, a chirp subset and the tile edges of the range-Doppler front end (rsl_fft.hip,
rsl_doppler_detect.hip) against a plain fp64 numpy FFT, through ctx.rds / ctx.rds_detect only.

Each of the 17 planned lengths (rds_ref.PLANNED) instantiates its own Stockham plan, tile height and kernel on either
axis, every other length takes the direct DFT, and the fused Doppler + detection kernel has a general and a register
tile body and three packed forms.  One case per instance; each case makes the same checks (common_checks), with DC
removal on and off:
  * rds against the reference within parity.RDS_ATOL_REL (1e-5 of max |ref|), the fallback lengths included: a CPU
    emulation of the fallback's sequential fp32 sum gave 1.1e-6 at N = 4093, 6.9e-7 at 997 and 1.1e-7 at 59 (measured
    on the device: 1.6e-6 at S = 4093, 2.6e-6 at C = 4093, at most 3.7e-7 at every planned length);
  * rds (and rsl_rds's c64 work) pre-filled with NaN hold none afterwards, and the 4096 sentinel elements before and
    after each buffer are bit-unchanged;
  * a chirp subset (C_total = C + 5, chirp0 = 2) gives the bits of the contiguous copy of those chirps at chirp0 = 0;
  * frame 0 / antenna 0 run alone gives the bits of its slice of the batch (for the persistent K1 kernels: the static
    tile walk against the per-XCD dequeue).
The table is random and complex, so a wrong table index shows.  Every measured error is printed (pytest -s).

S = 4096 and C = 4096 ask for 73 728 B and 69 640 B of dynamic LDS; both launch as written.  The largest measured
error of each kernel family is in DESIGN.md section 4."""
import numpy as np
import pytest

import cfar_ref
import parity as P
import rds_ref as R

pytestmark = pytest.mark.gpu

SEED = 41
FALLBACK_RANGE = (7, 96, 4093)
FALLBACK_DOPPLER = (7, 59, 4093)
FUSED_SHAPES = [  # (C, S)
    (8, 128), (16, 128), (512, 16), (1024, 8),  # general tile body
    (128, 64), (256, 32),                       # register body, two and four column chunks
    (64, 256), (128, 512), (256, 1024),         # packed
    (100, 50), (2048, 8),                       # unfused inside the library
]


def common_checks(ctx, run, cube, table, C, dc, label, work_c64):
    """run(cube on the device, chirp0) -> dict with the Guarded buffers 'rds' and 'work'; cube is [F, A, C + 5, S].
    Returns (the subset run, its rds on the host, the fp64 reference)."""
    ref = R.reference(cube, table, 2, C, dc)
    sub = run(ctx.to_dev(cube), 2)
    got = sub['rds'].host()
    err = P.rds_error(got, ref)
    print(f'\n{label} dc={int(dc)}: rds error {err:.3e}')
    assert not np.isnan(got).any(), 'rds holds NaN'
    if work_c64:
        assert not np.isnan(sub['work'].host()).any(), 'work holds NaN'
    assert sub['rds'].intact(), 'write outside rds'
    assert sub['work'].intact(), 'write outside work'
    assert err <= P.RDS_ATOL_REL, err
    copy = run(ctx.to_dev(cube[:, :, 2:2 + C]), 0)
    assert copy['rds'].host().tobytes() == got.tobytes(), 'chirp subset differs from its contiguous copy'
    one = run(ctx.to_dev(cube[:1, :1]), 2)
    assert one['rds'].host()[0, 0].tobytes() == got[0, 0].tobytes(), 'frame 0 / antenna 0 alone differs from the batch'
    return sub, got, ref


def rds_case(ctx, F, A, C, S, label):
    table = R.make_table(S, SEED)
    table_d = ctx.to_dev(table)
    cube = R.make_cube(F, A, C + 5, S, SEED)
    for dc in (True, False):
        def run(cube_d, chirp0):
            f, a = cube_d.shape[:2]
            out = dict(rds=R.Guarded(ctx, (f, a, S, C)), work=R.Guarded(ctx, (f, a, C, S)))
            ctx.rds(cube_d, table_d, chirp0=chirp0, num_chirps=C, dc_removal=dc, out=out['rds'].t, work=out['work'].t)
            ctx.torch.cuda.synchronize()
            return out
        common_checks(ctx, run, cube, table, C, dc, label, True)


@pytest.mark.parametrize('S', R.PLANNED + FALLBACK_RANGE)
def test_range_axis(ctx, S):
    """Every K1 instance (k_range_fft, the persistent k_range_fft_p with each window-table form, the direct DFT): a full
    tile and a partial one per (frame, antenna), at least 12 tiles."""
    assert (S in R.PLANNED) == (ctx.lib.rsl_fft_supported(S) == 1)
    C = min(R.rows_for(S), 64) + 3
    rds_case(ctx, 2, 3, C, S, f'range S={S} C={C}')


@pytest.mark.parametrize('C', R.PLANNED + FALLBACK_DOPPLER)
def test_doppler_axis(ctx, C):
    """Every k_doppler_fft instance and the direct DFT: a partial last tile of range bins and an odd S for the range
    fftshift (S itself through the range fallback)."""
    assert (C in R.PLANNED) == (ctx.lib.rsl_fft_supported(C) == 1)
    S = R.rows_for(C) + 3
    rds_case(ctx, 1, 2, C, S, f'doppler C={C} S={S}')


@pytest.mark.parametrize('shape', FUSED_SHAPES, ids=lambda s: 'C%d_S%d' % s)
def test_fused_axis(ctx, shape):
    """rsl_rds_detect at every fused tile body: the common checks on its rds, its detection outputs byte-equal to
    rsl_detect on that same rds, and its peaks against the fp64 reference's."""
    torch = ctx.torch
    C, S = shape
    F, A, W = 2, 2, (C + 63) // 64
    table = R.make_table(S, SEED)
    table_d = ctx.to_dev(table)
    cube = R.make_cube(F, A, C + 5, S, SEED)
    thr = R.mean_power(table, S, C)
    i_lo, i_hi = 0, S - 1

    def buffers(f, a):
        return dict(mask=ctx.empty((f, a, S, W), torch.int64), row_count=ctx.empty((f, a, S), torch.int32),
                    peak_pow=torch.full((f, a, S, C), float('nan'), dtype=torch.float32, device=ctx.device))

    for dc in (True, False):
        def run(cube_d, chirp0):
            f, a = cube_d.shape[:2]
            out = buffers(f, a)
            out.update(rds=R.Guarded(ctx, (f, a, S, C)), work=R.Guarded(ctx, (f, a, C, S)),
                       db=ctx.empty((f, a, S, C), torch.float32))
            out['group'] = ctx.rds_detect(cube_d, table_d, thr, i_lo, i_hi, rds=out['rds'].t, work=out['work'].t,
                                          mask=out['mask'], row_count=out['row_count'], peak_pow=out['peak_pow'],
                                          db_map=out['db'], chirp0=chirp0, num_chirps=C, dc_removal=dc)
            torch.cuda.synchronize()
            return out
        fused, got, ref = common_checks(ctx, run, cube, table, C, dc, f'fused C={C} S={S}', False)
        rds = fused['rds'].t
        plain = buffers(F, A)
        _, _, plain['db'] = ctx.detect(rds, thr, i_lo, i_hi, want_db=True, out=plain)
        plain['group'] = 1
        torch.cuda.synchronize()
        host = lambda t: t.cpu().numpy()
        m0, r0 = host(fused['mask']), host(fused['row_count'])
        assert r0.sum() > 0
        assert host(plain['mask']).tobytes() == m0.tobytes(), 'mask'
        assert host(plain['row_count']).tobytes() == r0.tobytes(), 'row_count'
        assert host(plain['db']).tobytes() == host(fused['db']).tobytes(), 'db_map'
        ne0, nc0, l0 = R.lists_of(ctx, rds, fused, C)
        ne, nc, l1 = R.lists_of(ctx, rds, plain, C)
        assert ne0 == int(r0.sum()) and (ne, nc) == (ne0, nc0)
        for k in R.LISTS:  # peak_pow (tile- or row-compact) through e_pdb
            assert l1[k] == l0[k], k
        gm = cfar_ref.mask_bool(m0, C)
        thr_db = 10 * np.log10(thr + 1e-12)
        for f in range(F):
            ng, nr, nd, nu = P.peak_diff(gm[f], ref[f], threshold_db=thr_db, gate=(i_lo, i_hi))
            print(f'  frame {f}: group {fused["group"]}, peaks {ng} (reference {nr}), differing {nd}, unexplained {nu}')
            assert nr > 0 and nu == 0, (f, ng, nr, nd, nu)
