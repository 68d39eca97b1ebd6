"""Spatially smoothed MUSIC (rsl_doa_smoothed / k_doa_smoothed) measurements, one GPU, one stream:

cells/s at (M, L) = (8, 6) and (16, 8) on 35 000 cells per frame x 64 frames (range-major cell lists over a
Gaussian-noise RDS c64 [64, M, 512, 128], G = 361, nmax = 3), with the order estimated (rel 0.05) and fixed at 2, and
beside it the existing one-angle Toeplitz scan (rsl_doa, MUSIC argmax) on the same cells in the same process.  ms per
launch from rsl_timing_* (RSL_K_DOA_SCAN) and from stream events.

Each (M, L) runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/ssmusic_bench.json.   python tools/ssmusic_bench.py [--frames 64] [--cells 35000] [--reps 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402

S, C, G = 512, 128, 361


def part(M, L, F, per_frame, reps):
    import numpy as np
    import torch
    import rsl
    from rsl import _lib, tables
    ctx = rsl.get_context(0)
    gen = torch.Generator(device=ctx.device)
    gen.manual_seed(1)
    rds = torch.view_as_complex(torch.randn((F, M, S, C, 2), generator=gen, device=ctx.device, dtype=torch.float32))
    rng = np.random.default_rng(2)
    rc = np.concatenate([np.sort(rng.choice(S * C, per_frame, replace=False)) for _ in range(F)]).astype(np.int32)
    fr = np.repeat(np.arange(F, dtype=np.int32), per_frame)
    N = int(rc.size)
    d_fr, d_rc = ctx.to_dev(fr), ctx.to_dev(rc)
    lam = 3e8 / 77e9
    st = tables.steering_matrix(np.linspace(-90.0, 90.0, G), np.arange(M) * lam / 2, lam)
    steer, sub = ctx.steering(st), ctx.steering_sub(st, L)
    out = dict(nsrc=ctx.empty((N,), torch.int32), idx=ctx.empty((N, 3), torch.int32),
               den=ctx.empty((N, 3), torch.float32))
    gidx = ctx.empty((N,), torch.int32)
    runs = {
        'doa_smoothed_estimate': lambda: ctx.doa_smoothed(rds, d_fr, d_rc, sub, n=N, nmax=3, num_sources=0, out=out),
        'doa_smoothed_fixed2': lambda: ctx.doa_smoothed(rds, d_fr, d_rc, sub, n=N, nmax=3, num_sources=2, out=out),
        'doa_toeplitz_scan': lambda: ctx.doa(rds, d_fr, d_rc, steer, _lib.METHOD_MUSIC, n=N, out_idx=gidx),
    }
    res = {'M': M, 'L': L, 'G': G, 'frames': F, 'cells_per_frame': per_frame, 'cells': N, 'reps': reps,
           'toeplitz_path': bool(steer['toeplitz'])}
    for name, fn in runs.items():
        r = B.timed(ctx, torch, fn, reps, 'doa_scan')
        r['cells_per_s'] = N / (r['ms_rsl_timing'] * 1e-3)
        res[name] = r
    runs['doa_smoothed_estimate']()  # the order the estimate mode chose on these cells
    torch.cuda.synchronize()
    res['mean_nsrc_estimate'] = float(out['nsrc'].float().mean().item())
    res['ratio_smoothed_over_scan'] = res['doa_smoothed_estimate']['ms_rsl_timing'] / \
        res['doa_toeplitz_scan']['ms_rsl_timing']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--cells', type=int, default=35000, help='cells per frame')
    B.add_arguments(ap, 'ssmusic_bench.json')
    args = ap.parse_args()
    if args.part:
        M, L = (int(v) for v in args.part.split(':'))
        B.emit_result(part(M, L, args.frames, args.cells, args.reps))
        return 0
    parts = ('8:6', '16:8')
    rc, res = B.run_parts(__file__, parts, ['--frames', args.frames, '--cells', args.cells, '--reps', args.reps],
                          args.limit)
    if rc:
        return rc
    B.write_json(args.out, {
        'what': 'spatially smoothed MUSIC (rsl_doa_smoothed) next to the Toeplitz one-angle scan (rsl_doa) on the '
                'same cells, one GPU, one stream (tools/ssmusic_bench.py)', 'runs': [res[p] for p in parts]})
    return 0


if __name__ == '__main__':
    sys.exit(main())
