"""Consensus velocity solve measurements at configs[2] (A8 C128 S512), F frames per launch, one GPU, one stream.

On the cfg2 chain's own lists (gidx, phase, c_amask, cell_base after one ch.run()), in one process:
k_velocity (rsl_velocity), k_velocity_robust with Tukey at a given scale (iters = 30, tol = 1e-9: 'tukey_fixed', the
dependable configuration of the robust solver) and k_velocity_consensus (rsl_velocity_consensus) at 64, 256 and 1024
hypotheses, refine = 3.  ms per launch from rsl_timing_* (RSL_K_VELOCITY) and from stream events, and the ratio to
k_velocity and to tukey_fixed in the same run.  The given scale is the median of rsl_velocity's per-frame rmse on
these lists (they hold no planted motion: the figure of interest here is the time, not the estimate).

The measurement runs in a child process under a time limit.  Writes profiles/vel_consensus_bench.json.
    python tools/vel_consensus_bench.py [--frames 2000] [--reps 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402
from bench_parts import A, C, S, TC  # noqa: E402

ITERS, TOL = 30, 1e-9
HYPS, REFINE, CUT = (64, 256, 1024), 3, 3.0


def measure(F, reps):
    import numpy as np
    import torch
    import rsl
    from bench import make_cubes
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC)
    ch = rsl.RadarChain(cfg, F, ctx)
    cube = make_cubes(ctx, 1, F, A, C, TC, 0)[0]
    ch.run(cube)
    torch.cuda.synchronize()
    ne, nc = ch.totals()
    common = dict(k=ch.k, ridge=cfg.ridge, bounds=cfg.bounds, amask=ch.lists['c_amask'], gidx=ch.gidx,
                  az_table=ch.az_table, n=ch.cell_cap)
    y, seg = ch.ext['phase'], ch.offs['cell_base']
    out = ctx.empty((F, 8), torch.float64)
    weight = ctx.empty((ch.cell_cap,), torch.float32)
    ls = ctx.velocity(None, y, seg, out=out, **common)[0].cpu().numpy()
    sigma = float(np.median(ls[:, 3]))
    runs = {'k_velocity': lambda: ctx.velocity(None, y, seg, out=out, **common),
            'tukey_fixed': lambda: ctx.velocity_robust(None, y, seg, loss='tukey', scale=sigma, iters=ITERS, tol=TOL,
                                                       out=out, want_weight=weight, **common)}
    for hyps in HYPS:
        runs[f'consensus_{hyps}'] = (lambda hyps=hyps: ctx.velocity_consensus(
            None, y, seg, scale=sigma, c=CUT, hyps=hyps, refine=REFINE, out=out, want_weight=weight, **common))
    res = {'frames': F, 'reps': reps, 'cells': nc, 'cells_per_frame': nc / F, 'iters': ITERS, 'tol': TOL,
           'refine': REFINE, 'c': CUT, 'given_scale': sigma, 'variants': {}}
    for name, fn in runs.items():
        r = B.timed(ctx, torch, fn, reps, 'velocity')
        o = out.cpu().numpy()
        if name == 'tukey_fixed':
            r.update(mean_iterations=float(np.abs(o[:, 7]).mean()),
                     mean_inlier_share=float((o[:, 4] / np.maximum(o[:, 5], 1)).mean()))
        elif name != 'k_velocity':
            r.update(mean_valid_share=float((o[:, 7] / int(name.split('_')[1])).mean()),
                     frames_without_winner=int((o[:, 6] < 0).sum()),
                     mean_inlier_share=float((o[:, 4] / np.maximum(o[:, 5], 1)).mean()),
                     residual_evaluations=int(nc) * (int(name.split('_')[1]) + REFINE + 1))
        res['variants'][name] = r
    base = res['variants']['k_velocity']['ms_rsl_timing']
    tukey = res['variants']['tukey_fixed']['ms_rsl_timing']
    for name, r in res['variants'].items():
        r['ratio_to_k_velocity'] = r['ms_rsl_timing'] / base
        r['ratio_to_tukey_fixed'] = r['ms_rsl_timing'] / tukey
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    B.add_arguments(ap, 'vel_consensus_bench.json', limit=300)
    args = ap.parse_args()
    if args.part:
        B.emit_result(measure(args.frames, args.reps))
        return 0
    rc, res = B.run_parts(__file__, ['measure'], ['--frames', args.frames, '--reps', args.reps], args.limit)
    if rc:
        return rc
    B.write_json(args.out, {
        'what': 'consensus velocity solve at configs[2] (A8 C128 S512) on the chain\'s own lists, one GPU, one stream '
                '(tools/vel_consensus_bench.py)', **res['measure']})
    return 0


if __name__ == '__main__':
    sys.exit(main())
