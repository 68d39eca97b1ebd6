"""CA-CFAR detector measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream:

* standalone: k_detect_cfar (default window) next to k_detect on the same RDS buffer (both read 8 B per cell):
  ms per launch from rsl_timing_* and from stream events, the ratio and the achieved TB/s of the 8 B/cell read;
* whole step: ms per ch.run() with detector='threshold' and detector='cfar' at Pfa 1e-2 and 1e-4, with the entry and
  cell totals and the per-kernel times of rsl_timing_read (K5 = doa_scan, emit, velocity, detect, ...).

Each measurement runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/cfar_bench.json.   python tools/cfar_bench.py [--frames 2000] [--reps 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402
from bench_parts import A, C, S, TC  # noqa: E402


def part_standalone(F, reps):
    import torch
    import rsl
    from bench import make_cubes
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC)
    ch = rsl.RadarChain(cfg, F, ctx)
    cube = make_cubes(ctx, 1, F, A, C, TC, 0)[0]
    ch.run_front(cube)  # fills ch.rds
    torch.cuda.synchronize()
    from rsl import tables
    alpha = tables.cfar_design_alpha('ca', cfg.cfar_pfa, cfg.cfar_guard, cfg.cfar_train)
    out = dict(mask=ch.mask, row_count=ch.row_count, peak_pow=ch.peak_pow)
    runs = {
        'k_detect': lambda: ctx.detect(ch.rds, ch.thr_p, ch.i_lo, ch.i_hi, out=out),
        'k_detect_cfar': lambda: ctx.detect_cfar(ch.rds, cfg.cfar_guard, cfg.cfar_train, alpha, ch.thr_p, ch.i_lo,
                                                 ch.i_hi, out=out),
    }
    res = {'frames': F, 'reps': reps, 'window': {'guard': cfg.cfar_guard, 'train': cfg.cfar_train},
           'bytes_read_floor': F * A * S * C * 8}
    for name, fn in runs.items():
        r = B.timed(ctx, torch, fn, reps, 'detect')
        res[name] = {**r, 'peaks': int(ch.row_count.sum().item()),
                     'tb_per_s': F * A * S * C * 8 / (r['ms_rsl_timing'] * 1e-3) / 1e12}
    res['ratio_cfar_over_detect'] = res['k_detect_cfar']['ms_rsl_timing'] / res['k_detect']['ms_rsl_timing']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    B.add_arguments(ap, 'cfar_bench.json')
    args = ap.parse_args()
    if args.part:
        kind, _, rest = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(args.frames, args.reps)
        else:
            det, _, pfa = rest.partition(':')
            pfa = float(pfa or 1e-4)
            res = B.chain_step(args.frames, args.reps,
                               lambda ch: {'detector': det, 'pfa': pfa if det == 'cfar' else None},
                               detector=det, cfar_pfa=pfa)
        B.emit_result(res)
        return 0
    parts = ['standalone', 'step:threshold', 'step:cfar:1e-2', 'step:cfar:1e-4']
    rc, res = B.run_parts(__file__, parts, ['--frames', args.frames, '--reps', args.reps], args.limit)
    if rc:
        return rc
    B.write_json(args.out, {
        'what': 'CA-CFAR detector at configs[2] (A8 C128 S512), one GPU, one stream (tools/cfar_bench.py)',
        'steps': [res[p] for p in parts[1:]], 'standalone': res['standalone']})
    return 0


if __name__ == '__main__':
    sys.exit(main())
