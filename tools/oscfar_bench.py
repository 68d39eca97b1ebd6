"""OS-CFAR detector measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream:

* standalone: k_detect_oscfar (default window, rank 0.75) next to k_detect_cfar and k_detect on the same RDS buffer:
  ms per launch from rsl_timing_* and from stream events, the peaks each finds, the ratios, and the ratio of
  k_detect_oscfar to the LDS-read model of DESIGN §3 (one 4-B LDS read per candidate and training cell at
  128 B/clk/CU);
* whole step: ms per ch.run() with detector='cfar' and cfar_method 'ca' and 'os' at Pfa 1e-2 and 1e-4, with the entry
  and cell totals and the per-kernel times of rsl_timing_read.

Each measurement runs in a child process of its own under its own time limit; the first failure ends the run
(tools/bench_parts.py).
Writes profiles/oscfar_bench.json.   python tools/oscfar_bench.py [--frames 2000] [--reps 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402
from bench_parts import A, C, S, TC  # noqa: E402

RANK = 0.75
MODEL_MS_AT_2000 = 2.5  # 1.2e8 candidates x 416 cells x 4 B over 256 CUs x 128 B/clk at 2.4 GHz


def part_standalone(F, reps):
    import torch
    import rsl
    from bench import make_cubes
    from rsl import tables
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC)
    ch = rsl.RadarChain(cfg, F, ctx)
    cube = make_cubes(ctx, 1, F, A, C, TC, 0)[0]
    ch.run_front(cube)  # fills ch.rds
    torch.cuda.synchronize()
    n = tables.cfar_training_cells(cfg.cfar_guard, cfg.cfar_train)
    a_ca = tables.cfar_design_alpha('ca', cfg.cfar_pfa, cfg.cfar_guard, cfg.cfar_train)
    a_os = tables.cfar_design_alpha('os', cfg.cfar_pfa, cfg.cfar_guard, cfg.cfar_train, RANK)
    out = dict(mask=ch.mask, row_count=ch.row_count, peak_pow=ch.peak_pow)
    runs = {
        'k_detect': lambda: ctx.detect(ch.rds, ch.thr_p, ch.i_lo, ch.i_hi, out=out),
        'k_detect_cfar': lambda: ctx.detect_cfar(ch.rds, cfg.cfar_guard, cfg.cfar_train, a_ca, ch.thr_p, ch.i_lo,
                                                 ch.i_hi, out=out),
        'k_detect_oscfar': lambda: ctx.detect_oscfar(ch.rds, cfg.cfar_guard, cfg.cfar_train, RANK, a_os, ch.thr_p,
                                                     ch.i_lo, ch.i_hi, out=out),
    }
    res = {'frames': F, 'reps': reps, 'window': {'guard': cfg.cfar_guard, 'train': cfg.cfar_train}, 'rank': RANK,
           'pfa': cfg.cfar_pfa, 'training_cells': n, 'cells': F * A * S * C}
    for name, fn in runs.items():
        res[name] = {**B.timed(ctx, torch, fn, reps, 'detect'), 'peaks': int(ch.row_count.sum().item())}
    # the candidates of the count: the 3x3 maxima inside the gate and above the floor = what k_detect marks
    res['candidates'] = res['k_detect']['peaks']
    t = {k: res[k]['ms_rsl_timing'] for k in runs}
    res['ratio_oscfar_over_cfar'] = t['k_detect_oscfar'] / t['k_detect_cfar']
    res['ratio_oscfar_over_detect'] = t['k_detect_oscfar'] / t['k_detect']
    res['model_ms'] = MODEL_MS_AT_2000 * F / 2000
    res['ratio_oscfar_over_model'] = t['k_detect_oscfar'] / res['model_ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    B.add_arguments(ap, 'oscfar_bench.json')
    args = ap.parse_args()
    if args.part:
        kind, _, rest = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(args.frames, args.reps)
        else:
            method, _, pfa = rest.partition(':')
            res = B.chain_step(args.frames, args.reps,
                               lambda ch: {'cfar_method': method, 'pfa': float(pfa), 'alpha': ch.cfar_alpha},
                               detector='cfar', cfar_method=method, cfar_rank=RANK, cfar_pfa=float(pfa))
        B.emit_result(res)
        return 0
    parts = ['standalone', 'step:ca:1e-2', 'step:os:1e-2', 'step:ca:1e-4', 'step:os:1e-4']
    rc, res = B.run_parts(__file__, parts, ['--frames', args.frames, '--reps', args.reps], args.limit)
    if rc:
        return rc
    B.write_json(args.out, {
        'what': 'OS-CFAR detector at configs[2] (A8 C128 S512), one GPU, one stream (tools/oscfar_bench.py)',
        'steps': [res[p] for p in parts[1:]], 'standalone': res['standalone']})
    return 0


if __name__ == '__main__':
    sys.exit(main())
