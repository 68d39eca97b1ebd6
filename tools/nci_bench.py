"""Non-coherent integration measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream:

* standalone, on the RDS of one batch: k_power_integrate alone (ms per launch from rsl_timing_* and from stream
  events, and its HBM rate over its algorithmic bytes (8 A + 4) S C per frame); rsl_detect_power for each rule on the
  summed map next to the per-antenna rsl_detect / rsl_detect_cfar / rsl_detect_oscfar on the same RDS, each CFAR rule
  at the same design Pfa (the summed map's factor designed for A looks), with the entries and union cells per frame
  of both;
* whole step: ms per ch.run() and frames/s with detect_on='antenna' and detect_on='sum' for each detector, with the
  entry and cell totals and the per-kernel times of rsl_timing_read.

Each measurement runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/nci_bench.json.   python tools/nci_bench.py [--frames 2000] [--reps 5] [--pfa 1e-4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402
from bench_parts import A, C, S, TC  # noqa: E402

DETECTORS = {'threshold': dict(detector='threshold'), 'ca': dict(detector='cfar', cfar_method='ca'),
             'os': dict(detector='cfar', cfar_method='os')}


def part_standalone(F, reps, pfa):
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
    guard, train, rank = cfg.cfar_guard, cfg.cfar_train, cfg.cfar_rank
    W = (C + 63) // 64
    power = ctx.empty((F, S, C), torch.float32)
    per = dict(mask=ch.mask, row_count=ch.row_count, peak_pow=ch.peak_pow)
    one = dict(mask=ctx.empty((F, 1, S, W), torch.int64), row_count=ctx.empty((F, 1, S), torch.int32),
               peak_pow=ctx.empty((F, 1, S, C), torch.float32))
    res = {'frames': F, 'reps': reps, 'pfa': pfa, 'window': {'guard': guard, 'train': train}, 'rank': rank,
           'integrate_bytes': F * (8 * A + 4) * S * C}
    r = B.timed(ctx, torch, lambda: ctx.integrate_power(ch.rds, out=power), reps, 'detect')
    res['k_power_integrate'] = {**r, 'tb_per_s': res['integrate_bytes'] / (r['ms_rsl_timing'] * 1e-3) / 1e12}

    def counts(out):
        offs = ctx.offsets(out['mask'], out['row_count'], C)
        return {'entries_per_frame': int(offs['entry_base'][F].item()) / F,
                'cells_per_frame': int(offs['cell_base'][F].item()) / F}
    for rule in ('threshold', 'ca', 'os'):
        a1 = aA = 1.0
        if rule != 'threshold':
            a1 = tables.cfar_design_alpha(rule, pfa, guard, train, rank)
            aA = tables.cfar_design_alpha(rule, pfa, guard, train, rank, looks=A)
        if rule == 'threshold':
            old = lambda: ctx.detect(ch.rds, ch.thr_p, ch.i_lo, ch.i_hi, out=per)
        else:
            old = lambda: ctx.detect_cfar(ch.rds, guard, train, a1, ch.thr_p, ch.i_lo, ch.i_hi, out=per, method=rule,
                                          rank=rank)
        new = lambda: ctx.detect_power(power, rule, guard, train, rank, aA, ch.thr_p, ch.i_lo, ch.i_hi, out=one)
        ra = {**B.timed(ctx, torch, old, reps, 'detect'), 'alpha': a1, **counts(per)}
        rs = {**B.timed(ctx, torch, new, reps, 'detect'), 'alpha': aA, **counts(one)}
        res[rule] = {'per_antenna': ra, 'summed': rs,
                     'ratio_summed_over_per_antenna': rs['ms_rsl_timing'] / ra['ms_rsl_timing'],
                     'ratio_integrate_plus_summed_over_per_antenna':
                         (res['k_power_integrate']['ms_rsl_timing'] + rs['ms_rsl_timing']) / ra['ms_rsl_timing']}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--pfa', type=float, default=1e-4)
    B.add_arguments(ap, 'nci_bench.json')
    args = ap.parse_args()
    if args.part:
        kind, _, rest = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(args.frames, args.reps, args.pfa)
        else:
            on, _, det = rest.partition(':')
            res = B.chain_step(args.frames, args.reps,
                               lambda ch: {'detect_on': on, 'detector': det, 'alpha': ch.cfar_alpha,
                                           'pfa': args.pfa if det != 'threshold' else None},
                               detect_on=on, cfar_pfa=args.pfa, **DETECTORS[det])
        B.emit_result(res)
        return 0
    parts = ['standalone'] + [f'step:{on}:{det}' for det in DETECTORS for on in ('antenna', 'sum')]
    rc, res = B.run_parts(__file__, parts, ['--frames', args.frames, '--reps', args.reps, '--pfa', args.pfa],
                          args.limit)
    if rc:
        return rc
    B.write_json(args.out, {
        'what': 'detection on the antenna-summed power map at configs[2] (A8 C128 S512), one GPU, one stream '
                '(tools/nci_bench.py)',
        'steps': [res[p] for p in parts[1:]], 'standalone': res['standalone']})
    return 0


if __name__ == '__main__':
    sys.exit(main())
