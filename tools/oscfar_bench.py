"""OS-CFAR detector measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream:

* standalone: k_detect_oscfar (default window, rank 0.75) next to k_detect_cfar and k_detect on the same RDS buffer:
  ms per launch from rsl_timing_* and from stream events, the peaks each finds, the ratios, and the ratio of
  k_detect_oscfar to the LDS-read model of DESIGN §3 (one 4-B LDS read per candidate and training cell at
  128 B/clk/CU);
* whole step: ms per ch.run() with detector='cfar' and cfar_method 'ca' and 'os' at Pfa 1e-2 and 1e-4, with the entry
  and cell totals and the per-kernel times of rsl_timing_read.

Each measurement runs in a child process of its own under its own time limit; the first failure ends the run (the
child processes and the event timer are those of tools/cfar_bench.py).
Writes profiles/oscfar_bench.json.   python tools/oscfar_bench.py [--frames 2000] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'radar-slam_amd'), ROOT, os.path.join(ROOT, 'tools')]
from cfar_bench import A, C, S, TC, _events  # noqa: E402

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
    a_ca = tables.cfar_alpha(cfg.cfar_pfa, n)
    a_os = tables.os_cfar_alpha(cfg.cfar_pfa, n, tables.os_cfar_rank(n, RANK))
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
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        ev_ms = _events(torch, fn, reps)
        ctx.timing(True)
        ctx.timing_reset()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms, k = ctx.timing_read()['detect']
        ctx.timing(False)
        res[name] = {'ms_events': ev_ms, 'ms_rsl_timing': ms / max(k, 1), 'launches_timed': k,
                     'peaks': int(ch.row_count.sum().item())}
    # the candidates of the count: the 3x3 maxima inside the gate and above the floor = what k_detect marks
    res['candidates'] = res['k_detect']['peaks']
    t = {k: res[k]['ms_rsl_timing'] for k in runs}
    res['ratio_oscfar_over_cfar'] = t['k_detect_oscfar'] / t['k_detect_cfar']
    res['ratio_oscfar_over_detect'] = t['k_detect_oscfar'] / t['k_detect']
    res['model_ms'] = MODEL_MS_AT_2000 * F / 2000
    res['ratio_oscfar_over_model'] = t['k_detect_oscfar'] / res['model_ms']
    return res


def part_step(F, reps, method, pfa):
    import torch
    import rsl
    from bench import make_cubes
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC, ridge=0.01, detector='cfar',
                          cfar_method=method, cfar_rank=RANK, cfar_pfa=pfa)
    ch = rsl.RadarChain(cfg, F, ctx)
    cube = make_cubes(ctx, 1, F, A, C, TC, 0)[0]
    for _ in range(2):
        ch.run(cube)
    torch.cuda.synchronize()
    ms_step = _events(torch, lambda: ch.run(cube), reps)
    ctx.timing(True)
    ctx.timing_reset()
    for _ in range(reps):
        ch.run(cube)
    torch.cuda.synchronize()
    t = ctx.timing_read()
    ctx.timing(False)
    ne, nc = ch.totals()
    return {'cfar_method': method, 'pfa': pfa, 'alpha': ch.cfar_alpha, 'frames': F, 'reps': reps,
            'ms_per_step': ms_step, 'frames_per_s': F / (ms_step * 1e-3), 'entries': ne, 'cells': nc,
            'entries_per_frame': ne / F, 'cells_per_frame': nc / F,
            'kernel_ms_per_step': {k: v[0] / reps for k, v in t.items() if v[1]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--limit', type=int, default=240, help='seconds per measurement (child process)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'oscfar_bench.json'))
    ap.add_argument('--part', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:
        kind, _, rest = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(args.frames, args.reps)
        else:
            method, _, pfa = rest.partition(':')
            res = part_step(args.frames, args.reps, method, float(pfa))
        print('RESULT ' + json.dumps(res), flush=True)
        return 0
    out = {'what': 'OS-CFAR detector at configs[2] (A8 C128 S512), one GPU, one stream (tools/oscfar_bench.py)',
           'steps': []}
    for p in ['standalone', 'step:ca:1e-2', 'step:os:1e-2', 'step:ca:1e-4', 'step:os:1e-4']:
        cmd = [sys.executable, os.path.abspath(__file__), '--part', p, '--frames', str(args.frames), '--reps',
               str(args.reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
        except subprocess.TimeoutExpired:
            print(f'{p}: time limit of {args.limit} s reached; stopping', file=sys.stderr)
            return 124
        line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
        if r.returncode != 0 or not line:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            print(f'{p}: failed with exit status {r.returncode}; stopping', file=sys.stderr)
            return r.returncode or 1
        res = json.loads(line[-1][7:])
        print(p, json.dumps(res), flush=True)
        if p == 'standalone':
            out['standalone'] = res
        else:
            out['steps'].append(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
