"""CA-CFAR detector measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream:

* standalone: k_detect_cfar (default window) next to k_detect on the same RDS buffer (both read 8 B per cell):
  ms per launch from rsl_timing_* and from stream events, the ratio and the achieved TB/s of the 8 B/cell read;
* whole step: ms per ch.run() with detector='threshold' and detector='cfar' at Pfa 1e-2 and 1e-4, with the entry and
  cell totals and the per-kernel times of rsl_timing_read (K5 = doa_scan, emit, velocity, detect, ...).

Each measurement runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/cfar_bench.json.   python tools/cfar_bench.py [--frames 2000] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'radar-slam_amd'), ROOT]
A, C, S, TC = 8, 128, 512, 51.2e-6


def _events(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


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
    alpha = tables.cfar_alpha(cfg.cfar_pfa, tables.cfar_training_cells(cfg.cfar_guard, cfg.cfar_train))
    out = dict(mask=ch.mask, row_count=ch.row_count, peak_pow=ch.peak_pow)
    runs = {
        'k_detect': lambda: ctx.detect(ch.rds, ch.thr_p, ch.i_lo, ch.i_hi, out=out),
        'k_detect_cfar': lambda: ctx.detect_cfar(ch.rds, cfg.cfar_guard, cfg.cfar_train, alpha, ch.thr_p, ch.i_lo,
                                                 ch.i_hi, out=out),
    }
    res = {'frames': F, 'reps': reps, 'window': {'guard': cfg.cfar_guard, 'train': cfg.cfar_train},
           'bytes_read_floor': F * A * S * C * 8}
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
        ms, n = ctx.timing_read()['detect']
        ctx.timing(False)
        peaks = int(ch.row_count.sum().item())
        res[name] = {'ms_events': ev_ms, 'ms_rsl_timing': ms / max(n, 1), 'launches_timed': n, 'peaks': peaks,
                     'tb_per_s': F * A * S * C * 8 / (ms / max(n, 1) * 1e-3) / 1e12}
    res['ratio_cfar_over_detect'] = res['k_detect_cfar']['ms_rsl_timing'] / res['k_detect']['ms_rsl_timing']
    return res


def part_step(F, reps, detector, pfa):
    import torch
    import rsl
    from bench import make_cubes
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC, ridge=0.01, detector=detector,
                          cfar_pfa=pfa)
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
    return {'detector': detector, 'pfa': pfa if detector == 'cfar' else None, 'frames': F, 'reps': reps,
            'ms_per_step': ms_step, 'frames_per_s': F / (ms_step * 1e-3), 'entries': ne, 'cells': nc,
            'entries_per_frame': ne / F, 'cells_per_frame': nc / F,
            'kernel_ms_per_step': {k: v[0] / reps for k, v in t.items() if v[1]}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--limit', type=int, default=240, help='seconds per measurement (child process)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cfar_bench.json'))
    ap.add_argument('--part', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:
        kind, _, rest = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(args.frames, args.reps)
        else:
            det, _, pfa = rest.partition(':')
            res = part_step(args.frames, args.reps, det, float(pfa or 1e-4))
        print('RESULT ' + json.dumps(res), flush=True)
        return 0
    out = {'what': 'CA-CFAR detector at configs[2] (A8 C128 S512), one GPU, one stream (tools/cfar_bench.py)',
           'steps': []}
    parts = ['standalone', 'step:threshold', 'step:cfar:1e-2', 'step:cfar:1e-4']
    for p in parts:
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
