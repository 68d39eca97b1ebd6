"""Robust velocity solve measurements at configs[2] (A8 C128 S512), F frames per launch, one GPU, one stream.

On the cfg2 chain's own lists (gidx, phase, c_amask, cell_base after one ch.run()), in one process:
k_velocity (rsl_velocity) and k_velocity_robust (rsl_velocity_robust) with Huber and Tukey, each with a given scale
and with the estimated scale, at iters = 30, tol = 1e-9.  ms per launch from rsl_timing_* (RSL_K_VELOCITY) and from
stream events, the mean iteration count, the share of frames that met the stop rule, and the ratio to rsl_velocity in
the same run.  The given scale is the median of rsl_velocity's per-frame rmse on these lists (they hold no planted
motion: the figure of interest here is the time, not the estimate).

The measurement runs in a child process under a time limit.  Writes profiles/vel_robust_bench.json.
    python tools/vel_robust_bench.py [--frames 2000] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'radar-slam_amd'), ROOT]
A, C, S, TC = 8, 128, 512, 51.2e-6
ITERS, TOL = 30, 1e-9


def _events(torch, fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


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
    runs = {'k_velocity': lambda: ctx.velocity(None, y, seg, out=out, **common)}
    for loss in ('huber', 'tukey'):
        for name, scale in (('fixed', sigma), ('auto', None)):
            runs[f'{loss}_{name}'] = (lambda loss=loss, scale=scale: ctx.velocity_robust(
                None, y, seg, loss=loss, scale=scale, iters=ITERS, tol=TOL, out=out, want_weight=weight, **common))
    res = {'frames': F, 'reps': reps, 'cells': nc, 'cells_per_frame': nc / F, 'iters': ITERS, 'tol': TOL,
           'given_scale': sigma, 'bytes_per_pass': nc * 16, 'variants': {}}
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
        ms, n = ctx.timing_read()['velocity']
        ctx.timing(False)
        r = {'ms_events': ev_ms, 'ms_rsl_timing': ms / max(n, 1), 'launches_timed': n}
        if name != 'k_velocity':
            o = out.cpu().numpy()
            it = np.abs(o[:, 7])
            passes = 2 + it * (4 if name.endswith('auto') else 1)  # LS start + output + per-iteration passes
            r.update(mean_iterations=float(it.mean()), max_iterations=float(it.max()),
                     stop_rule_met=float((o[:, 7] >= 0).mean()), mean_sigma=float(o[:, 6].mean()),
                     mean_inlier_share=float((o[:, 4] / np.maximum(o[:, 5], 1)).mean()),
                     mean_passes=float(passes.mean()),
                     streamed_tb_per_s=float((passes * np.diff(seg.cpu().numpy()) * 16).sum() /
                                             (r['ms_rsl_timing'] * 1e-3) / 1e12))
        res['variants'][name] = r
    base = res['variants']['k_velocity']['ms_rsl_timing']
    for name, r in res['variants'].items():
        r['ratio_to_k_velocity'] = r['ms_rsl_timing'] / base
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--limit', type=int, default=300, help='seconds for the measurement (child process)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vel_robust_bench.json'))
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print('RESULT ' + json.dumps(measure(args.frames, args.reps)), flush=True)
        return 0
    cmd = [sys.executable, os.path.abspath(__file__), '--child', '--frames', str(args.frames), '--reps',
           str(args.reps)]
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=args.limit)
    except subprocess.TimeoutExpired:
        print(f'time limit of {args.limit} s reached; stopping', file=sys.stderr)
        return 124
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        print(f'failed with exit status {r.returncode}', file=sys.stderr)
        return r.returncode or 1
    res = json.loads(line[-1][7:])
    out = {'what': 'robust velocity solve at configs[2] (A8 C128 S512) on the chain\'s own lists, one GPU, one stream '
                   '(tools/vel_robust_bench.py)', **res}
    for name, v in res['variants'].items():
        print(name, json.dumps(v), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
