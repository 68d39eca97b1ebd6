"""Spatially smoothed MUSIC (rsl_doa_smoothed / k_doa_smoothed) measurements, one GPU, one stream:

cells/s at (M, L) = (8, 6) and (16, 8) on 35 000 cells per frame x 64 frames (range-major cell lists over a
Gaussian-noise RDS c64 [64, M, 512, 128], G = 361, nmax = 3), with the order estimated (rel 0.05) and fixed at 2, and
beside it the existing one-angle Toeplitz scan (rsl_doa, MUSIC argmax) on the same cells in the same process.  ms per
launch from rsl_timing_* (RSL_K_DOA_SCAN) and from stream events.

Each (M, L) runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/ssmusic_bench.json.   python tools/ssmusic_bench.py [--frames 64] [--cells 35000] [--reps 5]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'radar-slam_amd'), ROOT]
S, C, G = 512, 128, 361


def _timed(ctx, torch, fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    ev_ms = a.elapsed_time(b) / reps
    ctx.timing(True)
    ctx.timing_reset()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    ms, n = ctx.timing_read()['doa_scan']
    ctx.timing(False)
    return {'ms_events': ev_ms, 'ms_rsl_timing': ms / max(n, 1), 'launches_timed': n}


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
        r = _timed(ctx, torch, fn, reps)
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
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--limit', type=int, default=240, help='seconds per measurement (child process)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ssmusic_bench.json'))
    ap.add_argument('--part', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.part:
        M, L = (int(v) for v in args.part.split(':'))
        print('RESULT ' + json.dumps(part(M, L, args.frames, args.cells, args.reps)), flush=True)
        return 0
    out = {'what': 'spatially smoothed MUSIC (rsl_doa_smoothed) next to the Toeplitz one-angle scan (rsl_doa) on the '
                   'same cells, one GPU, one stream (tools/ssmusic_bench.py)', 'runs': []}
    for p in ('8:6', '16:8'):
        cmd = [sys.executable, os.path.abspath(__file__), '--part', p, '--frames', str(args.frames), '--cells',
               str(args.cells), '--reps', str(args.reps)]
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
        out['runs'].append(res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(out, f, indent=1)
        f.write('\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
