"""Range-azimuth map measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream:

* standalone, on the RDS of one batch: k_range_cov alone (ms per launch from rsl_timing_* and from stream events, and
  its HBM read rate over the 8 A S C bytes per frame it reads) next to rsl_power_integrate on the same buffer, which
  reads the whole RDS once too; k_range_azimuth for both methods on that covariance (ms per launch, maps per second);
* whole step: ms per ch.run() and frames/s without ra_map and with ra_map='bartlett' / 'capon', with the per-kernel
  times of rsl_timing_read (the two new kernels are timed under doa_scan).

Each measurement runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/ra_map_bench.json.   python tools/ra_map_bench.py [--frames 2000] [--reps 5]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402
from bench_parts import A, C, S, TC  # noqa: E402

METHODS = ('bartlett', 'capon')


def part_standalone(F, reps):
    import torch
    import rsl
    from bench import make_cubes
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC, ra_map='capon')
    ch = rsl.RadarChain(cfg, F, ctx)
    cube = make_cubes(ctx, 1, F, A, C, TC, 0)[0]
    ch.run_front(cube)  # fills ch.rds
    torch.cuda.synchronize()
    G = len(ch.grid)
    rds_bytes = F * 8 * A * S * C
    res = {'frames': F, 'reps': reps, 'grid_points': G, 'rds_bytes': rds_bytes,
           'cov_bytes_written': F * S * A * A * 8, 'map_bytes_written': F * S * G * 4}
    power = ctx.empty((F, S, C), torch.float32)
    r = B.timed(ctx, torch, lambda: ctx.integrate_power(ch.rds, out=power), reps, 'detect')
    res['k_power_integrate'] = {**r, 'read_tb_per_s': rds_bytes / (r['ms_rsl_timing'] * 1e-3) / 1e12}
    r = B.timed(ctx, torch, ch.ra.cov, reps, 'doa_scan')
    res['k_range_cov'] = {**r, 'read_tb_per_s': rds_bytes / (r['ms_rsl_timing'] * 1e-3) / 1e12,
                          'mfma_per_range_bin': C // 4}
    res['cov_rate_over_integrate_rate'] = (res['k_range_cov']['read_tb_per_s'] /
                                           res['k_power_integrate']['read_tb_per_s'])
    for m in METHODS:
        r = B.timed(ctx, torch, lambda: ch.ra.launch(with_cov=False, method=m), reps, 'doa_scan')
        res[f'k_range_azimuth_{m}'] = {**r, 'rows_per_s': F * S / (r['ms_rsl_timing'] * 1e-3),
                                       'grid_points_per_s': F * S * G / (r['ms_rsl_timing'] * 1e-3)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    B.add_arguments(ap, 'ra_map_bench.json')
    args = ap.parse_args()
    if args.part:
        kind, _, m = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(args.frames, args.reps)
        else:
            res = B.chain_step(args.frames, args.reps, lambda ch: {'ra_map': m if m != 'none' else None},
                               ra_map=None if m == 'none' else m)
        B.emit_result(res)
        return 0
    parts = ['standalone'] + [f'step:{m}' for m in ('none',) + METHODS]
    rc, res = B.run_parts(__file__, parts, ['--frames', args.frames, '--reps', args.reps], args.limit)
    if rc:
        return rc
    B.write_json(args.out, {
        'what': 'range-azimuth maps at configs[2] (A8 C128 S512), one GPU, one stream (tools/ra_map_bench.py)',
        'standalone': res['standalone'], 'steps': [res[p] for p in parts[1:]]})
    return 0


if __name__ == '__main__':
    sys.exit(main())
