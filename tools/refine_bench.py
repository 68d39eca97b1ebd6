"""Point-cloud measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream:

* standalone, on the cell lists, grid indices and RDS of one chain batch: rsl_cell_refine with the power map given
  (ms per launch from rsl_timing_* and from stream events, cells per second, and the bytes it needs over that time)
  next to rsl_cell_extras on the same list (ESPRIT + phase, the chain's call: the yardstick of the byte model) and
  rsl_power_integrate on the same RDS; rsl_cell_refine without a power map (the per-call path) for the record;
* whole step: ms per ch.run() and frames/s without point_cloud, with it, and with velocity_az='refined', with the
  per-kernel times of rsl_timing_read (the refinement is timed under cell_extras, the integration under detect);
* the default step under the parent commit's library (radar-slam_amd/lib/librsl_ab.so, tools/build_ab.sh <parent>)
  and under the tree's, alternating, --rounds times each: the tree's values against the parent's run-to-run range.

Each measurement runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/refine_bench.json.   python tools/refine_bench.py [--frames 2000] [--reps 5] [--rounds 4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402
from bench_parts import A, C, S, TC  # noqa: E402

PARENT_LIB = os.path.join(B.ROOT, 'radar-slam_amd', 'lib', 'librsl_ab.so')
STEPS = {'none': {}, 'point_cloud': dict(point_cloud=True),
         'point_cloud_refined_az': dict(point_cloud=True, velocity_az='refined')}


def part_standalone(F, reps):
    import torch
    import rsl
    from bench import make_cubes
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC, ridge=0.01, point_cloud=True)
    ch = rsl.RadarChain(cfg, F, ctx)
    cube = make_cubes(ctx, 1, F, A, C, TC, 0)[0]
    ch.run(cube)  # fills the RDS, the lists, gidx and the power map
    torch.cuda.synchronize()
    _, nc = ch.totals()
    G = len(ch.grid)
    # what the algorithm needs per cell: the signature (A c64), 5 powers, frame + rc + gidx, one row and one double
    refine_bytes = nc * (8 * A + 5 * 4 + 3 * 4 + 32 + 8)
    extras_bytes = nc * (8 * A + 2 * 4 + 2 * 8)  # the signature, frame + rc, esprit + phase
    res = {'frames': F, 'reps': reps, 'cells': nc, 'cells_per_frame': nc / F, 'grid_points': G,
           'steer_table_bytes': G * A * 8, 'refine_bytes_needed': refine_bytes, 'extras_bytes_needed': extras_bytes}

    def extras():
        return ctx.cell_extras(**ch.cells(), esprit_scale=ch.esprit_scale, want_esprit=True, want_phase=True,
                               bufs=ch.ext)
    for name, fn, nbytes in (('k_cell_refine', ch.pc.launch, refine_bytes), ('k_cell_extras', extras, extras_bytes),
                             ('k_cell_refine_null_power', lambda: ch.pc.launch(power=None), None)):
        r = B.timed(ctx, torch, fn, reps, 'cell_extras')
        r['cells_per_s'] = nc / (r['ms_rsl_timing'] * 1e-3)
        if nbytes:
            r['needed_tb_per_s'] = nbytes / (r['ms_rsl_timing'] * 1e-3) / 1e12
        res[name] = r
    rds_bytes = F * 8 * A * S * C
    r = B.timed(ctx, torch, lambda: ctx.integrate_power(ch.rds, out=ch.power), reps, 'detect')
    res['k_power_integrate'] = {**r, 'read_tb_per_s': rds_bytes / (r['ms_rsl_timing'] * 1e-3) / 1e12}
    res['refine_over_extras'] = res['k_cell_refine']['ms_rsl_timing'] / res['k_cell_extras']['ms_rsl_timing']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=4)
    B.add_arguments(ap, 'refine_bench.json')
    args = ap.parse_args()
    if args.part:
        kind, _, m = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(args.frames, args.reps)
        elif kind == 'step':
            res = B.chain_step(args.frames, args.reps, lambda ch: {'config': m}, **STEPS[m])
        else:  # 'parent:k' / 'tree:k': the default step under one of the two libraries
            if kind == 'parent':
                os.environ['RSL_LIBRARY'] = PARENT_LIB  # read when rsl is first imported (inside chain_step)
            res = B.chain_step(args.frames, args.reps, lambda ch: {'library': kind, 'round': int(m)})
        B.emit_result(res)
        return 0
    ab = os.path.exists(PARENT_LIB)
    if not ab:
        print(f'{PARENT_LIB} absent (tools/build_ab.sh <parent commit>): no A/B of the default step', file=sys.stderr)
    parts = ['standalone'] + [f'step:{m}' for m in STEPS]
    # alternating, and the library that goes first alternates too: neither is always the one after a cold start
    ab_parts = [f'{lib}:{k}' for k in range(args.rounds)
                for lib in (('parent', 'tree') if k % 2 == 0 else ('tree', 'parent'))] if ab else []
    rc, res = B.run_parts(__file__, parts + ab_parts, ['--frames', args.frames, '--reps', args.reps], args.limit)
    if rc:
        return rc
    out = {'what': 'point cloud (rsl_cell_refine) at configs[2] (A8 C128 S512), one GPU, one stream '
                   '(tools/refine_bench.py)',
           'standalone': res['standalone'], 'steps': [res[p] for p in parts[1:]]}
    if ab:
        ms = {lib: [res[f'{lib}:{k}']['ms_per_step'] for k in range(args.rounds)] for lib in ('parent', 'tree')}
        lo, hi = min(ms['parent']), max(ms['parent'])
        med = sorted(ms['tree'])[len(ms['tree']) // 2]
        out['default_step_ab'] = {'ms_per_step': ms, 'parent_range_ms': [lo, hi],
                                  'tree_range_ms': [min(ms['tree']), max(ms['tree'])], 'tree_median_ms': med,
                                  'tree_median_inside_parent_range': lo <= med <= hi,
                                  'tree_median_over_parent_median': med / sorted(ms['parent'])[len(ms['parent']) // 2]}
    B.write_json(args.out, out)
    return 0


if __name__ == '__main__':
    sys.exit(main())
