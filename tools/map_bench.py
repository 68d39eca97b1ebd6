"""Grid map measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream, for the threshold
detector (the reference's rule: about 35.5 k cells per frame) and for detector='cfar', detect_on='sum':

* standalone, on the point cloud and cell_base of one chain batch and the poses of one TrajectoryReducer step on the
  chain's velocity rows: rsl_map_update with and without the free plane (ms per launch from rsl_timing_* and from stream
  events, frames per second, and from the stats rows the accepted points, hit cells and free cells per frame, hence the
  global integer adds per second of the flush), rsl_map_logodds, and rsl_cell_refine on the same list in the same run
  (the yardstick);
* the same update with every frame at the first pose: all frames' rays share the cells near the sensor, the
  most contended flush;
* the default step under the parent commit's library (radar-slam_amd/lib/librsl_ab.so, tools/build_ab.sh <parent>)
  and under the tree's, alternating, --rounds times each: the tree's values against the parent's run-to-run range.
  The map is no chain stage: an unused GridMap allocates and launches nothing.

The map: 0.25 m cells, r_max 77 m (Rw = 309: two 47.9 KB bitmaps per workgroup), the trajectory and 80 m around it.
Each measurement runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/map_bench.json.   python tools/map_bench.py [--frames 2000] [--reps 5] [--rounds 4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402
from bench_parts import A, C, TC  # noqa: E402

PARENT_LIB = os.path.join(B.ROOT, 'radar-slam_amd', 'lib', 'librsl_ab.so')
DETECTORS = {'threshold': {}, 'cfar_sum': dict(detector='cfar', detect_on='sum')}
MAP = dict(cell=0.25, r_min=0.5, r_max=77.0)
MARGIN, MOST = 80.0, 16384  # metres of map around the trajectory; the most cells per side


def map_around(poses):
    """GridMap arguments of a map that holds the trajectory and MARGIN around it (at most MOST cells per side)."""
    import math
    lo = [math.floor(float(poses[:, k].min()) - MARGIN) for k in (0, 1)]
    n = [min(MOST, int(math.ceil((float(poses[:, k].max()) + MARGIN - lo[k]) / MAP['cell']))) for k in (0, 1)]
    return dict(MAP, origin=(float(lo[0]), float(lo[1])), shape=(n[1], n[0]))


def part_standalone(det, F, reps):
    import torch
    import rsl
    from bench import make_cubes
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC, ridge=0.01, point_cloud=True,
                          **DETECTORS[det])
    ch = rsl.RadarChain(cfg, F, ctx)
    cube = make_cubes(ctx, 1, F, A, C, TC, 0)[0]
    ch.run(cube)  # fills the lists, the point cloud and the velocity rows
    red = rsl.TrajectoryReducer(ctx, F, dt=cfg.dt, smoothing=False, collective=False)
    red.step(ch.vel, vstride=8)
    torch.cuda.synchronize()
    _, nc = ch.totals()
    poses = red.poses.cpu().numpy()
    kw = map_around(poses)
    res = {'detector': det, 'frames': F, 'reps': reps, 'cells': nc, 'cells_per_frame': nc / F, 'map': kw,
           'pose_span_m': [float(poses[:, 0].min()), float(poses[:, 0].max()), float(poses[:, 1].min()),
                           float(poses[:, 1].max())]}

    def update(gm, poses_dev):
        return lambda: gm.update_chain(ch, poses_dev)

    same = red.poses[:1].expand(F, 7).contiguous()
    for name, free, pd in (('k_map_update', True, red.poses), ('k_map_update_no_free', False, red.poses),
                           ('k_map_update_same_pose', True, same)):
        gm = rsl.GridMap(ctx, free=free, **kw)
        r = B.timed(ctx, torch, update(gm, pd), reps, 'aux')
        st = gm.stats.cpu().numpy().astype('int64')
        r.update(frames_per_s=F / (r['ms_rsl_timing'] * 1e-3), flagged_frames=int(st[:, 3].sum()),
                 points_per_frame=float(st[:, 0].mean()), hit_cells_per_frame=float(st[:, 1].mean()),
                 free_cells_per_frame=float(st[:, 2].mean()),
                 global_adds_per_s=float(st[:, 1:3].sum() / (r['ms_rsl_timing'] * 1e-3)),
                 added_bytes_per_s=float(4 * st[:, 1:3].sum() / (r['ms_rsl_timing'] * 1e-3)))
        res[name] = r
        if name == 'k_map_update':
            res['k_map_logodds'] = B.timed(ctx, torch, gm.logodds, reps, 'aux')
            res['k_map_logodds']['bytes_per_s'] = 12 * gm.hits.numel() / (res['k_map_logodds']['ms_rsl_timing'] * 1e-3)
    res['k_cell_refine'] = B.timed(ctx, torch, ch.pc.launch, reps, 'cell_extras')
    for k in ('k_map_update', 'k_map_update_no_free', 'k_map_update_same_pose', 'k_map_logodds'):
        res[k + '_over_refine'] = res[k]['ms_rsl_timing'] / res['k_cell_refine']['ms_rsl_timing']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=4)
    B.add_arguments(ap, 'map_bench.json')
    args = ap.parse_args()
    if args.part:
        kind, _, m = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(m, args.frames, args.reps)
        else:  # 'parent:k' / 'tree:k': the default step under one of the two libraries
            if kind == 'parent':
                os.environ['RSL_LIBRARY'] = PARENT_LIB  # read when rsl is first imported (inside chain_step)
            res = B.chain_step(args.frames, args.reps, lambda ch: {'library': kind, 'round': int(m)})
        B.emit_result(res)
        return 0
    ab = os.path.exists(PARENT_LIB)
    if not ab:
        print(f'{PARENT_LIB} absent (tools/build_ab.sh <parent commit>): no A/B of the default step', file=sys.stderr)
    parts = [f'standalone:{d}' for d in DETECTORS]
    # alternating, and the library that goes first alternates too: neither is always the one after a cold start
    ab_parts = [f'{lib}:{k}' for k in range(args.rounds)
                for lib in (('parent', 'tree') if k % 2 == 0 else ('tree', 'parent'))] if ab else []
    rc, res = B.run_parts(__file__, parts + ab_parts, ['--frames', args.frames, '--reps', args.reps], args.limit)
    if rc:
        return rc
    out = {'what': 'grid map (rsl_map_update, rsl_map_logodds) at configs[2] (A8 C128 S512), one GPU, one stream '
                   '(tools/map_bench.py)',
           'standalone': [res[p] for p in parts]}
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
