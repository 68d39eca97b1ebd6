"""Scan-registration measurements at configs[2] (A8 C128 S512), F frames per step, one GPU, one stream, for the
threshold detector (the reference's rule: about 35.5 k cells per frame) and for detector='cfar', detect_on='sum':

* standalone, on the point cloud, cell_base, c_rc and velocity rows of one chain batch: the chain's own registration
  launch (ch.reg.launch: ms per launch of rsl_scan_register from rsl_timing_*, and from stream events with the stage's
  start row and its copy of the last frame, frame pairs per second), the same without rc (every pair tested: only where
  the cloud is small enough, --dense-limit cells per frame), and the chain's rsl_cell_refine launch on the same list in
  the same run (the yardstick);
* whole step: ms per ch.run() and frames/s with the point cloud and with the point cloud and the registration;
* the default step under the parent commit's library (radar-slam_amd/lib/librsl_ab.so, tools/build_ab.sh <parent>)
  and under the tree's, alternating, --rounds times each: the tree's values against the parent's run-to-run range.

Each measurement runs in a child process of its own under its own time limit; the first failure ends the run.
Writes profiles/register_bench.json.   python tools/register_bench.py [--frames 2000] [--reps 3] [--rounds 4]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench_parts as B  # noqa: E402
from bench_parts import A, C, TC  # noqa: E402

PARENT_LIB = os.path.join(B.ROOT, 'radar-slam_amd', 'lib', 'librsl_ab.so')
DETECTORS = {'threshold': {}, 'cfar_sum': dict(detector='cfar', detect_on='sum')}
STEPS = {f'{d}:{m}': dict(kw, point_cloud=True, **({'registration': True} if m == 'registration' else {}))
         for d, kw in DETECTORS.items() for m in ('point_cloud', 'registration')}


def part_standalone(det, F, reps, dense_limit):
    import torch
    import rsl
    from bench import make_cubes
    ctx = rsl.get_context(0)
    cfg = rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=TC, ridge=0.01, point_cloud=True,
                          registration=True, **DETECTORS[det])
    ch = rsl.RadarChain(cfg, F, ctx)
    cube = make_cubes(ctx, 1, F, A, C, TC, 0)[0]
    ch.run(cube)  # fills the lists, the point cloud, the velocity rows and the registration rows
    torch.cuda.synchronize()
    _, nc = ch.totals()
    rows = ch.reg.out['rows'].cpu().numpy()
    res = {'detector': det, 'frames': F, 'reps': reps, 'cells': nc, 'cells_per_frame': nc / F,
           'settings': dict(h=cfg.reg_h, h_coarse=cfg.reg_h_coarse, dtheta=cfg.reg_dtheta, k=cfg.reg_k,
                            iters=cfg.reg_iters, shrink=cfg.reg_shrink, tol=cfg.reg_tol, w_min=cfg.reg_w_min),
           'flags': {str(k): int((rows[:, 7] == k).sum()) for k in (0, 1, 2)},
           'updates_mean': float(rows[rows[:, 7] == 0, 6].mean()) if (rows[:, 7] == 0).any() else 0.0}
    # the chain's own launches: frame 0 without a reference, as in a first run (the stream-event time includes the
    # stage's start row and its copy of the last frame; rsl_timing_* times the kernel alone)
    r = B.timed(ctx, torch, lambda: ch.reg.launch(prev=None), reps, 'aux')
    r['frame_pairs_per_s'] = (F - 1) / (r['ms_rsl_timing'] * 1e-3)
    res['k_scan_register'] = r
    if nc / F <= dense_limit:
        r = B.timed(ctx, torch, lambda: ch.reg.launch(prev=None, rc=None, C=0, axes=None), reps, 'aux')
        res['k_scan_register_no_rc'] = r
        res['no_rc_over_rc'] = r['ms_rsl_timing'] / res['k_scan_register']['ms_rsl_timing']
    res['k_cell_refine'] = B.timed(ctx, torch, ch.pc.launch, reps, 'cell_extras')
    res['register_over_refine'] = res['k_scan_register']['ms_rsl_timing'] / res['k_cell_refine']['ms_rsl_timing']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=2000)
    ap.add_argument('--rounds', type=int, default=4)
    ap.add_argument('--dense-limit', type=float, default=2000.0)
    B.add_arguments(ap, 'register_bench.json')
    args = ap.parse_args()
    if args.part:
        kind, _, m = args.part.partition(':')
        if kind == 'standalone':
            res = part_standalone(m, args.frames, args.reps, args.dense_limit)
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
    parts = [f'standalone:{d}' for d in DETECTORS] + [f'step:{m}' for m in STEPS]
    # alternating, and the library that goes first alternates too: neither is always the one after a cold start
    ab_parts = [f'{lib}:{k}' for k in range(args.rounds)
                for lib in (('parent', 'tree') if k % 2 == 0 else ('tree', 'parent'))] if ab else []
    rc, res = B.run_parts(__file__, parts + ab_parts,
                          ['--frames', args.frames, '--reps', args.reps, '--dense-limit', args.dense_limit], args.limit)
    if rc:
        return rc
    out = {'what': 'scan registration (rsl_scan_register) at configs[2] (A8 C128 S512), one GPU, one stream '
                   '(tools/register_bench.py)',
           'standalone': [res[p] for p in parts[:len(DETECTORS)]], 'steps': [res[p] for p in parts[len(DETECTORS):]]}
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
