"""SHA-256 of the raw output bytes of the phase-model solvers (rsl_associate, rsl_phase_model, rsl_bvls,
rsl_wrapped_solve, rsl_wrapped_search; rows a25-a31) on the inputs of tests/golden/golden_wrapped.npz, and of the pose
evaluation (rsl_eval.hip: align / APE / RTE through the drop-in PoseErrorEvaluator, two seeded trajectories), under the
library RSL_LIBRARY: equal hashes across two libraries = bit-identical solvers.  The two wrapped calls are made on the
library itself, so that all 8 output doubles {x[6], cost, start index} are hashed.
GPU box:  RSL_LIBRARY=... python tools/solver_hash.py"""
import ctypes
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, 'radar-slam_amd')]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import rsl  # noqa: E402
from rsl import ops  # noqa: E402
from rsl.runtime import _ptr  # noqa: E402

SIX = ctypes.c_double * 6


def sha(*arrays):
    return hashlib.sha256(b''.join(np.ascontiguousarray(a).tobytes() for a in arrays)).hexdigest()[:12]


def pose_eval(N):
    """Every output of align_trajectories, compute_ape and compute_rte (segment lengths 1, 10, 100) on one seeded
    trajectory of N poses: a random-walk heading, the estimate rotated, shifted and noisy.  513 = two blocks of the
    256-thread eval kernels and one thread of a third."""
    from evaluation.compute_pose_error import PoseErrorEvaluator
    rs = np.random.RandomState(N)
    yaw = np.cumsum(0.01 * rs.randn(N))
    gt_p = np.cumsum(np.column_stack([np.cos(yaw), np.sin(yaw), 0.05 * rs.randn(N)]), axis=0)
    gt_q = np.column_stack([np.zeros(N), np.zeros(N), np.sin(yaw / 2), np.cos(yaw / 2)])  # scalar last
    c, s = np.cos(0.4), np.sin(0.4)
    est_p = gt_p @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]]) + [3, -1, 0.5] + 0.3 * rs.randn(N, 3)
    est_q = gt_q + 0.03 * rs.randn(N, 4)  # not unit: the device normalises, as Rotation.from_quat does
    est, gt = np.column_stack([est_p, est_q]), np.column_stack([gt_p, gt_q])
    ev = PoseErrorEvaluator(rte_segment_lengths=[1, 10, 100])
    al, T, info = ev.align_trajectories(est, gt)
    parts = [al, T] + [np.float64(info[k]) for k in sorted(info)]
    ape = ev.compute_ape(est, gt)
    parts += [np.float64(ape[k]) for k in sorted(ape) if k != 'alignment_info']
    rte = ev.compute_rte(est, gt)
    for key in sorted(rte):
        parts += [np.float64(rte[key][k]) for k in ('errors', 'rmse', 'mean', 'std', 'max', 'num_segments')]
    return sha(*parts)


def main():
    ctx = rsl.get_context(0)
    z = np.load(os.path.join(ROOT, 'tests', 'golden', 'golden_wrapped.npz'))
    xy = {p: np.stack([z[f'{p}_range_m'] * np.cos(z[f'{p}_azimuth_rad']),
                       z[f'{p}_range_m'] * np.sin(z[f'{p}_azimuth_rad'])], axis=1) for p in ('cur', 'prev')}
    r, az = z['cur_range_m'][z['assoc_cur']], z['cur_azimuth_rad'][z['assoc_cur']]
    pos = np.stack([r * np.cos(az), r * np.sin(az), np.zeros_like(r)], axis=1)
    ang, y, n = np.stack([az, np.zeros_like(az)], axis=1), z['assoc_phase'], len(r)
    k = 4 * np.pi * 0.1 / (3e8 / 77e9)
    prev6, x6 = z['advp_prev'], z['adv_de_x'][0]
    out = {'assoc': sha(*ops.associate(xy['cur'], xy['prev'], 2.0, ctx=ctx))}
    rs = np.random.RandomState(3)
    cur, prev = rs.uniform(-20, 20, (300, 2)), rs.uniform(-20, 20, (280, 2))
    out['assoc_300x280'] = sha(*ops.associate(cur, prev, 2.0, ctx=ctx))
    rows = (rs.randn(5, 300) + 1j * rs.randn(5, 300)).astype(np.complex64)  # the third block sum of rsl_aux.hip
    out['preprocess_dc'] = sha(ops.preprocess_rows(rows, np.exp(1j * rs.randn(300)), True, ctx=ctx))
    for wrap in (0, 1):
        m = ops.phase_model(pos, ang, x6, k, y=y, wrap=bool(wrap), ridge=0.01, ctx=ctx)
        out[f'phase_model_wrap{wrap}'] = sha(m['pred'], m['resid'], np.float64(m['cost']))
    lo, hi = [-50.0, -50.0, -10.0, -10.0, -10.0, -10.0], [50.0, 50.0, 10.0, 10.0, 10.0, 10.0]
    for nv in (3, 6):
        x, cost = ops.bvls(pos, ang, y, k, lo[:nv], hi[:nv], ridge=0.01, ctx=ctx)
        out[f'bvls_nv{nv}'] = sha(x, np.float64(cost))

    # the wrapped entry points on the library itself: fn(..., nv, *own, extra, nextra, iters, scratch, bytes, out)
    dp, da, dy = (ctx.to_dev(np.ascontiguousarray(a, np.float64).reshape(-1)) for a in (pos, ang, y))
    dprev = ctx.to_dev(np.ascontiguousarray(prev6, np.float64))
    extra = np.array([[1.0, -0.5, 0.0, 0.0, 0.0, 0.0], [-3.0, 2.0, 0.1, 0.01, -0.02, 0.03]])
    dex, o8 = ctx.to_dev(extra.reshape(-1)), ctx.empty((8,), torch.float64)

    def wrapped(fn, mode, nv, prev, lo, hi, own, nbytes):
        scratch = ctx.empty((nbytes // 8,), torch.float64)
        ctx._bind()
        ctx.check(fn(ctx.h, _ptr(dp), _ptr(da), n, _ptr(dy), k, mode, 0.01, 50.0, 10.0, _ptr(prev), SIX(*lo), SIX(*hi),
                     nv, *own, _ptr(dex), 2, 12, _ptr(scratch), nbytes, _ptr(o8)), 'wrapped')
        return sha(o8.cpu().numpy())

    for mode in (0, 1):
        for nv in (3, 6):
            for tag, prev in (('', None), ('_prev', dprev)):
                out[f'solve_m{mode}_nv{nv}{tag}'] = wrapped(ctx.lib.rsl_wrapped_solve, mode, nv, prev, lo, hi, (64,),
                                                            ctx.lib.rsl_wrapped_scratch_bytes(n, 64, 2))
    lo[:2], hi[:2] = [-2.0, -2.0], [2.0, 2.0]  # +-2 m/s at half a wrap period: about 1.7e5 stage-1 starts
    spacing = 0.5 * 2 * np.pi / k
    nbytes = ctx.lib.rsl_wrapped_search_scratch_bytes(n, SIX(*lo), SIX(*hi), spacing, 64, 2)
    for mode in (0, 1):
        out[f'search_m{mode}'] = wrapped(ctx.lib.rsl_wrapped_search, mode, 6, dprev if mode else None, lo, hi,
                                         (SIX(0, 0, 0, 0, 0, 0), spacing, 64), nbytes)
    for N in (513, 1000):
        out[f'pose_eval_n{N}'] = pose_eval(N)
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
