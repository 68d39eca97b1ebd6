"""Grid map in world coordinates from point clouds and poses (rsl_map_update / rsl_map_logodds, specified in
include/rsl.h): two planes of unsigned counts, per scan at most one hit or one free count per cell, and the clamped
log-odds derived from them at the end.

    gm = GridMap(ctx, origin=(-20.0, -60.0), shape=(480, 800))
    gm.update_chain(chain, reducer.poses)          # after chain.run(...) and reducer.step(...)
    occ = gm.results()['logodds'] > 0

Integer adds commute: the planes do not depend on the order of the frames nor on how they are split over calls or ranks,
and rank maps merge by adding the planes (``dist.all_reduce`` on ``gm.hits`` / ``gm.free``, which are int32 views of the
unsigned counts).  No collective is issued here.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import _lib


def check_params(*, origin, cell=0.25, shape, r_min=0.5, r_max=75.0, min_db=-math.inf, l_occ=0.85, l_free=0.4,
                 l_min=-4.0, l_max=4.0) -> dict:
    """The argument rules of rsl_map_update and rsl_map_logodds, on the host, as ValueError.  Returns the checked
    values: grid (x0, y0, cell), shape (ny, nx), the half window rw, and the rest by name."""
    try:
        x0, y0 = (float(v) for v in origin)
        ny, nx = (int(v) for v in shape)
    except (TypeError, ValueError):
        raise ValueError('grid map: origin = (x0, y0) and shape = (ny, nx) expected') from None
    cell, r_min, r_max, min_db = float(cell), float(r_min), float(r_max), float(min_db)
    if not (math.isfinite(x0) and math.isfinite(y0) and math.isfinite(cell) and cell > 0.0):
        raise ValueError('grid map: origin and cell must be finite, cell > 0')
    if not r_min >= 0.0:
        raise ValueError('grid map: r_min must be >= 0')
    if not (math.isfinite(r_max) and r_max >= r_min):
        raise ValueError('grid map: r_max must be finite, >= r_min')
    if math.isnan(min_db) or min_db == math.inf:
        raise ValueError('grid map: min_db is NaN or +inf')
    if nx <= 0 or ny <= 0 or nx * ny >= 2 ** 31:
        raise ValueError('grid map: shape = (ny, nx) must be positive with ny nx < 2^31')
    rw = math.ceil(r_max * (1.0 / cell)) + 1
    if not rw <= _lib.MAP_MAX_RW:
        raise ValueError(f'grid map: ceil(r_max / cell) + 1 = {rw} cells above the limit {_lib.MAP_MAX_RW} '
                         f'(two window bitmaps must fit the LDS of one CU): use a larger cell or a smaller r_max')
    lo = [float(v) for v in (l_occ, l_free, l_min, l_max)]
    if not all(math.isfinite(v) for v in lo):
        raise ValueError('grid map: l_occ, l_free, l_min and l_max must be finite')
    if lo[2] > lo[3]:
        raise ValueError('grid map: l_min > l_max')
    return dict(grid=(x0, y0, cell), shape=(ny, nx), rw=int(rw), r_min=r_min, r_max=r_max, min_db=min_db, l_occ=lo[0],
                l_free=lo[1], l_min=lo[2], l_max=lo[3])


class GridMap:
    """The hit and free count planes of one map on the device, and the calls that fill and read them.

    origin = (x0, y0): the world position of the corner of cell (0, 0); cell: the cell size in metres; shape = (ny, nx);
    r_min, r_max: the range gate of the points (r_max also bounds the rays: ceil(r_max / cell) + 1 <= 383 cells);
    min_db: points with a power_db below it are ignored; free=False: no free plane, no rays; l_occ, l_free, l_min,
    l_max: logodds = clamp(hits l_occ - free l_free, l_min, l_max).  Arguments are checked on the host, before any
    device use."""

    def __init__(self, ctx, *, origin, cell: float = 0.25, shape, r_min: float = 0.5, r_max: float = 75.0,
                 min_db: float = -math.inf, free: bool = True, l_occ: float = 0.85, l_free: float = 0.4,
                 l_min: float = -4.0, l_max: float = 4.0):
        p = check_params(origin=origin, cell=cell, shape=shape, r_min=r_min, r_max=r_max, min_db=min_db, l_occ=l_occ,
                         l_free=l_free, l_min=l_min, l_max=l_max)
        self.ctx = ctx
        self.grid, self.shape, self.rw = p['grid'], p['shape'], p['rw']
        self.gate = dict(r_min=p['r_min'], r_max=p['r_max'], min_db=p['min_db'])
        self.lo = dict(l_occ=p['l_occ'], l_free=p['l_free'], l_min=p['l_min'], l_max=p['l_max'])
        torch = ctx.torch
        self.hits = torch.zeros(self.shape, dtype=torch.int32, device=ctx.device)
        self.free = torch.zeros(self.shape, dtype=torch.int32, device=ctx.device) if free else None
        self.stats = None  # i32 [F, 4] of the last update

    def update(self, points, seg, poses, weight=None, n: Optional[int] = None):
        """Adds the F frames of one call: points f32 [N, 8], seg i64 [F + 1], poses f64 [F, 7], weight f32 [N] or None
        (device tensors; Context.map_update).  Returns the frames' stats (device i32 [F, 4])."""
        st = self.ctx.map_update(points, seg, poses, self.hits, grid=self.grid, free=self.free, weight=weight, n=n,
                                 **self.gate)
        self.stats = st[:int(seg.shape[0]) - 1]
        return self.stats

    def update_chain(self, chain, poses):
        """Adds the frames of `chain`'s last run, seen from `poses` f64 [F, 7] (TrajectoryReducer.poses): the chain's
        points, cell_base and cell capacity and, where its velocity solver made one, vel_weight (movers at 0)."""
        if chain.pc is None:
            raise ValueError('GridMap.update_chain needs a chain built with point_cloud=True')
        return self.update(chain.pc.out['points'], chain.offs['cell_base'], poses, weight=chain.vel_weight, n=chain.cell_cap)

    def logodds(self):
        """Device f32 [ny, nx]: clamp(hits l_occ - free l_free, l_min, l_max)."""
        return self.ctx.map_logodds(self.hits, self.free, **self.lo)

    def probability(self):
        """Device f32 [ny, nx]: the occupancy probability 1 / (1 + exp(-logodds))."""
        return self.ctx.torch.sigmoid(self.logodds())

    def reset(self):
        self.hits.zero_()
        if self.free is not None:
            self.free.zero_()
        self.stats = None

    def results(self):
        """Host arrays: hits u32 [ny, nx], free u32 [ny, nx] (None without a free plane), logodds f32 [ny, nx] and
        stats i32 [F, 4] of the last update (None before one)."""
        u32 = lambda t: None if t is None else t.cpu().numpy().view(np.uint32)  # noqa: E731
        return dict(hits=u32(self.hits), free=u32(self.free), logodds=self.logodds().cpu().numpy(),
                    stats=None if self.stats is None else self.stats.cpu().numpy())
