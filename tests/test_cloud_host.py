"""CPU: the one check every consumer of a point cloud makes (rsl.runtime.check_cloud) on CPU torch tensors, and the row
layout stated once on each side: RSL_POINT_* in include/rsl.h against ops.POINT_COLUMNS."""
import os
import re

import pytest
import torch

from rsl import ops
from rsl.runtime import check_cloud

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Allocator:
    """Stands in for Context.empty: counts the calls."""

    def __init__(self):
        self.calls = []

    def __call__(self, shape, dtype):
        self.calls.append((tuple(shape), dtype))
        return torch.empty(shape, dtype=dtype)


def cloud(rows=10, frames=3):
    return (torch.zeros((rows, 8), dtype=torch.float32), torch.arange(frames + 1, dtype=torch.int64),
            torch.ones(rows, dtype=torch.float32))


@pytest.mark.parametrize('fn', ['scan_register', 'map_update'])
def test_good_cloud_and_row_count(fn):
    points, seg, weight = cloud()
    alloc = Allocator()
    for n, want in ((None, 10), (4, 4), (10, 10), (25, 10)):  # N = min(n, rows)
        got, N = check_cloud(fn, points, seg, n, weight, alloc)
        assert got is points and N == want
    assert check_cloud(fn, points, seg, None, None, alloc) == (points, 10)
    assert check_cloud(fn, points, seg[:1], None, weight, alloc)[1] == 10  # F = 0
    assert check_cloud(fn, points, None, 7, weight[:7], alloc, 'prev ')[1] == 7  # a cloud without segments
    assert not alloc.calls


def test_empty_points_get_a_stand_in():
    points, seg, _ = cloud(rows=0)
    alloc = Allocator()
    got, N = check_cloud('map_update', points, seg, None, torch.ones(0, dtype=torch.float32), alloc)
    assert N == 0 and tuple(got.shape) == (1, 8) and got.dtype == torch.float32
    assert alloc.calls == [((1, 8), torch.float32)]


@pytest.mark.parametrize('fn', ['scan_register', 'map_update'])
def test_bad_clouds_are_refused(fn):
    points, seg, weight = cloud()
    alloc = Allocator()
    bad = {
        'points [N, 7]': dict(points=points[:, :7].contiguous()),
        'float64 points': dict(points=points.double()),
        'non-contiguous points': dict(points=torch.zeros((10, 16), dtype=torch.float32)[:, ::2]),
        'int32 seg': dict(seg=seg.to(torch.int32)),
        'two-axis seg': dict(seg=seg.reshape(2, 2)),
        'non-contiguous seg': dict(seg=torch.arange(8, dtype=torch.int64)[::2]),
        'empty seg': dict(seg=seg[:0]),
        'short weight': dict(weight=weight[:9]),
        'float64 weight': dict(weight=weight.double()),
    }
    for what, kw in bad.items():
        args = dict(points=points, seg=seg, n=None, weight=weight)
        args.update(kw)
        with pytest.raises(ValueError, match=f'^{fn}: '):
            check_cloud(fn, args['points'], args['seg'], args['n'], args['weight'], alloc)
            pytest.fail(what + ' accepted')
    # a weight as long as the rows in use is enough
    assert check_cloud(fn, points, seg, 9, weight[:9], alloc)[1] == 9
    with pytest.raises(ValueError, match='prev points'):
        check_cloud(fn, points.double(), None, None, None, alloc, 'prev ')
    with pytest.raises(ValueError, match='prev weight'):
        check_cloud(fn, points, None, None, weight[:9], alloc, 'prev ')
    assert not alloc.calls


def test_header_layout_is_point_columns():
    src = open(os.path.join(ROOT, 'include', 'rsl.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    ids = {m.group(1): int(m.group(2)) for m in re.finditer(r'^#define RSL_POINT_([A-Z_]+) (\d+)\s*$', src, flags=re.M)}
    assert ids.pop('COLS') == len(ops.POINT_COLUMNS) == 8
    assert ids == {name.upper(): i for i, name in enumerate(ops.POINT_COLUMNS)}
