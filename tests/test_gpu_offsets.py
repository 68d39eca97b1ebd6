"""rsl_peak_offsets (k_offsets + k_frame_scan) on random mask words against numpy: per-frame exclusive scans of the row
counts over (antenna, range), the union over antennas with its per-row counts and scan, and the bases over frames."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [  # (F, A, S, W)
    (300, 2, 24, 1),   # more frames than k_frame_scan has threads
    (3, 8, 512, 2),    # the 16-B union path and the int4 scan, 4 per thread
    (2, 3, 100, 3),    # scalar paths, W not a power of two
    (1, 2, 8192, 1),   # 16 int4 per thread: the second-pass loop past q = 8
]


def popcount(words):
    """Set bits of every u64 word."""
    w = np.ascontiguousarray(words)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape + (8,)), axis=-1).sum(-1).astype(np.int64)


def exclusive(x):
    return np.cumsum(x, axis=1) - x


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'F%d_A%d_S%d_W%d' % s)
def test_offsets_against_numpy(ctx, shape):
    F, A, S, W = shape
    rng = np.random.default_rng(F * 1000 + S)
    word = lambda: rng.integers(0, 1 << 64, size=(F, A, S, W), dtype=np.uint64)
    mask = word() & word()   # a quarter of the bits set, the top bit included
    mask[:, :, ::7] = 0      # some empty rows
    rows = popcount(mask).sum(-1)  # [F, A, S]
    offs = ctx.offsets(ctx.to_dev(mask.view(np.int64)), ctx.to_dev(rows.astype(np.int32)), 64 * W)
    ctx.torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in offs.items()}

    union = np.bitwise_or.reduce(mask, axis=1)  # [F, S, W]
    cells = popcount(union).sum(-1)             # [F, S]
    assert (got['union_mask'].view(np.uint64) == union).all()
    assert (got['scratch'].reshape(F, S) == cells).all()
    assert (got['entry_row_off'].reshape(F, A * S) == exclusive(rows.reshape(F, A * S))).all()
    assert (got['cell_row_off'].reshape(F, S) == exclusive(cells)).all()
    te, tc = rows.reshape(F, -1).sum(1), cells.sum(1)
    assert te.min() > 0 and tc.min() > 0
    assert (got['frame_counts'].reshape(F, 2) == np.stack([te, tc], 1)).all()
    assert (got['entry_base'] == np.concatenate([[0], np.cumsum(te)])).all()
    assert (got['cell_base'] == np.concatenate([[0], np.cumsum(tc)])).all()
