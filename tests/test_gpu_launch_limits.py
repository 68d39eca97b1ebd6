"""GPU: a block count that does not fit gridDim.x is refused by the launch, not truncated to 32 bits.
rsl_preprocess_rows launches one workgroup per row; rows = 2^32 + 1 truncates to one workgroup, which would process row
0 and report success.  The buffers hold that one row, so neither outcome leaves them."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def test_preprocess_rows_refuses_block_count_beyond_grid(ctx):
    from rsl.runtime import _ptr
    S = 8
    sentinel = np.complex64(-7.0 + 3.0j)
    d_in = ctx.to_dev(np.full(S, 1 + 2j, dtype=np.complex64))
    d_tab = ctx.to_dev(np.full(S, 2 - 1j, dtype=np.complex64))
    d_out = ctx.to_dev(np.full(S, sentinel, dtype=np.complex64))
    ctx._bind()
    with pytest.raises(RuntimeError):
        ctx.check(ctx.lib.rsl_preprocess_rows(ctx.h, _ptr(d_in), 2 ** 32 + 1, S, _ptr(d_tab), 0, _ptr(d_out)),
                  'rsl_preprocess_rows')
    ctx.sync()
    assert (d_out.cpu().numpy() == sentinel).all()
