"""GPU: Context.call, the one path from Python into librsl's status-returning entry points, on the smallest shapes:
the same launch as the Context method, the status mapped to the same exceptions, and the checks it makes before the
library is entered."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (1, 2, 4, 8)  # F, A, S, C


def rds_of(ctx):
    rs = np.random.RandomState(5)
    return ctx.to_dev((rs.randn(*SHAPE) + 1j * rs.randn(*SHAPE)).astype(np.complex64))


def test_call_equals_method(ctx):
    torch = ctx.torch
    rds = rds_of(ctx)
    out = torch.full(SHAPE[:1] + SHAPE[2:], float('nan'), dtype=torch.float32, device=ctx.device)
    assert ctx.call('rsl_power_integrate', rds, 1, 2, 4, 8, out) is None
    want = ctx.integrate_power(rds)
    torch.cuda.synchronize()
    assert torch.equal(out, want) and bool(torch.isfinite(out).all())
    z = rds.cpu().numpy().astype(np.complex128)
    assert np.allclose(out.cpu().numpy(), (np.abs(z) ** 2).sum(axis=1), rtol=1e-6)


def test_status_maps_to_value_error(ctx):
    rds = rds_of(ctx)
    out = ctx.empty((1, 4, 8), ctx.torch.float32)
    with pytest.raises(ValueError, match=r'^rsl_power_integrate: \S') as e:  # A = 0: refused on the host, no launch
        ctx.call('rsl_power_integrate', rds, 1, 0, 4, 8, out)
    assert 'is a tensor on' not in str(e.value)  # the library's message, not call's own check


def test_host_tensor_is_refused_before_the_library(ctx):
    rds = rds_of(ctx)
    out = ctx.empty((1, 4, 8), ctx.torch.float32)
    ctx.call('rsl_power_integrate', rds, 1, 2, 4, 8, out)
    ctx.torch.cuda.synchronize()
    before = out.clone()
    # A = 0 as well: had the library been entered, the message would be its own
    with pytest.raises(ValueError, match=r'^rsl_power_integrate: argument 1 is a tensor on cpu, not on cuda:0$'):
        ctx.call('rsl_power_integrate', rds.cpu(), 1, 0, 4, 8, out)
    with pytest.raises(ValueError, match=r'^rsl_power_integrate: argument 6 is a tensor on cpu, not on cuda:0$'):
        ctx.call('rsl_power_integrate', rds, 1, 2, 4, 8, out.cpu())
    ctx.torch.cuda.synchronize()
    assert ctx.torch.equal(out, before)


def test_argument_count(ctx):
    rds = rds_of(ctx)
    with pytest.raises(TypeError, match=r'^rsl_power_integrate: 6 arguments after the handle expected, 5 given$'):
        ctx.call('rsl_power_integrate', rds, 1, 2, 4, 8)
    with pytest.raises(KeyError):
        ctx.call('rsl_version')
