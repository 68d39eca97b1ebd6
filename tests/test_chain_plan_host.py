"""Which Context calls RadarChain makes, in which order and with which arguments, for every configuration that changes
the sequence: the chain driven on the CPU with a stand-in for runtime.Context that records instead of launching.

Only the chain's public API is used (ChainConfig, RadarChain, run / run_front / run_back / reset_registration), at the
smallest shape that reaches every branch: A8 C16 S64, F = 2 and F = 0.  For every call the scalar arguments are compared
by value, tensors by dtype and shape ('c64[2, 8, 64, 16]'), dicts of buffers key by key, and None stays None."""
import inspect

import numpy as np
import pytest
import torch

from rsl import ChainConfig, Context, RadarChain

BASE = dict(num_antennas=8, num_chirps=16, chirp_duration=6.4e-6)  # S = 64
A, C, S = 8, 16, 64
SHORT = {torch.complex64: 'c64', torch.float32: 'f32', torch.float64: 'f64', torch.int32: 'i32', torch.int64: 'i64'}


class RecordingContext:
    """What RadarChain needs of runtime.Context, on the CPU: buffers are zeros, tables are zeros of the right shape,
    and every launcher records (name, {argument name: value}) in .calls."""
    torch = torch
    device = torch.device('cpu')

    def __init__(self):
        self.calls, self.tensors = [], []

    def empty(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype)

    def to_dev(self, a):
        return torch.from_numpy(np.ascontiguousarray(a))

    def steering(self, steer_c128):
        G, M = steer_c128.shape
        return dict(G=G, M=M, toeplitz=True, tab=torch.zeros(1), c128=torch.zeros(1, dtype=torch.float64),
                    phase=torch.zeros((G, M), dtype=torch.float64))

    def steering_sub(self, steer_c128, L):
        return torch.zeros((steer_c128.shape[0], int(L)), dtype=torch.complex64)

    def steering_c64(self, steer_c128):
        return torch.zeros(steer_c128.shape, dtype=torch.complex64)

    def __getattr__(self, name):
        if name.startswith('_'):
            raise AttributeError(name)

        def launcher(*args, **kw):  # the arguments by name, as the real launcher would bind them (TypeError if not)
            named = dict(inspect.signature(getattr(Context, name)).bind(self, *args, **kw).arguments)
            del named['self']
            self.calls.append((name, describe(named)))
            self.tensors += tensors_of(named)
            return 1 if name == 'rds_detect' else None
        return launcher


def describe(v):
    if isinstance(v, torch.Tensor):
        return f'{SHORT[v.dtype]}{list(v.shape)}'
    if isinstance(v, dict):
        return {k: describe(x) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return tuple(describe(x) for x in v)
    if isinstance(v, (bool, str)) or v is None:
        return v
    if isinstance(v, (int, np.integer)):
        return int(v)
    return float(v)


def tensors_of(v):
    if isinstance(v, torch.Tensor):
        return [v]
    if isinstance(v, dict):
        v = tuple(v.values())
    return [t for x in v for t in tensors_of(x)] if isinstance(v, (tuple, list)) else []


def chain(F=2, **kw):
    ctx = RecordingContext()
    return RadarChain(ChainConfig(**BASE, **kw), F, ctx), ctx


def cube(F=2):
    return torch.zeros((F, A, C, S), dtype=torch.complex64)


# --- the buffers and tables the calls are handed, by what describe() makes of them (F = 2; cc = the cell capacity) ----
F = 2
CC = (F * S * C + 64 + 3) & ~3
G = 361
RDS, WORK, TABLE = f'c64[{F}, {A}, {S}, {C}]', f'c64[{F}, {A}, {C}, {S}]', f'c64[{S}]'
DET_A = dict(mask=f'i64[{F}, {A}, {S}, 1]', row_count=f'i32[{F}, {A}, {S}]', peak_pow=f'f32[{F}, {A}, {S}, {C}]')
DET_1 = dict(mask=f'i64[{F}, 1, {S}, 1]', row_count=f'i32[{F}, 1, {S}]', peak_pow=f'f32[{F}, 1, {S}, {C}]')
POWER = f'f32[{F}, {S}, {C}]'


def offs(da):
    return dict(entry_row_off=f'i32[{F * da * S}]', cell_row_off=f'i32[{F * S}]', scratch=f'i32[{F * S}]',
                entry_base=f'i64[{F + 1}]', cell_base=f'i64[{F + 1}]', frame_counts=f'i64[{2 * F}]',
                union_mask=f'i64[{F}, {S}, 1]')


def lists(da):
    ec = int(np.ceil(0.20 * F * da * S * C)) + 64
    return ec, dict(e_coord=f'i32[{ec}]', e_cell=f'i32[{ec}]', e_pdb=f'f32[{ec}]', c_frame=f'i32[{CC}]',
                    c_rc=f'i32[{CC}]', c_amask=f'i32[{CC}]')


STEER = dict(G=G, M=A, toeplitz=True, tab='f32[1]', c128='f64[1]', phase=f'f64[{G}, {A}]')
EXT = dict(esprit=f'f64[{CC}]', phase=f'f64[{CC}]', az=f'f64[{CC}]')
PC = dict(points=f'f32[{CC}, 8]', az=f'f64[{CC}]')
KEEP = dict(points=f'f32[{S * C}, 8]', rc=f'i32[{S * C}]', n_dev='i64[1]')


def expect(ch, *, da=A, detector=None, esprit=True, velocity=True, doa='fused', before=(), solver='ls',
           az='grid', weight=False, after=(), prev=None):
    """The calls of one whole run of `ch` (F = 2), from the parent's RadarChain, every argument by its name in
    runtime.Context: `da` antenna maps of the detector, `detector` the calls after rds_detect, `before` / `after` the
    optional stages around the velocity solve."""
    cfg = ch.cfg
    gate = dict(thr_power=ch.thr_p, i_lo=ch.i_lo, i_hi=ch.i_hi)
    det = DET_1 if da == 1 else DET_A
    ec, ls = lists(da)
    out = [('rds_detect', dict(cube=WORK, table=TABLE, **gate, rds=RDS, work=WORK, dc_removal=True, **DET_A))]
    if detector == 'cfar':
        out.append(('detect_cfar', dict(rds=RDS, guard=(2, 2), train=(8, 8), alpha=ch.cfar_alpha, **gate, out=DET_A,
                                        method=cfg.cfar_method, rank=0.75)))
    elif detector is not None:  # on the summed map: 'threshold' / 'ca' / 'os'
        out.append(('integrate_power', dict(rds=RDS, out=POWER)))
        out.append(('detect_power', dict(power=POWER, rule=detector, guard=(2, 2), train=(8, 8), rank=0.75,
                                         alpha=1.0 if detector == 'threshold' else ch.cfar_alpha, **gate, out=DET_1)))
    out.append(('offsets', dict(mask=det['mask'], row_count=det['row_count'], C=C, bufs=offs(da))))
    out.append(('emit', dict(rds=RDS, mask=det['mask'], offs=offs(da), entry_cap=ec, cell_cap=CC, want_pdb=True,
                             bufs=ls, peak_pow=det['peak_pow'], peak_pow_group=1)))
    cells = dict(rds=RDS, c_frame=f'i32[{CC}]', c_rc=f'i32[{CC}]', n=CC, n_dev='i64[1]')
    if doa == 'fused':
        out.append(('doa_extras', dict(cells, steer=STEER, method=ch.method, esprit_scale=ch.esprit_scale,
                                       out_idx=f'i32[{CC}]', esprit=EXT['esprit'] if esprit else None,
                                       phase=EXT['phase'] if velocity else None)))
    else:
        out.append(('doa', dict(cells, steer=STEER, method=ch.method, out_idx=f'i32[{CC}]', want_spec=True,
                                spec_blocked=True, out_spec=f'f32[{(CC + 31) // 32}, {G}, 32]')))
        if esprit or velocity:
            out.append(('cell_extras', dict(cells, esprit_scale=ch.esprit_scale, want_esprit=esprit,
                                            want_phase=velocity, bufs=EXT)))
    axes = (0.0, 0.15 * S / (S - 1), -5e6, 1e7 / (C - 1))
    for stage in before:
        if stage == 'ss':
            out.append(('doa_smoothed', dict(cells, steer_sub=f'c64[{G}, 6]', nmax=3, num_sources=0, rel=0.05,
                                             out=dict(nsrc=f'i32[{CC}]', idx=f'i32[{CC}, 3]', den=f'f32[{CC}, 3]'))))
        elif stage == 'ra':
            cov = f'c64[{F}, {S}, {A}, {A}]'
            out.append(('range_cov', dict(rds=RDS, doppler=(0, C), out=cov)))
            out.append(('range_azimuth', dict(cov=cov, steer_c64=f'c64[{G}, {A}]', method='capon', loading=1e-2,
                                              out=dict(map=f'f32[{F}, {S}, {G}]', arg=f'i32[{F}, {S}]'))))
        elif stage == 'integrate':
            out.append(('integrate_power', dict(rds=RDS, out=POWER)))
        elif stage == 'pc':
            out.append(('cell_refine', dict(cells, gidx=f'i32[{CC}]', az_table=f'f64[{G}]', steer_c64=f'c64[{G}, {A}]',
                                            power=POWER, range_mode='hann', doppler_mode='rect', axes=axes, out=PC)))
    if not velocity:
        return out
    w = f'f32[{CC}]' if weight else None
    prob = dict(az=None, y=EXT['phase'], seg=f'i64[{F + 1}]', k=ch.k, ridge=0.0, bounds=(-50.0, 50.0, -50.0, 50.0),
                amask=f'i32[{CC}]', out=f'f64[{F}, 8]', gidx=f'i32[{CC}]', az_table=f'f64[{G}]', n=CC)
    if az == 'refined':
        prob.update(az=f'f64[{CC}]', gidx=None, az_table=None)
    if solver == 'ls':
        out.append(('velocity', prob))
    elif solver == 'consensus':
        out.append(('velocity_consensus', dict(prob, scale=0.3, c=None, hyps=256, min_det=0.1, refine=3, seed=0,
                                               frame0=0, want_weight=w)))
    else:
        out.append(('velocity_robust', dict(prob, loss=solver, c=None, scale=None, iters=30, tol=1e-9,
                                            want_weight=w)))
    if 'reg' in after:
        out.append(('scan_register', dict(
            points=PC['points'], seg=f'i64[{F + 1}]', weight=w, rc=f'i32[{CC}]', C=C, axes=axes, prev=prev,
            init=f'f64[{F}, 3]', h=0.5, h_coarse=1.0, dtheta=np.radians(0.25), k=20, iters=10, shrink=0.7, tol=1e-9,
            w_min=3.0, dt=0.1, n=CC, out=dict(rows=f'f64[{F}, 8]', omega=f'f64[{F}, 3]'))))
    return out


ALL_ON = dict(detect_on='sum', multi_source=True, ra_map='capon', point_cloud=True, registration=True,
              velocity_loss='tukey', velocity_az='refined')
# name: (ChainConfig fields, run() arguments, expect() arguments)
RUNS = {
    'default': ({}, {}, {}),
    'spectrum': (dict(spectrum=True), {}, dict(doa='scan')),
    'cfar': (dict(detector='cfar'), {}, dict(detector='cfar')),
    'oscfar_sum': (dict(detector='cfar', cfar_method='os', detect_on='sum'), {}, dict(da=1, detector='os')),
    'everything': (ALL_ON, {}, dict(da=1, detector='threshold', before=('ss', 'ra', 'pc'), solver='tukey',
                                    az='refined', weight=True, after=('reg',))),
    'cloud_consensus': (dict(point_cloud=True, velocity_loss='consensus', velocity_scale=0.3), {},
                        dict(before=('integrate', 'pc'), solver='consensus', weight=True)),
    'no_velocity': (dict(point_cloud=True, registration=True), dict(velocity=False),
                    dict(velocity=False, before=('integrate', 'pc'))),
    'no_esprit': ({}, dict(esprit=False), dict(esprit=False)),
    'scan_no_extras': (dict(spectrum=True), dict(esprit=False, velocity=False),
                       dict(doa='scan', esprit=False, velocity=False)),
    'scan_phase_only': (dict(spectrum=True), dict(esprit=False), dict(doa='scan', esprit=False)),
}
NAMES = {
    'default': 'rds_detect offsets emit doa_extras velocity',
    'spectrum': 'rds_detect offsets emit doa cell_extras velocity',
    'cfar': 'rds_detect detect_cfar offsets emit doa_extras velocity',
    'oscfar_sum': 'rds_detect integrate_power detect_power offsets emit doa_extras velocity',
    'everything': 'rds_detect integrate_power detect_power offsets emit doa_extras doa_smoothed range_cov '
                  'range_azimuth cell_refine velocity_robust scan_register',
    'cloud_consensus': 'rds_detect offsets emit doa_extras integrate_power cell_refine velocity_consensus',
    'no_velocity': 'rds_detect offsets emit doa_extras integrate_power cell_refine',
    'no_esprit': 'rds_detect offsets emit doa_extras velocity',
    'scan_no_extras': 'rds_detect offsets emit doa',
    'scan_phase_only': 'rds_detect offsets emit doa cell_extras velocity',
}


def same(calls, want):
    assert [c[0] for c in calls] == [w[0] for w in want]
    for (name, got), (_, exp) in zip(calls, want):
        assert set(got) == set(exp), (name, sorted(set(got) ^ set(exp)))
        for k in exp:
            assert got[k] == exp[k], (name, k, got[k], exp[k])


@pytest.mark.parametrize('name', list(RUNS))
def test_calls_of_one_run(name):
    kw, run, exp = RUNS[name]
    ch, ctx = chain(**kw)
    ch.run(cube(), **run)
    assert ' '.join(c[0] for c in ctx.calls) == NAMES[name]
    same(ctx.calls, expect(ch, **exp))


def test_the_shapes_are_the_ones_the_expectations_assume():
    ch, _ = chain()
    assert (ch.A, ch.C, ch.S, ch.F, ch.cell_cap, len(ch.grid)) == (A, C, S, F, CC, G)
    assert ch.fused_doa and ch.cfar_alpha is None
    ch, _ = chain(spectrum=True)
    assert not ch.fused_doa and ch.spectrum_shape() == ((CC + 31) // 32, G, 32)


def test_split_run_is_the_default_sequence():
    """run_front(emit=False, offsets=False) + run_back(emit=True, offsets=True): the same calls as run()."""
    for kw, exp in (({}, {}), (dict(detector='cfar'), dict(detector='cfar')),
                    (dict(detect_on='sum'), dict(da=1, detector='threshold'))):
        ch, ctx = chain(**kw)
        ch.run_front(cube(), emit=False, offsets=False)
        n = len(ctx.calls)
        assert [c[0] for c in ctx.calls] == [w[0] for w in expect(ch, **exp)][:n] and ctx.calls[-1][0] != 'offsets'
        ch.run_back(emit=True, offsets=True)
        same(ctx.calls, expect(ch, **exp))
    # the compaction alone left to the back half
    ch, ctx = chain()
    ch.run_front(cube(), emit=False)
    assert [c[0] for c in ctx.calls] == ['rds_detect', 'offsets']
    ch.run_back(emit=True)
    same(ctx.calls, expect(ch))


@pytest.mark.parametrize('kw', [ALL_ON, dict(spectrum=True, velocity_loss='huber')], ids=['everything', 'spectrum'])
def test_buffers_swapped_on_the_chain_are_the_ones_launched(kw):
    """lists, gidx, ext and spec are read from the chain at every run: a caller may put another buffer there between
    runs (the benchmark rotates chain.spec, the overflow test lengthens the lists)."""
    ch, ctx = chain(**kw)
    held = lambda: list(ch.lists.values()) + [ch.ext['esprit'], ch.ext['phase'], ch.gidx] + [
        t for t in (ch.spec,) if t is not None]
    launched = lambda t: any(t is x for x in ctx.tensors)
    ch.run(cube())
    old = held()
    assert all(launched(t) for t in old)
    for d in (ch.lists, ch.ext):
        for k in d:
            d[k] = torch.zeros((d[k].shape[0] + 8,), dtype=d[k].dtype)
    ch.gidx = torch.zeros((CC + 8,), dtype=torch.int32)
    if ch.spec is not None:
        ch.spec = torch.zeros_like(ch.spec)
    del ctx.calls[:], ctx.tensors[:]
    ch.run(cube())
    assert all(launched(t) for t in held()) and not any(launched(t) for t in old)


@pytest.mark.parametrize('kw', [{}, ALL_ON, dict(detector='cfar', spectrum=True)], ids=['default', 'all', 'cfar'])
def test_empty_batch_launches_the_offsets_only(kw):
    ch, ctx = chain(F=0, **kw)
    ch.run(cube(0))
    da = 1 if kw.get('detect_on') == 'sum' else A
    assert ctx.calls == [('offsets', dict(mask=f'i64[0, {da}, {S}, 1]', row_count=f'i32[0, {da}, {S}]', C=C, bufs=dict(
        entry_row_off='i32[0]', cell_row_off='i32[0]', scratch='i32[0]', entry_base='i64[1]', cell_base='i64[1]',
        frame_counts='i64[0]', union_mask=f'i64[0, {S}, 1]')))]
    ch.run_back(emit=True, offsets=True)
    assert len(ctx.calls) == 1


@pytest.mark.parametrize('loss', ['ls', 'huber'])
def test_registration_keeps_the_last_cloud_between_runs(loss):
    """The first scan_register has no previous cloud, the next one the cloud kept from the run before (with the
    solver's weights where it makes them), and reset_registration() forgets it."""
    ch, ctx = chain(point_cloud=True, registration=True, velocity_loss=loss)
    keep = dict(KEEP, weight=f'f32[{S * C}]' if loss != 'ls' else None)
    exp = dict(before=('integrate', 'pc'), solver=loss, weight=loss != 'ls', after=('reg',))
    for prev in (None, keep, keep):
        del ctx.calls[:]
        ch.run(cube())
        same(ctx.calls, expect(ch, prev=prev, **exp))
    ch.reset_registration()
    for prev in (None, keep):
        del ctx.calls[:]
        ch.run(cube())
        same(ctx.calls, expect(ch, prev=prev, **exp))
    assert tuple(ch.omega.shape) == (F, 3) and ch.omega.dtype == torch.float64
    off, _ = chain(point_cloud=True)
    assert off.omega is None
    off.reset_registration()  # nothing to forget, no error


def test_guarded_chain_covers_every_stage_buffer():
    """guard=True: the same calls, and every tensor they are handed lies inside a guarded allocation (GUARD_BYTES of
    pad on both sides) except the cube and the uploaded tables; the pads are untouched."""
    from rsl.chain import GUARD_BYTES
    ctx = RecordingContext()
    ch = RadarChain(ChainConfig(**BASE, **ALL_ON), F, ctx, guard=True)
    ch.run(cube())
    same(ctx.calls, expect(ch, da=1, detector='threshold', before=('ss', 'ra', 'pc'), solver='tukey', az='refined',
                           weight=True, after=('reg',)))
    assert ch.guard_violations() == []

    def guarded(t):
        lo = t.storage_offset() * t.element_size()
        return lo >= GUARD_BYTES and t.untyped_storage().nbytes() - lo - t.numel() * t.element_size() >= GUARD_BYTES
    bare = {describe(t) for t in ctx.tensors if not guarded(t)}
    assert bare == {WORK, TABLE, f'f64[{G}]', f'c64[{G}, {A}]', f'c64[{G}, 6]', 'f32[1]', 'f64[1]', f'f64[{G}, {A}]'}
    assert sum(guarded(t) for t in ctx.tensors) >= 60
