"""GPU: the scene kernels (rsl_scene.hip) on inputs built directly, against tests/scene_ref.py.

rsl_peak_topk          one launch over many cubes given as entry_base / e_coord / e_pdb: every entry count around kmax,
                       the 256-thread chunking and several entries per thread; distinct, all-equal and 0.5-dB-quantised
                       powers (ties at the cut); the threshold's edges; one NaN; +0 / -0; the entry_cap clamp.  The
                       selection is exact against Python's own stable sort (scene_ref.topk_ref).
rsl_associate_nearest  a batch with empty, single-target and several-workgroup frames, planted exact ties and d == thr;
                       match exact against the oracle's associate_analyzer; dist bit-exact against the same rule with
                       IEEE products for the squares (scene_ref.associate_ieee: the oracle's ``** 2`` is libm's pow,
                       an ulp off x * x now and then); phase within 1e-14 rad (the device atan2 is not correctly
                       rounded: a few ulp at pi is 1e-15).
"""
import ctypes

import numpy as np
import pytest

import scene_ref as R

pytestmark = pytest.mark.gpu

C = 8192  # Doppler cells per range row: rc = range_bin * C + doppler_bin with 13-bit bins


# -- rsl_peak_topk ----------------------------------------------------------------------------------------------------
def _cubes(kmax, thr_db):
    """[(name, pdb f32 [n])]: the cubes of one launch."""
    rs = np.random.RandomState(100 + kmax)
    out = []
    counts = sorted({0, 1, max(kmax - 1, 0), kmax, kmax + 1, 255, 256, 257, 1000, 5000})
    for n in counts:
        out.append((f'distinct n={n}', rs.permutation(np.linspace(-60.0, 10.0, n + 2)[1:-1])))  # both signs of dB
        out.append((f'equal n={n}', np.full(n, -3.25)))
        out.append((f'quantised n={n}', np.round(rs.uniform(-40.0, 10.0, n) * 2) / 2))  # many below the threshold too
    t32 = np.float32(thr_db)
    lo32, hi32 = np.nextafter(t32, np.float32(-np.inf)), np.nextafter(t32, np.float32(np.inf))
    v = np.full(1000, float(lo32))
    v[rs.choice(1000, kmax, replace=False)] = rs.uniform(-20.0, 0.0, kmax)
    out.append(('exactly kmax above thr', v))
    # the f32 nearest thr_db and its two neighbours (thr_db itself where it is an f32: excluded by the strict '>')
    out.append(('threshold edge', np.tile(np.array([t32, lo32, hi32], np.float32), 40)))
    v = rs.uniform(-20.0, 0.0, 600)
    v[123] = np.nan
    out.append(('one NaN', v))
    out.append(('signed zeros', rs.choice(np.array([0.0, -0.0, 1.5, -1.5], np.float32), 700)))
    out.append(('cut by entry_cap', rs.uniform(-20.0, 0.0, 300)))
    out.append(('past entry_cap', rs.uniform(-20.0, 0.0, 300)))
    return [(name, np.asarray(p, np.float32)) for name, p in out]


@pytest.fixture(scope='module')
def topk_cases():
    cache = {}

    def get(kmax, thr_db):
        if (kmax, thr_db) not in cache:
            rs = np.random.RandomState(7)
            cubes = _cubes(kmax, thr_db)
            base = np.concatenate([[0], np.cumsum([len(p) for _, p in cubes])]).astype(np.int64)
            cap = int(base[-2]) - 120  # inside the last cube but one
            pdb = np.concatenate([p for _, p in cubes])
            rbin, dbin = rs.randint(0, 8192, len(pdb)), rs.randint(0, 8192, len(pdb))
            ant = rs.randint(1, 64, len(pdb))  # non-zero bits above bit 26: they must not leak into rc
            coord = ((ant.astype(np.uint64) << 26) | (rbin.astype(np.uint64) << 13) | dbin.astype(np.uint64))
            want = []
            for k, (name, p) in enumerate(cubes):
                b0, b1 = min(int(base[k]), cap), min(int(base[k + 1]), cap)
                want.append(np.array(R.topk_ref(pdb[b0:b1], thr_db, kmax), np.int64) + b0)
            cache[kmax, thr_db] = (cubes, base, cap, pdb, coord.astype(np.uint32), rbin * C + dbin, want)
        return cache[kmax, thr_db]
    return get


@pytest.mark.parametrize('thr_db', [-25.0, -25.1])  # -25.1 is not an f32: its two f32 neighbours fall on either side
@pytest.mark.parametrize('kmax', [1, 50, 256])
def test_peak_topk(ctx, topk_cases, kmax, thr_db):
    cubes, base, cap, pdb, coord, rc, want = topk_cases(kmax, thr_db)
    assert len(want[-1]) == 0 and 0 < len(want[-2]) <= 180  # the clamp is exercised
    se, sf, sr, sn = ctx.peak_topk(ctx.to_dev(base), cap, ctx.to_dev(coord.view(np.int32)), ctx.to_dev(pdb),
                                   thr_db=thr_db, kmax=kmax, C=C)
    se, sf, sr, sn = (t.cpu().numpy() for t in (se, sf, sr, sn))
    ncube = len(cubes)
    se, sf, sr = se.reshape(ncube, kmax), sf.reshape(ncube, kmax), sr.reshape(ncube, kmax)
    assert np.array_equal(sf, np.repeat(np.arange(ncube), kmax).reshape(ncube, kmax))
    for k, (name, p) in enumerate(cubes):
        n = len(want[k])
        assert sn[k] == n, (name, int(sn[k]), n)
        assert np.array_equal(se[k, :n], want[k]), (name, se[k, :n], want[k])
        assert np.array_equal(sr[k, :n], rc[want[k]]), name
        assert (se[k, n:] == -1).all() and (sr[k, n:] == 0).all(), name
    by_name = {name: len(w) for (name, _), w in zip(cubes, want)}
    assert by_name['exactly kmax above thr'] == kmax and by_name['threshold edge'] == min(40, kmax)


@pytest.mark.parametrize('kmax', [0, 257])
def test_peak_topk_kmax_unsupported(ctx, kmax):
    """kmax outside 1..256: the unsupported-argument error, and nothing is launched (the outputs keep their contents)."""
    from rsl import _lib
    from rsl.runtime import _ptr
    torch = ctx.torch
    base = ctx.to_dev(np.array([0, 4], np.int64))
    coord = ctx.to_dev(np.zeros(4, np.int32))
    pdb = ctx.to_dev(np.zeros(4, np.float32))
    outs = [torch.full((300,), 7777, dtype=torch.int32, device=ctx.device) for _ in range(4)]
    ctx._bind()
    rcode = ctx.lib.rsl_peak_topk(ctx.h, _ptr(base), 4, 1, _ptr(coord), _ptr(pdb), ctypes.c_double(-25.0), kmax, C,
                                  *[_ptr(o) for o in outs])
    assert rcode == _lib.RSL_ERR_UNSUPPORTED
    ctx.sync()
    assert all(bool((o == 7777).all()) for o in outs)
    with pytest.raises(ValueError, match='kmax'):
        ctx.peak_topk(base, 4, coord, pdb, thr_db=-25.0, kmax=kmax, C=C)


# -- rsl_associate_nearest --------------------------------------------------------------------------------------------
COUNTS = [0, 1, 3, 0, 0, 300, 700, 2]  # an empty first frame, consecutive empty frames, an empty previous frame, > 256
THR = 5.0


def _batch():
    """Targets of 8 frames.  The bulk lies within 200 m: half on a 0.5 m x 0.25 rad lattice (exact distance ties between
    different previous targets arise by themselves), half continuous.  Planted cases sit alone beyond 400 m."""
    rs = np.random.RandomState(11)
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int64)
    N = int(off[-1])
    r = np.where(rs.rand(N) < 0.5, rs.randint(0, 400, N) * 0.5, rs.uniform(0.0, 200.0, N))
    a = np.where(rs.rand(N) < 0.5, rs.randint(-6, 7, N) * 0.25, rs.uniform(-1.5, 1.5, N))
    r[off[5]:off[6]] *= 0.5  # previous targets within 100 m: current targets beyond 105 m stay unmatched
    s0 = rs.randn(N) + 1j * rs.randn(N)
    p, c = int(off[5]), int(off[6])  # previous frame 5 (300 targets), current frame 6 (700 targets)
    planted = {}
    # duplicate previous targets: the lower index wins
    r[p + 10], a[p + 10] = 500.0, 0.3
    r[p + 20], a[p + 20] = 500.0, 0.3
    r[c + 5], a[c + 5] = 501.0, 0.1
    planted['duplicate'] = (c + 5, 10)
    # two previous targets at exactly the same distance on either side, the farther index first in range
    r[p + 31], a[p + 31] = 600.5, -0.5
    r[p + 30], a[p + 30] = 599.5, -0.5
    r[c + 6], a[c + 6] = 600.0, -0.5
    planted['either side'] = (c + 6, 30)
    # d == thr exactly: no match; one ulp inside: a match
    r[p + 40], a[p + 40] = 705.0, 1.0
    r[c + 7], a[c + 7] = 700.0, 1.0
    planted['d == thr'] = (c + 7, -1)
    r[p + 50], a[p + 50] = np.nextafter(5.0, 0.0), 0.75
    r[c + 8], a[c + 8] = 0.0, 0.75
    r[p:c][(np.abs(r[p:c]) < 12) & (np.arange(300) != 50)] += 50.0  # keep target 50 alone near the origin
    planted['ulp inside'] = (c + 8, 50)
    # a current target on top of a previous one: d = 0 (matches at any thr > 0, never at thr = 0)
    r[p + 60], a[p + 60] = 800.0, 0.0
    r[c + 9], a[c + 9] = 800.0, 0.0
    planted['coincident'] = (c + 9, 60)
    # frame 2's targets around frame 1's only target
    r[off[1]], a[off[1]] = 50.0, 0.0
    r[off[2]:off[3]] = [52.0, 56.0, 50.0]
    a[off[2]:off[3]] = [0.5, 0.0, 0.0]
    return off, r, a, s0, planted


@pytest.fixture(scope='module')
def batch():
    off, r, a, s0, planted = _batch()
    return off, r, a, s0, planted, {thr: R.nearest_ref(r, a, s0, off, thr) for thr in (THR, 0.0)}


@pytest.mark.parametrize('thr', [THR, 0.0])
def test_associate_nearest(ctx, batch, thr):
    off, r, a, s0, planted, refs = batch
    m_ref, d_orc, m_ieee, d_ref, ph_ref = refs[thr]
    # the two restatements agree on this batch: the same matches, distances within an ulp
    assert np.array_equal(m_ref, m_ieee) and np.array_equal(np.isinf(d_orc), np.isinf(d_ref))
    hit = m_ref >= 0
    assert (np.abs(d_orc[hit] - d_ref[hit]) <= np.spacing(d_ref[hit])).all()
    if thr > 0:  # the planted cases are what they claim to be, in the reference
        for name, (i, j) in planted.items():
            assert m_ref[i] == j, (name, m_ref[i])
        assert d_ref[planted['ulp inside'][0]] < thr and np.isinf(d_ref[planted['d == thr'][0]])
        assert (m_ref[off[6]:off[7]] == -1).sum() > 50 and (m_ref[off[6]:off[7]] >= 0).sum() > 256
        assert list(m_ref[off[2]:off[3]]) == [0, -1, 0]
    else:
        assert (m_ref == -1).all()
    match, dist, phase = ctx.associate_nearest(ctx.to_dev(r), ctx.to_dev(a), ctx.to_dev(s0.view(np.float64)),
                                               ctx.to_dev(off), thr=thr)
    match, dist, phase = match.cpu().numpy(), dist.cpu().numpy(), phase.cpu().numpy()
    bad = np.nonzero(match != m_ref)[0]
    assert len(bad) == 0, (bad[:8], match[bad[:8]], m_ref[bad[:8]])
    assert np.array_equal(dist.view(np.int64), d_ref.view(np.int64)), np.nonzero(dist != d_ref)[0][:8]
    assert np.isinf(dist[m_ref < 0]).all() and (phase[m_ref < 0] == 0.0).all()
    assert np.abs(phase - ph_ref).max() <= 1e-14
    assert (match[:off[2]] == -1).all() and (match[off[5]:off[6]] == -1).all()  # no previous frame / an empty one
