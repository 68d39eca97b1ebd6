"""CPU: the numpy oracle of the consensus velocity solve (tests/vel_consensus_ref.py) on the scene it is meant for, the
index rule of its draws, and the host-side surface of the feature (ChainConfig fields, the ctypes row, the header's
constants).  The GPU parity is tests/test_gpu_vel_consensus.py."""
import os
import re

import numpy as np
import pytest

import philox_ref as P
import vel_consensus_ref as C
import vel_robust_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('seed', [0, 2])
def test_oracle_finds_the_minority_motion(seed):
    """600 cells on the 361-point grid, populations 0.4 / 0.2 / 0.2 / 0.2 with four motions, phase noise 0.05,
    multiplicities 0 .. 8 (scene(): grid indices, labels, noise, multiplicities drawn in that order).  Consensus
    (scale 0.05, c 3, 256 hypotheses, Philox seed 7, refine 3) lands within 1e-4 of the 40 % population's motion
    (measured 2.2e-5 and 2.0e-5) where Tukey IRLS with the same scale locks onto a mixture and misses it by more than
    1e-3 (measured 2.26e-3 and 2.15e-3); LS misses it by 2.7e-3 and 2.6e-3."""
    d = C.scene(600, seed)
    assert abs((d['label'] == 0).mean() - 0.4) < 0.05
    v = d['motions'][0]
    r = C.consensus_frame(d['az'], d['y'], d['m'], k=R.K_CHAIN, scale=0.05, c=3.0, hyps=256, seed=7, refine=3)
    rb = R.robust_frame(d['az'], d['y'], d['m'], k=R.K_CHAIN, loss='tukey', scale=0.05, iters=30, tol=1e-9)
    err, err_tukey, err_ls = (np.abs(x - v).max() for x in (r['x'], rb['x'], r['ls']))
    print(f'\nseed {seed}: consensus error {err:.2e} (best_h {r["best_h"]}, {r["n_valid"]} valid), tukey '
          f'{err_tukey:.2e}, LS {err_ls:.2e}')
    assert err < 1e-4
    assert err_tukey > 1e-3
    assert r['best_h'] >= 0 and r['n_valid'] > 0 and r['passes'] == 3
    C.assert_oracle_fit(dict(frames=[r]))
    # the winner is the valid hypothesis with the largest score, the lowest h among equals
    top = r['scores'][r['valid']].max()
    assert r['scores'][r['best_h']] == top and not (r['scores'][:r['best_h']][r['valid'][:r['best_h']]] == top).any()
    # the inlier mask is the static / moving labelling: population 0 is inside, the movers are outside
    pop0 = d['label'] == 0
    assert (d['m'][pop0] * r['weights'][pop0]).sum() >= 0.95 * d['m'][pop0].sum()
    assert (d['m'][~pop0] * r['weights'][~pop0]).sum() <= 0.25 * d['m'][~pop0].sum()
    assert r['n_in'] == (d['m'] * r['weights']).sum()


def test_index_rule_by_hand():
    """i = (x0 n) >> 32, j = (x1 (n - 1)) >> 32, j += (j >= i), on draws worked out by hand."""
    top, half = 0xFFFFFFFF, 0x80000000
    assert C.pair_from_draw(0, 0, 2) == (0, 1)            # j = 0 >= i = 0: bumped
    assert C.pair_from_draw(top, top, 2) == (1, 0)        # i = (2^33 - 2) >> 32 = 1, j = (2^32 - 1) >> 32 = 0
    assert C.pair_from_draw(half, 0, 2) == (1, 0)         # i = 2^32 >> 32 = 1
    assert C.pair_from_draw(half - 1, half, 2) == (0, 1)  # i = (2^32 - 2) >> 32 = 0, j = 0 -> 1
    assert C.pair_from_draw(half, half, 3) == (1, 2)      # i = 1.5 -> 1, j = 2^32 >> 32 = 1 >= 1 -> 2
    assert C.pair_from_draw(top, top, 3) == (2, 1)        # i = 2, j = (2^33 - 2) >> 32 = 1
    assert C.pair_from_draw(0, top, 3) == (0, 2)          # j = 1 >= 0 -> 2
    big = 2 ** 31 - 1
    assert C.pair_from_draw(top, top, big) == (big - 1, big - 2)   # (2^32 - 1)(2^31 - 1) >> 32 = 2^31 - 2
    assert C.pair_from_draw(half, half, big) == (2 ** 30 - 1, 2 ** 30)  # i = 2^30 - .5 -> 2^30 - 1 = j, bumped
    assert C.pair_from_draw(0, 0, big) == (0, 1)


@pytest.mark.parametrize('nf', [2, 3, 2 ** 31 - 1, 2 ** 40 + 12345])
def test_index_rule_on_philox_draws(nf):
    """The vectorised rule of the oracle against the integer definition on real draws: distinct, both below n_f."""
    hyps, seed, frame = 512, 0x123456789ABCDEF, 2 ** 33 + 5
    i, j = C.draw_pairs(nf, hyps, seed, frame)
    x0, x1, _, _ = P.philox4x32_10(np.arange(hyps, dtype=np.uint32), np.full(hyps, frame & 0xFFFFFFFF, np.uint32),
                                   np.full(hyps, frame >> 32, np.uint32), np.zeros(hyps, np.uint32),
                                   seed & 0xFFFFFFFF, seed >> 32)
    want = [C.pair_from_draw(a, b, nf) for a, b in zip(x0, x1)]
    assert [(int(a), int(b)) for a, b in zip(i, j)] == want
    assert (i != j).all() and (i >= 0).all() and (j >= 0).all() and (i < nf).all() and (j < nf).all()
    if nf == 2:
        assert set(zip(i.tolist(), j.tolist())) == {(0, 1), (1, 0)}
    # another frame or another seed draws other pairs
    if nf > 3:
        assert (C.draw_pairs(nf, hyps, seed, frame + 1)[0] != i).any()
        assert (C.draw_pairs(nf, hyps, seed + 1, frame)[0] != i).any()


def test_philox_known_answer():
    """The counter layout (h, frame low, frame high, 0) on the generator's published known answer (Random123 kat
    vectors: counter and key of all ones)."""
    x = P.philox4x32_10(np.array([0xFFFFFFFF], np.uint32), np.array([0xFFFFFFFF], np.uint32),
                        np.array([0xFFFFFFFF], np.uint32), np.array([0xFFFFFFFF], np.uint32), 0xFFFFFFFF, 0xFFFFFFFF)
    assert [int(v[0]) for v in x] == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_degenerate_frames_keep_the_ls_start():
    d = C.scene(50, 5)
    kw = dict(k=R.K_CHAIN, scale=0.05, hyps=64, seed=1)
    one = C.consensus_frame(d['az'][:1], d['y'][:1], np.array([3]), ridge=1e5, **kw)
    assert one['best_h'] == -1 and one['n_valid'] == 0 and one['n'] == 3
    none = C.consensus_frame(d['az'], d['y'], np.zeros(50, np.int64), **kw)
    assert none['best_h'] == -1 and none['n'] == 0 and none['passes'] == 0 and (none['x'] == none['ls']).all()
    same = C.consensus_frame(np.full(50, 0.3), d['y'], d['m'], ridge=1e5, refine=0, **kw)
    assert same['best_h'] == -1 and same['n_valid'] == 0 and (same['x'] == same['ls']).all()
    raw = C.consensus_frame(d['az'], d['y'], d['m'], refine=0, **kw)
    assert raw['best_h'] >= 0 and (raw['x'] == raw['x_h'][raw['best_h']]).all()


def test_chain_config_consensus():
    import rsl
    with pytest.raises(ValueError):
        rsl.ChainConfig(velocity_loss='consensus')  # the scale is required
    with pytest.raises(ValueError):
        rsl.ChainConfig(velocity_loss='consensus', velocity_scale=0.0)
    cfg = rsl.ChainConfig(velocity_loss='consensus', velocity_scale=0.05)
    assert (cfg.velocity_c, cfg.velocity_hyps, cfg.velocity_min_det, cfg.velocity_refine, cfg.velocity_seed) == \
        (None, 256, 0.1, 3, 0)
    for bad in (dict(velocity_hyps=0), dict(velocity_hyps=4097), dict(velocity_min_det=0.0),
                dict(velocity_min_det=1.5), dict(velocity_refine=-1), dict(velocity_refine=101)):
        with pytest.raises(ValueError):
            rsl.ChainConfig(velocity_loss='consensus', velocity_scale=0.05, **bad)
    with pytest.raises(ValueError):
        rsl.ChainConfig(velocity_loss='ransac')
    # the other losses do not look at the new fields
    assert rsl.ChainConfig().velocity_loss == 'ls'
    assert rsl.ChainConfig(velocity_loss='tukey').velocity_scale is None


def test_ctypes_row():
    from ctypes import c_longlong, c_ulonglong
    from rsl import _lib
    res, args = _lib.SIGNATURES['rsl_velocity_consensus']
    assert len(args) == 23
    assert args[18] is c_ulonglong and args[19] is c_longlong  # seed, frame0
    assert _lib.CONSENSUS_MAX_H == C.MAX_H == 4096 and _lib.CONSENSUS_DEFAULT_C == C.DEFAULT_C == 3.0
    assert hasattr(_lib.load(), 'rsl_velocity_consensus')


def test_header_constants():
    """The addition is additive: the ABI version and the timing slots stay."""
    with open(os.path.join(ROOT, 'include', 'rsl.h')) as f:
        h = f.read()
    define = lambda name: int(re.search(rf'#define\s+{name}\s+(\d+)', h).group(1))
    assert define('RSL_VERSION') == 2
    assert define('RSL_K_COUNT') == 10
    assert define('RSL_K_VELOCITY') == 8
    assert define('RSL_CONSENSUS_MAX_H') == 4096
    assert 'int rsl_velocity_consensus(' in h
    with open(os.path.join(ROOT, 'radar-slam_amd', 'csrc', 'rsl_vel_consensus.hip')) as f:
        assert int(re.search(r'kCvChunk\s*=\s*(\d+)', f.read()).group(1)) == C.CHUNK
