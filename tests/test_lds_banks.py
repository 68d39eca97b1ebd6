"""LDS bank model of the configs[4] kernels' round-5 layouts (rsl_fft.hip, rsl_doppler_detect.hip), restated on the CPU: the access patterns
DESIGN section 3 calls conflict-free, under MI355X_MICROARCH.md's per-instruction banking (ds_write_b64: 16-lane
contiguous groups, bank = dword mod 32; ds_read_b64: 32-lane groups, dword mod 64; ds_read_b128: the four 16-lane
groups of the guide's table, dword mod 64).  A group costs one extra cycle per extra distinct dword on a bank."""
import pytest

W64 = [list(range(16 * g, 16 * g + 16)) for g in range(4)]
R64 = [list(range(32 * g, 32 * g + 32)) for g in range(2)]
_B128 = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
R128 = _B128 + [[x + 32 for x in g] for g in _B128]


def extra_cycles(pos, groups, nbank, dwords):
    """pos: lane -> float2 position (None: inactive); each lane touches `dwords` dwords from 2 * pos."""
    tot = 0
    for g in groups:
        banks = {}
        for lane in g:
            p = pos.get(lane)
            if p is None:
                continue
            for w in range(dwords):
                d = 2 * p + w
                banks.setdefault(d % nbank, set()).add(d)
        if banks:
            tot += max(len(v) for v in banks.values()) - 1
    return tot


def r1k_tw(j, k):  # k_range_fft_r1024's twiddle table slot of W1024^(j k)
    return j * 16 + (k ^ (((j >> 1) ^ (j >> 5)) & 15))


def test_r1024_twiddle_reads():
    # stage 1: lane j reads W^(j k); the radix-4 step: lane h = l % 4 reads row j = 16 h
    for k in range(1, 16):
        assert extra_cycles({l: r1k_tw(l, k) for l in range(64)}, R64, 64, 2) == 0
        assert extra_cycles({l: r1k_tw(16 * (l & 3), k) for l in range(64)}, R64, 64, 2) == 0
    # every row's 16 slots distinct, and the tile hand-off word's slot (j = 0, k = 0) is never a twiddle read
    for j in range(64):
        assert sorted(r1k_tw(j, k) - 16 * j for k in range(16)) == list(range(16))
    assert r1k_tw(0, 0) == 0


def test_r1024_exchange_and_output():
    S = 1024
    for wave in range(8):
        lts = [64 * wave + l for l in range(64)]
        for k in range(16):  # stage-1 exchange writes xbuf[q][k][j ^ 4k]
            pos = {l: (lt >> 6) * S + k * 64 + ((lt & 63) ^ ((4 * k) & 63)) for l, lt in enumerate(lts)}
            assert extra_cycles(pos, W64, 32, 2) == 0
        for i in range(16):  # stage-2 reads
            pos = {l: (lt >> 6) * S + ((lt >> 2) & 15) * 64 + 4 * (i ^ ((lt >> 2) & 15)) + (lt & 3) for l, lt in enumerate(lts)}
            assert extra_cycles(pos, R64, 64, 2) == 0
        for k in range(16):  # output writes obuf[q][bin ^ 4 s]
            pos = {}
            for l, lt in enumerate(lts):
                h = lt & 3
                s = (h >> 1) | ((h & 1) << 1)
                pos[l] = (lt >> 6) * S + ((((lt >> 2) & 15) ^ (4 * s)) + 256 * s) + 16 * k
            assert extra_cycles(pos, W64, 32, 2) == 0
        for q in range(8):  # the Doppler step's 16-B reads of bins 2p, 2p + 1
            pos = {l: q * S + ((2 * lt) ^ (4 * ((lt >> 7) & 3))) for l, lt in enumerate(lts)}
            assert extra_cycles(pos, R128, 64, 4) == 0


@pytest.mark.parametrize('skew,new_map,expect', [(1, False, 64), (6, True, 0)])
def test_r256_halo_row_writes(skew, new_map, expect):
    """k_doppler_detect_r256's halo rows (threads 256-287): row 0 and row 17 (skewed), column k1 + 8 k + 129 h.  The
    round-5 lane map (one k1 parity per 16-lane group) with the row skew 6 is conflict-free; round 4's (k1 = u / 4,
    skew 1) cost 64 extra cycles per tile."""
    tot = 0
    for k in range(16):
        pos = {}
        for u in range(32):
            hh, side = u & 1, (u >> 1) & 1
            k1 = 2 * ((u >> 2) & 3) + ((u >> 4) & 1) if new_map else u >> 2
            b2 = 17 if side else 0
            pos[u] = b2 * 258 + (skew if b2 == 17 else 0) + k1 + 129 * hh + 8 * k
        tot += extra_cycles(pos, W64, 32, 2)
    assert tot == expect


def test_r256_interior_row_writes():
    tot = 0
    for wave in range(4):
        for k in range(16):
            pos = {}
            for l in range(64):
                t = 64 * wave + l
                pos[l] = (((t >> 1) & 15) + 1) * 258 + (t >> 5) + 129 * (t & 1) + 8 * k
            tot += extra_cycles(pos, W64, 32, 2)
    assert tot == 0
