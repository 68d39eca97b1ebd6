"""bench.py --dump-outputs: a plain run (no --full) of 3 timed steps on 40-frame batches writes what its last timed step
computed.  The dumped arrays are float32 / float64 .npy files under the size limit, and they are that step's results:
the same batch (the bench's seeded device generator, batch (steps - 1) mod 2) through a fresh rsl.RadarChain in this
process gives the same RDS (the FFT kernels are deterministic: bit-equal), the same per-frame peak / cell counts and
dense per-cell maps, and the same velocity rows (the LS sums run over atomically compacted lists, whose order may
differ from run to run: 1e-9 of the array's largest magnitude, three digits above the ~3e4 x 2^-53 = 3e-12 relative
rounding of an f64 sum over a frame's ~3e4 cells).  The plain line carries the headline keys and none of the
measurements that --full adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F, STEPS = 40, 3
FULL_ONLY = ('cpu_baseline', 'pcie_inclusive', 'configs_1_spectrum', 'configs_4_frame', 'kernel_ms_standalone',
             'kernel_rooflines_standalone', 'fft_stage_standalone')


@pytest.fixture(scope='module')
def dumped(tmp_path_factory):
    out = tmp_path_factory.mktemp('dump')
    env = {k: v for k, v in os.environ.items() if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'MASTER_PORT')}
    r = subprocess.run([sys.executable, '-u', os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', str(STEPS),
                        '--warmup', '1', '--frames-per-step', str(F), '--dump-outputs', str(out)],
                       env=env, capture_output=True, text=True, timeout=110)
    assert r.returncode == 0, r.stderr[-3000:]
    js = [json.loads(l) for l in r.stdout.splitlines() if l.lstrip().startswith('{')]
    assert len(js) == 1, r.stdout[-2000:]
    arrays = {f[:-4]: np.load(os.path.join(out, f), allow_pickle=False) for f in sorted(os.listdir(out))}
    return js[0], arrays


def test_plain_line(dumped):
    line, _ = dumped
    assert line['steps'] == STEPS and line['n_gpus'] == 1 and line['unit'] == 'frames/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['value'] == pytest.approx(F * STEPS / (line['ms_per_step'] * STEPS / 1e3), rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    assert 'frac_standalone' not in line['roofline']


def test_dump_files(dumped):
    _, a = dumped
    assert set(a) == {'velocity', 'peaks_per_frame', 'cells_per_frame', 'poses', 'smoothed_positions',
                      'sample_frames', 'rds', 'peak_power_db', 'cell_antennas', 'doa_azimuth', 'esprit_azimuth',
                      'phase'}
    assert all(v.dtype in (np.float32, np.float64) for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64e6
    assert all(np.isfinite(v).all() for v in a.values())
    assert a['velocity'].shape == (F, 8) and a['poses'].shape == (F, 7)
    assert a['sample_frames'].tolist() == [0, F - 1]
    assert a['rds'].shape == (2, 8, 512, 128, 2) and a['doa_azimuth'].shape == (2, 512, 128)


def test_dump_is_the_last_steps_result(dumped, ctx):
    import torch
    import bench
    import rsl
    _, a = dumped
    A, C, Tc = 8, 128, 51.2e-6
    last = (STEPS - 1) % 2
    cube = bench.make_cubes(ctx, 2, F, A, C, Tc, 0)[last]
    ch = rsl.RadarChain(rsl.ChainConfig(num_antennas=A, num_chirps=C, chirp_duration=Tc, ridge=0.01), F, ctx)
    ch.run(cube)
    torch.cuda.synchronize()
    want = bench.chain_outputs([(ch, 0)])
    assert np.array_equal(a['rds'], want['rds'])
    assert a['peaks_per_frame'].sum() > 0 and a['cells_per_frame'].min() > 0
    for k in ('peaks_per_frame', 'cells_per_frame', 'peak_power_db', 'cell_antennas', 'doa_azimuth'):
        assert np.array_equal(a[k], want[k]), k
    for k in ('esprit_azimuth', 'phase', 'velocity'):
        np.testing.assert_allclose(a[k], want[k], rtol=1e-9, atol=1e-9 * np.abs(want[k]).max(), err_msg=k)
    assert np.count_nonzero(a['cell_antennas'][0]) == a['cells_per_frame'][0]
    assert np.count_nonzero(a['cell_antennas'][1]) == a['cells_per_frame'][F - 1]
