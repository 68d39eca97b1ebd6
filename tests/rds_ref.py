"""What the range-Doppler front-end tests share (tests/test_gpu_fft_sizes.py, tests/test_gpu_detectors_agree.py): the
plain fp64 numpy reference of rsl_rds, seeded inputs with a random complex table (an all-ones table hides a wrong table
index), output buffers with sentinels around them, and the emitted peak lists of a detector's outputs."""
import numpy as np

# RSL_FFT_SIZES (rsl_internal.h): the lengths with a Stockham plan; every other length up to 4096 is a direct DFT
PLANNED = (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 25, 50, 100, 200, 400, 800, 1600)
CUBE_VAR = 0.02  # E |x|^2 of a cube sample
GUARD = 4096     # sentinel elements on each side of a guarded buffer
LISTS = ('e_coord', 'e_cell', 'e_pdb', 'c_frame', 'c_rc', 'c_amask')


def rows_for(n):
    """rsl_common.h: rows of an n-point FFT per workgroup."""
    return max(1, min(4096 // n, 64))


def make_table(S, seed):
    """complex64 [S]: unit-modulus random phase times a random real in [0.5, 1]."""
    rng = np.random.default_rng([seed, S])
    return (rng.uniform(0.5, 1.0, S) * np.exp(2j * np.pi * rng.uniform(0.0, 1.0, S))).astype(np.complex64)


def make_cube(F, A, Ct, S, seed):
    """complex64 [F, A, Ct, S]: complex Gaussian of variance CUBE_VAR."""
    rng = np.random.default_rng([seed, F, A, Ct, S])
    cube = np.empty((F, A, Ct, S), np.complex64)
    sd = np.float32(np.sqrt(CUBE_VAR / 2))
    cube.real = rng.standard_normal(cube.shape, dtype=np.float32) * sd
    cube.imag = rng.standard_normal(cube.shape, dtype=np.float32) * sd
    return cube


def mean_power(table, S, C):
    """The mean RDS power of a make_cube cube under `table`."""
    return S * C * CUBE_VAR * float(np.mean(np.abs(table.astype(np.complex128)) ** 2))


def reference(cube, table, chirp0, C, dc_removal):
    """fp64 rds [F, A, S, C] of the complex64 inputs as they are (their rounding to fp32 is not part of the error)."""
    y = cube[:, :, chirp0:chirp0 + C, :].astype(np.complex128) * table.astype(np.complex128)
    if dc_removal:
        y = y - y.mean(axis=3, keepdims=True)
    return np.fft.fftshift(np.fft.fft2(y.transpose(0, 1, 3, 2), axes=(2, 3)), axes=(2, 3))


class Guarded:
    """A complex64 device tensor `t` of `shape`, NaN-filled, inside a larger allocation with GUARD sentinel elements
    (distinct bit patterns) before and after it."""

    def __init__(self, ctx, shape):
        n = int(np.prod(shape))
        host = np.full(2 * (n + 2 * GUARD), np.nan, np.float32)
        bits = host.view(np.uint32)
        self.pat = np.uint32(0x4A000000) + np.arange(2 * GUARD, dtype=np.uint32)
        bits[:2 * GUARD] = self.pat
        bits[-2 * GUARD:] = self.pat
        self.buf = ctx.to_dev(host)
        self.t = ctx.torch.view_as_complex(self.buf.view(-1, 2))[GUARD:GUARD + n].view(shape)

    def host(self):
        return self.t.cpu().numpy()

    def intact(self):
        bits = self.buf.cpu().numpy().view(np.uint32)
        return bool((bits[:2 * GUARD] == self.pat).all() and (bits[-2 * GUARD:] == self.pat).all())


def lists_of(ctx, rds, det, C):
    """offsets + emit on one detector's outputs -> (ne, nc, the six lists cut to their counts, as bytes)."""
    F = rds.shape[0]
    offs = ctx.offsets(det['mask'], det['row_count'], C)
    ne, nc = int(offs['entry_base'][F].item()), int(offs['cell_base'][F].item())
    out = ctx.emit(rds, det['mask'], offs, ne, nc, want_pdb=True, peak_pow=det['peak_pow'],
                   peak_pow_group=det['group'])
    cut = {k: out[k][:(ne if k.startswith('e_') else nc)].cpu().numpy().tobytes() for k in LISTS}
    return ne, nc, cut
