"""fp64 numpy oracle of the range-azimuth maps (rsl_range_cov / rsl_range_azimuth, specified in include/rsl.h), the
inputs of their tests and the resolution scene.  Everything works on the very complex64 values the kernels read,
widened to complex128: einsum for the covariance, np.linalg.inv for Capon, eigvalsh for the condition number."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32


# -- the estimators -------------------------------------------------------------------------------------------------
def cov_ref(z, c0=0, c1=None):
    """z c64 [F, A, S, C] -> cov c128 [F, S, A, A] = (1/Cw) sum over the Doppler window of x x^H."""
    x = np.asarray(z).astype(np.complex128)
    c1 = x.shape[-1] if c1 is None else c1
    w = x[..., c0:c1]
    return np.einsum('fprc,fqrc->frpq', w, w.conj()) / (c1 - c0)


def cov_bound(ref, Cw):
    """The sequential fp32 bound per element: 2 (Cw + 4) u sqrt(ref_pp ref_qq)."""
    d = np.sqrt(np.abs(np.einsum('...pp->...p', ref).real))
    return 2.0 * (Cw + 4) * U * d[..., :, None] * d[..., None, :]


def hermitian(c):
    """The Hermitian matrix that the upper triangle and the diagonal's real part of c [.., A, A] define."""
    c = np.asarray(c).astype(np.complex128)
    up = np.triu(c, 1)
    d = np.einsum('...pp->...p', c).real
    out = up + np.conj(np.swapaxes(up, -1, -2))
    idx = np.arange(c.shape[-1])
    out[..., idx, idx] = d
    return out


def map_ref(cov, steer, method, loading=1e-2):
    """cov [n, A, A], steer [G, A] (the c64 values, widened) -> dict(map f64 [n, G], t [n], kappa [n] (Capon: the
    condition number of R_l from its fp64 eigenvalues; 1 for empty rows)).  Rows with t <= 0 are all 0."""
    R = hermitian(cov)
    a = np.asarray(steer).astype(np.complex128)
    n, A = R.shape[0], R.shape[-1]
    t = np.einsum('npp->n', R).real
    ok = t > 0
    out = np.zeros((n, a.shape[0]))
    kappa = np.ones(n)
    if method == 'bartlett':
        out[ok] = np.einsum('gp,npq,gq->ng', a.conj(), R[ok], a).real / A ** 2
    else:
        Rl = R[ok] + (loading * t[ok] / A)[:, None, None] * np.eye(A)
        ev = np.linalg.eigvalsh(Rl)
        kappa[ok] = ev[:, -1] / ev[:, 0]
        out[ok] = 1.0 / np.einsum('gp,npq,gq->ng', a.conj(), np.linalg.inv(Rl), a).real
    return dict(map=out, t=t, kappa=kappa)


def map_bound(ref, method, A):
    """Per element: Bartlett (2 A^2 + 8) u t / A; Capon 8 A u kappa(R_l) ref."""
    if method == 'bartlett':
        return np.broadcast_to(((2 * A * A + 8) * U * ref['t'] / A)[:, None], ref['map'].shape)
    return 8 * A * U * ref['kappa'][:, None] * ref['map']


# -- inputs -----------------------------------------------------------------------------------------------------------
def steering(grid_deg, pos):
    """exp(j 2 pi pos sin(theta)), pos in wavelengths: c128 [G, A]."""
    return np.exp(2j * np.pi * np.sin(np.radians(np.asarray(grid_deg, float)))[:, None] * np.asarray(pos, float)[None])


def ula(A):
    return 0.5 * np.arange(A)


def perturbed(A, seed=5):
    """A non-uniform array: half-wavelength positions moved by up to a fifth of a wavelength."""
    return ula(A) + np.random.default_rng(seed).uniform(-0.2, 0.2, A)


def grid(G):
    return np.array([0.0]) if G == 1 else np.linspace(-90.0, 90.0, G)


COV_CASES = [  # (F, A, S, C, window or None)
    (1, 2, 1, 1, None), (1, 3, 2, 3, None), (1, 7, 2, 5, (1, 5)), (3, 8, 33, 64, None), (1, 8, 5, 65, (1, 65)),
    (1, 8, 5, 65, (0, 63)), (1, 8, 5, 64, (7, 8)), (1, 9, 3, 4, None), (1, 15, 2, 63, (3, 62)), (3, 16, 33, 128, None),
    (1, 16, 1, 256, (255, 256))]


def cov_input(F, A, S, C, seed):
    """Unit complex Gaussian c64 [F, A, S, C] with one antenna scaled by 1e3 and one all-zero range bin; returns
    (z, the zero bin).  With a single range bin there is no room for both: the bin keeps its data and the zero bin is
    None (the test then runs the zeroed input as well)."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((F, A, S, C)) + 1j * rng.standard_normal((F, A, S, C))) / np.sqrt(2.0)
    z[:, A // 2] *= 1e3
    zero = S // 2 if S > 1 else None
    if zero is not None:
        z[:, :, zero] = 0.0
    return z.astype(np.complex64), zero


def psd_covs(A, n, seed):
    """n host-built Hermitian positive semi-definite c64 covariances [n, A, A]: K snapshots (K cycles through 1 .. 2A,
    so ranks from 1 to full) of unit noise plus up to two sources of 0 to 30 dB, and two all-zero rows (t = 0) where
    n allows."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, A, A), np.complex128)
    pos = ula(A)
    for i in range(n):
        K = 1 + i % (2 * A)
        x = (rng.standard_normal((A, K)) + 1j * rng.standard_normal((A, K))) / np.sqrt(2.0)
        for _ in range(i % 3):
            amp = 10.0 ** (rng.uniform(0.0, 30.0) / 20.0)
            sv = steering([rng.uniform(-80.0, 80.0)], pos)[0]
            x += amp * sv[:, None] * np.exp(2j * np.pi * rng.uniform(size=K))[None]
        out[i] = x @ x.conj().T / K
    out = hermitian(out.astype(np.complex64))
    if n > 3:
        out[[2, n - 1]] = 0.0
    return out.astype(np.complex64)


# -- the resolution scene ---------------------------------------------------------------------------------------------
RES = dict(A=8, C=32, G=181, S=200, sep=10.0, snr_db=20.0, loading=1e-2, seed=7, tol=2.0)


def resolution_scene(seed=RES['seed'], sep=RES['sep']):
    """rds c64 [A, S, C]: in every range bin two sources at -sep/2 and +sep/2 degrees, each in its own 4 Doppler bins
    with random phases at snr_db over unit complex Gaussian noise.  Returns (rds, truth angles, grid, steer c128)."""
    A, C, S = RES['A'], RES['C'], RES['S']
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal((A, S, C)) + 1j * rng.standard_normal((A, S, C))) / np.sqrt(2.0)
    truth = (-sep / 2, sep / 2)
    amp = 10.0 ** (RES['snr_db'] / 20.0)
    for k, (ang, bins) in enumerate(zip(truth, (slice(4, 8), slice(20, 24)))):
        sv = steering([ang], ula(A))[0]
        ph = np.exp(2j * np.pi * rng.uniform(size=(S, 4)))
        z[:, :, bins] += amp * sv[:, None, None] * ph[None]
    g = grid(RES['G'])
    return z.astype(np.complex64), truth, g, steering(g, ula(A))


def resolved(row, grid_deg, truth, tol=RES['tol']):
    """Both sources resolved: for each true angle a local maximum of the row (above its left neighbour, not below its
    right one) within tol degrees of it, the two at different grid points."""
    row = np.asarray(row)
    left = np.r_[True, row[1:] > row[:-1]]
    right = np.r_[row[:-1] >= row[1:], True]
    peaks = np.nonzero(left & right)[0]
    hit = [set(peaks[np.abs(grid_deg[peaks] - a) <= tol].tolist()) for a in truth]
    return bool(hit[0]) and bool(hit[1]) and len(hit[0] | hit[1]) >= 2


def count_resolved(maps, grid_deg, truth):
    return sum(resolved(r, grid_deg, truth) for r in maps)
