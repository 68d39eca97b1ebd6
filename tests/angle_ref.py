"""fp64 references of the per-signature angle kernels: k_music_subspace and k_esprit_subspace (rsl_subspace.hip),
k_confidence and k_cell_extras (rsl_doa.hip).  Plain numpy, complex128, no GPU.  The inputs the GPU tests use are built
here too, so that tests/test_angle_host.py can prove them sound (and measure the references' own spread) on a CPU."""
import numpy as np

import radar_oracle as O

ESPRIT_SCALE = 1 / np.pi   # lambda / (2 pi d) at half-wavelength spacing


# -- MUSIC ------------------------------------------------------------------------------------------------------------
def music_lo(M, K):
    """First noise column of V[:, K:] (Python slicing)."""
    return len(range(M)[:K])


def music_basis(s):
    """V = [s/|s|, Householder completion] of rsl_subspace.hip's file comment, as the explicit matrix
    P = I - 2ww^H/w^Hw (P s = alpha e_1, alpha = -e^{i arg s_0}|s|, arg 0 = 0).  A zero signature: eigh(0) = identity
    in reversed order."""
    s = np.asarray(s, complex)
    M = len(s)
    nx = np.linalg.norm(s)
    if nx == 0:
        return np.eye(M, dtype=complex)[:, ::-1]
    ph = s[0] / abs(s[0]) if abs(s[0]) > 0 else 1.0
    w = s.copy()
    w[0] -= -ph * nx
    return np.eye(M) - 2 * np.outer(w, w.conj()) / np.vdot(w, w).real


def music_den(s, a, K):
    """den = sum over the noise columns j >= K (Python slicing) of |a^H v_j|^2."""
    lo = music_lo(len(s), K)
    return float(np.sum(np.abs(np.asarray(a, complex).conj() @ music_basis(s)[:, lo:]) ** 2))


def music_den_all(sigs, steer):
    """music_den for every signature, steering row and first noise column: f64 [n, G, M + 1], [.., lo] the den with
    the noise columns lo .. M-1 (lo = M: none, 0)."""
    n, M = sigs.shape
    out = np.zeros((n, steer.shape[0], M + 1))
    for c, s in enumerate(sigs):
        p = np.abs(steer.conj() @ music_basis(s)) ** 2           # [G, M]: |a_g^H v_j|^2
        out[c, :, :M] = np.cumsum(p[:, ::-1], axis=1)[:, ::-1]
    return out


def music_steering(M):
    """The [37, M] table of the MUSIC test: steering rows with an amplitude taper, so that |a_j| differs between the
    antennas and the column order of a zero signature's identity basis shows in den."""
    return steering_table(M)[1] * (1 + 0.05 * np.arange(M))


def music_signatures(M, steer, seed):
    """The 25 MUSIC test signatures [25, M]: 20 random, s[0] = 0, zero, a steering row, and rows 0 and 1 repeated at
    the last two indices (so the first and the last index hold the same signature)."""
    rs = np.random.RandomState(seed)
    s = rs.randn(25, M) + 1j * rs.randn(25, M)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    s[20, 0] = 0
    s[20] /= max(np.linalg.norm(s[20]), 1e-300)   # M = 1: a second zero signature
    s[21] = 0
    s[22] = steer[len(steer) // 3] / np.sqrt(M)
    s[23], s[24] = s[1], s[0]
    return s


# -- ESPRIT -----------------------------------------------------------------------------------------------------------
def esprit_kk(M, K):
    """Columns of Us = U[:, :K] of the (M-1) x (M-1) U (Python slicing)."""
    return len(range(M - 1)[:K])


def span_columns(s, kk, rel=1e-9):
    """The first kk independent columns of [left singular vectors of X = [s[:-1], s[1:]] in sigma order, e_0, e_1, ..]
    (the span rsl_subspace.hip documents), (M-1) x kk, not yet orthonormal.  A singular vector whose sigma is below
    rel * the largest one (X of rank < 2) and an e_j within rel of the span so far are skipped."""
    s = np.asarray(s, complex)
    L = len(s) - 1
    X = np.column_stack([s[:-1], s[1:]])
    U, sv, _ = np.linalg.svd(X, full_matrices=False)
    cand = [U[:, j] for j in range(2) if sv[j] > rel * max(sv[0], np.finfo(float).tiny) and sv[j] > 0]
    cand += [np.eye(L, dtype=complex)[:, j] for j in range(L)]
    cols, Q = [], np.zeros((L, 0), complex)
    for v in cand:
        if len(cols) == kk:
            break
        r = v - Q @ (Q.conj().T @ v)
        r = r - Q @ (Q.conj().T @ r)
        if np.linalg.norm(r) > rel:
            cols.append(v)
            Q = np.column_stack([Q, r / np.linalg.norm(r)])
    return np.column_stack(cols), Q


def basis_gs(s, kk):
    """Orthonormal basis of the span by two-pass Gram-Schmidt in column order."""
    return span_columns(s, kk)[1]


def basis_qr(s, kk):
    """Orthonormal basis of the same span by LAPACK's Householder QR of the same columns."""
    return np.linalg.qr(span_columns(s, kk)[0])[0]


def esprit_phi(s, K, basis=basis_gs):
    """Phi = pinv(B[:-1]) B[1:] for the orthonormal basis B of the span; None where it is empty (kk = 0 or M <= 2)."""
    M = len(s)
    kk = esprit_kk(M, K)
    if kk == 0 or M <= 2:
        return None
    B = basis(s, kk)
    return np.linalg.pinv(B[:-1]) @ B[1:]


def esprit_candidates(s, K, scale=ESPRIT_SCALE, basis=basis_gs):
    """(eigenvalues of Phi by descending modulus, their phases np.angle, their angles in degrees) or None where Phi is
    empty.  The eigenvalues are those of the shift restricted to the span, so they do not depend on the basis."""
    Phi = esprit_phi(s, K, basis)
    if Phi is None:
        return None
    lam = np.linalg.eigvals(Phi)
    lam = lam[np.argsort(-np.abs(lam), kind='stable')]
    ph = np.angle(lam)
    with np.errstate(invalid='ignore'):
        return lam, ph, np.degrees(np.arcsin(ph * scale))


def deg_to_phase(deg, scale=ESPRIT_SCALE):
    """The eigenvalue phase an ESPRIT angle stands for: sin(radians(deg)) / scale."""
    return np.sin(np.radians(np.asarray(deg, float))) / scale


def wrap(d):
    """d modulo 2 pi into (-pi, pi]."""
    return -((-np.asarray(d, float) + np.pi) % (2 * np.pi) - np.pi)


def phase_err(deg, ph_ref, scale=ESPRIT_SCALE):
    """|wrapped difference| between the phase of an ESPRIT angle in degrees and a reference eigenvalue phase: keeps the
    arcsin end and the +-90 degree alias (phase +-pi) out of the tolerance."""
    return np.abs(wrap(deg_to_phase(deg, scale) - ph_ref))


def esprit_signatures(M, seed):
    """The 130 ESPRIT test signatures [130, M], unit norm: 100 random, 20 single exponentials (|omega| <= 3.1) with
    5 % noise, 10 noiseless exponentials (X of rank 1)."""
    rs = np.random.RandomState(seed)
    s = rs.randn(130, M) + 1j * rs.randn(130, M)
    om = rs.uniform(-3.1, 3.1, 30)
    e = np.exp(1j * om[:, None] * np.arange(M))
    s[100:120] = e[:20] + 0.05 * s[100:120]
    s[120:] = e[20:]
    return s / np.linalg.norm(s, axis=1, keepdims=True)


REPEATS = (63, 64, 129)   # indices that repeat signature 0: either side of a 64-thread block edge, and the last


def cluster_signatures(M, seed):
    """130 random unit signatures [130, M]; the one at index 0 again at REPEATS."""
    rs = np.random.RandomState(seed)
    s = rs.randn(130, M) + 1j * rs.randn(130, M)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    s[list(REPEATS)] = s[0]
    return s


ESPRIT_M = (3, 4, 5, 8, 9, 15, 16)      # determined cases: K = 1, -(M-2) at all, K = 2, -(M-3) at M >= 4
CLUSTER_M = (5, 8, 12, 16)              # 3 <= kk < M - 1


def determined_seed(M):
    return 100 + M


def cluster_seed(M):
    return 200 + M


def cluster_K(M):
    """K of the 3 <= kk < M - 1 cases: 3, M-3, M-2 and -1 (kk = M-2), without repeats of one kk's K."""
    return [K for K in dict.fromkeys((3, M - 3, M - 2, -1)) if 3 <= esprit_kk(M, K) < M - 1]


def k2_sound(lam, ph):
    """A K = 2 input determines both candidates: moduli > 1e-3, phases more than 1e-3 rad apart."""
    return bool(np.abs(lam[1]) > 1e-3 and abs(wrap(ph[0] - ph[1])) > 1e-3)


def cluster_sound(lam, ph):
    """A 3 <= kk < M - 1 input separates the two non-zero eigenvalues from the zero cluster: third modulus <= half the
    second, the two largest more than 1e-3 rad apart."""
    return bool(np.abs(lam[2]) <= 0.5 * np.abs(lam[1]) and abs(wrap(ph[0] - ph[1])) > 1e-3)


# -- confidence and cell extras ---------------------------------------------------------------------------------------
def normalise32(sig32):
    """The fp32 signatures [n, A] cast to fp64 and normalised (rows of zero power stay zero)."""
    s = np.asarray(sig32).astype(np.complex128)
    p = np.sum(s.real ** 2 + s.imag ** 2, axis=-1, keepdims=True)
    return s / np.sqrt(np.where(p > 0, p, 1.0))


def confidence(sig, a):
    """O.angle_confidence (robust_angle_estimation.py:88-138) with the steering vector passed in: any A, any angle."""
    sig = np.asarray(sig, complex)
    a = np.asarray(a, complex)
    corr = np.abs(np.vdot(a, sig))
    sp = np.sum(np.abs(sig) ** 2)
    nc = corr / np.sqrt(sp) if sp > 0 else 0.0
    perr = np.mean(np.abs(np.angle(np.exp(1j * (np.angle(sig) - np.angle(a))))))
    pc = np.exp(-perr)
    pw = np.abs(sig) ** 2
    nf = np.percentile(pw, 20)
    snrc = min(1.0, np.log10(np.mean(pw) / nf) / 3.0) if nf > 0 else 0.0
    return min(1.0, max(0.0, nc * 0.4 + pc * 0.3 + snrc * 0.3))


def cell_extras(sig32):
    """From the fp32 signatures [n, A]: (the fp64-normalised signature, angle(s1 conj(s0)), O.esprit_closed in degrees
    (None at A = 2, where the closed form has no rows to regress))."""
    s = normalise32(sig32)
    phase = np.angle(s[:, 1] * np.conj(s[:, 0]))
    esp = O.esprit_closed(s) if s.shape[1] >= 3 else None
    return s, phase, esp


LAYOUT = dict(F=4, S=8, C=16, n=300, G=37)


def steering_table(A, G=LAYOUT['G']):
    """[G, A] steering matrix over -90 .. 90 degrees and its grid in degrees."""
    grid = np.linspace(-90.0, 90.0, G)
    return grid, O.steering_matrix(grid, A)


def layout_case(A, seed, plant):
    """A random c64 RDS [F, A, S, C], n cells drawn without replacement from all frames (cell 0 of frame 0 first, the
    last cell of the last frame second, the rest in random order), random grid indices, and the planted signatures of
    `plant(sig, steer, gidx)` written into the RDS at the cells it names.  Returns (rds, frame, rc, gidx, sig32)."""
    F, S, C, n, G = (LAYOUT[k] for k in ('F', 'S', 'C', 'n', 'G'))
    rs = np.random.RandomState(seed)
    rds = (rs.randn(F, A, S, C) + 1j * rs.randn(F, A, S, C)).astype(np.complex64)
    flat = rs.permutation(np.arange(1, F * S * C - 1))[:n - 2]
    flat = np.concatenate([[0, F * S * C - 1], flat])
    frame, rc = (flat // (S * C)).astype(np.int32), (flat % (S * C)).astype(np.int32)
    gidx = rs.randint(0, G, n).astype(np.int32)
    _, steer = steering_table(A)
    sig = rds[frame, :, rc // C, rc % C]
    plant(sig, steer, gidx)
    rds[frame, :, rc // C, rc % C] = sig
    return rds, frame, rc, gidx, rds[frame, :, rc // C, rc % C]


# -- the ESPRIT cases with their references, computed once and shared by the host and the GPU tests ---------------------
_CASES = {}


def _case(kind, M):
    """sigs [130, M] and, per K, a dict: kk; ph [130, min(kk, 2)], the phases of the largest-modulus candidates from the
    Gram-Schmidt basis, and ph_qr, the same from the QR basis; mod [130, min(kk, 3)], the largest moduli; sound, bool
    [130]: the input determines its candidates (k2_sound / cluster_sound; True at kk = 1); rank1, bool [130]: X has
    rank 1 and kk >= 2, so there are no candidates (NaN) and the input is left out by construction, not dropped."""
    key = (kind, M)
    if key in _CASES:
        return _CASES[key]
    if kind == 'determined':
        sigs = esprit_signatures(M, determined_seed(M))
        Ks = [1, -(M - 2)] + ([2, -(M - 3)] if M >= 4 else [])
    else:
        sigs = cluster_signatures(M, cluster_seed(M))
        Ks = cluster_K(M)
    per = {}
    for K in Ks:
        kk = esprit_kk(M, K)
        top, nmod = min(kk, 2), min(kk, 3)
        rank1 = np.zeros(len(sigs), bool)
        if kind == 'determined' and kk >= 2:
            rank1[120:] = True
        ph, phq, mod = (np.full((len(sigs), k), np.nan) for k in (top, top, nmod))
        sound = np.zeros(len(sigs), bool)
        for c in np.flatnonzero(~rank1):
            lam, p, _ = esprit_candidates(sigs[c], K, basis=basis_gs)
            ph[c], phq[c], mod[c] = p[:top], esprit_candidates(sigs[c], K, basis=basis_qr)[1][:top], np.abs(lam[:nmod])
            sound[c] = True if kk == 1 else k2_sound(lam, p) if kk == 2 else cluster_sound(lam, p)
        per[K] = dict(kk=kk, ph=ph, ph_qr=phq, mod=mod, sound=sound, rank1=rank1)
    _CASES[key] = (sigs, per)
    return _CASES[key]


def determined_case(M):
    return _case('determined', M)


def cluster_case(M):
    return _case('cluster', M)


def set_distance(pa, pb):
    """Largest wrapped phase distance from a candidate of one set [n, k] to the nearest of the other, per row [n]."""
    d = np.abs(wrap(pa[:, :, None] - pb[:, None, :]))
    return np.maximum(d.min(axis=2).max(axis=1), d.min(axis=1).max(axis=1))


def case_spread(kind, M, K):
    """Largest phase difference (rad) between the candidates of the two basis constructions over the sound inputs of
    one (M, K)."""
    r = _case(kind, M)[1][K]
    ok = r['sound']
    return float(set_distance(r['ph'][ok], r['ph_qr'][ok]).max()) if ok.any() else 0.0


def reference_spread(kind):
    """The reference spread of one family of GPU-test inputs: 'determined' (kk <= 2) or 'cluster' (3 <= kk < M - 1)."""
    Ms = ESPRIT_M if kind == 'determined' else CLUSTER_M
    return max(case_spread(kind, M, K) for M in Ms for K in _case(kind, M)[1])


MARGIN = 100   # the kernel's elimination order and QR iteration round differently from LAPACK


def esprit_tol():
    """Phase tolerance (rad) of every reference-determined ESPRIT value (kk <= 2, and k_cell_extras)."""
    return MARGIN * reference_spread('determined')


def cluster_tol(M, K):
    """Phase tolerance (rad) of the 3 <= kk < M - 1 match at one (M, K): that case's own spread where it is larger."""
    return MARGIN * max(reference_spread('determined'), case_spread('cluster', M, K))


# -- planted cells of the k_confidence / k_cell_extras cases (indices into the n-cell list) ----------------------------
CONF_A = (2, 3, 4, 5, 6, 8, 9, 16, 31, 32)
EXTRAS_A = (2, 3, 4, 5, 8, 16, 17, 32)
SIGNS = ((1, 1), (1, -1), (-1, 1), (-1, -1))
PLANTED = dict(zero=2, one_zero=3, pct_zero=4, matched=5, wrap=6, s0_zero=(7, 8, 9, 10), s1_zero=(11, 12, 13, 14),
               snr_clip=15)


def plant_confidence(sig, steer, gidx):
    """zero: a zero signature.  one_zero: one antenna exactly 0 (np.angle(0) = 0).  pct_zero: the lowest powers are 0
    up to the percentile's upper neighbour, so the 20th percentile is exactly 0.  matched: the signature is its own
    steering row (0.4 sqrt(A) > 1 from A = 7 on: the clip at 1.0; all powers equal).  wrap: phase -pi on every antenna
    against the +pi of the odd antennas at +90 degrees.  snr_clip: the powers up to the percentile's upper neighbour
    are 1e-6 of the rest, so log10(mean / percentile) / 3 > 1 (from A = 3 on: at A = 2 the percentile is a fifth of
    the larger power at least)."""
    A = sig.shape[1]
    P = PLANTED
    sig[P['zero']] = 0
    sig[P['one_zero'], A // 2] = 0
    sig[P['pct_zero'], :min(int(np.floor(0.2 * (A - 1))) + 2, A)] = 0
    sig[P['matched']] = steer[gidx[P['matched']]]
    gidx[P['wrap']] = len(steer) - 1
    sig[P['wrap']] = -1 - 1e-30j
    sig[P['snr_clip'], :min(int(np.floor(0.2 * (A - 1))) + 2, A - 1)] *= 1e-3


def plant_extras(sig, steer, gidx):
    """zero: a zero signature.  s0_zero / s1_zero: antenna 0 / antenna 1 exactly 0 and the other of the two with every
    combination of signs (the products with a zero are then zeros of either sign)."""
    P = PLANTED
    sig[P['zero']] = 0
    for c0, c1, (sr, si) in zip(P['s0_zero'], P['s1_zero'], SIGNS):
        sig[c0, 0], sig[c0, 1] = 0, complex(0.75 * sr, 0.5 * si)
        sig[c1, 1], sig[c1, 0] = 0, complex(0.75 * sr, 0.5 * si)
