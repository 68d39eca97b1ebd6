"""CPU: the C-ABI library loads and exports exactly the symbols include/rsl.h declares; host-side helpers
(fp64 tables, steering operand layout, range gate) and the drop-in module surface (names, parameters,
defaults) match the reference."""
import ast
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import radar_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, 'include', 'rsl.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    return sorted(set(re.findall(r'^\s*(?:[a-z_ ]+\*?\s+)?\**(rsl_[a-z0-9_]+)\s*\(', src, flags=re.M)))


def test_library_exports_header():
    import rsl
    from rsl import _lib
    lib = rsl.load()
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f'{n} declared in rsl.h but not exported'
    assert sorted(_lib.SIGNATURES) == names, 'ctypes signature table out of sync with rsl.h'
    assert lib.rsl_version() == 2


def header_code():
    """include/rsl.h without comments and preprocessor lines."""
    src = open(os.path.join(ROOT, 'include', 'rsl.h')).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    src = re.sub(r'//[^\n]*', '', src)
    return '\n'.join(ln for ln in src.splitlines() if not ln.lstrip().startswith('#'))


_C_SCALARS = {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'unsigned long long': ctypes.c_ulonglong,
              'double': ctypes.c_double, 'float': ctypes.c_float}


def c_type(text):
    """The ctypes type of a C type as include/rsl.h writes it."""
    words = text.replace('*', ' * ').split()
    const = words[0] == 'const'
    words = words[1:] if const else words
    stars = words.count('*')
    base = ' '.join(w for w in words if w != '*')
    assert stars <= 1, text
    if not stars:
        return ctypes.c_void_p if base == 'rsl_handle' else _C_SCALARS[base]
    if base == 'void':
        return ctypes.c_void_p
    if base == 'char':
        assert const, text
        return ctypes.c_char_p
    return ctypes.POINTER(ctypes.c_void_p if base == 'rsl_handle' else _C_SCALARS[base])


def param_type(decl):
    """c_type of a parameter declaration `<type> <name>`."""
    return c_type(re.fullmatch(r'(.*?)\b[A-Za-z_]\w*\s*', decl, flags=re.S).group(1))


def test_signature_table_matches_header_types():
    """Every prototype of include/rsl.h against rsl._lib.SIGNATURES: the restype and every argument type, by identity,
    and no table entry without a prototype.  Context.call converts its arguments by this table."""
    from rsl import _lib
    protos = re.findall(r'([A-Za-z_][\w\s\*]*?)\b(rsl_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', header_code())
    assert len(protos) >= 57 and len({p[1] for p in protos}) == len(protos)
    seen = set()
    for ret, name, params in protos:
        assert name in _lib.SIGNATURES, f'{name} declared in rsl.h but not in SIGNATURES'
        res, args = _lib.SIGNATURES[name]
        assert c_type(ret) is res, (name, ret, res)
        want = [] if params.strip() == 'void' else [param_type(p) for p in params.split(',')]
        assert len(want) == len(args), (name, len(want), len(args))
        for i, (w, a, p) in enumerate(zip(want, args, params.split(','))):
            assert w is a, f'{name}: argument {i} is `{p.strip()}` in rsl.h, {a.__name__} in SIGNATURES'
        seen.add(name)
    assert seen == set(_lib.SIGNATURES), sorted(set(_lib.SIGNATURES) - seen)


# constants of include/rsl.h that the Python side does not mirror (a new constant goes here or into rsl/_lib.py)
HEADER_ONLY = ('RSL_VERSION', r'RSL_K_\w+', r'RSL_CFAR_MAX_\w+', 'RSL_SS_MAX_SWEEPS', 'RSL_SS_OFF_TOL',
               r'RSL_POINT_\w+')


def test_constants_match_header():
    """Every `#define RSL_<NAME> <number>` of include/rsl.h equals its mirror in rsl/_lib.py (<NAME> or RSL_<NAME>) or
    is on HEADER_ONLY; K_NAMES are the RSL_K_* ids in order."""
    from rsl import _lib
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rsl.h')).read(), flags=re.S)
    defs = dict(re.findall(r'^\s*#\s*define\s+(RSL_\w+)[ \t]+([-+]?(?:0x[0-9a-fA-F]+|[0-9.]+(?:e[-+]?\d+)?))f?[ \t]*$',
                           src, flags=re.M))
    assert len(defs) >= 53, sorted(defs)
    mirrored = 0
    for name, text in defs.items():
        if any(re.fullmatch(pat, name) for pat in HEADER_ONLY):
            continue
        value = int(text, 0) if re.fullmatch(r'[-+]?(0x[0-9a-fA-F]+|\d+)', text) else float(text)
        short = name[len('RSL_'):]
        assert hasattr(_lib, short) or hasattr(_lib, name), f'{name} is neither mirrored in rsl/_lib.py nor HEADER_ONLY'
        got = getattr(_lib, short) if hasattr(_lib, short) else getattr(_lib, name)
        assert got == value and type(got) is type(value), (name, got, value)
        mirrored += 1
    assert mirrored >= 27
    ids = {int(v, 0): k for k, v in defs.items() if k.startswith('RSL_K_') and k != 'RSL_K_COUNT'}
    assert len(_lib.K_NAMES) == int(defs['RSL_K_COUNT']) == len(ids)
    for i, n in enumerate(_lib.K_NAMES):
        assert ids[i] == 'RSL_K_' + n.upper(), (i, n, ids[i])


def test_library_reads_no_environment():
    """The product librsl.so selects no kernel variant from its caller's environment: it does not
    import getenv / secure_getenv at all.  The ablation switches exist only in the development build
    (make dev -> librsl_dev.so, -DRSL_DEV_KNOBS), which the runtime loads only when RSL_LIBRARY names it."""
    import subprocess
    from rsl import _lib
    path = os.path.join(ROOT, 'radar-slam_amd', 'lib', 'librsl.so')
    assert os.path.abspath(_lib.LIB_PATH) == os.path.abspath(path) or 'RSL_LIBRARY' in os.environ
    out = subprocess.run(['nm', '-D', '--undefined-only', path], capture_output=True, text=True, check=True).stdout
    syms = {ln.split()[-1].split('@')[0] for ln in out.splitlines() if ln.strip()}
    assert not syms & {'getenv', 'secure_getenv', '__secure_getenv'}, sorted(syms & {'getenv', 'secure_getenv'})
    srcs = os.path.join(ROOT, 'radar-slam_amd', 'csrc')
    for fn in sorted(os.listdir(srcs)):
        if fn.endswith(('.hip', '.h')):
            src = open(os.path.join(srcs, fn)).read()
            # every getenv in the kernel sources sits inside an RSL_DEV_KNOBS block
            for m in re.finditer(r'getenv\(', src):
                head = src[:m.start()]
                assert head.rfind('#ifdef RSL_DEV_KNOBS') > head.rfind('#endif'), f'{fn}: getenv outside RSL_DEV_KNOBS'


def test_fft_support_table():
    import rsl
    lib = rsl.load()
    for n in (8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096, 25, 50, 100, 200, 400, 800, 1600):
        assert lib.rsl_fft_supported(n) == 1
    for n in (1, 3, 11, 13, 59, 300, 4095):
        assert lib.rsl_fft_supported(n) == 2
    for n in (0, -4, 4097, 8192):
        assert lib.rsl_fft_supported(n) == 0


def test_fft_support_table_exhaustive():
    """1 exactly for the 17 planned lengths (the list tests/test_gpu_fft_sizes.py runs one case each for), 2 for every
    other length up to 4096, 0 outside."""
    import rsl
    import rds_ref
    lib = rsl.load()
    assert len(set(rds_ref.PLANNED)) == 17
    assert sorted(rds_ref.PLANNED) == [8, 16, 25, 32, 50, 64, 100, 128, 200, 256, 400, 512, 800, 1024, 1600, 2048, 4096]
    for n in range(1, 4097):
        assert lib.rsl_fft_supported(n) == (1 if n in rds_ref.PLANNED else 2), n
    for n in (0, -1, 4097):
        assert lib.rsl_fft_supported(n) == 0, n


def test_wrapped_scratch_sizes():
    """The ABI's scratch sizes of the two wrapped solvers, whatever lays the buffers out: rsl_wrapped_scratch_bytes =
    8 (6 n + 36 + 8 (g^2 + e)); rsl_wrapped_search_scratch_bytes = 8 (9 n + 42 + 4 ceil(gx gy / 256) + 14 (nbest + e))
    with ceil(width / spacing) points per axis clamped to [1, 32768]; -1 for arguments out of range."""
    import math
    import rsl
    lib = rsl.load()
    for n, g, e in ((0, 0, 0), (1, 0, 1), (4, 0, 3), (7, 1, 0), (20, 3, 2), (61, 64, 5), (1000, 512, 0)):
        assert lib.rsl_wrapped_scratch_bytes(n, g, e) == 8 * (6 * n + 36 + 8 * (g * g + e)), (n, g, e)
    for bad in ((-1, 4, 0), (4, -1, 0), (4, 4, -1)):
        assert lib.rsl_wrapped_scratch_bytes(*bad) == -1, bad

    six = ctypes.c_double * 6

    def search_bytes(n, lo, hi, spacing, nbest, e):
        return lib.rsl_wrapped_search_scratch_bytes(n, six(*lo, 0, 0, 0, 0), six(*hi, 0, 0, 0, 0), spacing, nbest, e)

    def points(width, spacing):
        return min(max(math.ceil(width / spacing), 1), 32768)

    # the last boxes: a collapsed axis (lo == hi) gets one point; an axis of more than 32768 spacings is clamped
    for n, lo, hi, spacing, nbest, e in ((0, (-1.0, -1.0), (1.0, 1.0), 0.5, 1, 0),
                                         (4, (-2.0, -1.0), (2.0, 3.0), 0.25, 64, 2),
                                         (7, (0.0, 0.0), (10.0, 0.3), 0.03, 3, 0),
                                         (20, (-2.0, -2.0), (2.0, 2.0), 0.0097, 64, 5),
                                         (61, (-1.0, 5.0), (1.0, 5.0), 0.125, 8, 1),
                                         (5, (3.0, -4.0), (3.0, -4.0), 0.1, 2, 0),
                                         (9, (-50.0, 0.0), (50.0, 0.001), 0.001, 1024, 0)):
        gx, gy = points(hi[0] - lo[0], spacing), points(hi[1] - lo[1], spacing)
        want = 8 * (9 * n + 42 + 4 * ((gx * gy + 255) // 256) + 14 * (nbest + e))
        assert search_bytes(n, lo, hi, spacing, nbest, e) == want, (n, lo, hi, spacing, nbest, e, gx, gy)
    box = ((-1.0, -1.0), (1.0, 1.0), 0.5)
    for n, nbest, e in ((-1, 4, 0), (4, 0, 0), (4, 4, -1)):
        assert search_bytes(n, *box, nbest, e) == -1, (n, nbest, e)
    assert lib.rsl_wrapped_search_scratch_bytes(4, None, six(), 0.5, 4, 0) == -1
    assert lib.rsl_wrapped_search_scratch_bytes(4, six(), None, 0.5, 4, 0) == -1


def test_null_handle_errors():
    import rsl
    lib = rsl.load()
    assert lib.rsl_sync(None) == 1
    assert lib.rsl_rds(None, None, 1, 8, 64, 0, 64, 256, None, 1, None, None) == 1
    assert lib.rsl_last_error(None) == b'null handle'
    # every entry point that takes the handle first and returns a status, with a null handle and zero / null arguments:
    # RSL_ERR_INVALID before anything is read, no message stored anywhere.  rsl_destroy(NULL) is a no-op by contract;
    # rsl_timing_spans returns a count, -1 for a refusal.
    from rsl import _lib
    walked = []
    for name, (res, args) in _lib.SIGNATURES.items():
        if res is not ctypes.c_int or not args or args[0] is not ctypes.c_void_p:
            continue
        zeros = [None if t is ctypes.c_void_p or issubclass(t, ctypes._Pointer) else t(0).value for t in args[1:]]
        want = {'rsl_destroy': 0, 'rsl_timing_spans': -1}.get(name, 1)
        assert getattr(lib, name)(None, *zeros) == want, name
        assert lib.rsl_last_error(None) == b'null handle', name
        walked.append(name)
    assert walked == list(_lib.CONVERTERS) and len(walked) >= 48  # the other rows of the table take no handle
    group = ctypes.c_int(7)  # nothing is written through a null handle either
    assert lib.rsl_rds_detect(None, None, 0, 0, 0, 0, 0, 0, None, 0, None, None, 0.0, 0, 0, None, None, None, None,
                              ctypes.byref(group)) == 1 and group.value == 7


def test_steer_table_layout():
    """MFMA A-operand layout (v_mfma_f32_16x16x4_f32: lane l holds A[l&15][4s + (l>>4)]) built by the
    library's host helper equals a direct construction from the [Re; Im] stacked steering rows."""
    import rsl
    lib = rsl.load()
    G, M = 361, 8
    grid = O.azimuth_grid()
    st = O.steering_matrix(grid, M)
    n = lib.rsl_steer_table_floats(G, M)
    out = np.zeros(n, np.float32)
    nt, fl = ctypes.c_int(), ctypes.c_int()
    flat = np.ascontiguousarray(st).view(np.float64)
    rc = lib.rsl_steer_table_build(flat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), G, M,
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(nt),
                                   ctypes.byref(fl))
    assert rc == 0 and nt.value == (2 * G + 15) // 16 and fl.value == 1
    rows = np.zeros((nt.value * 16, 2 * M))
    rows[0:2 * G:2] = np.concatenate([st.real, st.imag], axis=1)
    rows[1:2 * G:2] = np.concatenate([-st.imag, st.real], axis=1)
    n32 = nt.value * 64 * 4
    tab = out[:n32].reshape(nt.value, 1, 64, 4)
    for t in range(nt.value):
        for lane in range(64):
            for s in range(4):
                assert tab[t, 0, lane, s] == np.float32(rows[16 * t + (lane & 15), 4 * s + (lane >> 4)])
    # the real GEMM on these rows reproduces |a^H s|^2
    rs = np.random.RandomState(0)
    s = rs.randn(5, M) + 1j * rs.randn(5, M)
    S = np.concatenate([s.real, s.imag], axis=1).T
    D = rows[:2 * G] @ S
    g = D[0::2] ** 2 + D[1::2] ** 2
    assert np.allclose(g.T, np.abs(s @ st.conj().T) ** 2)


def test_host_tables_match_oracle():
    from rsl import tables
    for Tc in (3.2e-6, 25.6e-6, 40e-6, 51.2e-6):
        S = tables.samples_per_chirp(Tc, 10e6)
        ref = O.reference_chirp(77e9, 1e9, Tc, 10e6)
        assert np.array_equal(tables.reference_chirp(77e9, 1e9, Tc, 10e6), ref)
        t = tables.chirp_table(77e9, 1e9, Tc, 10e6, 'hann', S)
        assert np.array_equal(t, np.conj(ref) * O.window('hann', S))
        i_lo, i_hi = tables.range_gate(1e9, S, 1.0, 200.0)
        r = O.range_axis(1e9, S)
        ok = (r >= 1.0) & (r <= 200.0)
        assert ok[i_lo:i_hi + 1].all() and ok.sum() == i_hi - i_lo + 1
    with pytest.raises(ValueError):
        tables.chirp_table(77e9, 1e9, 40e-6, 10e6, 'hann', 256)
    with pytest.raises(ValueError):
        tables.window_values('kaiser', 16)
    assert np.array_equal(tables.azimuth_grid(), O.azimuth_grid())
    st = tables.steering_matrix(O.azimuth_grid(), np.arange(8) * (3e8 / 77e9 / 2), 3e8 / 77e9)
    assert np.array_equal(st, O.steering_matrix(O.azimuth_grid(), 8))
    # threshold: p + 1e-12 > 10^(thr/10)  <=>  p > thr_p
    thr = tables.power_threshold(-20.0)
    for p in (0.0099999, 0.01, 0.0100001):
        assert (p > thr) == (10 * np.log10(p + 1e-12) > -20.0)


def _norm_default(v):
    if v is None:
        return None
    try:
        return repr(ast.literal_eval(v))
    except Exception:
        return v.replace(' ', '')


def _norm_obj(d):
    if d is inspect.Parameter.empty:
        return None
    if isinstance(d, np.ndarray):
        return f"np.array({d.tolist()})".replace(' ', '')
    return repr(d)


def test_dropin_surface_matches_reference():
    import importlib
    ref = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'ref_signatures.json')))
    for mod, members in ref.items():
        m = importlib.import_module(mod)
        for name, spec in members.items():
            obj = getattr(m, name)
            if isinstance(spec, dict):
                for meth, params in spec.items():
                    sig = inspect.signature(getattr(obj, meth))
                    got = [[p.name, _norm_obj(p.default)] for p in sig.parameters.values()]
                    want = [[n, _norm_default(d)] for n, d in params]
                    if meth != '__init__' or name != 'PoseIntegrator':
                        assert got == want, (mod, name, meth, got, want)
                    else:
                        assert [g[0] for g in got] == [w[0] for w in want]
            else:
                sig = inspect.signature(obj)
                got = [[p.name, _norm_obj(p.default)] for p in sig.parameters.values()]
                want = [[n, _norm_default(d)] for n, d in spec]
                assert got == want, (mod, name, got, want)


def test_pose_integration_dropin_needs_device(golden):
    """The drop-in PoseIntegrator integrates on the device (no CPU fallback): without one it raises; its golden
    parity is tests/test_gpu_traj.py::test_pose_integration_dropin_vs_golden."""
    import torch
    from src.pose_integration.pose_integration import PoseIntegrator
    if torch.cuda.is_available():
        pytest.skip('device present')
    z = golden('pose')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        PoseIntegrator().integrate_translational_velocity(z['vel'], z['ts'])
    with pytest.raises(ValueError, match='Unknown integration method'):
        PoseIntegrator(integration_method='rk4').integrate_translational_velocity(z['vel'], z['ts'])
    # [N, 2] velocities: the reference's 3-vector + 2-vector broadcast error (pose_integration.py:88), before any
    # device work
    with pytest.raises(ValueError, match='broadcast'):
        PoseIntegrator().integrate_translational_velocity(z['vel'][:, :2], z['ts'])


def test_product_path_has_no_oracle_import():
    """The product package never imports the oracle (test infrastructure only)."""
    pkg = os.path.join(ROOT, 'radar-slam_amd')
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith('.py'):
                txt = open(os.path.join(dp, f)).read()
                assert 'radar_oracle' not in txt and "'oracle'" not in txt, f


def test_context_requires_device():
    import torch
    import rsl
    if torch.cuda.is_available():
        pytest.skip('device present')
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rsl.Context(0)


def test_steer_table_fp64_transposed():
    """The table's last section is the reference's fp64 steering matrix transposed, steerT[m][g] (complex128), at a
    16-B aligned offset: k_doa_fixup's exact re-scan reads it (built once here instead of per rsl_doa call)."""
    import rsl
    lib = rsl.load()
    for G, M in ((361, 8), (181, 16), (91, 4)):
        st = O.steering_matrix(O.azimuth_grid(search_resolution=180.0 / (G - 1)), M)
        assert st.shape == (G, M)
        n = lib.rsl_steer_table_floats(G, M)
        out = np.zeros(n, np.float32)
        nt, fl = ctypes.c_int(), ctypes.c_int()
        flat = np.ascontiguousarray(st).view(np.float64)
        assert lib.rsl_steer_table_build(flat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), G, M,
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(nt),
                                         ctypes.byref(fl)) == 0
        off = n - 4 * G * M
        assert off % 4 == 0
        tT = out[off:].view(np.complex128).reshape(M, G)
        assert np.array_equal(tT, st.T)


def _toeplitz_rows(lib, st):
    """Decode the Toeplitz f16 hi/lo section of the steering table into T_hi, T_lo [rows, 16*KB]."""
    G, M = st.shape
    n = lib.rsl_steer_table_floats(G, M)
    out = np.zeros(n, np.float32)
    nt, fl = ctypes.c_int(), ctypes.c_int()
    flat = np.ascontiguousarray(st).view(np.float64)
    assert lib.rsl_steer_table_build(flat.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), G, M,
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), ctypes.byref(nt),
                                     ctypes.byref(fl)) == 0
    KB = 1 if M <= 8 else 2
    nt32 = (G + 31) // 32
    nt32 += nt32 & 1
    o = nt.value * 64 * 4 * (1 if M <= 8 else 2)
    h = out[o:o + nt32 * KB * 2 * 64 * 4].view(np.float16).reshape(nt32, KB, 2, 64, 8)
    T = np.zeros((2, nt32 * 32, 16 * KB))
    for t in range(nt32):
        for kb in range(KB):
            for lane in range(64):
                for j in range(8):
                    k = 16 * kb + 8 * (lane >> 5) + j
                    T[0, 32 * t + (lane & 31), k] = h[t, kb, 0, lane, j]
                    T[1, 32 * t + (lane & 31), k] = h[t, kb, 1, lane, j]
    return fl.value, T


@pytest.mark.parametrize('M', [8, 16, 4])
def test_toeplitz_table_reproduces_steering_scan(M):
    """|a^H s|^2 = r0 + 2 sum_k (Re r_k cos k phi + Im r_k sin k phi): the f16 hi/lo Toeplitz operand of the
    DoA fast path (rsl_doa_toep.hip) reproduces the reference beamforming spectrum to < 1e-6."""
    import rsl
    lib = rsl.load()
    grid = O.azimuth_grid()
    st = O.steering_matrix(grid, M)
    flags, T = _toeplitz_rows(lib, st)
    assert flags == 1
    G = len(grid)
    Tf = T[0] + T[1]
    rs = np.random.RandomState(1)
    s = rs.randn(20, M) + 1j * rs.randn(20, M)
    s /= np.linalg.norm(s, axis=1, keepdims=True)
    e = np.zeros((20, Tf.shape[1]))
    e[:, 0] = 1.0
    for k in range(1, M):
        r = np.sum(s[:, k:] * np.conj(s[:, :M - k]), axis=1)
        e[:, 2 * k - 1], e[:, 2 * k] = r.real, r.imag
    P = e @ Tf[:G].T
    ref = np.abs(s @ st.conj().T) ** 2
    assert np.abs(P - ref).max() < 1e-6
    assert (Tf[G:] == Tf[G - 1]).all()  # padding rows replicate the last grid point


def test_toeplitz_flag_off_for_nonuniform_array():
    import rsl
    lib = rsl.load()
    grid = O.azimuth_grid()
    st = O.steering_matrix(grid, 8)
    st[:, 3] *= np.exp(0.3j)  # not a uniform linear array
    flags, _ = _toeplitz_rows(lib, st)
    assert flags == 0
