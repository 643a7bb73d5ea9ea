"""Test helper: csvdc with job = 11 (singular vectors) and the pseudo-inverse assembly of csrc/linpack_f32.h built by g++ as
serial host code (tests/cpp/linpack_full_host.cc); the reference's own compiled csvdc with its U and V; and the numpy
restatement of pseudoinverse()'s assembly (beamformer/beamformer.cc:262-280) that the tests use as the expected value."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_lib = None


def lib():
    global _lib
    if _lib is None:
        out = os.path.join(tempfile.mkdtemp(prefix="lpkf_"), "liblpkfullhost.so")
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC",
                               "-I" + os.path.join(ROOT, "distant_speech_recognition_amd", "csrc"),
                               os.path.join(ROOT, "tests", "cpp", "linpack_full_host.cc"), "-o", out])
        _lib = C.CDLL(out)
        _lib.lpk_host_csvdc_full.restype = C.c_int
        _lib.lpk_host_csvdc_full.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.lpk_host_pinv_assemble.restype = C.c_int
        _lib.lpk_host_pinv_assemble.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p]
    return _lib


def _p(x):
    return x.ctypes.data_as(C.c_void_p)


def csvdc_full(A):
    """A complex [n][p] -> (s [m], e [m], U [n][n], V [p][p], info), m = min(n + 1, p); U[i, k] is the reference's u[i + k * ldu]."""
    A = np.ascontiguousarray(A, np.complex64)
    n, p = A.shape
    m = min(n + 1, p)
    s = np.zeros(m, np.float32)
    e = np.zeros(m, np.float32)
    u = np.zeros((n, n), np.complex64, order="F")
    v = np.zeros((p, p), np.complex64, order="F")
    info = lib().lpk_host_csvdc_full(_p(A), n, p, _p(s), _p(e), _p(u), _p(v))
    return s, e, u, v, int(info)


def ref_csvdc_full(orc, A):
    """The reference's compiled csvdc (oracle/_ref) with job = 11: (s, e, U, V, info) as csvdc_full."""
    ref = orc.ref_lib()
    A = np.asarray(A).astype(np.complex64)
    n, p = A.shape
    a = np.asfortranarray(A).copy(order="F")
    s = np.zeros(n + p, np.complex64)
    e = np.zeros(n + p, np.complex64)
    u = np.zeros((n, n), np.complex64, order="F")
    v = np.zeros((p, p), np.complex64, order="F")
    info = ref.ref_csvdc(_p(a), n, n, p, _p(s), _p(e), _p(u), n, _p(v), p, 11)
    m = min(n + 1, p)
    return np.ascontiguousarray(s[:m].real), np.ascontiguousarray(e[:m].real), u, v, int(info)


def pinv_assemble(s, U, V, threshold=1.0e-8):
    """The host build of pinv_assemble: (invA complex64 [N][M], number of singular values under the threshold)."""
    M, N = U.shape[0], V.shape[0]
    s = np.ascontiguousarray(s[:N], np.float32)
    u = np.asfortranarray(U, np.complex64)
    v = np.asfortranarray(V, np.complex64)
    inv = np.zeros((N, M), np.complex64)
    below = lib().lpk_host_pinv_assemble(M, N, _p(s), _p(u), _p(v), float(threshold), _p(inv))
    return inv, int(below)


def pinv_restated(s, U, V, info=0, threshold=1.0e-8):
    """pseudoinverse() after csvdc, beamformer.cc:262-280, in numpy: real and imaginary parts as separate float32 arrays and one
    ufunc call per arithmetic operation, so that each rounds once to float32 and nothing fuses; k outermost and serial (the
    source's left-to-right sum); 1 / s[k] through float64 (complex division in the next wider type).  Returns
    (invA complex64 [N][M], ok)."""
    f32 = np.float32
    M, N = U.shape[0], V.shape[0]
    s = np.asarray(s[:N], f32)
    ok = info == 0
    sinv = np.zeros(N, f32)
    for k in range(N):
        if f32(np.sqrt(np.float64(s[k]) * np.float64(s[k]))) < f32(threshold):
            ok = False
        else:
            c = np.float64(s[k])
            sinv[k] = f32(c / (c * c))
    ur, ui = np.ascontiguousarray(U.real, f32), np.ascontiguousarray(U.imag, f32)
    vr, vi = np.ascontiguousarray(V.real, f32), np.ascontiguousarray(V.imag, f32)
    zero = f32(0.0)
    xr = np.zeros((N, M), f32)
    xi = np.zeros((N, M), f32)
    for k in range(N):
        # (v[j, k] * sinv[k]): (a + ib)(c + i0) = (a c - b 0) + i (a 0 + b c)
        a, b, c = vr[:, k], vi[:, k], sinv[k]
        pr = np.subtract(np.multiply(a, c), np.multiply(b, zero))
        pi = np.add(np.multiply(a, zero), np.multiply(b, c))
        # ... * conj(u[i, k]) = (pr + i pi)(g - ih): (pr g - pi (-h)) + i (pr (-h) + pi g)
        g, h = ur[:, k], np.negative(ui[:, k])
        tr = np.subtract(np.multiply.outer(pr, g), np.multiply.outer(pi, h))
        ti = np.add(np.multiply.outer(pr, h), np.multiply.outer(pi, g))
        xr = np.add(xr, tr)
        xi = np.add(xi, ti)
    return (xr + 1j * xi).astype(np.complex64), bool(ok)


def mvdr_from_inverse(inv, ok, d):
    """calc_mvdr_weights after pseudoinverse() (beamformer.cc:2381-2396) in float64: (w complex128 [N], Lambda)."""
    d = np.asarray(d, np.complex128)
    N = d.shape[0]
    inv = np.asarray(inv, np.complex128) if ok else np.eye(N, dtype=np.complex128)
    t = inv.conj().T @ d
    lam = np.vdot(t, d)
    return t / (lam * N), lam
