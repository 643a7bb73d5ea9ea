"""Closed forms of the fixed MVDR design (csrc/mvdr_kernels.hip and its solvers chol_blocked.h / chol_reg.h), in float64 numpy.

No GPU, no oracle, no library code.  tests/test_mvdr_cpu.py proves what makes these forms usable as truth (two float64 routes agree,
every input is well conditioned, the planted pivot failures fail where they are planted); tests/test_gpu_mvdr_closed_form.py holds
every solver form to them under closed_forms.accept.

    diffuse model   Gamma_mn[k] = sinc(2 fs k d_mn / (M c)), k = 0 .. M/2, sinc(x) = sin(pi x) / (pi x), coincident microphones 1
    loading         R_ii += w                      divide_nondiagonal   R_mn /= 1 + mu for m != n
    design          z = R^-1 d,  Lambda = d^H z,  w = z / (N Lambda);  a bin whose factorisation stops: z = d (identity_answer)
    conventions     weights: global bin 0 (every stream's bin 0 of stacked streams) is the all-ones row; Lambda is computed for every bin

design_f32 evaluates the design in complex64 / float32 the plain way -- a column-by-column right-looking Cholesky, column sweeps for the
two substitutions -- and, as a second summation order, as a blocked left-looking factorisation with 16-column panels.  The first is the
YARDSTICK of the GPU tests (what float32 achieves on the same inputs), the second tells a kernel whose own order is legitimately worse
from one that is wrong.
"""
import functools
import os
import re

import numpy as np

from tests.closed_forms import FACTOR, FLOOR, accept, cfratio_line  # noqa: F401  (re-exported for the two test modules)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SSPEED = 343740.0                     # mm / s, the engine's default


# --------------------------------------------------------------------------- float64 closed forms
def diffuse_cf(mpos, M, fs, c=SSPEED, bins=None):
    """mpos [N][3] (the float32 values the kernel reads, widened) -> Gamma float64 [M/2+1][N][N] (bins: only these rows of it)."""
    p = np.asarray(mpos, np.float32).astype(np.float64)
    dist = np.sqrt(np.sum((p[:, None, :] - p[None, :, :]) ** 2, axis=-1))
    k = np.arange(M // 2 + 1, dtype=np.float64) if bins is None else np.asarray(bins, np.float64)
    x = (2.0 * float(fs) * k / (float(M) * float(c)))[:, None, None] * dist[None]
    return np.where(x == 0.0, 1.0, np.sinc(x))


def load_cf(R, w):
    """R [..][N][N] -> R + w I in float64 / complex128 (w: the float32 value the kernel receives)."""
    R = np.array(R, np.complex128 if np.iscomplexobj(R) else np.float64)
    n = R.shape[-1]
    R[..., np.arange(n), np.arange(n)] += float(np.float32(w))
    return R


def divide_nondiag_cf(R, mu):
    """R_mn / (1 + mu) for m != n, the diagonal as it is (mu: the float32 value the kernel receives)."""
    R = np.array(R, np.complex128 if np.iscomplexobj(R) else np.float64)
    n = R.shape[-1]
    off = ~np.eye(n, dtype=bool)
    R[..., off] = R[..., off] / (1.0 + float(np.float32(mu)))
    return R


def design_cf(R, d):
    """R complex64 [K][N][N], d complex64 [K][N], widened -> (w complex128 [K][N], Lambda complex128 [K]).  Every bin is solved: the
    all-ones rows are a convention of the weights alone (dc_rows), never of Lambda."""
    R, d = np.asarray(R).astype(np.complex128), np.asarray(d).astype(np.complex128)
    N = R.shape[-1]
    z = np.linalg.solve(R, d[..., None])[..., 0]
    lam = np.sum(np.conj(d) * z, axis=-1)
    return z / (N * lam[:, None]), lam


def design_cf_chol(R, d):
    """The same design by a second float64 route: numpy's (LAPACK) Cholesky factor and two triangular solves written out here."""
    R, d = np.asarray(R).astype(np.complex128), np.asarray(d).astype(np.complex128)
    K, N = d.shape
    L = np.linalg.cholesky(R)
    z = np.empty_like(d)
    for k in range(K):
        y = np.linalg.solve(L[k], d[k])                          # (general solves of triangular matrices: LU without a row swap is
        z[k] = np.linalg.solve(L[k].conj().T, y)                 #  the substitution itself)
    lam = np.sum(np.conj(d) * z, axis=-1)
    return z / (N * lam[:, None]), lam


def dc_rows(w, first_bin=0, kper=0):
    """The weights' convention: global bin 0 (kper = 0, the slice starting at first_bin) or every stream's bin 0 (kper > 0) is all ones."""
    w = np.array(w)
    for k in range(w.shape[0]):
        if ((k % kper) == 0) if kper > 0 else (k + first_bin == 0):
            w[k] = 1.0
    return w


def identity_answer(d):
    """invR = I: w = d / (N d^H d), float64.  d [..][N]."""
    d = np.asarray(d).astype(np.complex128)
    N = d.shape[-1]
    return d / (N * np.sum(np.abs(d) ** 2, axis=-1, keepdims=True))


# --------------------------------------------------------------------------- the float32 yardstick
def chol_f32(R, order="plain"):
    """Complex64 Cholesky factor of a batch R [K][N][N] -> (L with garbage above the diagonal, pivots float32 [K][N]).
    "plain": right-looking, column by column.  "blocked": left-looking 16-column panels, the update a complex64 matmul, the panel itself
    column by column.  A pivot <= 0 is recorded and the factorisation runs on into NaN: callers look at the pivots."""
    A = np.array(R, np.complex64)
    K, N, _ = A.shape
    piv = np.zeros((K, N), np.float32)

    def column(j, hi):
        p = A[:, j, j].real.copy()
        piv[:, j] = p
        dj = np.sqrt(p)
        A[:, j, j] = dj
        col = A[:, j + 1:, j] / dj[:, None]
        A[:, j + 1:, j] = col
        if j + 1 < hi:
            A[:, j + 1:, j + 1:hi] -= col[:, :, None] * np.conj(col[:, None, :hi - j - 1])

    with np.errstate(invalid="ignore", divide="ignore"):
        if order == "plain":
            for j in range(N):
                column(j, N)
        else:
            assert order == "blocked"
            for jb in range(0, N, 16):
                hi = min(jb + 16, N)
                if jb:
                    A[:, jb:, jb:hi] -= A[:, jb:, :jb] @ np.conj(A[:, jb:hi, :jb]).transpose(0, 2, 1)
                for j in range(jb, hi):
                    column(j, hi)
    assert A.dtype == np.complex64 and piv.dtype == np.float32
    return A, piv


def design_f32(R, d, order="plain"):
    """design_cf in complex64: chol_f32, forward and back substitution as column sweeps, Lambda = z^H d summed in complex64 (the order of
    the reference's zdotc(z, d); for a Hermitian R the same real number as d^H z), w = z / (N Lambda).  -> (w complex64 [K][N], Lambda [K])."""
    d = np.asarray(d, np.complex64)
    K, N = d.shape
    L, _ = chol_f32(R, order)
    dg = L[:, np.arange(N), np.arange(N)].real
    z = d.copy()
    for j in range(N):
        z[:, j] /= dg[:, j]
        z[:, j + 1:] -= L[:, j + 1:, j] * z[:, j:j + 1]
    for j in range(N - 1, -1, -1):
        z[:, j] /= dg[:, j]
        z[:, :j] -= np.conj(L[:, j, :j]) * z[:, j:j + 1]
    lam = np.sum(np.conj(z) * d, axis=-1)
    w = z / (np.float32(N) * lam)[:, None]
    assert w.dtype == np.complex64 and lam.dtype == np.complex64
    return w, lam


# --------------------------------------------------------------------------- inputs: complex64, exactly Hermitian, real diagonal
def _hermitian64(R):
    R = np.asarray(R).astype(np.complex64)
    lo = np.tril(R, -1)
    out = lo + lo.conj().T
    n = R.shape[-1]
    out[np.arange(n), np.arange(n)] = R[np.arange(n), np.arange(n)].real
    return out


def wishart(N, extra=40, load=0.05, seed=0):
    """A A^H / (N + extra) + load I, A complex normal [N][N + extra]: dense complex."""
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(N, N + extra)) + 1j * rng.normal(size=(N, N + extra))
    return _hermitian64(A @ A.conj().T / (N + extra) + load * np.eye(N))


def ula(N, spacing=20.0):
    """N microphones on the x axis, `spacing` mm apart, centred.  float32 [N][3]."""
    p = np.zeros((N, 3), np.float32)
    p[:, 0] = (np.arange(N) - (N - 1) / 2.0) * spacing
    return p


def diffuse_loaded(N, k, mu=0.01, M=64, fs=16000.0):
    """The product's own input: bin k of the diffuse model of a 20 mm ULA, rounded to float32, plus float32 loading.  Real valued."""
    g = diffuse_cf(ula(N), M, fs, bins=[k])[0].astype(np.float32)
    g[np.arange(N), np.arange(N)] += np.float32(mu)
    return _hermitian64(g)


def scaled_identity(N, c):
    """c I: z = d / c, Lambda = d^H d / c, w = d / (N d^H d) whatever c is."""
    return (np.float32(c) * np.eye(N)).astype(np.complex64)


def fails_at(N, j, seed=0):
    """A Wishart matrix whose diagonal entry j is lowered until the Schur complement of the leading j x j block -- pivot j of any Cholesky
    order -- is -0.5 of what it was (float64, from the leading block).  The leading block is untouched: every earlier pivot stays."""
    R = wishart(N, 40, 0.05, seed)
    A = R.astype(np.complex128)
    s = A[j, j].real
    if j > 0:
        s -= np.vdot(A[:j, j], np.linalg.solve(A[:j, :j], A[:j, j])).real
    assert s > 0.0
    R[j, j] = np.float32(A[j, j].real - 1.5 * s)
    return R


def unit_d(K, N, seed=0):
    """exp(j phi) / N, complex64 [K][N]: d^H d = 1 / N, every channel counts the same."""
    rng = np.random.default_rng(seed + 4242)
    return (np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, (K, N))) / N).astype(np.complex64)


# --------------------------------------------------------------------------- the case lists of the GPU module
KINDS = ("wishart", "diffuse", "identity")
DIFFUSE_BINS = (3, 1, 9, 32)          # the model bin behind each row of a case (model bin 0, all ones + loading, has cond 100 N)
IDENTITY_C = (0.7, 0.3, 3.0, 11.0)
K_CASE = 4                            # bin 0 and three solved bins
SIZES = {
    "lds": (1, 2, 3, 16, 17, 63, 64, 100, 137),
    "reg": (1, 2, 14, 15, 16, 31, 32, 63, 64, 127, 128, 137, 255, 256, 270, 271),
    "panel": (1, 15, 16, 17, 33, 64, 65, 255, 256, 257, 272, 273, 287, 289, 300),
    "default": (63, 64, 137, 271, 272),
}
DEFAULT_RUNS = {63: "lds", 64: "reg", 137: "reg", 271: "reg", 272: "panel"}     # the form the shipped dispatch claims per size
EVERY_SIZE = tuple(range(137, 272))   # one system each on the register-resident solver
MODE_N = {"lds": 16, "reg": 160, "panel": 273}
FAIL_N = {"lds": (40,), "reg": (40, 200), "panel": (40, 273)}
ENV = {
    "lds": {"BTK_MVDR_REG_MIN": "100000"},
    "reg": {"BTK_MVDR_REG_MIN": "1"},
    "panel": {"BTK_MVDR_REG_MIN": "1", "BTK_WPE_SOLVE_PANEL": "1"},
    "default": {},
}
LDS_CAP = 150 * 1024


def panel_lds_bytes(P):
    """cholb::lds_bytes of csrc/chol_blocked.h, its constants read from the header."""
    src = open(os.path.join(ROOT, "distant_speech_recognition_amd", "csrc", "chol_blocked.h")).read()
    nb = int(re.search(r"constexpr int CH_NB = (\d+);", src).group(1))
    assert re.search(r"constexpr int CH_LD = CH_NB \+ 1;", src)
    assert ("inline size_t lds_bytes(int P) { return sizeof(float2) * (size_t)((P + 1) & ~1) + sizeof(float) * 512 + "
            "sizeof(float2) * (size_t)P * CH_LD; }") in src, "cholb::lds_bytes changed: restate it here"
    return 8 * ((P + 1) & ~1) + 4 * 512 + 8 * P * (nb + 1)


@functools.lru_cache(maxsize=None)
def panel_max():
    """The largest N whose panel fits the LDS cap of the blocked solver's launch."""
    P = 1
    while panel_lds_bytes(P + 1) <= LDS_CAP:
        P += 1
    return P


def fail_columns(N):
    return (0, 1, 15, 16, 17, N - 17, N - 16, N - 1)


def case_list(form):
    """[(kind, N, K)] of the weight / Lambda cases of a form."""
    out = [(kind, N, K_CASE) for N in SIZES[form] for kind in KINDS]
    if form == "reg":
        out += [("wishart", N, 2) for N in EVERY_SIZE]
    if form == "panel":
        out += [(kind, panel_max(), 2) for kind in KINDS]
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(kind, N, K):
    """(R complex64 [K][N][N], d complex64 [K][N]) of one case; the same arrays in every process that asks."""
    if kind == "wishart":
        R = np.stack([wishart(N, 40, 0.05, 1000 * N + 10 * K + b) for b in range(K)])
    elif kind == "diffuse":
        R = np.stack([diffuse_loaded(N, DIFFUSE_BINS[b]) for b in range(K)])
    else:
        assert kind == "identity"
        R = np.stack([scaled_identity(N, IDENTITY_C[b]) for b in range(K)])
    d = unit_d(K, N, 31 * N + KINDS.index(kind))
    R.setflags(write=False); d.setflags(write=False)
    return R, d


@functools.lru_cache(maxsize=None)
def case_forms(kind, N, K, order="plain"):
    """(w_cf, Lambda_cf, w_f32, Lambda_f32) of a case, computed once per process."""
    R, d = case_inputs(kind, N, K)
    w, lam = design_cf(R, d)
    w32, lam32 = design_f32(R, d, order)
    return w, lam, w32, lam32


def fail_inputs(N, first_bin=1):
    """(R [19][N][N], d, planted flags [19]): a bin failing at each of fail_columns(N) and one with a NaN diagonal entry, every one
    between two solvable bins; R_clean has the planted bins replaced by the identity."""
    cols = fail_columns(N)
    K = 2 * (len(cols) + 1) + 1
    R = np.stack([wishart(N, 40, 0.05, 77 * N + b) for b in range(K)])
    flags = np.zeros(K, np.int32)
    for i, j in enumerate(cols):
        R[2 * i + 1] = fails_at(N, j, 77 * N + 2 * i + 1)
        flags[2 * i + 1] = 1
    R[K - 2, N // 2, N // 2] = np.nan
    flags[K - 2] = 1
    clean = R.copy()
    clean[flags == 1] = np.eye(N, dtype=np.complex64)
    return R, clean, unit_d(K, N, 5 * N), flags


def mode_inputs(N, S=3, K=5):
    """(R [S][K][N][N], d [S][K][N]) of the slice / stacked-stream comparisons: bit equality, so no closed form."""
    R = np.stack([np.stack([wishart(N, 40, 0.05, 500 * N + 10 * s + b) for b in range(K)]) for s in range(S)])
    return R, unit_d(S * K, N, 9 * N).reshape(S, K, N)


def distortionless_miss(w, d):
    """|w^H d - 1/N| per row, float64."""
    w, d = np.asarray(w).astype(np.complex128), np.asarray(d).astype(np.complex128)
    return np.abs(np.sum(np.conj(w) * d, axis=-1) - 1.0 / d.shape[-1])
