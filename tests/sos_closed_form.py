"""Closed forms of the batch second-order-statistics path in float64 numpy: covariance accumulation, the frame gate, the mask
counters, finalize_stats, the trace normalisation and the blind MVDR and GEV weight designs (lib/pybeamformer.py:1075-1093,
:1127-1147, :1200-1207, :1225-1263, :1280-1328), the input builders, the mutants and the acceptance rules that
tests/test_sos_cpu.py and tests/test_gpu_sos_closed_form.py share.  No GPU, no oracle, no library code, no tests.

Engine layouts: snapshots X [S][K][N][T] complex64, TF mask tf [S][K][T], frame gate fw [S][T], R [S][K][N][N].

    cov_form              R[s][k] = R0 + sum_t tf[s][k][t] fw[s][t] x x^H; a frame of weight 0 contributes nothing, whatever it holds
    mask_count_form       sum_t floor(tf) fw over tf > 0 (the reference's counters are integer arrays)
    gate_form             (energy > thr) * label, and its sum
    finalize_form         R / count, then (R + gamma tr(R) / N I) / (1 + gamma) when gamma > 0; count [S] or [S][K]
    trace_normalize_form  R / (tr R / N), the trace complex
    bmvdr_form            Z = solve(Rn, Rt), wqH = conj(Z[:, ref] / (offset + tr Z))
    gev_form              principal generalised eigenvector, v^H Rn v = 1, bin m times exp(-j angle <w_m, conj w_m-1>), conjugated

Every function takes dtype: np.float64 is the closed form; np.float32 evaluates the same sums in float32 / complex64, the
straightforward way (frame after frame added to a complex64 sum), and is the YARDSTICK: what float32 arithmetic achieves on
the given inputs.  accept_matrix is the element-wise rule built on it with closed_forms.FACTOR and closed_forms.FLOOR.

Phase of the GEV weights.  scipy leaves the phase of bin 0 open and the alignment chain hands it on: replacing w_0 by c w_0
(|c| = 1) multiplies EVERY aligned bin by c, so two correct results differ by ONE unit-modulus factor shared by all bins
(global_factor).  The kernel's own convention is a separate known answer: bin 0 is rotated so that its component of largest
modulus is real and positive (bin0="largest_real").
"""
import numpy as np

from tests.closed_forms import FACTOR, FLOOR

MUTANTS = ("weight_squared", "conj_swapped", "drop_last_odd_frame", "weak_channel_row_off", "mask_and_gate_not_multiplied",
           "trace_without_offset", "ref_row_for_column", "second_eigenvector", "no_phase_alignment", "unnormalised_gev")
COV_MUTANTS, BMVDR_MUTANTS, GEV_MUTANTS = MUTANTS[:5], MUTANTS[5:7], MUTANTS[7:]
OLD_FROBENIUS = 1e-5            # the per-bin rule of the older covariance tests, kept to show what it lets through


def _types(dtype):
    rt = np.dtype(dtype)
    assert rt in (np.dtype(np.float64), np.dtype(np.float32))
    return rt.type, (np.complex128 if rt == np.dtype(np.float64) else np.complex64)


# --------------------------------------------------------------------------------------------------- covariance
def frame_weights(shape, tf=None, fw=None, dtype=np.float64, mutant=None):
    """[S][K][T]: the weight of every frame in every bin (1 without weights)."""
    rt, _ = _types(dtype)
    S, K, T = shape
    w = np.ones((S, K, T), rt)
    if tf is not None:
        w = w * np.asarray(tf).astype(rt)
    if fw is not None and not (mutant == "mask_and_gate_not_multiplied" and tf is not None):
        w = w * np.asarray(fw).astype(rt)[:, None, :]
    if mutant == "weight_squared":
        w = w * w
    if mutant == "drop_last_odd_frame" and T % 2:
        w[..., T - 1] = 0
    assert w.dtype == rt
    return w


def cov_form(X, tf=None, fw=None, R0=None, dtype=np.float64, mutant=None):
    """X [S][K][N][T] -> R [S][K][N][N]."""
    assert mutant is None or mutant in COV_MUTANTS
    rt, ct = _types(dtype)
    X = np.asarray(X)
    S, K, N, T = X.shape
    w = frame_weights((S, K, T), tf, fw, dtype, mutant)
    live = w != 0
    Xc = X.astype(ct)
    R = np.zeros((S, K, N, N), ct) if R0 is None else np.asarray(R0).astype(ct).copy()
    if rt == np.float64:
        for s in range(S):
            for k in range(K):
                x = Xc[s, k][:, live[s, k]]                                  # a gated-off frame is never touched
                R[s, k] += (x * w[s, k][live[s, k]]) @ np.conj(x.T)
    else:
        for t in range(T):
            for s in range(S):
                for k in range(K):
                    if live[s, k, t]:
                        x = Xc[s, k, :, t]
                        R[s, k] += np.outer(x, (w[s, k, t] * np.conj(x)).astype(ct))
    assert R.dtype == ct
    if mutant == "conj_swapped":
        R = np.ascontiguousarray(np.swapaxes(R, -1, -2))
    if mutant == "weak_channel_row_off":
        for s in range(S):
            for k in range(K):
                i = int(np.argmin(np.diagonal(R[s, k]).real))
                R[s, k, i, :] *= 1.001
                R[s, k, :, i] *= 1.001
    return R


def mask_count_form(tf, fw=None, count0=None, dtype=np.float64):
    """[S][K]: count0 + sum_t floor(tf) fw over the frames with tf > 0."""
    rt, _ = _types(dtype)
    tf = np.asarray(tf).astype(rt)
    g = np.ones(tf.shape, rt) if fw is None else np.broadcast_to(np.asarray(fw).astype(rt)[:, None, :], tf.shape)
    c = np.zeros(tf.shape[:2], rt) if count0 is None else np.asarray(count0).astype(rt).copy()
    for t in range(tf.shape[-1]):
        c += np.where(tf[..., t] > 0, np.floor(tf[..., t]) * g[..., t], rt(0))
    return c


def gate_form(energy, threshold, label=None, count0=None, dtype=np.float64):
    """energy [S][T] float32, the threshold a float32 number -> (w [S][T], count [S])."""
    rt, _ = _types(dtype)
    e = np.asarray(energy, np.float32)
    w = (e > np.float32(threshold)).astype(rt)
    if label is not None:
        w = w * np.asarray(label).astype(rt)
    c = np.zeros(e.shape[0], rt) if count0 is None else np.asarray(count0).astype(rt).copy()
    for t in range(e.shape[1]):
        c += w[:, t]
    return w, c


def finalize_form(R, count, gamma=0.0, dtype=np.float64):
    """R [S][K][N][N], count [S] (per stream) or [S][K] (per bin)."""
    rt, ct = _types(dtype)
    R = np.asarray(R).astype(ct)
    N = R.shape[-1]
    c = np.asarray(count).astype(rt)
    c = c[:, None] if c.ndim == 1 else c
    R = R / c[:, :, None, None]
    if gamma > 0:
        scale = rt(gamma) * np.trace(R, axis1=-2, axis2=-1) / rt(N)
        R = (R + np.eye(N, dtype=rt) * scale[..., None, None]) / (rt(1) + rt(gamma))
    assert R.dtype == ct
    return R


def trace_normalize_form(R, dtype=np.float64):
    rt, ct = _types(dtype)
    R = np.asarray(R).astype(ct)
    out = R / (np.trace(R, axis1=-2, axis2=-1) / rt(R.shape[-1]))[..., None, None]
    assert out.dtype == ct
    return out


# --------------------------------------------------------------------------------------------------- weight designs
def bmvdr_form(Rt, Rn, ref_micx=0, offset=0.0, dtype=np.float64, mutant=None):
    """Rt, Rn [K][N][N] -> wqH [K][N]."""
    assert mutant is None or mutant in BMVDR_MUTANTS
    rt, ct = _types(dtype)
    Rt, Rn = np.asarray(Rt).astype(ct), np.asarray(Rn).astype(ct)
    K, N, _ = Rt.shape
    W = np.zeros((K, N), ct)
    for k in range(K):
        Z = np.linalg.solve(Rn[k], Rt[k])
        den = np.trace(Z) + (rt(0) if mutant == "trace_without_offset" else rt(offset))
        col = Z[ref_micx, :] if mutant == "ref_row_for_column" else Z[:, ref_micx]
        W[k] = np.conj(col / den)
    return W


def gev_pairs(Rt, Rn, route="scipy"):
    """(eigenvalues ascending [N], eigenvectors [N][N] with V^H Rn V = I) of one bin, float64, by one of two routes."""
    Rt, Rn = np.asarray(Rt, np.complex128), np.asarray(Rn, np.complex128)
    if route == "scipy":
        import scipy.linalg
        return scipy.linalg.eigh(Rt, Rn)
    assert route == "cholesky"
    Li = np.linalg.inv(np.linalg.cholesky(Rn))
    C = Li @ Rt @ np.conj(Li.T)
    e, V = np.linalg.eigh(0.5 * (C + np.conj(C.T)))
    return e, np.conj(Li.T) @ V


def gev_form(Rt, Rn, route="scipy", bin0=None, mutant=None):
    """Rt, Rn [K][N][N] -> wqH [K][N] complex128.  bin0="largest_real" states the kernel's convention for the phase of bin 0."""
    assert mutant is None or mutant in GEV_MUTANTS
    K, N, _ = np.asarray(Rt).shape
    W = np.zeros((K, N), np.complex128)
    for m in range(K):
        _, V = gev_pairs(Rt[m], Rn[m], route)
        v = V[:, -2 if (mutant == "second_eigenvector" and N > 1) else -1]
        if mutant == "unnormalised_gev":
            v = v / np.linalg.norm(v)
        if m == 0 and bin0 == "largest_real":
            v = v * np.exp(-1j * np.angle(v[np.argmax(np.abs(v))]))
        if m > 0 and mutant != "no_phase_alignment":
            v = v * np.exp(-1j * np.angle(np.inner(v, np.conj(W[m - 1]))))
        W[m] = v
    return np.conj(W)


def global_factor(W, Wcf):
    """The ONE unit-modulus c, computed over all bins jointly, that brings the closed form closest to W: W ~ c Wcf."""
    c = np.vdot(np.asarray(Wcf, np.complex128), np.asarray(W, np.complex128))
    return c / abs(c) if abs(c) > 0 else 1.0 + 0j


def weight_errors(W, Wcf, c=1.0):
    """Per bin: max_i |W - c Wcf| / max_i |Wcf|."""
    W, Wcf = np.asarray(W, np.complex128), np.asarray(Wcf, np.complex128)
    return np.max(np.abs(W - c * Wcf), axis=-1) / np.max(np.abs(Wcf), axis=-1)


def accept_weights(W, Wcf, up_to_factor=False):
    """max_i |W - c Wcf| <= FLOOR max_i |Wcf| in every bin.  Returns (ok, worst error)."""
    e = weight_errors(W, Wcf, global_factor(W, Wcf) if up_to_factor else 1.0)
    return bool(np.all(np.isfinite(e)) and np.all(e <= FLOOR)), float(np.max(e))


# --------------------------------------------------------------------------------------------------- acceptance of matrices
def e_elem(R, Rcf):
    """[..][N][N]: |R - Rcf|_ij / sqrt(Rcf_ii Rcf_jj), diagonals included; where a diagonal of Rcf is zero: 0 if R == Rcf, else inf."""
    R, Rcf = np.asarray(R, np.complex128), np.asarray(Rcf, np.complex128)
    d = np.abs(np.diagonal(Rcf, axis1=-2, axis2=-1))
    den = np.sqrt(d[..., :, None] * d[..., None, :])
    diff = np.abs(R - Rcf)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, diff / den, np.where(diff == 0, 0.0, np.inf))


def accept_matrix(R, R32, Rcf):
    """The element-wise rule.  R: the kernel's matrices, R32: the float32 yardstick, Rcf: the float64 closed form, [..][N][N].
         max e(R) <= max(FACTOR max e(R32), FLOOR),  e_ij = |R - Rcf|_ij / sqrt(Rcf_ii Rcf_jj)
       and a matrix whose closed form is exactly zero must be exactly zero.  Returns (ok, dict(e, y))."""
    R, R32, Rcf = np.asarray(R), np.asarray(R32), np.asarray(Rcf)
    assert R.shape == R32.shape == Rcf.shape
    finite = bool(np.all(np.isfinite(R.real)) and np.all(np.isfinite(R.imag)))
    zero = ~np.any(Rcf != 0, axis=(-2, -1))
    exact = not np.any(R[zero] != 0)
    e = float(np.max(e_elem(R, Rcf))) if finite else np.inf
    y = float(np.max(e_elem(R32, Rcf)))
    return bool(finite and exact and e <= max(FACTOR * y, FLOOR)), {"e": e, "y": y}


def old_rule(R, Rcf):
    """The rule of the older tests: per matrix |R - Rcf|_F <= 1e-5 |Rcf|_F."""
    R, Rcf = np.asarray(R, np.complex128), np.asarray(Rcf, np.complex128)
    return bool(np.all(np.linalg.norm(R - Rcf, axis=(-2, -1)) <= OLD_FROBENIUS * np.linalg.norm(Rcf, axis=(-2, -1))))


# --------------------------------------------------------------------------------------------------- covariance inputs
def cov_input(S, K, N, T, seed=0):
    """A coherent source plus diffuse noise on channels whose gains spread over 60 dB, permuted; bin 0 real.
    dict(X [S][K][N][T] complex64, tf [S][K][T] float32 in [0, 1] with about 30 % exact zeros, fw [S][T] float32 0/1,
    R0 [S][K][N][N] complex64 Hermitian, non-zero).  The last frame carries weight in every bin."""
    rng = np.random.default_rng(100003 * N + 101 * T + seed)
    gain = np.logspace(0.0, -3.0, N)[rng.permutation(N)] if N > 1 else np.ones(1)
    diffuse = (rng.normal(size=(S, K, N, T)) + 1j * rng.normal(size=(S, K, N, T))) * 15.0
    source = (rng.normal(size=(S, K, 1, T)) + 1j * rng.normal(size=(S, K, 1, T))) * 300.0
    steer = np.exp(2j * np.pi * rng.random((S, K, N, 1)))
    steer[:, 0] = np.where(steer[:, 0].real >= 0, 1.0, -1.0)
    diffuse[:, 0], source[:, 0] = diffuse[:, 0].real, source[:, 0].real
    X = ((diffuse + source * steer) * gain[None, None, :, None]).astype(np.complex64)
    tf = (rng.random((S, K, T)) * (rng.random((S, K, T)) > 0.3)).astype(np.float32)
    fw = (rng.random((S, T)) > 0.3).astype(np.float32)
    fw[:, -1] = 1.0                                                   # the last frame always counts: the tail of a tile must be read
    tf[..., -1] = np.where(tf[..., -1] == 0, np.float32(0.5), tf[..., -1])
    B = (rng.normal(size=(S, K, N, 3)) + 1j * rng.normal(size=(S, K, N, 3))) * gain[None, None, :, None]
    B[:, 0] = B[:, 0].real
    R0 = (B @ np.conj(np.swapaxes(B, -1, -2))) * (0.1 * T * 300.0 ** 2 / 3.0)
    R0 = (0.5 * (R0 + np.conj(np.swapaxes(R0, -1, -2)))).astype(np.complex64)
    return dict(X=X, tf=tf, fw=fw, R0=R0, gain=gain)


WEIGHT_VARIANTS = ("none", "gate", "mask", "both")


def variant(inp, name):
    """(tf, fw, R0) of a weight variant; "both" accumulates into the non-zero Hermitian R0."""
    assert name in WEIGHT_VARIANTS
    return (inp["tf"] if name in ("mask", "both") else None, inp["fw"] if name in ("gate", "both") else None,
            inp.get("R0") if name == "both" else None)


def exact_input(S, K, N, T, seed=0):
    """Integer-valued snapshots (|Re|, |Im| <= 64) and weights in {0, 1, 2}: every float32 product and sum is an integer
    below 2^24, so any summation order gives the closed form bit for bit."""
    assert T * 4 * 64 * 64 < 2 ** 24
    rng = np.random.default_rng(7000 + 31 * N + T + seed)
    X = (rng.integers(-64, 65, (S, K, N, T)) + 1j * rng.integers(-64, 65, (S, K, N, T))).astype(np.complex64)
    X[:, 0] = X[:, 0].real
    tf = rng.integers(0, 3, (S, K, T)).astype(np.float32)
    fw = rng.integers(0, 2, (S, T)).astype(np.float32)
    return dict(X=X, tf=tf, fw=fw)


def poison(X, tf, fw, how, seed=0):
    """Copies (Xp, Xz, tf', fw') with NaN / Inf snapshots in frames that carry weight 0 through the gate ("gate"), through a
    mask zero ("mask", where the whole frame column of the mask is zeroed for one bin) or through both; Xz has them zeroed."""
    rng = np.random.default_rng(seed)
    S, K, N, T = X.shape
    Xp, tf, fw = X.copy(), tf.copy(), fw.copy()
    dead = np.zeros((S, K, T), bool)
    for s in range(S):
        frames = rng.choice(T, size=max(1, T // 4), replace=False)
        if how in ("gate", "both"):
            fw[s, frames] = 0.0
            dead[s][:, frames] = True
        if how in ("mask", "both"):
            more = rng.choice(T, size=max(1, T // 4), replace=False)
            for k in range(K):
                tf[s, k, more[k % len(more):: 2]] = 0.0
            dead[s] |= tf[s] == 0
    bad = np.array([np.nan, np.inf, -np.inf, complex(np.nan, np.inf)], np.complex64)
    idx = np.nonzero(dead)
    for n in range(N):
        Xp[idx[0], idx[1], n, idx[2]] = bad[(idx[2] + n) % 4]
    Xz = Xp.copy()
    Xz[idx[0], idx[1], :, idx[2]] = 0
    return Xp, Xz, tf, fw


def to_frames(Xe):
    """engine [K][N][T] -> frames [T][N][M] complex128 with the mirror bins, M = 2 (K - 1)."""
    K = Xe.shape[0]
    M = 2 * (K - 1)
    X = np.transpose(np.asarray(Xe, np.complex128), (2, 1, 0))
    full = np.zeros(X.shape[:2] + (M,), np.complex128)
    full[..., :K] = X
    full[..., K:] = np.conj(X[..., M // 2 - 1:0:-1])
    return full


# --------------------------------------------------------------------------------------------------- design inputs
DESIGN_N = (1, 2, 15, 16, 17, 37, 38, 65, 66)      # one N on each side of: scalar / MFMA squaring (16), the 48 KB LDS attribute
GEV_GAP_N = (4, 16, 17, 65, 66)                    # (37 | 38) and LDS / L2 scratch (65 | 66)
GEV_GAPS = (0.5, 1e-2, 1e-4, 1e-6)
DESIGN_K = 5
MAX_COND = 1e4
MAX_SPREAD = 2.0 ** -26


def _herm(A):
    return 0.5 * (A + np.conj(np.swapaxes(A, -1, -2)))


def design_input(N, K=DESIGN_K, gap=0.5, bin0_real=True, seed=0, degenerate=False):
    """Rn = Wishart + 0.05 I (condition about 15), Rt = L Q diag(lambda) Q^H L^H with L = chol(Rn), lambda = (1, 1 - gap, U(0, 0.5)...):
    the generalised eigenvalues of (Rt, Rn) are lambda and the relative gap of the two largest is `gap` (0 when degenerate).
    Both rounded to complex64.  Returns (Rt, Rn) [K][N][N] complex64."""
    rng = np.random.default_rng(900001 * N + 7919 * seed + int(round(-1000 * np.log10(gap))) + (0 if bin0_real else 500000))
    Rt, Rn = np.zeros((K, N, N), np.complex128), np.zeros((K, N, N), np.complex128)
    for k in range(K):
        real = bin0_real and k == 0
        cplx = (lambda *sh: rng.normal(size=sh) + 0j) if real else (lambda *sh: rng.normal(size=sh) + 1j * rng.normal(size=sh))
        A = cplx(N, 3 * N)
        Rn[k] = _herm(A @ np.conj(A.T) / (3 * N) + 0.05 * np.eye(N))
        Q, _ = np.linalg.qr(cplx(N, N))
        lam = np.concatenate([[1.0, 1.0 if degenerate else 1.0 - gap], rng.uniform(0.0, 0.5, max(N - 2, 0))])[:N]
        L = np.linalg.cholesky(Rn[k])
        Rt[k] = _herm(L @ (Q * lam) @ np.conj(Q.T) @ np.conj(L.T))
    return Rt.astype(np.complex64), Rn.astype(np.complex64)


def design_cases():
    """Every (N, gap, bin0_real) the GPU design tests use."""
    cases = [(N, 0.5, b) for N in DESIGN_N for b in (True, False)]
    cases += [(N, g, True) for N in GEV_GAP_N for g in GEV_GAPS if (N, g, True) not in cases]
    return cases


def measured_gap(Rt, Rn):
    """Relative gap of the two largest generalised eigenvalues per bin (scipy, float64)."""
    out = []
    for k in range(Rt.shape[0]):
        e, _ = gev_pairs(Rt[k], Rn[k])
        out.append((e[-1] - e[-2]) / e[-1] if len(e) > 1 else np.inf)
    return np.array(out)


def known_answer_input(N, jstar, K=3):
    """Rn = I, Rt diagonal with top entries 1 (at jstar) and 1 - 2^-23, the others smaller: the answer is exactly e_jstar."""
    assert N >= 2
    Rt = np.zeros((K, N, N), np.complex64)
    for k in range(K):
        d = np.linspace(0.1, 0.6, N).astype(np.float32)
        d[(jstar + 1 + k) % N] = np.float32(1.0 - 2.0 ** -23)
        d[jstar] = 1.0
        Rt[k] = np.diag(d)
    Rn = np.broadcast_to(np.eye(N, dtype=np.complex64), (K, N, N)).copy()
    return Rt, Rn


def rn_norm(W, Rn):
    """w^H Rn w per bin for the weights wqH = conj(w)."""
    w = np.conj(np.asarray(W, np.complex128))
    return np.einsum("ki,kij,kj->k", np.conj(w), np.asarray(Rn, np.complex128), w).real


def rayleigh(W, Rt):
    w = np.conj(np.asarray(W, np.complex128))
    return np.einsum("ki,kij,kj->k", np.conj(w), np.asarray(Rt, np.complex128), w).real
