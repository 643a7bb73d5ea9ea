"""Multi-channel WPE dereverberation in plain numpy, written from the equations (no GPU, no engine code, no ctypes): what the
kernels of csrc/wpe_kernels.hip have to compute, stage by stage (reference dereverberation/dereverberation.cc:312-698).

Layout of the engine: X [S][K][C][T] (stream, bin, channel, frame), G [S][C][K][C*L] with tap p = c' L + l, L = upper - lower + 1.

  band      lo = M/2 for band_width 0, else int(band_width / (samplerate / 2) * (M/2)); up = M - lo; bin k is estimated and
            filtered unless lo < k < up
  lags      ybar_p(t) = y_c'(t - lower - l), zero before the first frame
  predict   e_c(t) = y_c(t) - sum_p conj(g_c[p]) ybar_p(t) for t >= lower on an active bin, y_c(t) otherwise.  At apply time the
            reference keeps a ring of the last L frames only, so lag l reaches a frame still in the ring iff l <= L - 1 - lower
  weights   w_c(t) = 1 / max(|e_c(t)|, 1e-3)^2
  normal    R_c = sum_{t >= lower} w_c(t) ybar(t) ybar(t)^H,  r_c = sum_{t >= lower} w_c(t) conj(y_c(t)) ybar(t)
  loading   R_ii += bias, then R_ii <- |R_ii| + max_i |R_ii| 10^(load_db / 10)
  solve     g_c = R_c^-1 r_c by Cholesky

normal_equations, load_and_solve and estimate take dtype = complex128 or complex64: with complex64 every array and every
operation stays in single precision, which gives the rounding level of a float32 implementation of the same equations."""
import numpy as np

FLOOR = 1.0e-3


def band(M, band_width, samplerate=16000.0):
    if band_width == 0.0:
        lo = M // 2
    else:
        if band_width > samplerate / 2.0:
            raise ValueError("Bandwidth is greater than the Nyquist rate.")
        lo = int((band_width / (samplerate / 2.0)) * (M // 2))
    return lo, M - lo


def active(k, lo, up):
    return not (lo < k < up)


def active_bins(K, lo, up):
    return np.array([k for k in range(K) if active(k, lo, up)], dtype=np.int64)


def lag_matrix(X, lower, upper):
    """X [S][K][C][T] -> A [S][K][C*L][T], A[.., c' L + l, t] = X[.., c', t - lower - l] (zero before frame 0)"""
    S, K, C, T = X.shape
    L = upper - lower + 1
    A = np.zeros((S, K, C, L, T), X.dtype)
    for l in range(L):
        sh = lower + l
        if sh < T:
            A[:, :, :, l, sh:] = X[..., :T - sh]
    return A.reshape(S, K, C * L, T)


def predict(X, G, lower, upper, lo, up, apply):
    """-> (e [S][K][C][T], mag [S][K][C][T]) with mag = |y| + sum_p |g_p| |ybar_p|, the magnitude sum of the terms of e"""
    S, K, C, T = X.shape
    L = upper - lower + 1
    A = lag_matrix(X, lower, upper)
    Gk = np.transpose(G, (0, 2, 1, 3)).copy()                    # [S][K][C][P]
    if apply:                                                    # the ring rule: lags beyond L - 1 - lower see nothing
        dead = np.tile(np.arange(L) > L - 1 - lower, C)
        Gk[..., dead] = 0
    out = X.copy()
    mag = np.abs(X)
    rt = X.real.dtype
    for k in range(K):
        if not active(k, lo, up):
            continue
        pred = np.matmul(np.conj(Gk[:, k]), A[:, k])             # [S][C][T]
        pm = np.matmul(np.abs(Gk[:, k]).astype(rt), np.abs(A[:, k]).astype(rt))
        out[:, k, :, lower:] = X[:, k, :, lower:] - pred[..., lower:]
        mag[:, k, :, lower:] += pm[..., lower:]
    return out, mag


def weights(residual):
    a = np.maximum(np.abs(residual), residual.real.dtype.type(FLOOR))
    return 1 / (a * a)


def normal_equations(X, W, lower, upper, dtype=np.complex128):
    """X [S][K][C][T], W [S][K][C][T] -> R [S][C][K][P][P], r [S][C][K][P], summed over t >= lower"""
    dtype = np.dtype(dtype)
    rt = np.zeros(0, dtype).real.dtype
    X = X.astype(dtype)
    W = W.astype(rt).copy()
    W[..., :lower] = 0
    A = lag_matrix(X, lower, upper)                              # [S][K][P][T]
    AH = np.conj(np.swapaxes(A, -1, -2))                         # [S][K][T][P]
    S, K, C, T = X.shape
    P = A.shape[2]
    R = np.zeros((S, C, K, P, P), dtype)
    r = np.zeros((S, C, K, P), dtype)
    for c in range(C):
        AW = A * W[:, :, c, None, :]
        R[:, c] = np.matmul(AW, AH)
        r[:, c] = np.matmul(AW, np.conj(X[:, :, c, :, None]))[..., 0]
    return R, r


def load(R, load_db, diagonal_bias):
    """the loaded matrix: bias on the diagonal, then R_ii <- |R_ii| + max_i |R_ii| 10^(load_db / 10)"""
    rt = R.real.dtype.type
    R = R.copy()
    P = R.shape[-1]
    i = np.arange(P)
    d = np.abs(R[..., i, i] + rt(diagonal_bias))
    R[..., i, i] = d + np.max(d, axis=-1, keepdims=True) * rt(10.0 ** (load_db / 10.0))
    return R


def cholesky_solve(A, b):
    """A x = b for Hermitian positive definite A [..][P][P] (lower triangle read), b [..][P], in the arrays' own precision"""
    P = A.shape[-1]
    Lm = np.zeros_like(A)
    for j in range(P):
        row = Lm[..., j, :j]
        d = A[..., j, j].real - np.sum(row.real * row.real + row.imag * row.imag, axis=-1)
        if not np.all(d > 0):
            raise ArithmeticError("Cholesky failed")
        d = np.sqrt(d)
        Lm[..., j, j] = d
        if j + 1 < P:
            col = A[..., j + 1:, j] - np.matmul(Lm[..., j + 1:, :j], np.conj(row)[..., None])[..., 0]
            Lm[..., j + 1:, j] = col / d[..., None]
    x = b.copy()
    for j in range(P):                                           # L y = b
        x[..., j] = (x[..., j] - np.sum(Lm[..., j, :j] * x[..., :j], axis=-1)) / Lm[..., j, j].real
    for j in range(P - 1, -1, -1):                               # L^H x = y
        x[..., j] = (x[..., j] - np.sum(np.conj(Lm[..., j + 1:, j]) * x[..., j + 1:], axis=-1)) / Lm[..., j, j].real
    return x


def load_and_solve(R, r, load_db, diagonal_bias, dtype=np.complex128):
    dtype = np.dtype(dtype)
    return cholesky_solve(load(R.astype(dtype), load_db, diagonal_bias), r.astype(dtype))


def estimate(X, lower, upper, iterations, load_db, diagonal_bias, lo, up, dtype=np.complex128, return_loaded=False):
    """-> G [S][C][K][C*L] (zero on the bins outside the band); with return_loaded also the loaded matrices of the last
    iteration on the active bins, [S][C][Ka][P][P]"""
    dtype = np.dtype(dtype)
    X = X.astype(dtype)
    S, K, C, T = X.shape
    P = C * (upper - lower + 1)
    ks = active_bins(K, lo, up)
    Xa = X[:, ks]
    G = np.zeros((S, C, K, P), dtype)
    Rl = None
    for _ in range(iterations):
        e, _ = predict(Xa, G[:, :, ks], lower, upper, K, K, apply=False)
        R, r = normal_equations(Xa, weights(e), lower, upper, dtype)
        Rl = load(R, load_db, diagonal_bias)
        G[:, :, ks] = cholesky_solve(Rl, r)
    return (G, Rl) if return_loaded else G


def apply(X, G, lower, upper, lo, up):
    return predict(X, G, lower, upper, lo, up, apply=True)[0]
