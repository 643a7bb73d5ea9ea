"""Closed forms of the oversampled modulated-DFT filter banks and the fixed-weight beamformer, in float64 numpy.

An independent statement of SURVEY rows a3 (analysis) and a18 (synthesis): no GPU, no oracle, no library code -- the delays
come from the small restatement of the delay rule below.  The tests hold the oracle (test_closed_forms_cpu.py) and the fused
kernels (test_gpu_fused_closed_form.py) against these functions.

    analysis   frame t has newest sample n_t = (t + laN + 1) D - 1;  p[i] = sum_k h[i + M k] x[n_t - (i + M k)];  X_t = M ifft(p)
    beamformer Y[k][t] = sum_n conj(W[k][n]) X[t][n][k]
    synthesis  v_t = Re fft(Y_t);  s_t[i] = sum_k g[M-1-i+M k] v_{t-R k}[i] for t >= pd;  block b = frame pd + b:
               out[D-1-d] = sum_j s_{t-(R-1-j)}[d + j D]

plain_f32 / synthesis_f32 evaluate the same sums in float32 / complex64 numpy, the straightforward way.  They are the YARDSTICK of
the GPU tests: what float32 arithmetic achieves on given inputs, measured against the float64 closed form.  `accept` is the
acceptance rule built on it.
"""
import numpy as np

FLOOR = 2.0 ** -22          # four float32 ulps of the largest value: the bound never goes below this fraction of max|Y_cf|
FACTOR = 4.0                # kernel error <= FACTOR x yardstick error (see accept)


# --------------------------------------------------------------------------- geometry
def fb_delays(m, r, synthesis, dct):
    """(processing delay, look-ahead) in frames of OverSampledDFTFilterBank for delay-compensation type dct."""
    R = 1 << r
    if dct == 1:
        return m * R - 1, 0
    if dct == 2:
        return (m * R // 2, 0) if synthesis else (m * R - 1, m * R // 2 - 1)
    return 2 * m - 1, 0


def num_frames(nsamples, M, m, r, dct):
    """ceil(len / D) - laN + pd; 0 when the source ends inside the look-ahead."""
    D = M >> r
    pd, la = fb_delays(m, r, False, dct)
    nblk = -(-int(nsamples) // D)
    return 0 if nblk < la else nblk - la + pd


def num_samples(T, M, m, r, dct):
    """The recording length (a multiple of D) that gives exactly T frames (T >= pd)."""
    pd, la = fb_delays(m, r, False, dct)
    nblk = T - pd + la
    assert nblk >= la and nblk >= 0, "no recording gives %d frames" % T
    return nblk * (M >> r)


# --------------------------------------------------------------------------- float64 closed forms
def _windows(x, T, M, m, r, la, dtype):
    """[T][m M]: row t holds x[n_t - l], l = 0 .. m M - 1, zero outside the recording."""
    D, L = M >> r, m * M
    x = np.asarray(x, dtype)
    hi = (T + la + 1) * D + L
    xp = np.concatenate([np.zeros(L, dtype), x, np.zeros(max(0, hi - len(x)), dtype)])
    nt = (np.arange(T) + la + 1) * D - 1 + L
    return xp[nt[:, None] - np.arange(L)[None, :]]


def analysis_cf(h, M, m, r, dct, x):
    """SURVEY a3.  x [len] -> complex128 [T][M]."""
    h = np.asarray(h, np.float64)
    assert h.shape == (m * M,)
    _, la = fb_delays(m, r, False, dct)
    T = num_frames(len(x), M, m, r, dct)
    if T == 0:
        return np.zeros((0, M), np.complex128)
    p = (_windows(x, T, M, m, r, la, np.float64) * h[None, :]).reshape(T, m, M).sum(axis=1)
    return np.fft.ifft(p, axis=1) * M


def beamform_cf(W, X):
    """W [K][N], X [T][N][M] -> Y [K][T] = sum_n conj(W[k][n]) X[t][n][k], complex128."""
    W = np.asarray(W, np.complex128)
    K = W.shape[0]
    return np.einsum("kn,tnk->kt", np.conj(W), np.asarray(X, np.complex128)[:, :, :K])


def fused_cf(h, M, m, r, dct, pcm, W):
    """pcm [N][L], W [K][N] -> Y complex128 [K][T]: the fused kernels' operation."""
    W = np.asarray(W, np.complex128)
    K = W.shape[0]
    Y = np.zeros((K, num_frames(pcm.shape[1], M, m, r, dct)), np.complex128)
    for n in range(pcm.shape[0]):                                  # channel by channel: [T][N][M] need not exist at once
        Y += np.conj(W[:, n])[:, None] * analysis_cf(h, M, m, r, dct, pcm[n])[:, :K].T
    return Y


def hermitian(Yh, M):
    """[K][T] (bins 0 .. M/2) -> [T][M] with the mirror bins, as an analysis bank on real input delivers them."""
    K, T = Yh.shape
    assert K == M // 2 + 1
    full = np.zeros((T, M), Yh.dtype)
    full[:, :K] = Yh.T
    full[:, K:] = np.conj(full[:, M // 2 - 1:0:-1])
    return full


def synthesis_cf(g, M, m, r, dct, Y):
    """SURVEY a18.  Y complex [T][M] -> float64 [B D], B = T - pd."""
    g = np.asarray(g, np.float64)
    R, D = 1 << r, M >> r
    pd, _ = fb_delays(m, r, True, dct)
    T = Y.shape[0]
    B = T - pd
    if B <= 0:
        return np.zeros(0)
    v = np.fft.fft(np.asarray(Y, np.complex128), axis=1).real
    vp = np.concatenate([np.zeros((m * R, M)), v])                  # frames before the first are zero
    gi = g.reshape(m, M)[:, ::-1]                                   # gi[k][i] = g[M-1-i+M k]
    s = np.zeros((T, M))
    for k in range(m):
        s += gi[k][None, :] * vp[m * R - R * k: m * R - R * k + T]
    s[:pd] = 0.0                                                    # the output ring starts with the first block
    sp = np.concatenate([np.zeros((R, M)), s])
    out = np.zeros((B, D))
    for j in range(R):
        out += sp[R + pd - (R - 1 - j): R + pd - (R - 1 - j) + B, j * D:(j + 1) * D]
    return out[:, ::-1].reshape(-1)


# --------------------------------------------------------------------------- the float32 yardstick
def analysis_f32(h, M, m, r, dct, x):
    """analysis_cf in float32 / complex64: float32 products, taps summed in order k = 0 .. m-1, complex64 FFT."""
    h32 = np.asarray(h, np.float32)
    _, la = fb_delays(m, r, False, dct)
    T = num_frames(len(x), M, m, r, dct)
    if T == 0:
        return np.zeros((0, M), np.complex64)
    w = (_windows(x, T, M, m, r, la, np.float32) * h32[None, :]).reshape(T, m, M)
    p = w[:, 0]
    for k in range(1, m):
        p = p + w[:, k]
    assert p.dtype == np.float32
    X = np.fft.ifft(p.astype(np.complex64), axis=1, norm="forward")
    assert X.dtype == np.complex64, "numpy >= 2 keeps complex64 through np.fft"
    return X


def plain_f32(h, M, m, r, dct, pcm, W):
    """fused_cf in float32 / complex64: channel after channel added to a complex64 sum.  [K][T] complex64."""
    W = np.asarray(W)
    K, N = W.shape
    T = num_frames(pcm.shape[1], M, m, r, dct)
    out = np.zeros((K, T), np.complex64)
    for n in range(N):
        X = analysis_f32(h, M, m, r, dct, pcm[n])
        out += np.conj(W[:, n]).astype(np.complex64)[:, None] * X[:, :K].T
    assert out.dtype == np.complex64
    return out


def synthesis_f32(g, M, m, r, dct, Y):
    """synthesis_cf in float32: complex64 FFT, float32 polyphase sums and overlap-add."""
    g32 = np.asarray(g, np.float32)
    R, D = 1 << r, M >> r
    pd, _ = fb_delays(m, r, True, dct)
    T = Y.shape[0]
    B = T - pd
    if B <= 0:
        return np.zeros(0, np.float32)
    V = np.fft.fft(np.asarray(Y, np.complex64), axis=1)
    assert V.dtype == np.complex64
    v = V.real
    vp = np.concatenate([np.zeros((m * R, M), np.float32), v])
    gi = g32.reshape(m, M)[:, ::-1]
    s = np.zeros((T, M), np.float32)
    for k in range(m):
        s += gi[k][None, :] * vp[m * R - R * k: m * R - R * k + T]
    s[:pd] = 0.0
    sp = np.concatenate([np.zeros((R, M), np.float32), s])
    out = np.zeros((B, D), np.float32)
    for j in range(R):
        out += sp[R + pd - (R - 1 - j): R + pd - (R - 1 - j) + B, j * D:(j + 1) * D]
    assert out.dtype == np.float32
    return out[:, ::-1].reshape(-1)


# --------------------------------------------------------------------------- inputs
def dense_prototype(M, m, seed=0):
    """Taps +-U(0.5, 1) rounded to float32: every tap, tap 0 included, carries weight."""
    rng = np.random.default_rng(1000003 * M + 101 * m + seed)
    mag = rng.uniform(0.5, 1.0, m * M)
    sgn = np.where(rng.integers(0, 2, m * M) == 1, 1.0, -1.0)
    return (mag * sgn).astype(np.float32).astype(np.float64)


def int_pcm(S, N, L, seed=0):
    """Integer-valued samples in the int16 range, float32 [S][N][L] (exact in float32 and int16)."""
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0.0, 3000.0, (S, N, L))), -32767, 32767).astype(np.float32)


def unit_weights(S, K, N, seed=0):
    """exp(j phi) / N, complex64 [S][K][N]: every channel counts the same in every bin."""
    rng = np.random.default_rng(seed + 77)
    return (np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, (S, K, N))) / N).astype(np.complex64)


def one_hot_weights(K, N):
    """Bin k takes channel k mod N only: the result must equal that channel's own analysis.  complex64 [K][N]."""
    W = np.zeros((K, N), np.complex64)
    W[np.arange(K), np.arange(K) % N] = 1.0
    return W


# --------------------------------------------------------------------------- error metrics and the acceptance rule
def e_max(Y, Ycf):
    """max |Y - Y_cf| / max |Y_cf|."""
    s = float(np.max(np.abs(Ycf))) if Ycf.size else 0.0
    d = float(np.max(np.abs(Y - Ycf))) if Ycf.size else 0.0
    return d / s if s > 0 else (0.0 if d == 0 else np.inf)


def e_bin(Y, Ycf):
    """Per row k: max_t |Y - Y_cf|[k, t] / rms_t |Y_cf[k, :]| (inf for a row the closed form has at zero and Y not)."""
    d = np.max(np.abs(Y - Ycf), axis=-1)
    rms = np.sqrt(np.mean(np.abs(Ycf) ** 2, axis=-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(rms > 0, d / rms, np.where(d == 0, 0.0, np.inf))
    return e


def accept(Y, Y32, Ycf, factor=FACTOR):
    """The acceptance rule.  Y: the kernel's output, Y32: the float32 yardstick on the same inputs, Ycf: the float64 closed
    form; all [rows][T] (rows = bins) or 1-D (one row).  Returns (ok, figures).

      * e_max(Y) <= max(factor * e_max(Y32), FLOOR)
      * every row k:  e_bin(Y)[k] <= factor * max_k e_bin(Y32), or its absolute error <= FLOOR * max|Y_cf|
        (one-hot bins and other outputs float32 produces exactly have a yardstick of 0)
      * Y_cf identically zero: Y must be exactly zero.
    """
    Y, Y32, Ycf = (np.atleast_2d(np.asarray(a)) for a in (Y, Y32, Ycf))
    assert Y.shape == Ycf.shape == Y32.shape, (Y.shape, Y32.shape, Ycf.shape)
    assert np.all(np.isfinite(Y.view(np.float32) if Y.dtype == np.complex64 else np.abs(Y)))
    scale = float(np.max(np.abs(Ycf))) if Ycf.size else 0.0
    if scale == 0.0:
        ok = not np.any(Y)
        return ok, {"e_max": 0.0 if ok else np.inf, "y_max": 0.0, "e_bin": 0.0 if ok else np.inf, "y_bin": 0.0, "ratio": 0.0 if ok else np.inf}
    em, ym = e_max(Y, Ycf), e_max(Y32, Ycf)
    eb, yb = e_bin(Y, Ycf), e_bin(Y32, Ycf)
    ybm = float(np.max(yb))
    over = np.max(np.abs(Y - Ycf), axis=-1) > FLOOR * scale            # rows whose error is above the floor
    with np.errstate(divide="ignore", invalid="ignore"):
        r_bin = float(np.max(np.where(over, eb / ybm, 0.0)))          # yardstick 0 and a row above the floor: inf
    r_max = em / max(ym, FLOOR / factor)
    ratio = max(r_max, r_bin)
    return bool(ratio <= factor), {"e_max": em, "y_max": ym, "e_bin": float(np.max(eb)), "y_bin": ybm, "ratio": ratio,
                                   "bad_rows": np.nonzero(np.where(over, eb / max(ybm, 1e-300), 0.0) > factor)[0][:8].tolist()}


def cfratio_line(label, fig):
    """The line the GPU modules print per case; their docstring tables are made from these."""
    return ("CFRATIO %-58s ratio %7.3f  e_max %.3e (f32 %.3e)  e_bin %.3e (f32 %.3e)" %
            (label, fig["ratio"], fig["e_max"], fig["y_max"], fig["e_bin"], fig["y_bin"]))


def judge(label, Y, Y32, Ycf, factor=FACTOR, show=True):
    """Print the figures, then assert the rule (show=False: print only a case that fails; the caller prints its worst)."""
    ok, fig = accept(Y, Y32, Ycf, factor)
    if show or not ok:
        print(cfratio_line(label, fig))
    assert ok, (label, fig)
    return fig
