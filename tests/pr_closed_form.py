"""Closed forms of the cosine-modulated perfect-reconstruction (PR) banks and the windowed FFT bank, in float64 numpy.

Three statements of each bank, none of which touches the GPU or the library:

  *_cf       the closed form (M2 = 2 M, R = 2^r, D = M / R, q = r + 2, pd = 2 m - 1; x = 0 outside the recording)
             analysis   frame t has newest sample n_t = (t + 1) D - 1;  p[i] = sum_{k<m} (-1)^k h[i + M2 k] x[n_t - q k D - i];
                        X_t[kappa] = 1/M2 sum_i p[i] e^{-j pi i/M2} e^{+j 2 pi kappa i/M2};  ceil(L / D) + pd frames
             synthesis  v_f[i] = Re(e^{+j pi i/M2} sum_kappa Y_f[kappa] e^{-j 2 pi kappa i/M2});  block j uses newest frame f = j + pd;
                        s_j[i] = sum_{k<m} (-1)^{k+m-1} h[i + M2 (m-1-k)] v_{f - q k}[i];
                        out_j[D-1-d] = sum_{sx<2R} s_{j-(2R-1-sx)}[d + sx D] / R;  frames and blocks before 0 are zero
             STFT       X_t[kappa] = sum_{i<M} win[i] x[n_t - M + 1 + i] e^{-j 2 pi kappa i/M};  ceil(L / D) + 1 frames
  *_literal  the ring buffers and next() loops of the banks restated step by step (a ring of blocks, a ring of reversed
             windows, the float32 output vector the synthesis bank adds into)
  *_f32      the closed form in float32 / complex64 numpy, the straightforward way: the YARDSTICK of the GPU tests, as
             analysis_f32 / synthesis_f32 of closed_forms.py are for the oversampled banks.
"""
import numpy as np


# --------------------------------------------------------------------------- geometry
def geom(M, m, r):
    R = 1 << r
    return 2 * M, R, M // R, r + 2, 2 * m - 1          # M2, R, D, q, pd


def pr_num_frames(L, M, m, r):
    _, _, D, _, pd = geom(M, m, r)
    return -(-int(L) // D) + pd


def pr_num_blocks(T, m):
    return max(T - (2 * m - 1), 0)


def stft_num_frames(L, M, r):
    return -(-int(L) // (M >> r)) + 1


def get_window_cf(window_type, n):
    i = np.arange(n, dtype=np.float64)
    if window_type == 0:
        return np.ones(n)
    if window_type == 2:
        return 0.5 * (1 - np.cos((2.0 * np.pi * i) / (n - 1)))
    return 0.54 - 0.46 * np.cos(2.0 * np.pi / (n - 1) * i)


def sine_prototype(M):
    """h[n] = sin(pi (n + 1/2) / M2), the m = 1 prototype with which analysis -> synthesis returns the input."""
    M2 = 2 * M
    return np.sin(np.pi * (np.arange(M2) + 0.5) / M2)


def random_prototype(M, m, seed=0):
    """Taps +-U(0.5, 1) rounded to float32 (closed_forms.dense_prototype's rule), length 2 M m."""
    rng = np.random.default_rng(1000003 * M + 101 * m + seed)
    mag = rng.uniform(0.5, 1.0, 2 * M * m)
    sgn = np.where(rng.integers(0, 2, 2 * M * m) == 1, 1.0, -1.0)
    return (mag * sgn).astype(np.float32).astype(np.float64)


# --------------------------------------------------------------------------- closed forms (dtype float64) and yardsticks (float32)
def _pr_windows(x, M, m, r, dtype):
    """[T][m][M2]: entry (t, k, i) = x[n_t - q k D - i]."""
    M2, _, D, q, _ = geom(M, m, r)
    T = pr_num_frames(len(x), M, m, r)
    Z = q * (m - 1) * D + M2
    xp = np.concatenate([np.zeros(Z, dtype), np.asarray(x, dtype), np.zeros(max(0, T * D - len(x)), dtype)])
    nt = (np.arange(T) + 1) * D - 1 + Z
    return xp[nt[:, None, None] - q * D * np.arange(m)[None, :, None] - np.arange(M2)[None, None, :]]


def _signed_taps(h, M, m, synthesis, dtype):
    """[m][M2]: analysis row k = (-1)^k h[i + M2 k]; synthesis row k = (-1)^{k+m-1} h[i + M2 (m-1-k)]."""
    hk = np.asarray(h, np.float64).reshape(m, 2 * M)
    k = np.arange(m)
    if synthesis:
        return (hk[::-1] * ((-1.0) ** (k + m - 1))[:, None]).astype(dtype)
    return (hk * ((-1.0) ** k)[:, None]).astype(dtype)


def pr_analysis_cf(h, M, m, r, x):
    """x [L] -> complex128 [T][M2]."""
    M2 = 2 * M
    assert np.asarray(h).shape == (M2 * m,)
    p = (_pr_windows(x, M, m, r, np.float64) * _signed_taps(h, M, m, False, np.float64)[None]).sum(axis=1)
    return np.fft.ifft(p * np.exp(-1j * np.pi * np.arange(M2) / M2)[None, :], axis=1)


def pr_analysis_f32(h, M, m, r, x):
    """pr_analysis_cf in float32 / complex64: float32 products, taps summed in order k = 0 .. m-1, a complex64 rotation table with
    the 1/M2 folded in, complex64 FFT."""
    M2 = 2 * M
    w = _pr_windows(x, M, m, r, np.float32) * _signed_taps(h, M, m, False, np.float32)[None]
    p = w[:, 0]
    for k in range(1, m):
        p = p + w[:, k]
    assert p.dtype == np.float32
    rot = (np.exp(-1j * np.pi * np.arange(M2) / M2) / M2).astype(np.complex64)
    X = np.fft.ifft(p * rot[None, :], axis=1, norm="forward")
    assert X.dtype == np.complex64, "numpy >= 2 keeps complex64 through np.fft"
    return X


def _pr_synthesis(h, M, m, r, Y, f32):
    M2, R, D, q, pd = geom(M, m, r)
    ft, ct = (np.float32, np.complex64) if f32 else (np.float64, np.complex128)
    T = Y.shape[0]
    B = pr_num_blocks(T, m)
    if B == 0:
        return np.zeros(0, ft)
    V = np.fft.fft(np.asarray(Y, ct), axis=1) * np.exp(1j * np.pi * np.arange(M2) / M2).astype(ct)[None, :]
    assert V.dtype == ct
    v = V.real
    Z = q * (m - 1)
    vp = np.concatenate([np.zeros((Z, M2), ft), v])                 # frames before the first are zero
    g = _signed_taps(h, M, m, True, ft)
    s = np.zeros((B, M2), ft)                                       # s_j, j = 0 .. B-1; newest frame j + pd
    for k in range(m):
        s += g[k][None, :] * vp[Z + pd - q * k: Z + pd - q * k + B]
    sp = np.concatenate([np.zeros((2 * R - 1, M2), ft), s])         # blocks before the first are zero
    out = np.zeros((B, D), ft)
    for sx in range(2 * R):
        out += sp[sx: sx + B, sx * D:(sx + 1) * D] / ft(R)
    assert out.dtype == ft
    return out[:, ::-1].reshape(-1)


def pr_synthesis_cf(h, M, m, r, Y):
    """Y complex [T][M2] -> float64 [B D], B = T - pd."""
    return _pr_synthesis(h, M, m, r, Y, False)


def pr_synthesis_f32(h, M, m, r, Y):
    """pr_synthesis_cf in float32: complex64 FFT and rotation, float32 polyphase sums and overlap-add."""
    return _pr_synthesis(h, M, m, r, Y, True)


def _stft_windows(x, M, r, dtype):
    D = M >> r
    T = stft_num_frames(len(x), M, r)
    xp = np.concatenate([np.zeros(M, dtype), np.asarray(x, dtype), np.zeros(max(0, T * D - len(x)), dtype)])
    nt = (np.arange(T) + 1) * D - 1 + M
    return xp[nt[:, None] - M + 1 + np.arange(M)[None, :]]


def stft_cf(M, r, window_type, x):
    """x [L] -> complex128 [T][M]."""
    return np.fft.fft(_stft_windows(x, M, r, np.float64) * get_window_cf(window_type, M)[None, :], axis=1)


def stft_f32(M, r, window_type, x):
    X = np.fft.fft((_stft_windows(x, M, r, np.float32) * get_window_cf(window_type, M).astype(np.float32)[None, :]).astype(np.complex64), axis=1)
    assert X.dtype == np.complex64
    return X


# --------------------------------------------------------------------------- the literal restatement
class Ring:
    """A ring of `nsamp` vectors of length `n`: sample(0, .) is the vector pushed last."""

    def __init__(self, n, nsamp):
        self.buf = np.zeros((nsamp, n))
        self.nsamp = nsamp
        self.zero = nsamp - 1

    def push(self, v=None, reverse=False):
        self.zero = (self.zero + 1) % self.nsamp
        if v is None:
            self.buf[self.zero] = 0.0
        else:
            v = np.asarray(v, np.float64)
            assert v.shape == self.buf[self.zero].shape
            self.buf[self.zero] = v[::-1] if reverse else v

    def sample(self, time, i):
        assert time < self.nsamp
        return self.buf[(self.zero + self.nsamp - time) % self.nsamp][i]


def _blocks(x, D):
    """The blocks a sample source hands out: D samples each, a short last block padded with zeros."""
    x = np.asarray(x, np.float32)
    nblk = -(-len(x) // D)
    xp = np.concatenate([x, np.zeros(nblk * D - len(x), np.float32)])
    return [xp[b * D:(b + 1) * D] for b in range(nblk)]


def _frames_of_windows(x, D, nblocks_in_window, nsamp, pd):
    """Yield the window ring after every update: one per source block, then pd zero blocks."""
    blocks = _blocks(x, D)
    gsi = Ring(D, nblocks_in_window)
    buf = Ring(D * nblocks_in_window, nsamp)
    convert = np.zeros(D * nblocks_in_window)
    for blk in blocks + [None] * pd:
        gsi.push(blk)
        for sx in range(nblocks_in_window):
            for d in range(D):
                convert[d + sx * D] = gsi.sample(nblocks_in_window - sx - 1, d)
        buf.push(convert, reverse=True)
        yield buf


def pr_analysis_literal(h, M, m, r, x):
    M2, R, D, q, pd = geom(M, m, r)
    h = np.asarray(h, np.float64)
    w = np.exp(-1j * np.pi * np.arange(M2) / M2)
    out = []
    for buf in _frames_of_windows(x, D, 2 * R, m * q, pd):
        z = np.zeros(M2, np.complex128)
        for i in range(M2):
            total, flip = 0.0, 1
            for k in range(m):
                total += flip * h[i + M2 * k] * buf.sample(q * k, i)
                flip = -flip
            z[i] = w[i] * total
        out.append(np.fft.ifft(z))
    return np.array(out).reshape(-1, M2)


def pr_synthesis_literal(h, M, m, r, Y):
    """Returns (out float32 [B D], bound [B D]): bound = sum |terms| 2^-24 (2R), what the float32 running sum of the output
    vector can lose against an exact sum of the same terms."""
    M2, R, D, q, pd = geom(M, m, r)
    h = np.asarray(h, np.float64)
    Y = np.asarray(Y, np.complex128)
    w = np.exp(1j * np.pi * np.arange(M2) / M2)
    buf, gsi = Ring(M2, m * q), Ring(M2, 2 * R)

    def update(f):
        buf.push((np.fft.fft(Y[f]) * w).real)

    T = Y.shape[0]
    out, bound = [], []
    if T <= pd:
        return np.zeros(0, np.float32), np.zeros(0)
    for f in range(pd):
        update(f)
    for j in range(T - pd):
        update(j + pd)
        conv = np.zeros(M2)
        for i in range(M2):
            total, flip = 0.0, (1 if m % 2 == 1 else -1)
            for k in range(m):
                total += flip * h[i + M2 * (m - k - 1)] * buf.sample(q * k, i)
                flip = -flip
            conv[i] = total
        gsi.push(conv)
        vec = np.zeros(D, np.float32)
        mag = np.zeros(D)
        for sx in range(2 * R):
            for d in range(D):
                term = gsi.sample(2 * R - sx - 1, d + sx * D) / R
                vec[D - d - 1] = np.float32(np.float64(vec[D - d - 1]) + term)
                mag[D - d - 1] += abs(term)
        out.append(vec)
        bound.append(mag * 2.0 ** -24 * (2 * R))
    return np.concatenate(out), np.concatenate(bound)


def stft_literal(M, r, window_type, x):
    R, D = 1 << r, M >> r
    win = get_window_cf(window_type, M)
    out = []
    for buf in _frames_of_windows(x, D, R, R, 1):
        z = np.array([win[i] * buf.sample(0, M - i - 1) for i in range(M)])
        out.append(np.fft.fft(z))
    return np.array(out).reshape(-1, M)


def int_signal(L, seed=0):
    """Integer-valued samples at int16 scale, float32 [L]."""
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(rng.normal(0.0, 3000.0, L)), -32767, 32767).astype(np.float32)
