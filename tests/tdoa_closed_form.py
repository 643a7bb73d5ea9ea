"""GCC-PHAT time delay of arrival in float64 numpy, written from the equations (no GPU, no engine code): what
btk_tdoa_spectra and btk_tdoa_gcc_peaks have to compute.

  frames    frame t = samples t D .. t D + D - 1, zero beyond the signal, T = ceil(len / D)
  window    w[i] = 0.54 - 0.46 cos(2 pi i / (D - 1)); w[i] x[i] in float64, rounded to float32 (the reference keeps the
            windowed frame in a float vector)
  spectra   X = rfft of the frame zero-padded to L (forward, unnormalised), energy = 2 sum_{k=0}^{L/2} |X_k|^2
  gate      both energies <= threshold: no peak
  PHAT      P_k = X_a[k] conj X_b[k] / |X_a[k] conj X_b[k]|; a product of magnitude exactly zero: no peak (0/0 makes every
            lag NaN and no NaN compares greater)
  gcc       g = irfft(P): 1/L, imaginary parts of bins 0 and L/2 ignored
  peak      the first n with the largest |g[n]|; lag = n for n < L/2, else n - L; height = |g[n]|
"""
import numpy as np

NO_PEAK = -(1 << 31)


def hamming(D):
    return 0.54 - 0.46 * np.cos(2.0 * np.pi * np.arange(D, dtype=np.float64) / (D - 1))


def n_frames(nsamples, D):
    return -(-int(nsamples) // int(D))


def windowed_frames(pcm, D, window=True):
    """pcm [..., len] -> float32 [..., T, D]: the zero-padded frames times the window, the product rounded to float32
    (window=False: the frames as they are)."""
    pcm = np.asarray(pcm)
    n = pcm.shape[-1]
    T = n_frames(n, D)
    x = np.zeros(pcm.shape[:-1] + (T * D,), np.float64)
    x[..., :n] = pcm
    x = x.reshape(pcm.shape[:-1] + (T, D))
    return (x * hamming(D) if window else x).astype(np.float32)


def spectra(pcm, D, L, window=True):
    """-> (X complex128 [..., T, L/2+1], energy float64 [..., T])"""
    X = np.fft.rfft(windowed_frames(pcm, D, window).astype(np.float64), n=L, axis=-1)
    return X, energy(X)


# ---- the signal of the long-transform cases (tests/test_gpu_tdoa.py's test_long_transforms, tests/test_tdoa_cpu.py) -----------
LONG_CASES = [(4096, 8192), (2048, 4096), (3000, 4096)]          # (D, L)
LONG_S, LONG_C, LONG_T = 2, 3, 3
LONG_PAIRS = [(0, 1), (0, 2), (1, 2), (2, 1)]
LONG_THRESHOLD = 1.0e9
LONG_DELAY = 5
LONG_ZERO = (1, 2, 1)                                            # (stream, channel, frame) that is all zero
LONG_QUIET = (0, 1)                                              # (stream, frame) in which channels 0 and 1 are below the threshold
# a case whose first seed left a peak closer than 2 gcc_bound(L) to the runner-up gets another seed, never a looser condition
LONG_SEED_SHIFT = {}


def long_case_pcm(D, L):
    """float32 [S][C][len], len ending inside the third frame.  Channel 0: white noise; channel 1: channel 0 delayed by
    LONG_DELAY samples plus weaker noise; channel 2: independent noise.  Frame LONG_ZERO of one channel is all zero (a zero
    spectrum: its pairs have no peak, and are not gated because the other channel is loud); in LONG_QUIET channels 0 and 1 are
    scaled below LONG_THRESHOLD, so the pair (0, 1) is gated there and the pairs with channel 2 are not: the gate is an AND."""
    S, C, T, d = LONG_S, LONG_C, LONG_T, LONG_DELAY
    n = (T - 1) * D + D // 2 + 3
    rng = np.random.default_rng(7000 + D + L + LONG_SEED_SHIFT.get((D, L), 0))
    x = np.zeros((S, C, n))
    x[:, 0] = rng.normal(size=(S, n)) * 1000.0
    x[:, 1, d:] = x[:, 0, :n - d]
    x[:, 1] += rng.normal(size=(S, n)) * 300.0
    x[:, 2] = rng.normal(size=(S, n)) * 1000.0
    s, t = LONG_QUIET
    x[s, :2, t * D:(t + 1) * D] *= 1.0e-3
    s, c, t = LONG_ZERO
    x[s, c, t * D:(t + 1) * D] = 0.0
    return x.astype(np.float32)


def energy(X):
    return 2.0 * np.sum(X.real ** 2 + X.imag ** 2, axis=-1)


def gcc(Xa, Xb):
    """The generalised cross-correlation of one frame (half spectra of L/2+1 bins), or None where a bin product is zero."""
    c = np.asarray(Xa, np.complex128) * np.conj(np.asarray(Xb, np.complex128))
    m = np.abs(c)
    if np.any(m == 0.0):
        return None
    return np.fft.irfft(c / m)


def peak(g):
    """(lag, height, margin): first index of the largest |g| as a signed lag; margin = largest minus second largest |g|
    (how far the choice is from changing).  (NO_PEAK, 0, inf) where nothing is positive."""
    a = np.abs(g)
    n = int(np.argmax(a))                      # numpy's argmax is the first maximum
    if not a[n] > 0.0:
        return NO_PEAK, 0.0, np.inf
    L = len(a)
    top2 = np.partition(a, L - 2)[L - 2:]
    return (n if n < L // 2 else n - L), float(a[n]), float(top2[1] - top2[0])


def gcc_peaks(X, en, pairs, threshold, want_gcc=False):
    """X complex [C][T][K], en [C][T], pairs [(a, b)] -> lag int64 [P][T], height [P][T], margin [P][T], gated bool [P][T],
    zero bool [P][T] (and gcc [P][T][L], zeros where gated, NaN where a bin is zero)."""
    C, T, K = X.shape
    L = 2 * (K - 1)
    P = len(pairs)
    lag = np.full((P, T), NO_PEAK, np.int64)
    height = np.zeros((P, T))
    margin = np.full((P, T), np.inf)
    gated = np.zeros((P, T), bool)
    zero = np.zeros((P, T), bool)
    g_all = np.zeros((P, T, L)) if want_gcc else None
    for p, (a, b) in enumerate(pairs):
        for t in range(T):
            if en[a, t] <= threshold and en[b, t] <= threshold:
                gated[p, t] = True
                continue
            g = gcc(X[a, t], X[b, t])
            if g is None:
                zero[p, t] = True
                if want_gcc:
                    g_all[p, t] = np.nan
                continue
            lag[p, t], height[p, t], margin[p, t] = peak(g)
            if want_gcc:
                g_all[p, t] = g
    out = (lag, height, margin, gated, zero)
    return out + (g_all,) if want_gcc else out
