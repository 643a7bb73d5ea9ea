"""Float64 numpy restatement of DOAEstimatorSRPBase / DOAEstimatorSRPDSBLA (reference beamformer/beamformer.cc:2876-3251),
halfBandShift == false: the yardstick of the steered-response-power tests.  Written from the formulas, no engine code."""
import numpy as np

RESET_RP = -10e10


def grid(min_theta=-np.pi / 2, max_theta=np.pi / 2, width_theta=0.1):
    """set_search_param stores floats; nTheta = (unsigned)((max - min) / width + 0.5) (float quotient, + 0.5 in double);
    theta starts at min and grows by width in double (:3052, :3071)."""
    lo, hi, w = np.float32(min_theta), np.float32(max_theta), np.float32(width_theta)
    if lo > hi:
        raise ValueError("minTheta > maxTheta")
    n = int(np.float64(np.float32(np.float32(hi - lo) / w)) + 0.5)
    out = np.zeros(n, np.float64)
    theta = np.float64(lo)
    for i in range(n):
        out[i] = theta
        theta = theta + np.float64(w)
    return out


def delays(positions, theta):
    """set_look_direction_(int, float theta) (:3193-3207): |p_n - p_0| cos(theta), theta rounded to float by the signature."""
    p = np.asarray(positions, np.float64)
    return np.abs(p - p[0]) * np.cos(np.float64(np.float32(theta)))


def mainlobe_row(M, k, fs, d):
    """wq_k of calcMainlobe (:528-552), 1 <= k <= M/2."""
    N = len(d)
    fs = np.float64(np.float32(fs))
    if k < M // 2:
        val = -2.0 * np.pi * k * d * fs / M
    else:
        val = -np.pi * fs * d
    return (np.cos(val) + 1j * np.sin(val)) / N


def table(M, fs, positions, thetas, fmin=1, fmax=None):
    """svTbl_ (:3046-3089): [U][K][N], ones in bin 0, calcMainlobe rows on fmin..fmax, zero elsewhere."""
    fmax = M // 2 if fmax is None else fmax
    N, K = len(positions), M // 2 + 1
    sv = np.zeros((len(thetas), K, N), np.complex128)
    sv[:, 0, :] = 1.0
    for u, th in enumerate(thetas):
        d = delays(positions, th)
        for k in range(fmin, fmax + 1):
            sv[u, k] = mainlobe_row(M, k, fs, d)
    return sv


def bin_weights(M, fmin, fmax):
    k = np.arange(fmin, fmax + 1)
    return np.where(k < M // 2, 2.0, 1.0)


def response_power(X, sv, M, fmin=1, fmax=None):
    """calc_response_power_ (:3091-3122) for every direction and frame.  X [K][N][T] -> (rp [U][T], e [U][T]) with
    e = sum_k c_k (sum_n |sv| |x|)^2 / nb, the magnitude sum the rounding bound of a float32 evaluation scales with."""
    fmax = M // 2 if fmax is None else fmax
    X = np.asarray(X, np.complex128)
    c = bin_weights(M, fmin, fmax)
    nb = fmax - fmin + 1.0
    svk = np.ascontiguousarray(sv[:, fmin:fmax + 1].transpose(1, 0, 2))     # [nb][U][N]
    Y = np.matmul(np.conj(svk), X[fmin:fmax + 1])                           # [nb][U][T]
    rp = np.einsum("k,kut->ut", c, np.abs(Y) ** 2) / nb
    A = np.matmul(np.abs(svk), np.abs(X[fmin:fmax + 1]))
    e = np.einsum("k,kut->ut", c, A ** 2) / nb
    return rp, e


def energy(X, M, fmin=1, fmax=None):
    """calc_energy (:3221-3251): it squares the squared norm.  X [K][N][T] -> [T]."""
    fmax = M // 2 if fmax is None else fmax
    X = np.asarray(X, np.complex128)
    N = X.shape[1]
    nrm = np.sum(np.abs(X[fmin:fmax + 1]) ** 2, axis=1)                  # [nb][T]
    return np.einsum("k,kt->t", bin_weights(M, fmin, fmax), nrm ** 2) / (2 * (M // 2) * N)


def nbest_insert(values, nbest):
    """The insertion loop of :3157-3187 / :2942-2981 over one vector of powers: strict >, so of equal powers the earlier grid
    index ranks first.  -> (rps [nbest], idx [nbest]), (RESET_RP, -1) where nothing was inserted."""
    rps = [RESET_RP] * nbest
    idx = [-1] * nbest
    for u in range(len(values)):
        rp = float(values[u])
        if rp > rps[nbest - 1]:
            for n1 in range(nbest):
                if rp > rps[n1]:
                    for n2 in range(nbest - 1, n1, -1):
                        rps[n2] = rps[n2 - 1]
                        idx[n2] = idx[n2 - 1]
                    rps[n1] = rp
                    idx[n1] = u
                    break
    return np.array(rps, np.float64), np.array(idx, np.int64)


def run(X, sv, M, nbest, fmin=1, fmax=None, threshold=0.0, acc=None):
    """next() over the frames of X [K][N][T]: per-frame N-best, gate, accumulated powers (float64)."""
    rp, _ = response_power(X, sv, M, fmin, fmax)
    en = energy(X, M, fmin, fmax)
    U, T = rp.shape
    acc = np.zeros(U) if acc is None else acc
    nb_rp = np.full((T, nbest), RESET_RP)
    nb_idx = np.full((T, nbest), -1, np.int64)
    gate = np.zeros(T, bool)
    for t in range(T):
        if en[t] < threshold:
            continue
        gate[t] = True
        acc += rp[:, t]
        nb_rp[t], nb_idx[t] = nbest_insert(rp[:, t], nbest)
    return rp, en, nb_rp, nb_idx, gate, acc


def plane_wave_snapshots(rng, M, fs, positions, thetas_src, T, snr_db=None, amp=1.0):
    """Subband snapshots [K][N][T] of plane waves from the given directions: channel n carries s_k[t] exp(-j w_k d_n) with
    d_n the delays above and an independent complex Gaussian s per source, bin and frame; plus independent complex Gaussian
    noise per channel at snr_db (None: noiseless).  Returns (X complex128, S [nsrc][K][T])."""
    N, K = len(positions), M // 2 + 1
    X = np.zeros((K, N, T), np.complex128)
    src = []
    for th in thetas_src:
        d = delays(positions, th)
        s = amp * (rng.normal(size=(K, T)) + 1j * rng.normal(size=(K, T))) / np.sqrt(2.0)
        for k in range(K):
            a = N * mainlobe_row(M, k, fs, d) if k >= 1 else np.ones(N)
            X[k] += a[:, None] * s[k][None, :]
        src.append(s)
    if snr_db is not None:
        sigma = amp * np.sqrt(len(thetas_src)) * 10.0 ** (-snr_db / 20.0)
        X += sigma * (rng.normal(size=X.shape) + 1j * rng.normal(size=X.shape)) / np.sqrt(2.0)
    return X, np.array(src)
