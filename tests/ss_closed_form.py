"""float64 numpy closed forms of the single-channel enhancement nodes (csrc/ss_kernels.hip, include/btkhip.h), over whole
blocks in the engine's layout, with per-frame flags -- what tests/test_gpu_ss.py holds the kernels against and what
tests/test_ss_cpu.py holds against a frame-by-frame restatement of the reference's loops.

    ss_closed_form      SpectralSubtractor::next + AveragePSDEstimator::add_sample   X [S][K][C][T] -> Y [S][K][T]
    ss_finish_training  AveragePSDEstimator::average
    ss_clear            clear_noise_samples() / clear()
    wiener_closed_form  WienerFilter::next                                            Sx, Nx [S][K][T] -> Y [S][K][T]
    highpass_closed_form HighPassFilter::next

The forms are vectorised over streams and bins and walk frames and channels in order; the state is a dict of numpy arrays in
the engine's shapes and is updated in place, so a sequence of calls continues a stream.  CASES is the table of shapes and flag
schedules the GPU tests run."""
import numpy as np

TRAIN, SUBTRACT = 1, 2
UPDATE_NOISE = 1


def f32(v):
    """A parameter as the kernels and the reference hold it: rounded to float32."""
    return float(np.float32(v))


def ss_new_state(S, C, M):
    K = M // 2 + 1
    return dict(est=np.zeros((S, C, K)), acc=np.zeros((S, C, K)), count=np.zeros((S, C), np.int64),
                added=np.zeros((S, C), np.uint8), frames_done=0)


def ss_copy_state(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def ss_closed_form(X, flags, ft, floor, alphas, st):
    """X complex [S][K][C][T]; flags uint8 [T]; alphas [C] (< 0: averaging channel).  Returns Y complex128 [S][K][T]."""
    X = np.asarray(X, np.complex128)
    S, K, C, T = X.shape
    Y = np.zeros((S, K, T), np.complex128)
    for t in range(T):
        acc_y = np.zeros((S, K), np.complex128)
        for c in range(C):
            x = X[:, :, c, t]
            p = x.real * x.real + x.imag * x.imag
            if flags[t] & TRAIN:
                if alphas[c] >= 0:
                    fresh = (st["added"][:, c] == 0)[:, None]
                    st["est"][:, c] = np.where(fresh, p, alphas[c] * st["est"][:, c] + (1.0 - alphas[c]) * p)
                    st["added"][:, c] = 1
                else:
                    st["acc"][:, c] += p
                    st["count"][:, c] += 1
            if flags[t] & SUBTRACT:
                s2 = p - ft * st["est"][:, c]
                s2 = np.where(s2 <= floor, floor, s2)
                mag = np.sqrt(s2)
                with np.errstate(invalid="ignore", divide="ignore"):
                    term = np.where(p == 0, mag + 0j, x * (mag / np.sqrt(p)))
            else:
                term = x
            acc_y += term
        Y[:, :, t] = acc_y / C
    st["frames_done"] += T
    return Y


def ss_term_magnitudes(X, flags, ft, floor, alphas, st):
    """Per channel: |term| [S][K][C][T], the estimate each frame was subtracted with, est [S][K][C][T], and |X|^2 -- the
    quantities the error bound of tests/test_gpu_ss.py is built from.  `st` is walked on a copy."""
    st = ss_copy_state(st)
    X = np.asarray(X, np.complex128)
    S, K, C, T = X.shape
    mag = np.zeros((S, K, C, T))
    est = np.zeros((S, K, C, T))
    P = X.real ** 2 + X.imag ** 2
    for t in range(T):
        ss_closed_form(X[..., t:t + 1], flags[t:t + 1], ft, floor, alphas, st)
        est[..., t] = st["est"].transpose(0, 2, 1)
        if flags[t] & SUBTRACT:
            s2 = P[..., t] - ft * est[..., t]
            mag[..., t] = np.sqrt(np.where(s2 <= floor, floor, s2))
        else:
            mag[..., t] = np.sqrt(P[..., t])
    return mag, est, P


def ss_finish_training(alphas, st):
    """average(): est = acc * (1.0/(float)count) on averaging channels; count = 0 gives 0 * inf = NaN."""
    for c, a in enumerate(alphas):
        if a < 0:
            with np.errstate(divide="ignore", invalid="ignore"):
                scale = 1.0 / np.float32(st["count"][:, c]).astype(np.float64)
                st["est"][:, c] = st["acc"][:, c] * scale[:, None]


def ss_clear(st, everything):
    st["acc"][:] = 0
    st["count"][:] = 0
    if everything:
        st["added"][:] = 0


def wiener_new_state(S, M):
    K = M // 2 + 1
    return dict(psd_s=np.zeros((S, K)), psd_n=np.zeros((S, K)), frames_done=0)


def wiener_closed_form(Sx, Nx, flags, alpha, floor, beta, st):
    """Sx, Nx complex [S][K][T]; flags uint8 [T], bit 0 = the frame updates the noise PSD.  Returns Y complex128 [S][K][T]."""
    Sx = np.asarray(Sx, np.complex128)
    Nx = np.asarray(Nx, np.complex128)
    S, K, T = Sx.shape
    Y = np.zeros((S, K, T), np.complex128)
    for t in range(T):
        a = alpha if st["frames_done"] + t >= 2 else 0.0           # frame_no_ > 0 before the increment
        Y[:, 0, t] = Sx[:, 0, t]
        s, n = Sx[:, 1:, t], Nx[:, 1:, t]
        ps = a * st["psd_s"][:, 1:] + (1.0 - a) * (s.real ** 2 + s.imag ** 2)
        if flags[t] & UPDATE_NOISE:
            pn_now = n.real ** 2 + n.imag ** 2
            pn_now = np.where(pn_now < floor, floor, pn_now)
            pn = a * st["psd_n"][:, 1:] + (1.0 - a) * pn_now
            st["psd_n"][:, 1:] = pn
        else:
            pn = st["psd_n"][:, 1:]
        with np.errstate(invalid="ignore", divide="ignore"):
            H = ps / (ps + beta * pn)
        Y[:, 1:, t] = H * s
        st["psd_s"][:, 1:] = ps
    st["frames_done"] += T
    return Y


def highpass_closed_form(X, cutoff):
    """Bins 0 .. cutoff-1 zero (DC included), the others copied; cutoff = 0 copies everything."""
    Y = np.array(X, np.complex128)
    Y[:, :cutoff] = 0
    return Y


def highpass_cutoff_bin(M, cut_off_freq, samplerate):
    return int(np.float32(M) * np.float32(cut_off_freq) / np.float32(samplerate))


# ---------------------------------------------------------------------------------------------------- inputs and schedules
def make_input(S, K, C, T, seed, zeros=True):
    """complex64 [S][K][C][T] of unit-variance noise with a slowly varying level, a few exact zeros and a loud burst."""
    rng = np.random.default_rng(seed)
    X = (rng.normal(size=(S, K, C, T)) + 1j * rng.normal(size=(S, K, C, T))) * (0.5 + rng.random((S, K, C, 1)))
    if T > 8:
        X[..., T // 2:T // 2 + 3] *= 4.0
    if zeros:
        X[0, 0, 0, 0] = 0
        X[-1, K - 1, C - 1, T - 1] = 0
    return X.astype(np.complex64)


def schedule(name, T, seed=0):
    """Flag schedules of the subtractor, uint8 [T]."""
    f = np.zeros(T, np.uint8)
    if name == "train_then_subtract":
        n = max(1, T // 3)
        f[:n] = TRAIN
        f[n:] = SUBTRACT
    elif name == "both":
        f[:] = TRAIN | SUBTRACT
    elif name == "vad":                          # a pseudo voice-activity label: noise frames train, every frame is subtracted
        rng = np.random.default_rng(100 + seed)
        f[:] = SUBTRACT
        f[rng.random(T) < 0.4] |= TRAIN
        f[0] = SUBTRACT                          # the first frame is subtracted against the untouched state
    elif name == "all_off":
        pass
    elif name == "subtract":
        f[:] = SUBTRACT
    else:
        raise KeyError(name)
    return f


# M, S, C, T, T_stride - T, alphas, schedule, ft, floor
CASES = [
    (8, 1, 1, 1, 3, (0.75,), "both", 1.0, 1e-3),
    (8, 3, 2, 63, 1, (0.5, -1.0), "train_then_subtract", 1.5, 1e-2),
    (8, 1, 3, 64, 0, (0.9375, -1.0, 0.0), "vad", 1.0, 1e-2),
    (32, 3, 1, 65, 7, (0.75,), "both", 2.0, 1e-2),
    (32, 1, 2, 130, 2, (-1.0, -1.0), "train_then_subtract", 1.0, 1e-3),
    (32, 3, 3, 200, 8, (0.875, -1.0, 0.5), "vad", 1.25, 1e-2),
    (8, 1, 2, 200, 5, (0.96875, 0.25), "both", 1.0, 0.0),
    (32, 1, 1, 130, 1, (0.5,), "all_off", 1.0, 1e-3),
    (8, 3, 3, 65, 3, (0.5, -1.0, 0.75), "all_off", 1.0, 1e-3),
]
