"""Float64 closed forms of the energy family of btk20.sad (reference sad/sad.cc), vectorised numpy, restated here.

Frames are summed in index order (a loop over the element index, vectorised over frames), windows are compared by counting,
the hangover machine is expressed through run lengths.  tests/test_vad_cpu.py holds every function against a literal per-frame
restatement of the reference's loops; tests/test_gpu_vad.py holds the kernels against these."""
import numpy as np

POWER, NORMALIZED, TSPS = 0, 1, 2
SINGLE, MI, MULTISTAGE = 0, 1, 2
E0_DEFAULT = {POWER: 1.0, NORMALIZED: 1.0, TSPS: 5000.0}


def frame_energy(x):
    """x [..., T, D] float32 or complex64 -> float64 [..., T]: sum_n |x_n|^2 in index order"""
    x = np.asarray(x)
    acc = np.zeros(x.shape[:-1], np.float64)
    for n in range(x.shape[-1]):
        if np.iscomplexobj(x):
            re, im = x[..., n].real.astype(np.float64), x[..., n].imag.astype(np.float64)
            acc = acc + (re * re + im * im)
        else:
            v = x[..., n].astype(np.float64)
            acc = acc + v * v
    return acc


def pcm_frames(pcm, D, shift):
    """pcm [S][L] -> [S][T][D], T = (L - D) // shift + 1 whole frames"""
    pcm = np.asarray(pcm)
    T = (pcm.shape[-1] - D) // shift + 1 if pcm.shape[-1] >= D else 0
    idx = np.arange(T)[:, None] * shift + np.arange(D)[None, :]
    return pcm[..., idx]


def band_limits(fftLen, samplerate, low, high):
    """(lowX, highX, binN); ValueError where the reference throws jdimension_error"""
    lowX, highX = 0, fftLen // 2
    if not low < 0.0:
        if low >= samplerate / 2.0:
            raise ValueError("low cutoff")
        lowX = int((low / samplerate) * fftLen)
    if not high < 0.0:
        if high >= samplerate / 2.0:
            raise ValueError("high cutoff")
        highX = int((high / samplerate) * fftLen + 0.5)
    return lowX, highX, (2 * (highX - lowX + 1) if lowX > 0 else 2 * (highX - lowX) + 1)


def band_power(spec, fftLen, lowX, highX):
    """spec float32 [S][C][T][powN] -> P float64 [S][C][T]; the weight 1 sits at k == 0 and k == fftLen/2 + 1 (sic)"""
    spec = np.asarray(spec)
    P = np.zeros(spec.shape[:-1], np.float64)
    for k in range(lowX, highX + 1):
        v = spec[..., k].astype(np.float64)
        P = P + (v if (k == 0 or k == fftLen // 2 + 1) else 2.0 * v)
    return P / float(fftLen)


def band_decision(P, kind, E0=None):
    """P [S][C][T] -> (score [S][T], value [S][T] = +-1); the channel sums run in channel order"""
    E0 = E0_DEFAULT[kind] if E0 is None else float(E0)
    Cn = P.shape[1]
    total = np.zeros(P[:, 0].shape, np.float64)
    for c in range(Cn):
        total = total + (np.sqrt(P[:, c]) if kind == NORMALIZED else P[:, c])
    with np.errstate(all="ignore"):
        if kind == POWER:
            score = P[:, 0] / total
            speech = score > E0 / Cn
        elif kind == NORMALIZED:
            score = np.sqrt(P[:, 0]) / total
            speech = score > E0 / Cn
        else:
            score = np.log(P[:, 0] / (total - P[:, 0])) - np.log(E0 / total)
            speech = score > 0.0
    return score, np.where(speech, 1.0, -1.0)


def tsps_terms(P, E0=5000.0):
    """(|log a| + |log b| + |score|) of the TSPS score log a - log b: what its error bound scales with"""
    total = np.zeros(P[:, 0].shape, np.float64)
    for c in range(P.shape[1]):
        total = total + P[:, c]
    with np.errstate(all="ignore"):
        la, lb = np.log(P[:, 0] / (total - P[:, 0])), np.log(E0 / total)
    return np.abs(la) + np.abs(lb) + np.abs(la - lb)


class EnergyMetricState:
    """window [S][N] in time order (oldest first), recognizing, above, below [S]"""

    def __init__(self, S, energiesN, initial_energy):
        self.initial = float(initial_energy)
        self.window = np.full((S, energiesN), self.initial, np.float64)
        self.recognizing = np.zeros(S, bool)
        self.above = np.zeros(S, np.int64)
        self.below = np.zeros(S, np.int64)

    def reset(self):
        self.recognizing[:] = False
        self.above[:] = 0
        self.below[:] = 0

    def next_speaker(self):
        self.reset()
        self.window[:] = self.initial


def energy_metric(energy, st, threshold, headN, tailN):
    """energy float64 [S][T] -> float64 [S][T] of 1.0 / 0.0; st is carried on.  sum > sorted[medianX]  <=>  #{e_i < sum} > medianX"""
    S, T = energy.shape
    N = st.window.shape[1]
    medianX = int(threshold * N)
    assert 0 <= medianX < N
    out = np.zeros((S, T), np.float64)
    for t in range(T):
        e = energy[:, t]
        with np.errstate(invalid="ignore"):
            above = (st.window < e[:, None]).sum(axis=1) > medianX
        shift = ~st.recognizing & (st.above == 0)
        st.window[shift] = np.concatenate([st.window[shift, 1:], e[shift, None]], axis=1)
        rec = st.recognizing.copy()
        # recognizing: a detection clears the misses, the tailN-th miss in a row ends the recognition
        st.below = np.where(rec, np.where(above, 0, st.below + 1), st.below)
        stop = rec & ~above & (st.below == tailN)
        # waiting: the headN-th detection in a row starts it
        st.above = np.where(~rec, np.where(above, st.above + 1, 0), st.above)
        go = ~rec & above & (st.above == headN)
        st.recognizing = (rec & ~stop) | go
        st.above = np.where(stop, 0, st.above)
        st.below = np.where(go, 0, st.below)
        out[:, t] = above
    return out


def simple_energy(energy, s0, threshold, gamma):
    """energy [S][T], s0 [S] -> (is_speech bool [S][T], smoothed [S][T]); three roundings per step"""
    S, T = energy.shape
    s = np.array(s0, np.float64)
    sm = np.zeros((S, T), np.float64)
    for t in range(T):
        s = gamma * s + (1.0 - gamma) * energy[:, t]
        sm[:, t] = s
    with np.errstate(all="ignore"):
        return energy / sm > threshold, sm


def detections(values, thresholds, rule, dm0=0):
    """values [R][T] -> (above bool [T], decision_metric code after each frame int [T]) of one stream"""
    v = np.asarray(values, np.float64)
    R, T = v.shape
    if rule == SINGLE:
        return v[0] > thresholds[0], np.full(T, dm0, np.int64)
    if rule == MULTISTAGE and R < 3:
        return np.zeros(T, bool), np.full(T, dm0, np.int64)
    veto = v[0] < 0.5
    if rule == MI:
        a, b = v[1] < 0.5, v[2] > 0.5
        code = np.where(veto, -1, np.where(a, 2, np.where(b, 3, -3)))
        return ~veto & (a | b), code
    wins = v[1:] > 0.5                                  # [R-1][T]
    anyw = wins.any(axis=0)
    first = np.argmax(wins, axis=0) + 2                 # stage m (from 1) -> code m + 1
    code = np.where(veto, -1, np.where(anyw, first, -R))
    return ~veto & anyw, code


def _run_lengths(flags):
    """run[t] = length of the run of True that ends at t (0 where flags[t] is False)"""
    flags = np.asarray(flags, bool)
    idx = np.arange(flags.size)
    last_false = np.maximum.accumulate(np.where(~flags, idx, -1))
    return np.where(flags, idx - last_false, 0)


def hangover_segments(above, headN, tailN, restart=False):
    """above bool [T] of one stream from frame 0 -> list of (start, end) with end exclusive and None where the source ended first.
    Onset: the first q whose run of detections reaches headN, start = q - headN + 1; end: the first frame after q on which a run
    of misses (counted from q + 1) reaches tailN."""
    above = np.asarray(above, bool)
    T, out, t0 = above.size, [], 0
    while t0 < T:
        run = _run_lengths(above[t0:])
        hit = np.nonzero(run == headN)[0]
        if hit.size == 0:
            break
        q = t0 + int(hit[0])
        miss = _run_lengths(~above[q + 1:])
        stop = np.nonzero(miss == tailN)[0] if tailN > 0 else np.zeros(0, int)
        if stop.size == 0:
            out.append((q - headN + 1, None))
            break
        end = q + 1 + int(stop[0])
        out.append((q - headN + 1, end))
        if not restart:
            break
        t0 = end + 1
    return out


def segments_to_labels(segments, shiftlen, samplerate):
    delta = shiftlen / float(samplerate)
    out = []
    for a, b in segments:
        ea = eb = 0.0
        for t in range(b - 1):
            eb += delta
            if t + 1 == a:
                ea = eb
        out.append([ea if a > 0 else 0.0, eb])
    return out
