"""Closed forms of the objective measures (csrc/obj_kernels.hip, include/btkhip.h) in numpy: element-wise steps in np.float32,
sums with math.fsum (the correctly rounded float64 sum), and a float32 restatement of the reference's calcSNR / calcISDistance
(objective_measure/objective_measure.cc:42-185, :284-331) written from their description: running float sums in index order."""
import math

import numpy as np

F32 = np.float32
FLT_MAX = F32(np.finfo(np.float32).max)
MEAN, PEAK, POWER, PROJECT = 1, 2, 4, 8


def fsum(a):
    return math.fsum(np.asarray(a, np.float64).ravel().tolist())


# ------------------------------------------------------------------ SNR
def snr_scales(x1, x2, option):
    """mu1, mu2, a1, a2 (np.float32) of the closed form; x1, x2 float32 vectors of n1, n2 samples."""
    x1, x2 = np.asarray(x1, F32), np.asarray(x2, F32)
    mu1 = mu2 = F32(0)
    if option & MEAN:
        mu1, mu2 = F32(fsum(x1) / len(x1)), F32(fsum(x2) / len(x2))
    c1, c2 = (x1 - mu1).astype(F32), (x2 - mu2).astype(F32)
    a1 = a2 = F32(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        if option & PEAK:
            a1 = F32(1) / max(F32(-10000), c1.max())
            a2 = F32(1) / max(F32(-10000), c2.max())
        elif option & POWER:
            p1 = np.float64(fsum(c1.astype(np.float64) ** 2)) / len(x1)
            p2 = np.float64(fsum(c2.astype(np.float64) ** 2)) / len(x2)
            a2 = F32(np.sqrt(p1 / p2))
        elif option & PROJECT:
            if len(x1) < len(x2):
                raise ValueError("option 8 needs n1 >= n2")
            n2 = len(x2)
            a2 = F32(np.float64(fsum(c1[:n2].astype(np.float64) * c2.astype(np.float64))) / np.float64(fsum(c2.astype(np.float64) ** 2)))
    return mu1, mu2, F32(a1), F32(a2)


def snr_values(x1, x2, mu1, mu2, a1, a2):
    """v1, v2: the centred and scaled samples, float32."""
    with np.errstate(invalid="ignore", over="ignore"):
        v1 = ((np.asarray(x1, F32) - F32(mu1)).astype(F32) * F32(a1)).astype(F32)
        v2 = ((np.asarray(x2, F32) - F32(mu2)).astype(F32) * F32(a2)).astype(F32)
    return v1, v2


def snr_sums(x1, x2, mu1, mu2, a1, a2):
    """sum, err for given means and scales: over i < nmin v1^2 and f32(v1 - v2)^2, the longer tail's v^2 in both."""
    v1, v2 = snr_values(x1, x2, mu1, mu2, a1, a2)
    nmin = min(len(v1), len(v2))
    d = (v1[:nmin] - v2[:nmin]).astype(F32)
    tail = (v1 if len(v1) > len(v2) else v2)[nmin:].astype(np.float64) ** 2
    return (fsum(np.concatenate([v1[:nmin].astype(np.float64) ** 2, tail])),
            fsum(np.concatenate([d.astype(np.float64) ** 2, tail])))


def snr_db(sum_, err):
    """err > 0 ? 10 log10f(f32(sum / err)) : FLT_MAX in float32 steps, the logarithm correctly rounded."""
    if not err > 0:
        return FLT_MAX
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        ratio = F32(np.float64(sum_) / np.float64(err))
        return F32(10) * F32(np.log10(np.float64(ratio)))


def snr(x1, x2, option):
    sc = snr_scales(x1, x2, option)
    s, e = snr_sums(x1, x2, *sc)
    return snr_db(s, e), sc, s, e


def segment_rows(x1, x2, mu1, mu2, a1, a2, L):
    """sum_b, err_b float64 [B][2] of the whole L-sample segments below nmin."""
    v1, v2 = snr_values(x1, x2, mu1, mu2, a1, a2)
    B = min(len(v1), len(v2)) // L
    rows = np.zeros((B, 2), np.float64)
    for b in range(B):
        w1, w2 = v1[b * L:(b + 1) * L], v2[b * L:(b + 1) * L]
        rows[b] = fsum(w1.astype(np.float64) ** 2), fsum((w1 - w2).astype(F32).astype(np.float64) ** 2)
    return rows


def segmental_snr(rows, lo=-10.0, hi=35.0):
    """Mean over the segments of 10 log10(sum_b / err_b) clamped to [lo, hi]; err_b = 0: hi, sum_b = 0: lo; no segment: NaN."""
    vals = []
    for s, e in rows:
        if e == 0:
            vals.append(hi)
        elif s == 0:
            vals.append(lo)
        else:
            vals.append(min(max(10.0 * math.log10(s / e), lo), hi))
    return fsum(vals) / len(vals) if vals else float("nan")


def calc_snr_f32(x1, x2, option):
    """calcSNR as the reference runs it (ignoreSizeDifference false): every value and every running sum a float."""
    def run(a):                                   # float s = 0; for (...) s += a[i];
        return np.add.accumulate(np.asarray(a, F32), dtype=F32)[-1] if len(a) else F32(0)
    x1, x2 = np.array(x1, F32), np.array(x2, F32)
    n1, n2 = len(x1), len(x2)
    nmin = min(n1, n2)
    if option & MEAN:
        x1 = (x1 + -(run(x1) / F32(n1))).astype(F32)
        x2 = (x2 + -(run(x2) / F32(n2))).astype(F32)
    a1 = a2 = F32(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if option & PEAK:
            a1 = F32(1.0 / float(max(F32(-10000), x1.max())))
            a2 = F32(1.0 / float(max(F32(-10000), x2.max())))
        elif option & POWER:
            s1, s2 = run(x1 * x1) / F32(n1), run(x2 * x2) / F32(n2)
            a2 = F32(math.sqrt(float(s1 / s2)))
        elif option & PROJECT:
            a2 = run(x1[:n2] * x2) / run(x2 * x2)
        v1, v2 = (x1 * a1).astype(F32), (x2 * a2).astype(F32)
        d = (v1[:nmin] - v2[:nmin]).astype(F32)
        tail = (v1 if n1 > n2 else v2)[nmin:]
        sum_ = run(np.concatenate([v1[:nmin] * v1[:nmin], tail * tail]))
        err = run(np.concatenate([d * d, tail * tail]))
        return F32(10) * np.log10(F32(sum_ / err)) if err > 0 else FLT_MAX


# ------------------------------------------------------------------ Itakura-Saito distance
def get_window(window_type, M):
    """get_window (modulated.cc:47-72): 0 rectangular, 2 Hann, anything else Hamming."""
    i = np.arange(M, dtype=np.float64)
    if window_type == 0:
        return np.ones(M)
    if window_type == 2:
        return 0.5 * (1 - np.cos(2.0 * math.pi * i / (M - 1)))
    return 0.54 - 0.46 * np.cos(2. * math.pi / (M - 1) * i)


def num_frames(n, D):
    return (n + D - 1) // D + 1


def stft64(x, M, r, window_type=1):
    """Frames of the windowed FFT bank in float64: window rounded to float32 as the plan holds it, frame t the samples
    (t + 1) D - M .. (t + 1) D - 1 (zero outside the signal) -> complex128 [F][M]."""
    x = np.asarray(x, np.float64)
    D = M >> r
    F = num_frames(len(x), D)
    pad = np.concatenate([np.zeros(M), x, np.zeros(M + D)])
    win = get_window(window_type, M).astype(F32).astype(np.float64)
    fr = np.stack([pad[(t + 1) * D: (t + 1) * D + M] for t in range(F)])
    return np.fft.fft(fr * win, axis=1)


def eis_rows(X1, X2):
    """Eis_t of spectra [F][M] (bins 1 .. M/2) -> (eis float64 [F], bound (a) float64 [F]: sum over the frame's terms of
    4 2^-52 max(ratio, |log ratio|, 1), divided by M/2 like the terms)."""
    X1, X2 = np.asarray(X1), np.asarray(X2)
    F = min(len(X1), len(X2))
    H = X1.shape[1] // 2
    eis, bound = np.zeros(F), np.zeros(F)
    for t in range(F):
        a, b = X1[t, 1:H + 1], X2[t, 1:H + 1]
        P1 = (a.real.astype(np.float64) ** 2 + a.imag.astype(np.float64) ** 2).astype(F32)
        P2 = (b.real.astype(np.float64) ** 2 + b.imag.astype(np.float64) ** 2).astype(F32)
        ok = (P1 > 0) & (P2 > 0)
        ratio = (P1[ok] / P2[ok]).astype(F32).astype(np.float64)
        lg = np.log(ratio)
        eis[t] = fsum(ratio - lg - 1.0) / H
        bound[t] = fsum(4 * 2.0 ** -52 * np.maximum(np.maximum(ratio, np.abs(lg)), 1.0)) / H
    return eis, bound


def frame_range(F, bframe, eframe):
    """The frames bframe <= t < F with t <= eframe unless eframe < 0 -> (lo, hi), hi exclusive."""
    hi = F if eframe < 0 else min(F, eframe + 1)
    return bframe, max(hi, bframe)


def is_distance(eis, bframe=0, eframe=-1):
    lo, hi = frame_range(len(eis), bframe, eframe)
    return fsum(eis[lo:hi]) / (hi - lo) if hi > lo else float("nan")


def calc_is_f32(X1, X2, bframe=0, eframe=-1):
    """calcISDistance as the reference runs it on its float64 spectra: P, ratio, the terms, Eis and the sums are floats."""
    F = min(len(X1), len(X2))
    H = X1.shape[1] // 2
    sum_dist, n = F32(0), 0
    for t in range(F):
        if t >= bframe and (t <= eframe or eframe < 0):
            P1 = (X1[t, 1:H + 1].real ** 2 + X1[t, 1:H + 1].imag ** 2).astype(F32)
            P2 = (X2[t, 1:H + 1].real ** 2 + X2[t, 1:H + 1].imag ** 2).astype(F32)
            ok = (P1 > 0) & (P2 > 0)
            ratio = (P1[ok] / P2[ok]).astype(F32)
            terms = ((ratio - np.log(ratio).astype(F32)).astype(F32) - F32(1)).astype(F32)
            e = np.add.accumulate(terms, dtype=F32)[-1] if len(terms) else F32(0)
            sum_dist = F32(sum_dist + F32(e / F32(H)))
            n += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return F32(sum_dist) / F32(n)
