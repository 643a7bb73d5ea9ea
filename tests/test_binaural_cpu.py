"""CPU: the closed forms of tests/binaural_closed_form.py against a plain per-frame, per-bin restatement of the reference's loops
(postfilter/binauralprocessing.cc), and the two host entry points of the C-ABI (btk_binaural_candidates, btk_binaural_threshold)
against both.  The loops below follow the reference's text line by line -- one frame, one candidate, one bin at a time, float
members as float32 -- and are the only place where that text is restated without vectorisation."""
import math

import numpy as np
import pytest

from tests import binaural_closed_form as cf

M, T, S = 16, 7, 2
K = M // 2 + 1


def _inputs(seed=0):
    rng = np.random.default_rng(seed)
    shape = (S, K, T)
    XL = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    XR = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    return XL, XR


# ---- the reference, loop by loop -------------------------------------------------------------------------------------------
def _arg(z):
    return 0.0 if (z.real == 0 and z.imag == 0) else math.atan2(z.imag, z.real)


def _calc_itd(k, fft_len, xl, xr):                                # calcITDf, :17-38
    al, ar = _arg(xl), _arg(xr)
    d1, d2, d3 = abs(al - ar), abs(al - ar - 2 * math.pi), abs(al - ar + 2 * math.pi)
    pd = d1 if d1 < d2 else d2
    if d3 < pd:
        pd = d3
    den = 2 * math.pi * k / fft_len
    if den == 0:
        return math.nan if pd == 0 else math.inf
    return pd / den


def _loop_mask(XL, XR, kind, chan, threshold, alpha, eta, prev_mu, thresholds=None):
    """masking1 frame by frame (:138-179, :441-485); prev_mu float64 [K] in place; returns Y [K][T] and threshold_ at the end"""
    alpha, eta, threshold = cf.f32(alpha), cf.f32(eta), cf.f32(threshold)
    om = cf.f32(np.float32(1) - np.float32(alpha))
    ome = cf.f32(np.float32(om) * np.float32(eta))
    Kb, Tn = XL.shape
    Y = np.zeros((Kb, Tn), np.complex128)
    for t in range(Tn):
        Y[0, t] = XL[0, t]
        for k in range(1, Kb):
            if kind == cf.KIM:
                le = _calc_itd(k, 2 * (Kb - 1), complex(XL[k, t]), complex(XR[k, t])) <= threshold
                b = (om if le else ome) if chan == 0 else (ome if le else om)
                x = XL[k, t] if chan == 0 else XR[k, t]
            else:
                if thresholds is not None:
                    threshold = cf.f32(thresholds[k])
                xt, xi = (XL[k, t], XR[k, t]) if chan == 0 else (XR[k, t], XL[k, t])
                b = ome if abs(complex(xt)) <= abs(complex(xi)) + threshold else om
                x = xt
            mu = alpha * prev_mu[k] + b
            Y[k, t] = complex(x) * mu
            prev_mu[k] = mu
    return Y, threshold


def _loop_stats(XL, XR, kind, lo, hi, width, eta, pc, k0, k1):
    """the three accumStats1 frame by frame (:314-353, :548-603, :794-838) with the candidate walk as written there"""
    eta, pc = cf.f32(eta), cf.f32(pc)
    lo, hi, width = np.float32(lo), np.float32(hi), np.float32(width)
    n_cand = int(np.float64(np.float32(hi - lo) / width) + 1.5)
    Kb, Tn = XL.shape
    sums = np.zeros((Kb, n_cand, 3)) if kind == cf.FDIID else np.zeros((n_cand, cf.NV[kind]))
    for t in range(Tn):
        if kind == cf.FDIID:
            for k in range(1, Kb):
                i, thr = 0, lo
                while thr <= hi:
                    pt, pi = abs(complex(XL[k, t])), abs(complex(XR[k, t]))
                    mt = eta if pt <= pi + float(thr) else 1.0
                    mi = eta if pi <= pt + float(thr) else 1.0
                    y1t = abs(complex(XL[k, t]) * mt) ** (2.0 * pc)
                    y1i = abs(complex(XR[k, t]) * mi) ** (2.0 * pc)
                    y2t, y2i = y1t * y1t, y1i * y1i
                    sums[k, i, 0] += y2t * y2t + y2i * y2i
                    sums[k, i, 1] += y1t + y1i
                    sums[k, i, 2] += y2t + y2i
                    thr = np.float32(thr + width)
                    i += 1
            continue
        i, thr = 0, lo
        while thr <= hi:
            if kind == cf.KIM:
                PT = PI = 0.0
                for k in range(k0, k1):
                    xl, xr = complex(XL[k, t]), complex(XR[k, t])
                    mt, mi = (1.0, eta) if _calc_itd(k, 2 * (Kb - 1), xl, xr) <= float(thr) else (eta, 1.0)
                    PT += (xl.real * mt) ** 2 + (xl.imag * mt) ** 2
                    PI += (xr.real * mi) ** 2 + (xr.imag * mi) ** 2
                RT, RI = PT ** pc, PI ** pc
                sums[i] += (RT * RI, RT, RI, RT * RT, RI * RI)
            else:
                acc = np.zeros(6)
                for k in range(k0, k1):
                    xl, xr = complex(XL[k, t]), complex(XR[k, t])
                    pt, pi = abs(xl), abs(xr)
                    mt = eta if pt <= pi + float(thr) else 1.0
                    mi = eta if pi <= pt + float(thr) else 1.0
                    y1t, y1i = abs(xl * mt) ** (2.0 * pc), abs(xr * mi) ** (2.0 * pc)
                    y2t, y2i = y1t * y1t, y1i * y1i
                    acc += (y1t, y2t, y2t * y2t, y1i, y2i, y2i * y2i)
                sums[i] += acc
            thr = np.float32(thr + width)
            i += 1
    return sums, n_cand


def _loop_threshold(kind, sums, n, lo, hi, width, beta=3.0):
    """the three calc_threshold (:382-407, :632-660, :867-898) on a copy of the sums"""
    lo, hi, width = np.float32(lo), np.float32(hi), np.float32(width)
    if kind == cf.FDIID:
        arg, best = np.float32(0), 1000000.0
        per_bin = np.zeros(sums.shape[0])
        for k in range(1, sums.shape[0]):
            local, i, thr = 1000000.0, 0, lo
            while thr <= hi:
                sigma = sums[k, i, 2] / n
                rho = -(sums[k, i, 0] / n - beta * sigma * sigma)
                if rho <= best:
                    arg, best = thr, rho
                if rho <= local:
                    per_bin[k], local = float(thr), rho
                thr = np.float32(thr + width)
                i += 1
        return float(arg), per_bin
    arg, best, i, thr = lo, 1000000.0, 0, lo
    while thr <= hi:
        v = sums[i]
        if kind == cf.KIM:
            mt, mi = v[1] / n, v[2] / n
            st, si = v[3] / n - mt * mt, v[4] / n - mi * mi
            rho = abs((v[0] / n - mt * mi) / (math.sqrt(st) * math.sqrt(si)))
        else:
            sig2 = v[1] / n + v[4] / n
            rho = -((v[2] / n + v[5] / n) - beta * sig2 * sig2)
        if rho < best:
            arg, best = thr, rho
        thr = np.float32(thr + width)
        i += 1
    return float(arg), None


# ---- closed form against the loops ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [cf.KIM, cf.IID])
@pytest.mark.parametrize("chan", [0, 1])
@pytest.mark.parametrize("alpha", [0.0, 0.6])
def test_mask_closed_form_matches_the_loops(kind, chan, alpha):
    XL, XR = _inputs(1)
    thr = 0.9 if kind == cf.KIM else 0.3
    mu0 = np.ones((S, K))
    Y, mu = cf.mask_closed_form(XL, XR, kind, chan, thr, alpha, 0.01, mu0)
    for s in range(S):
        pm = np.ones(K)
        Yl, _ = _loop_mask(XL[s], XR[s], kind, chan, thr, alpha, 0.01, pm)
        np.testing.assert_allclose(Y[s], Yl, rtol=1e-14, atol=0)
        np.testing.assert_allclose(mu0[s, 1:], pm[1:], rtol=1e-14)
        assert mu0[s, 0] == 1.0


def test_mask_bin0_is_the_left_input_and_per_bin_thresholds_leave_the_last():
    XL, XR = _inputs(2)
    thrs = np.linspace(-1, 1, K)
    for chan in (0, 1):
        mu0 = np.ones((S, K))
        Y, _ = cf.mask_closed_form(XL, XR, cf.IID, chan, 0.0, 0.5, 0.1, mu0, thresholds=thrs)
        assert np.array_equal(Y[:, 0], XL[:, 0].astype(np.complex128))
        Yl, last = _loop_mask(XL[0], XR[0], cf.IID, chan, 0.0, 0.5, 0.1, np.ones(K), thresholds=thrs)
        np.testing.assert_allclose(Y[0], Yl, rtol=1e-14)
        assert last == cf.f32(thrs[-1])                              # threshold() after a frame: the last bin's value
    # Kim ignores per-bin thresholds
    a = cf.mask_closed_form(XL, XR, cf.KIM, 0, 0.7, 0.5, 0.1, np.ones((S, K)), thresholds=thrs)[0]
    b = cf.mask_closed_form(XL, XR, cf.KIM, 0, 0.7, 0.5, 0.1, np.ones((S, K)))[0]
    assert np.array_equal(a, b)


def test_exact_ties():
    XL, _ = _inputs(3)
    # XL == XR: ITD is exactly 0 <= 0 -> the target is kept (mu = 1 at alpha = 0); IID: |X_T| <= |X_I| + 0 -> eta
    Y, mu = cf.mask_closed_form(XL, XL, cf.KIM, 0, 0.0, 0.0, 0.25, np.ones((S, K)))
    assert np.all(mu[:, 1:] == 1.0)
    Y, mu = cf.mask_closed_form(XL, XL, cf.IID, 0, 0.0, 0.0, 0.25, np.ones((S, K)))
    assert np.all(mu[:, 1:] == 0.25)


@pytest.mark.parametrize("kind,rng_,k0,k1", [(cf.KIM, (-2.0, 2.0, 0.25), 1, K), (cf.KIM, (0.0, 2.0, 0.1), 0, K - 2),
                                             (cf.IID, (-1.0, 1.0, 0.125), 1, K), (cf.IID, (0.0, 1.0, 0.1), 0, 5),
                                             (cf.FDIID, (-1.0, 1.0, 0.25), 1, K)])
def test_stats_closed_form_matches_the_loops(kind, rng_, k0, k1):
    XL, XR = _inputs(4)
    walk, n_cand = cf.candidates(*rng_)
    sums, pf = cf.stats_closed_form(XL, XR, kind, walk, n_cand, 0.01, 1 / 15.0, k0, k1)
    for s in range(S):
        ls, n = _loop_stats(XL[s], XR[s], kind, *rng_, 0.01, 1 / 15.0, k0, k1)
        assert n == n_cand
        np.testing.assert_allclose(sums[s], ls, rtol=1e-12, atol=0)
        if pf is not None:
            assert np.all(pf[s, :, len(walk):] == 0)
        thr = cf.threshold_closed_form(kind, sums[s], T, walk, n_cand)
        lt, per_bin = _loop_threshold(kind, ls, T, *rng_)
        assert thr[0] == lt
        if kind == cf.FDIID:
            assert np.array_equal(thr[2], per_bin)


def test_bin0_never_passes_the_itd_test():
    XL, XR = _inputs(5)
    d = cf.itd(XL, XR)
    assert not np.any(d[:, 0] <= 1e30)
    walk, n = cf.candidates(0.0, 100.0, 50.0)
    with_0 = cf.stats_closed_form(XL, XR, cf.KIM, walk, n, 0.5, 0.2, 0, 1)[1]      # bin 0 alone: (mu_T, mu_I) = (eta, 1) always
    eta = cf.f32(0.5)
    pt = (XL[:, 0].real.astype(np.float64) * eta) ** 2 + (XL[:, 0].imag.astype(np.float64) * eta) ** 2
    np.testing.assert_allclose(with_0[:, :, 0, 0], pt ** cf.f32(0.2), rtol=1e-15)


# ---- the candidate walk -----------------------------------------------------------------------------------------------------
COUNTS = [((0.0, 2.0, 0.1), 20, 21), ((0.0, 1.0, 0.1), 10, 11), ((-9.4118, 9.4118, 0.02), 942, 942), ((-1e5, 1e5, 1e3), 201, 201)]


@pytest.mark.parametrize("rng_,n_walk,n_cand", COUNTS)
def test_candidate_counts(rng_, n_walk, n_cand):
    walk, n = cf.candidates(*rng_)
    assert (len(walk), n) == (n_walk, n_cand)
    from distant_speech_recognition_amd import engine as eng
    w2, n2 = eng.binaural_candidates(*rng_)
    assert n2 == n_cand and w2.dtype == np.float32 and np.array_equal(w2, walk)


def test_kim_default_range_has_942_candidates():
    lo, hi = np.float32(-0.2 * 16000 / 340), np.float32(0.2 * 16000 / 340)
    walk, n = cf.candidates(lo, hi, 0.02)
    assert (len(walk), n) == (942, 942)


def test_a_walk_longer_than_the_arrays_is_cut():
    from distant_speech_recognition_amd import engine as eng
    # (0, 0.35, 0.1): nCand_ = (int)(3.5 + 1.5) = 5 >= walk of 4; find a range whose walk would overrun and check the cut
    for rng_ in [(0.0, 0.35, 0.1), (0.0, 0.3, 0.3), (0.0, 7.0, 1.0)]:
        walk, n = eng.binaural_candidates(*rng_)
        w2, n2 = cf.candidates(*rng_)
        assert n == n2 and np.array_equal(walk, w2) and len(walk) <= n


# ---- calc_threshold through the C-ABI: tie rules ----------------------------------------------------------------------------
class _State:
    """what engine.binaural_threshold reads of a BinauralStatsState, on the host"""

    def __init__(self, kind, sums, count, Mfft):
        import torch
        self.kind, self.M, self.Kb = kind, Mfft, Mfft // 2 + 1
        self.n_cand = sums.shape[-2]
        self.sums = torch.from_numpy(sums[None].copy())
        self.count = torch.tensor([count])


@pytest.mark.parametrize("kind", [cf.KIM, cf.IID, cf.FDIID])
def test_threshold_entry_point_matches_the_closed_form(kind):
    from distant_speech_recognition_amd import engine as eng
    XL, XR = _inputs(6)
    rng_ = (0.0, 2.0, 0.1)                                       # walk 20, slots 21
    walk, n_cand = cf.candidates(*rng_)
    sums = cf.stats_closed_form(XL, XR, kind, walk, n_cand, 0.01, 1 / 15.0)[0][0]
    ref = cf.threshold_closed_form(kind, sums, T, walk, n_cand)
    got = eng.binaural_threshold(kind, _State(kind, sums, T, M), (walk, n_cand))
    assert got[0] == ref[0]
    np.testing.assert_allclose(got[1], ref[1], rtol=1e-14, atol=0)
    assert np.all(got[1][..., len(walk):] == 0)
    if kind == cf.FDIID:
        assert np.array_equal(got[2], ref[2])
    # idempotent: the sums are not divided in place
    again = eng.binaural_threshold(kind, _State(kind, sums, T, M), (walk, n_cand))
    assert again[0] == got[0] and np.array_equal(again[1], got[1])


def test_tie_rules():
    from distant_speech_recognition_amd import engine as eng
    walk, n_cand = cf.candidates(0.0, 3.0, 1.0)                 # 0, 1, 2, 3
    assert len(walk) == 4 and n_cand == 4
    # IID: all four candidates have the same cost -> the FIRST wins
    row = np.array([1.0, 2.0, 30.0, 1.0, 2.0, 30.0])
    sums = np.tile(row, (4, 1))
    for f in (cf.threshold_closed_form, None):
        thr = (f(cf.IID, sums, 2, walk, n_cand) if f else eng.binaural_threshold(cf.IID, _State(cf.IID, sums, 2, 4), (walk, n_cand)))[0]
        assert thr == 0.0
    # Kim: rho equal for candidates 1 and 2 and smaller than for 0 and 3 -> candidate 1
    def kim_row(c):                                              # n = 1: mean_T = mean_I = 1, sigma = 1, rho = |c - 1|
        return np.array([c, 1.0, 1.0, 2.0, 2.0])
    sums = np.stack([kim_row(1.5), kim_row(1.25), kim_row(1.25), kim_row(2.0)])
    for f in (cf.threshold_closed_form, None):
        thr = (f(cf.KIM, sums, 1, walk, n_cand) if f else eng.binaural_threshold(cf.KIM, _State(cf.KIM, sums, 1, 4), (walk, n_cand)))[0]
        assert thr == 1.0
    # FD-IID: equal costs -> the LAST wins, per bin and over all bins (bins 1 and 2 of M = 4)
    sums = np.zeros((3, 4, 3))
    sums[1:] = np.array([30.0, 1.0, 2.0])
    sums[2, 1, 0] = 40.0                                         # bin 2: candidate 1 alone is best there and overall ...
    sums[1, 3, 0] = 40.0                                         # ... tied by bin 1, candidate 3, which bin 2 then ties again at 1
    for f in (cf.threshold_closed_form, None):
        r = f(cf.FDIID, sums, 1, walk, n_cand) if f else eng.binaural_threshold(cf.FDIID, _State(cf.FDIID, sums, 1, 4), (walk, n_cand))
        assert r[2][1] == 3.0 and r[2][2] == 1.0 and r[0] == 1.0
    sums[:] = 0.0
    sums[1:] = np.array([30.0, 1.0, 2.0])
    r = eng.binaural_threshold(cf.FDIID, _State(cf.FDIID, sums, 1, 4), (walk, n_cand))
    assert r[0] == 3.0 and r[2][1] == 3.0 and r[2][2] == 3.0 and r[2][0] == 0.0
