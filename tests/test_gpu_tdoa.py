"""GPU: btk_tdoa_spectra and btk_tdoa_gcc_peaks (engine.tdoa_*) against the float64 closed form of tests/tdoa_closed_form.py.

Bounds (derived, not tuned).  u = 2^-24.

Spectra, per frame, 2-norm, against the float64 transform of the float32-rounded windowed samples:
    ||X_gpu - X_64||_2 <= (log2 L + 1) eta ||X_64||_2,   eta = mu + gamma_4 (sqrt 2 + mu),  gamma_4 = 4u / (1 - 4u)
(Higham, Accuracy and Stability, Thm 24.2: log2 N radix-2 stages, each eta).  mu = 2^-24: the twiddles are one table computed in
float64 and rounded to float32.  The kernel runs the L-point real transform as an L/2-point complex one -- log2 L - 1 radix-2
stages' worth -- plus the split step (the "+1"; one table twiddle and two additions per point, i.e. no more than a stage).  Its
passes are radix 4: one radix-4 pass applies ONE twiddle product and two levels of additions to a point where the two radix-2
stages it replaces apply two products and two levels (the multiplication by -i is exact), so its error is within 2 eta and the
per-stage constant is unchanged.  The kernel therefore has log2 L stages' worth against the log2 L + 1 allowed.

Energy: the float32 sum of L/2 + 1 squares, each square from two products and an addition, then a factor 2 (exact):
relative error <= (L/2 + 4) u, plus twice the spectra bound for the error of X itself (|X|^2 is quadratic).  Gate decisions
derived from the float64 energy are compared only where that energy is outside this band around the threshold.

Correlation and height, against the closed form ON THE GPU'S OWN float32 spectra (stage 2 is tested as a function of its input):
every |P_k| = 1, so ||g||_2 = 1 by Parseval and |g_gpu - g_64|_inf <= ||g_gpu - g_64||_2 <= B,
    B = (log2 L + 1) eta + 4u,
the transform as above (pre-twist in place of the split step), 4u for forming and normalising P_k (a complex product of exactly
scaled operands with one fused multiply-add per component, a square root of a sum of squares, a division).

Lag: equal to the float64 lag wherever the two largest |g_64| are more than 2B apart (each may move by B); the other frames are
left out and counted, at most 1 % of a case.  Selection is exact: with gcc requested, lag is the first argmax of |gcc| as
written and height = |gcc[n]| bit for bit.

Every test prints its largest error / bound ratio and its left-out count (pytest -s shows them).
"""
import math

import numpy as np
import pytest

from tests import tdoa_closed_form as cf

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
MU = 2.0 ** -24
G4 = 4 * U / (1 - 4 * U)
ETA = MU + G4 * (math.sqrt(2.0) + MU)
KINECT_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def spectra_bound(L):
    return (math.log2(L) + 1) * ETA


def gcc_bound(L):
    return (math.log2(L) + 1) * ETA + 4 * U


def energy_bound(L):
    return (L // 2 + 4) * U + 2 * spectra_bound(L)


def _eng():
    from distant_speech_recognition_amd import engine
    return engine


def check_spectra(dev, pcm, D, L, window=True):
    """pcm float32 [S][C][len]: stage 1 against the closed form.  Returns the device tensors (X, energy)."""
    import torch
    eng = _eng()
    S, C, n = pcm.shape
    T = cf.n_frames(n, D)
    Xd, ed = eng.tdoa_spectra(torch.from_numpy(pcm).to(dev), D, L, window=window)
    assert tuple(Xd.shape) == (S, C, T, L // 2 + 1) and tuple(ed.shape) == (S, C, T) and eng.tdoa_frames(n, D) == T
    X, e = Xd.cpu().numpy().astype(np.complex128), ed.cpu().numpy().astype(np.float64)
    X64, e64 = cf.spectra(pcm, D, L, window)
    num = np.sqrt(np.sum(np.abs(X - X64) ** 2, axis=-1))
    den = np.sqrt(np.sum(np.abs(X64) ** 2, axis=-1))
    rs = float(np.max(num / np.where(den > 0, den, 1.0)) / spectra_bound(L))
    assert np.all(num <= spectra_bound(L) * den), rs
    assert np.all(X[..., 0].imag == 0) and np.all(X[..., L // 2].imag == 0)
    re = float(np.max(np.abs(e - e64) / np.where(e64 > 0, e64, 1.0)) / energy_bound(L))
    assert np.all(np.abs(e - e64) <= energy_bound(L) * e64), re
    print("spectra D=%d L=%d frames=%d: error/bound %.3f, energy error/bound %.4f" % (D, L, T, rs, re))
    return Xd, ed


def check_gcc(dev, Xd, ed, pairs, threshold, L, label, e64=None):
    """Stage 2 against the closed form on the same float32 spectra.  Returns (lag, height, closed-form tuple) of stream-major arrays."""
    eng = _eng()
    S, C, T, K = Xd.shape
    assert K == L // 2 + 1
    P = len(pairs)
    lag_d, h_d, g_d = eng.tdoa_gcc_peaks(Xd, ed, pairs, threshold, want_gcc=True)
    lag2_d, h2_d = eng.tdoa_gcc_peaks(Xd, ed, pairs, threshold)
    lag, h, g = lag_d.cpu().numpy(), h_d.cpu().numpy(), g_d.cpu().numpy()
    assert lag.shape == (S, P, T) and h.shape == (S, P, T) and g.shape == (S, P, T, L)
    # the NULL-gcc launch is the same computation
    assert np.array_equal(lag, lag2_d.cpu().numpy()) and np.array_equal(h.view(np.uint32), h2_d.cpu().numpy().view(np.uint32))
    X, e = Xd.cpu().numpy().astype(np.complex128), ed.cpu().numpy().astype(np.float64)
    B = gcc_bound(L)
    worst_g = worst_h = 0.0
    left_out = mismatches = 0
    refs = []
    for s in range(S):
        rl, rh, rm, rgate, rzero, rg = cf.gcc_peaks(X[s], e[s], pairs, threshold, want_gcc=True)
        refs.append((rl, rh, rm, rgate, rzero))
        nopeak = rgate | rzero
        # no peak: reserved lag, height 0; gated rows are zeros, zero-bin rows NaN
        assert np.array_equal(lag[s] == cf.NO_PEAK, nopeak | (rl == cf.NO_PEAK))
        assert np.all(h[s][nopeak] == 0)
        assert np.all(g[s][rgate] == 0) and np.all(np.isnan(g[s][rzero]))
        ok = ~nopeak
        # selection, exact, on the correlation as the kernel wrote it
        a = np.abs(g[s][ok])
        n = np.argmax(a, axis=-1)
        assert np.array_equal(lag[s][ok], np.where(n < L // 2, n, n - L))
        assert np.array_equal(h[s][ok].view(np.uint32), np.take_along_axis(a, n[:, None], axis=-1)[:, 0].view(np.uint32))
        # correlation and height within B
        dg = np.max(np.abs(g[s][ok] - rg[ok]), axis=-1) if ok.any() else np.zeros(0)
        worst_g = max(worst_g, float(dg.max(initial=0.0)) / B)
        assert np.all(dg <= B), worst_g
        dh = np.abs(h[s][ok] - rh[ok])
        worst_h = max(worst_h, float(dh.max(initial=0.0)) / B)
        assert np.all(dh <= B), worst_h
        # lag where the choice is more than 2B from changing
        sure = ok & (rm > 2 * B)
        left_out += int(np.sum(ok & ~sure))
        mismatches += int(np.sum(lag[s][sure] != rl[sure]))
        if e64 is not None:
            # gate decisions from the float64 energy, outside the band around the threshold
            band = energy_bound(L) * e64[s]
            clear = np.abs(e64[s] - threshold) > band
            for p, (ca, cb) in enumerate(pairs):
                both = clear[ca] & clear[cb]
                g64 = (e64[s][ca] <= threshold) & (e64[s][cb] <= threshold)
                assert np.array_equal(rgate[p][both], g64[both])
    total = S * P * T
    print("%s: |g| error/bound %.3f, height error/bound %.3f, left out %d of %d, lag mismatches outside them %d, gated %d, zero-bin %d"
          % (label, worst_g, worst_h, left_out, total, mismatches, sum(int(r[3].sum()) for r in refs), sum(int(r[4].sum()) for r in refs)))
    assert mismatches == 0
    assert left_out <= 0.01 * total, (left_out, total)
    return lag, h, refs


@pytest.mark.parametrize("D,L", [(8192, 16384), (256, 512), (128, 256), (1000, 1024), (512, 2048)],
                         ids=["script", "short", "smallest", "odd-window", "long-padding"])
def test_kinect(dev, kinect_pcm, D, L):
    pcm = kinect_pcm[None]
    assert cf.n_frames(pcm.shape[-1], D) == {8192: 10, 256: 305, 128: 610, 1000: 79, 512: 153}[D]
    Xd, ed = check_spectra(dev, pcm, D, L)
    e64 = cf.spectra(pcm, D, L)[1]
    check_gcc(dev, Xd, ed, KINECT_PAIRS, 128.0, L, "kinect D=%d L=%d" % (D, L), e64=e64)


def test_full_window(dev):
    """D = L: no padding at all."""
    rng = np.random.default_rng(5)
    pcm = (rng.normal(size=(1, 2, 8 * 512)) * 1000).astype(np.float32)
    Xd, ed = check_spectra(dev, pcm, 512, 512)
    check_gcc(dev, Xd, ed, [(0, 1)], 64.0, 512, "full window")


@pytest.mark.parametrize("D,L", cf.LONG_CASES, ids=["D%d-L%d" % c for c in cf.LONG_CASES])
def test_long_transforms(dev, D, L):
    """L = 4096 and 8192, which the Kinect cases leave out: both stages against float64 on tdoa_closed_form.long_case_pcm (two
    streams, three channels, a delayed copy, a zero frame, a gated frame).  No frame may be left out of the lag comparison at 24
    work units; tests/test_tdoa_cpu.py shows that the closed form's own margins admit that."""
    pcm = cf.long_case_pcm(D, L)
    S, C, T = cf.LONG_S, cf.LONG_C, cf.LONG_T
    assert pcm.shape[:2] == (S, C) and cf.n_frames(pcm.shape[-1], D) == T and pcm.shape[-1] % D != 0
    Xd, ed = check_spectra(dev, pcm, D, L)
    e64 = cf.spectra(pcm, D, L)[1]
    lag, h, refs = check_gcc(dev, Xd, ed, cf.LONG_PAIRS, cf.LONG_THRESHOLD, L, "long D=%d L=%d" % (D, L), e64=e64)
    # the frames without a peak are the ones the signal was built to have, and no others
    gated = np.zeros((S, len(cf.LONG_PAIRS), T), bool)
    zero = np.zeros_like(gated)
    gated[cf.LONG_QUIET[0], cf.LONG_PAIRS.index((0, 1)), cf.LONG_QUIET[1]] = True
    for p, pair in enumerate(cf.LONG_PAIRS):
        zero[cf.LONG_ZERO[0], p, cf.LONG_ZERO[2]] = cf.LONG_ZERO[1] in pair
    assert np.array_equal(np.stack([r[3] for r in refs]), gated) and np.array_equal(np.stack([r[4] for r in refs]), zero)
    assert np.array_equal(lag == cf.NO_PEAK, gated | zero)
    # the delayed copy: channel 1 lags channel 0 wherever both are loud
    p01 = cf.LONG_PAIRS.index((0, 1))
    loud = ~(gated | zero)[:, p01]
    assert np.all(lag[:, p01][loud] == -cf.LONG_DELAY)
    # (2, 1) mirrors (1, 2)
    a, b = lag[:, cf.LONG_PAIRS.index((1, 2))], lag[:, cf.LONG_PAIRS.index((2, 1))]
    ok = a != cf.NO_PEAK
    assert np.array_equal(b[ok], np.where((a[ok] == 0) | (a[ok] == -L // 2), a[ok], -a[ok]))


def test_no_window_full_frame_l8192(dev):
    """window=False with D = L = 8192: the transform with nothing in front of it."""
    rng = np.random.default_rng(12)
    L = 8192
    pcm = (rng.normal(size=(2, 2, 2 * L + 777)) * 1000).astype(np.float32)
    check_spectra(dev, pcm, L, L, window=False)


def test_all_pairs_64_channels(dev):
    """2016 pairs of 64 channels: the grid decomposition over pairs, channels shared between pairs."""
    rng = np.random.default_rng(6)
    C, D, L, T = 64, 256, 512, 4
    n = T * D - 37                                   # ragged last frame
    common = rng.normal(size=n + C) * 2000
    pcm = np.stack([common[C - c: C - c + n] for c in range(C)]) + rng.normal(size=(C, n)) * 500   # channel c lags by c samples
    pcm = pcm.astype(np.float32)[None]
    pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]
    assert len(pairs) == 2016
    Xd, ed = check_spectra(dev, pcm, D, L)
    lag, h, refs = check_gcc(dev, Xd, ed, pairs, 64.0, L, "all pairs")
    # the common signal makes most pairs peak at minus their channel distance
    want = np.array([a - b for a, b in pairs])
    assert np.mean(lag[0][:, 1] == want) > 0.9


def test_two_streams_reversed_and_repeated_pairs(dev):
    import torch
    rng = np.random.default_rng(7)
    S, C, D, L, T = 2, 3, 256, 512, 16
    pcm = (rng.normal(size=(S, C, T * D)) * 1500).astype(np.float32)
    pcm[:, 1, 5:] += 2.0 * pcm[:, 0, :-5]              # a delayed copy of channel 0 in channel 1
    pairs = [(0, 1), (1, 0), (0, 1)]
    Xd, ed = check_spectra(dev, pcm, D, L)
    lag, h, refs = check_gcc(dev, Xd, ed, pairs, 64.0, L, "two streams")
    assert not np.array_equal(h[0], h[1])                # the streams hold different noise
    # a repeated pair repeats the bits; each stream alone gives the block's bits
    assert np.array_equal(lag[:, 0], lag[:, 2]) and np.array_equal(h[:, 0].view(np.uint32), h[:, 2].view(np.uint32))
    eng = _eng()
    for s in range(S):
        l1, h1 = eng.tdoa_estimate(torch.from_numpy(pcm[s:s + 1]).to(dev), D, L, pairs, 64.0)
        assert np.array_equal(l1.cpu().numpy()[0], lag[s]) and np.array_equal(h1.cpu().numpy()[0].view(np.uint32), h[s].view(np.uint32))
    # (b, a) mirrors (a, b): g_ba[n] = g_ab[-n], so lag -> -lag except at 0 and -L/2, wherever the choice is clear
    B = gcc_bound(L)
    for s in range(S):
        rm = refs[s][2]
        sure = (rm[0] > 2 * B) & (rm[1] > 2 * B)
        fwd, rev = lag[s][0][sure], lag[s][1][sure]
        assert sure.sum() > T // 2
        assert np.array_equal(rev, np.where((fwd == 0) | (fwd == -L // 2), fwd, -fwd))


def _upload_spectra(dev, X):
    """Supplied spectra: complex64 on the device with their energies, computed in float64 and rounded."""
    import torch
    X = np.ascontiguousarray(X.astype(np.complex64))
    e = cf.energy(X.astype(np.complex128)).astype(np.float32)
    return torch.from_numpy(X).to(dev), torch.from_numpy(e).to(dev)


@pytest.mark.parametrize("d", [1, 7, 100])
def test_delayed_copy(dev, d):
    """Channel 1 is channel 0 delayed by d samples inside the zero padding: lag = -d exactly, height close to 1."""
    rng = np.random.default_rng(100 + d)
    D, L, T = 2048, 4096, 3
    x = np.zeros((2, T, L))
    x[0, :, :D] = rng.normal(size=(T, D)) * 1000
    x[1, :, d:] = x[0, :, :L - d]
    Xd, ed = _upload_spectra(dev, np.fft.rfft(x, axis=-1)[None])
    lag, h = _eng().tdoa_gcc_peaks(Xd, ed, [(0, 1), (1, 0)], 64.0)
    lag, h = lag.cpu().numpy()[0], h.cpu().numpy()[0]
    print("delayed copy d=%d: lags %s heights %s (floor 1/sqrt(L) = %.4f)" % (d, lag.tolist(), np.round(h, 4).tolist(), L ** -0.5))
    assert np.all(lag[0] == -d) and np.all(lag[1] == d)
    assert np.all(h > 0.9)


def test_gate_is_an_and(dev):
    import torch
    rng = np.random.default_rng(8)
    L, T = 512, 4
    X = np.fft.rfft(rng.normal(size=(2, T, L)) * 100, axis=-1)
    thr = 64.0
    e = cf.energy(X)
    X[:, 0] = 0                                          # frame 0: all zero
    X[:, 1] *= np.sqrt(0.5 * thr / e[:, 1])[:, None]     # frame 1: both energies at half the threshold
    X[0, 2] *= np.sqrt(0.5 * thr / e[0, 2])              # frame 2: channel 0 below, channel 1 above
    Xd, ed = _upload_spectra(dev, X[None])
    en = ed.cpu().numpy()[0]
    assert np.all(en[:, 0] == 0) and np.all(en[:, 1] < thr) and en[0, 2] < thr < en[1, 2] and np.all(en[:, 3] > thr)
    lag, h, g = _eng().tdoa_gcc_peaks(Xd, ed, [(0, 1), (1, 0)], thr, want_gcc=True)
    lag, h, g = lag.cpu().numpy()[0], h.cpu().numpy()[0], g.cpu().numpy()[0]
    assert np.all(lag[:, :2] == cf.NO_PEAK) and np.all(h[:, :2] == 0) and np.all(g[:, :2] == 0)
    assert np.all(lag[:, 2:] != cf.NO_PEAK) and np.all(h[:, 2:] > 0)
    # with a threshold of zero only the all-zero frame is gated (0 <= 0)
    lag0, h0 = _eng().tdoa_gcc_peaks(Xd, ed, [(0, 1)], 0.0)
    assert lag0.cpu().numpy()[0, 0].tolist()[0] == cf.NO_PEAK and np.all(lag0.cpu().numpy()[0, 0, 1:] != cf.NO_PEAK)
    assert _eng().TDOA_NO_PEAK == cf.NO_PEAK


def test_zero_bin_is_no_peak(dev):
    rng = np.random.default_rng(9)
    L, T = 1024, 4
    X = np.fft.rfft(rng.normal(size=(3, T, L)) * 100, axis=-1)
    X[0, 1, 37] = 0                                      # one bin of one channel, frame 1
    X[2, 2, L // 2] = 0                                  # the Nyquist bin of channel 2, frame 2
    X[1, 3, 0] = 0                                       # bin 0 of channel 1, frame 3
    Xd, ed = _upload_spectra(dev, X[None])
    pairs = [(0, 1), (1, 2), (2, 0)]
    lag, h, g = _eng().tdoa_gcc_peaks(Xd, ed, pairs, 64.0, want_gcc=True)
    lag, h, g = lag.cpu().numpy()[0], h.cpu().numpy()[0], g.cpu().numpy()[0]
    want = np.zeros((3, T), bool)
    want[0, 1] = want[2, 1] = True                       # pairs with channel 0 in frame 1
    want[1, 2] = want[2, 2] = True                       # pairs with channel 2 in frame 2
    want[0, 3] = want[1, 3] = True                       # pairs with channel 1 in frame 3
    assert np.array_equal(lag == cf.NO_PEAK, want) and np.all(h[want] == 0) and np.all(h[~want] > 0)
    assert np.all(np.isnan(g[want])) and np.all(np.isfinite(g[~want]))
    rl = cf.gcc_peaks(Xd.cpu().numpy()[0].astype(np.complex128), ed.cpu().numpy()[0].astype(np.float64), pairs, 64.0)
    assert np.array_equal(rl[4], want) and np.array_equal(lag[~want], rl[0][~want])


def test_limits_return_dimension_error(dev):
    import torch
    from distant_speech_recognition_amd import _lib
    eng = _eng()
    pcm = torch.zeros((1, 2, 40000), dtype=torch.float32, device=dev)
    for D, L in [(64, 128), (8192, 32768), (500, 1000), (600, 512), (1, 256)]:
        with pytest.raises(_lib.BtkError) as ei:
            eng.tdoa_spectra(pcm, D, L)
        assert ei.value.code == _lib.BTK_ERR_DIMENSION, (D, L)
    for L in (128, 32768, 1000):
        X = torch.zeros((1, 2, 2, L // 2 + 1), dtype=torch.complex64, device=dev)
        e = torch.ones((1, 2, 2), dtype=torch.float32, device=dev)
        with pytest.raises(_lib.BtkError) as ei:
            eng.tdoa_gcc_peaks(X, e, [(0, 1)], 64.0)
        assert ei.value.code == _lib.BTK_ERR_DIMENSION, L
    X = torch.zeros((1, 2, 2, 257), dtype=torch.complex64, device=dev)
    e = torch.ones((1, 2, 2), dtype=torch.float32, device=dev)
    with pytest.raises(_lib.BtkError):
        eng.tdoa_gcc_peaks(X, e, [(0, 2)], 64.0)         # channel 2 of 2
    # a device pair list is not range-checked on the host: the kernel reports no peak for the bad pair and reads nothing
    bad = torch.tensor([[0, 1], [0, 7], [-1, 0]], dtype=torch.int32, device=dev)
    X = torch.ones((1, 2, 2, 257), dtype=torch.complex64, device=dev)
    lag, h = eng.tdoa_gcc_peaks(X, e, bad, 0.5)
    assert lag.cpu().numpy()[0, 0].tolist() == [0, 0] and np.all(lag.cpu().numpy()[0, 1:] == cf.NO_PEAK)
