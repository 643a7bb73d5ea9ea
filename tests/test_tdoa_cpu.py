"""CPU: the float64 closed form of the TDOA kernels (tests/tdoa_closed_form.py) against the reference's own results
(tests/golden/pytdoa_golden.npz, written by tests/golden/gen_golden_pytdoa.py from the reference's lib/pytdoa.py on the same
complex64-rounded spectra), and btk20.pytdoa's host arithmetic -- observation lists, mic_pair_tdoa() and the position
estimators -- fed the golden's own [delay, height]."""
import os

import numpy as np
import pytest

from tests import tdoa_closed_form as cf

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FS = 16000
SSPEED = 343740.0
KINECT_MPOS = np.array([[-113.0, 0.0, 2.0], [36.0, 0.0, 2.0], [76.0, 0.0, 2.0], [113.0, 0.0, 2.0]])
KINECT_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
KINECT_CONF = dict(energy_threshold=128, minimum_pairs=5, threshold=0.12)
CIRC_CONF = dict(energy_threshold=64, minimum_pairs=3, threshold=0.12)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "pytdoa_golden.npz"))


def cases(golden, kinect_pcm):
    """(name, array type, pcm, D, L, pairs, mpos, conf)"""
    pairs_c = [tuple(int(v) for v in p) for p in golden["circ_pairs"]]
    return [("kinect_D8192", "linear", kinect_pcm, 8192, 16384, KINECT_PAIRS, KINECT_MPOS, KINECT_CONF),
            ("kinect_D256", "linear", kinect_pcm, 256, 512, KINECT_PAIRS, KINECT_MPOS, KINECT_CONF),
            ("circ", "circular", golden["circ_pcm"].astype(np.float32), 256, 512, pairs_c, golden["circ_mpos"], CIRC_CONF)]


def rounded_spectra(pcm, D, L):
    """the closed-form spectra as the golden's sources served them: rounded to complex64 and widened back"""
    X = cf.spectra(pcm, D, L)[0].astype(np.complex64).astype(np.complex128)
    return X, cf.energy(X)


@pytest.mark.parametrize("which", [0, 1, 2], ids=["kinect-script", "kinect-short", "circular"])
def test_closed_form_matches_the_reference(golden, kinect_pcm, which):
    name, _, pcm, D, L, pairs, _, conf = cases(golden, kinect_pcm)[which]
    X, e = rounded_spectra(pcm, D, L)
    lag, height, margin, gated, zero = cf.gcc_peaks(X, e, pairs, conf["energy_threshold"])
    peaks = golden[name + "_peaks"]                                # [T][P][2]
    assert peaks.shape == (X.shape[1], len(pairs), 2)
    none = np.isnan(peaks[..., 0]).T
    assert np.array_equal(lag == cf.NO_PEAK, none) and np.array_equal(gated | zero, none)
    assert np.all(peaks[..., 1].T[none] == 0)
    want_lag = np.rint(peaks[..., 0].T[~none] * FS).astype(np.int64)
    assert np.array_equal(lag[~none], want_lag)
    assert np.array_equal(lag[~none] * (1.0 / FS), peaks[..., 0].T[~none])       # the delay is float(lag) * Ts, bit for bit
    assert np.max(np.abs(height - peaks[..., 1].T)) <= 1e-12
    if name == "circ":
        assert zero.sum() == 80 and not gated.any()                # the silent stretches of microphone 5: five pairs, 16 frames


def test_closed_form_gate_and_zero_bin():
    rng = np.random.default_rng(3)
    L, T = 256, 4
    X = np.fft.rfft(rng.normal(size=(2, T, L)) * 50, axis=-1)
    thr = 64.0
    e = cf.energy(X)
    X[:, 0] = 0
    X[:, 1] *= np.sqrt(0.5 * thr / e[:, 1])[:, None]
    X[0, 2] *= np.sqrt(0.5 * thr / e[0, 2])
    X[1, 3, 17] = 0
    lag, height, margin, gated, zero, g = cf.gcc_peaks(X, cf.energy(X), [(0, 1), (1, 0)], thr, want_gcc=True)
    assert gated.tolist() == [[True, True, False, False]] * 2 and zero.tolist() == [[False, False, False, True]] * 2
    assert np.all(lag[:, [0, 1, 3]] == cf.NO_PEAK) and np.all(height[:, [0, 1, 3]] == 0) and np.all(lag[:, 2] != cf.NO_PEAK)
    assert np.all(g[:, :2] == 0) and np.all(np.isnan(g[:, 3]))
    # (b, a) mirrors (a, b); Parseval: |P_k| = 1 makes ||g||_2 = 1
    assert lag[1, 2] == (-lag[0, 2] if lag[0, 2] not in (0, -L // 2) else lag[0, 2])
    assert abs(np.sum(g[0, 2] ** 2) - 1.0) < 1e-12
    # a delayed copy peaks at minus the delay with height 1; ties go to the first index
    x = np.zeros((2, L)); x[0, :100] = rng.normal(size=100); x[1, 9:109] = x[0, :100]
    Xd = np.fft.rfft(x, axis=-1)
    assert cf.peak(cf.gcc(Xd[0], Xd[1]))[0] == -9 and abs(cf.peak(cf.gcc(Xd[0], Xd[1]))[1] - 1.0) < 1e-12
    assert cf.peak(np.array([0.0, 0.5, -0.5, 0.2]))[:2] == (1, 0.5) and cf.peak(np.zeros(8))[0] == cf.NO_PEAK
    assert cf.peak(np.array([0.0, 0.1, -0.7, 0.2]))[0] == -2


@pytest.mark.parametrize("D,L", cf.LONG_CASES, ids=["D%d-L%d" % c for c in cf.LONG_CASES])
def test_long_case_signal_leaves_no_frame_out(D, L):
    """The signal of tests/test_gpu_tdoa.py's test_long_transforms, by the closed form alone: exactly the built-in frames are
    gated or zero, every other peak is more than 2 gcc_bound(L) ahead of the runner-up (so the GPU test, whose 1 % cap admits
    no left-out frame at 24 work units, can hold every lag to the closed form's), and the delayed copy is found."""
    from tests.test_gpu_tdoa import gcc_bound, energy_bound
    pcm = cf.long_case_pcm(D, L)
    S, C, T, pairs = cf.LONG_S, cf.LONG_C, cf.LONG_T, cf.LONG_PAIRS
    assert pcm.shape == (S, C, (T - 1) * D + D // 2 + 3) and pcm.dtype == np.float32 and cf.n_frames(pcm.shape[-1], D) == T
    assert 0.01 * S * len(pairs) * T < 1                     # the cap of check_gcc admits no left-out frame
    X, e = rounded_spectra(pcm, D, L)
    # every energy is clear of the threshold by far more than the kernel's energy bound
    assert np.all(np.abs(e - cf.LONG_THRESHOLD) > 100 * energy_bound(L) * e)
    smallest = np.inf
    for s in range(S):
        lag, height, margin, gated, zero = cf.gcc_peaks(X[s], e[s], pairs, cf.LONG_THRESHOLD)
        for p, pair in enumerate(pairs):
            for t in range(T):
                assert gated[p, t] == ((s, t) == cf.LONG_QUIET and pair == (0, 1)), (s, p, t)
                assert zero[p, t] == ((s, t) == (cf.LONG_ZERO[0], cf.LONG_ZERO[2]) and cf.LONG_ZERO[1] in pair), (s, p, t)
        ok = ~(gated | zero)
        smallest = min(smallest, float(margin[ok].min()))
        assert np.all(margin[ok] > 2 * gcc_bound(L)), (s, float(margin[ok].min()), 2 * gcc_bound(L))
        assert np.all(lag[0][ok[0]] == -cf.LONG_DELAY)
    print("long case D=%d L=%d: smallest margin %.3g against 2B = %.3g" % (D, L, smallest, 2 * gcc_bound(L)))


def test_closed_form_without_window():
    x = np.arange(1, 11, dtype=np.float32)
    f = cf.windowed_frames(x, 4, window=False)
    assert f.dtype == np.float32 and np.array_equal(f, [[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 0, 0]])
    X, e = cf.spectra(x, 4, 8, window=False)
    assert np.allclose(X, np.fft.rfft(f.astype(np.float64), n=8, axis=-1)) and X[0, 0] == 10


def test_closed_form_window_and_frames():
    x = np.arange(1, 11, dtype=np.float32)
    f = cf.windowed_frames(x, 4)
    assert f.shape == (3, 4) and f.dtype == np.float32 and cf.n_frames(10, 4) == 3
    w = cf.hamming(4)
    assert abs(w[0] - 0.08) < 1e-15 and abs(w[3] - 0.08) < 1e-15 and np.array_equal(f[2], (np.array([9, 10, 0, 0]) * w).astype(np.float32))
    X, e = cf.spectra(x, 4, 8)
    assert X.shape == (3, 5) and np.allclose(e, 2 * np.sum(np.abs(X) ** 2, axis=-1))


class GoldenPeaks:
    """stands where a TDOAFeature stands: serves the golden's [delay, height] of one pair"""

    def __init__(self, peaks):
        self.peaks = peaks

    def next(self, frame_no):
        if frame_no >= len(self.peaks):
            raise StopIteration
        d, h = self.peaks[frame_no]
        return [None if np.isnan(d) else float(d), float(h)]

    def reset(self):
        pass


@pytest.mark.parametrize("which", [0, 1, 2], ids=["kinect-script", "kinect-short", "circular"])
def test_pytdoa_host_arithmetic_matches_the_reference(golden, kinect_pcm, which):
    from btk20.pytdoa import (MicrophonePairSource, FarfieldLinearArrayTDOAFeatureVector, FarfieldCircularArrayTDOAFeatureVector,
                              MicrophonePairObservation)
    name, kind, _, D, L, pairs, mpos, conf = cases(golden, kinect_pcm)[which]
    peaks = golden[name + "_peaks"]
    T = peaks.shape[0]
    srcs = [MicrophonePairSource(p, a, b, GoldenPeaks(peaks[:, p])) for p, (a, b) in enumerate(pairs)]
    cls = FarfieldLinearArrayTDOAFeatureVector if kind == "linear" else FarfieldCircularArrayTDOAFeatureVector
    fe = cls(srcs, np.array(mpos), conf["minimum_pairs"], conf["threshold"], SSPEED)
    seen = 0
    for t, obs in enumerate(fe):
        seen += 1
        assert (obs is not None) == bool(golden[name + "_has_obs"][t])
        got = np.zeros(len(pairs), bool)
        for o in (obs or []):
            assert isinstance(o, MicrophonePairObservation) and (o.first_micx, o.second_micx) == pairs[o.pairx]
            assert o.observation == peaks[t, o.pairx, 0]
            got[o.pairx] = True
        if obs is not None:
            assert np.array_equal(got, golden[name + "_observed"][t])
        buf = fe.mic_pair_tdoa()
        assert sorted((a, b) for a in buf for b in buf[a]) == sorted(pairs)
        for p, (a, b) in enumerate(pairs):
            d = golden[name + "_tdoa"][t, p]
            assert (buf[a][b] is None) if np.isnan(d) else (buf[a][b] == d)
        pos = fe.instantaneous_position(t)
        want = golden[name + "_positions"][t]
        assert pos.shape == want.shape and np.max(np.abs(pos - want)) <= 1e-12, (t, pos, want)
    assert seen == T


def test_position_edge_cases():
    from btk20.pytdoa import MicrophonePairSource, FarfieldLinearArrayTDOAFeatureVector, FarfieldCircularArrayTDOAFeatureVector, TDOAFeatureVector
    # linear: too few pairs above the threshold -> [-1e10]; a delay beyond the baseline is clamped
    peaks = np.array([[[1e-3, 0.5]], [[1e-5, 0.05]]])
    fe = FarfieldLinearArrayTDOAFeatureVector([MicrophonePairSource(0, 0, 1, GoldenPeaks(peaks[:, 0]))], KINECT_MPOS[:2], 1, 0.12, SSPEED)
    assert fe.instantaneous_position(0)[0] == 0.0 and fe.instantaneous_position(1)[0] == -1e10
    assert fe.next(1) is None and fe.mic_pair_tdoa() == {0: {1: 1e-5}}
    # circular: a planar array (no pair out of the xy-plane) takes the two-component rules
    ang = 2 * np.pi * np.arange(4) / 4
    mpos = np.stack([50 * np.cos(ang), 50 * np.sin(ang), np.zeros(4)], axis=1)
    u = np.array([np.sin(1.0) * np.cos(0.5), np.sin(1.0) * np.sin(0.5), np.cos(1.0)])
    pairs = [(0, 1), (0, 2), (1, 3)]
    srcs = [MicrophonePairSource(p, a, b, GoldenPeaks(np.array([[np.dot(u, mpos[b] - mpos[a]) / SSPEED, 0.9]]))) for p, (a, b) in enumerate(pairs)]
    fe = FarfieldCircularArrayTDOAFeatureVector(srcs, mpos, 2, 0.12, SSPEED)
    pos = fe.instantaneous_position(0)
    assert abs(pos[0] - 1.0) < 1e-9 and abs(pos[1] - 0.5) < 1e-9              # exact delays of the direction (1.0, 0.5)
    with pytest.raises(ValueError):
        FarfieldCircularArrayTDOAFeatureVector(srcs, mpos[:2], 2, 0.12, SSPEED)
    # the base class has no position estimate
    assert TDOAFeatureVector(srcs, mpos).instantaneous_position(0) is None


def test_are_collinear_and_consistent_direction():
    from btk20.pytdoa import are_collinear_and_consistent_direction as ok
    assert ok(KINECT_MPOS)
    assert ok(np.array([[0.0, 0, 0], [1, 1, 1], [3, 3, 3], [2, 2, 2]]))
    assert not ok(np.array([[0.0, 0, 0], [1, 0, 0], [2, 0.5, 0]]))             # off the line
    assert not ok(np.array([[0.0, 0, 0], [1, 0, 0], [-2, 0, 0]]))              # behind the first point
    assert not ok(KINECT_MPOS[[1, 0, 2, 3]])                                   # the first sensor is not the tail
    with pytest.raises(ValueError):
        from btk20.pytdoa import FarfieldLinearArrayTDOAFeatureVector
        FarfieldLinearArrayTDOAFeatureVector([], KINECT_MPOS[[1, 0, 2, 3]])


def test_front_end_factory_without_gpu():
    from btk20.pytdoa import make_tdoa_front_end
    with pytest.raises(NotImplementedError):
        make_tdoa_front_end("planar", [(0, 1)], [GoldenPeaks(np.zeros((1, 2)))] * 2, 512, 16000, KINECT_MPOS, 64, 2, 0.12)


def test_library_refuses_bad_lengths_before_any_launch():
    """the limits are the library's: refused with BTK_ERR_DIMENSION before a pointer is looked at"""
    from distant_speech_recognition_amd import _lib
    L = _lib.lib()
    for D, n in [(64, 128), (8192, 32768), (500, 1000), (600, 512), (1, 256)]:
        assert L.btk_tdoa_spectra(None, 4096, 4096, 1, 1, D, n, 1, None, None, None) == _lib.BTK_ERR_DIMENSION, (D, n)
    for n in (128, 32768, 1000):
        assert L.btk_tdoa_gcc_peaks(None, None, None, 1, 64.0, 1, 2, 1, n, None, None, None, None) == _lib.BTK_ERR_DIMENSION
    assert L.btk_tdoa_frames(78064, 8192) == 10 and L.btk_tdoa_frames(1024, 256) == 4 and L.btk_tdoa_frames(0, 256) == 0
    assert _lib.BTK_TDOA_NO_PEAK == cf.NO_PEAK == -2147483648
