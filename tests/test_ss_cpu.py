"""CPU: the closed forms of tests/ss_closed_form.py (what the GPU tests hold the kernels against) against a frame-by-frame,
channel-by-channel, bin-by-bin restatement of the reference's loops (postfilter/spectralsubtraction.cc:52-129, :185-285,
:314-362; postfilter/postfilter.cc:1206-1239) written here in plain Python floats, plus hand-computed cases, the C-ABI's
declarations and limits, and the noise file format."""
import cmath
import ctypes
import math
import os
import re

import numpy as np
import pytest

from tests import ss_closed_form as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------- the reference's loops, restated
class _Estimator:
    """AveragePSDEstimator: a list of training frames that is averaged on demand (alpha < 0) or a recursive average."""

    def __init__(self, K, alpha=-1.0):
        self.alpha = float(np.float32(alpha))            # float alpha_
        self.est = [0.0] * K
        self.samples = []
        self.added = False

    def add_sample(self, frame):
        tmp = [v.real * v.real + v.imag * v.imag for v in frame[: len(self.est)]]
        if self.alpha < 0:
            self.samples.append(tmp)
        elif not self.added:                             # the first sample ever: copied
            self.est = tmp
            self.added = True
        else:
            self.est = [self.alpha * e + (1.0 - self.alpha) * t for e, t in zip(self.est, tmp)]

    def average(self):
        if self.alpha < 0:
            est = [0.0] * len(self.est)
            for s in self.samples:
                est = [e + v for e, v in zip(est, s)]
            n = np.float32(len(self.samples))            # 1.0/(float)sampleN: 1/0 = inf, 0 x inf = NaN
            with np.errstate(divide="ignore", invalid="ignore"):
                scale = float(np.float64(1.0) / np.float64(n))
                self.est = [float(np.float64(e) * scale) for e in est]

    def clear_samples(self):
        self.samples = []

    def clear(self):
        self.added = False
        self.samples = []


class _Subtractor:
    """SpectralSubtractor: next() pulls one frame per channel; add_sample comes before the subtraction of the same frame."""

    def __init__(self, M, ft=1.0, floor=0.001):
        self.M, self.K = M, M // 2 + 1
        self.ft, self.floor = float(np.float32(ft)), float(np.float32(floor))
        self.training, self.subtracting = True, False
        self.estimators = []

    def set_channel(self, alpha=-1.0):
        self.estimators.append(_Estimator(self.K, alpha))

    def stop_training(self):
        self.training = False
        for e in self.estimators:
            e.average()

    def next(self, frames):
        M, K = self.M, self.K
        out = [0j] * M
        for frame, e in zip(frames, self.estimators):
            if self.training:
                e.add_sample(frame)
            if not self.subtracting:
                for k in range(len(frame)):
                    out[k] += frame[k]
            else:
                for k in range(K):
                    x = frame[k]
                    s2 = (x.real * x.real + x.imag * x.imag) - self.ft * e.est[k]
                    if s2 <= self.floor:
                        s2 = self.floor
                    v = out[k] + cmath.rect(math.sqrt(s2), cmath.phase(x))
                    out[k] = v
                    if 0 < k < M // 2:
                        out[M - k] = v.conjugate()
        scale = 1.0 / len(frames)
        return [v * scale for v in out]


class _Wiener:
    def __init__(self, M, alpha=0.0, floor=0.001, beta=1.0):
        self.M, self.K = M, M // 2 + 1
        self.alpha, self.floor, self.beta = float(np.float32(alpha)), float(np.float32(floor)), float(np.float32(beta))
        self.ps, self.pn = [0.0] * self.K, [0.0] * self.K
        self.update = True
        self.frame_no = -1                               # FeatureStream's counter before the first frame

    def next(self, s, n):
        alpha = self.alpha if self.frame_no > 0 else 0.0
        out = [0j] * self.M
        out[0] = s[0]
        for k in range(1, self.K):
            ps = alpha * self.ps[k] + (1 - alpha) * (s[k].real ** 2 + s[k].imag ** 2)
            if self.update:
                cur = n[k].real ** 2 + n[k].imag ** 2
                if cur < self.floor:
                    cur = self.floor
                pn = alpha * self.pn[k] + (1 - alpha) * cur
            else:
                pn = self.pn[k]
            with np.errstate(invalid="ignore"):
                H = float(np.float64(ps) / np.float64(ps + self.beta * pn))
            out[k] = s[k] * H
            self.ps[k] = ps
            if self.update:
                self.pn[k] = pn
        self.frame_no += 1
        return out


def _mirror(x, M):
    """bins 0 .. M/2 -> the M-bin vector a reference node hands over"""
    K = M // 2 + 1
    v = [complex(c) for c in x] + [0j] * (M - K)
    for k in range(1, M // 2):
        v[M - k] = v[k].conjugate()
    return v


def _run_reference_ss(X, flags, ft, floor, alphas, M):
    """One subtractor per stream; the flags are applied as mode switches between two next() calls."""
    S, K, C, T = X.shape
    Y = np.zeros((S, K, T), np.complex128)
    nodes = []
    for s in range(S):
        node = _Subtractor(M, ft, floor)
        for a in alphas:
            node.set_channel(a)
        for t in range(T):
            node.training = bool(flags[t] & cf.TRAIN)    # start_training() / (stop_training() without the average)
            node.subtracting = bool(flags[t] & cf.SUBTRACT)
            out = node.next([_mirror(X[s, :, c, t], M) for c in range(C)])
            Y[s, :, t] = out[:K]
            if flags[t] & cf.SUBTRACT:
                for k in range(1, M // 2):
                    assert out[M - k] == out[k].conjugate()
        nodes.append(node)
    return Y, nodes


@pytest.mark.parametrize("i", [0, 1, 2, 3, 5, 6, 8])
def test_closed_form_is_the_references_loop(i):
    M, S, C, T, pad, alphas, sched, ft, floor = cf.CASES[i]
    alphas, ft, floor = tuple(cf.f32(a) for a in alphas), cf.f32(ft), cf.f32(floor)
    T = min(T, 70)                                       # (the pure-Python loop is slow; 70 frames pass every branch)
    flags = cf.schedule(sched, T, seed=T)
    X = cf.make_input(S, M // 2 + 1, C, T, seed=i)
    st = cf.ss_new_state(S, C, M)
    Y = cf.ss_closed_form(X, flags, ft, floor, alphas, st)
    Yr, nodes = _run_reference_ss(X, flags, ft, floor, alphas, M)
    assert np.max(np.abs(Y - Yr)) <= 1e-13 * max(1.0, np.max(np.abs(Yr)))
    for s, node in enumerate(nodes):
        for c, e in enumerate(node.estimators):
            if e.alpha >= 0:
                assert np.allclose(st["est"][s, c], e.est, rtol=1e-13, atol=0)
                assert bool(st["added"][s, c]) == e.added
            else:
                assert st["count"][s, c] == len(e.samples) and not st["added"][s, c]
                assert np.allclose(st["acc"][s, c], np.sum(e.samples, axis=0) if e.samples else 0.0, rtol=1e-13, atol=0)
    # average(): the 1.0/(float)N scale, and 0 x inf for a channel that never trained
    cf.ss_finish_training(alphas, st)
    for s, node in enumerate(nodes):
        node.stop_training()
        for c, e in enumerate(node.estimators):
            assert np.allclose(st["est"][s, c], e.est, rtol=1e-13, atol=0, equal_nan=True)
            if e.alpha < 0 and not e.samples:
                assert np.isnan(e.est).all() and np.isnan(st["est"][s, c]).all()


def test_update_comes_before_the_subtraction_and_first_sample_is_copied():
    M, K = 8, 5
    X = np.zeros((1, K, 1, 3), np.complex64)
    X[0, :, 0, 0] = 2.0                                  # p = 4
    X[0, :, 0, 1] = 1.0j                                 # p = 1
    X[0, :, 0, 2] = 3.0                                  # p = 9, not trained
    flags = np.array([cf.TRAIN | cf.SUBTRACT, cf.TRAIN | cf.SUBTRACT, cf.SUBTRACT], np.uint8)
    st = cf.ss_new_state(1, 1, M)
    st["est"][:] = 100.0                                 # whatever was there: the first sample replaces it
    Y = cf.ss_closed_form(X, flags, 0.5, 0.25, (0.5,), st)
    # frame 0: est = 4 (copied), S2 = 4 - 2 = 2;  frame 1: est = .5 4 + .5 1 = 2.5, S2 = 1 - 1.25 -> floor, phase kept;
    # frame 2: est stays 2.5, S2 = 9 - 1.25 = 7.75
    assert np.allclose(Y[0, :, 0], math.sqrt(2.0)) and np.allclose(Y[0, :, 1], 0.5j) and np.allclose(Y[0, :, 2], math.sqrt(7.75))
    assert np.all(st["est"] == 2.5) and st["added"][0, 0] == 1 and st["frames_done"] == 3


def test_hand_computed_subtraction_cases():
    M, K, C = 8, 5, 3
    floor = 0.25
    # X = 0 on every channel: each term is (sqrt(floor), 0), i.e. sqrt(floor)/C per channel
    X = np.zeros((1, K, C, 1), np.complex64)
    st = cf.ss_new_state(1, C, M)
    st["est"][:] = 7.0
    sub = np.array([cf.SUBTRACT], np.uint8)
    assert np.array_equal(cf.ss_closed_form(X, sub, 1.0, floor, (-1.0,) * C, st), np.full((1, K, 1), 0.5 + 0j))
    # two silent channels and one loud one below its noise estimate: 2 sqrt(floor)/C + sqrt(floor) e^{j arg X}/C
    X[0, :, 2, 0] = -2.0j
    Y = cf.ss_closed_form(X, sub, 1.0, floor, (-1.0,) * C, st)
    assert np.allclose(Y, (0.5 + 0.5 - 0.5j) / 3)
    # a frame exactly AT the floor (p - ft est == floor: `<=` floors it, to the same value) and one just above
    X1 = np.ones((1, K, 1, 2), np.complex64)
    X1[..., 1] = 1.5                                     # p = 2.25
    st1 = cf.ss_new_state(1, 1, M)
    st1["est"][:] = 0.75                                 # S2 = 0.25 and 1.5
    Y = cf.ss_closed_form(X1, np.array([cf.SUBTRACT] * 2, np.uint8), 1.0, floor, (-1.0,), st1)
    assert np.array_equal(Y[0, :, 0], np.full(K, 0.5 + 0j)) and np.allclose(Y[0, :, 1], math.sqrt(1.5))
    # no subtraction: the mean of the channels, whatever the model
    rng = np.random.default_rng(0)
    X2 = (rng.normal(size=(2, K, C, 4)) + 1j * rng.normal(size=(2, K, C, 4))).astype(np.complex64)
    Y = cf.ss_closed_form(X2, np.zeros(4, np.uint8), 1.0, floor, (0.5,) * C, cf.ss_new_state(2, C, M))
    assert np.allclose(Y, X2.astype(np.complex128).mean(axis=2), rtol=1e-15, atol=1e-15)


def test_clear_and_clear_noise_samples():
    st = cf.ss_new_state(2, 2, 8)
    X = cf.make_input(2, 5, 2, 6, seed=1)
    cf.ss_closed_form(X, np.full(6, cf.TRAIN, np.uint8), 1.0, 0.01, (-1.0, 0.5), st)
    est = st["est"].copy()
    assert st["count"][0, 0] == 6 and st["count"][0, 1] == 0 and st["added"][0, 1] == 1 and st["added"][0, 0] == 0
    cf.ss_clear(st, False)
    assert not st["acc"].any() and not st["count"].any() and st["added"][0, 1] == 1 and np.array_equal(st["est"], est)
    cf.ss_clear(st, True)
    assert not st["added"].any() and np.array_equal(st["est"], est)


@pytest.mark.parametrize("alpha,sched", [(0.0, "on"), (0.75, "stop_mid"), (0.9375, "never"), (0.5, "alternate")])
def test_wiener_closed_form_is_the_references_loop(alpha, sched):
    M, S, T = 8, 2, 40
    K = M // 2 + 1
    Sx = cf.make_input(S, K, 1, T, seed=3)[:, :, 0]
    Nx = (0.3 * cf.make_input(S, K, 1, T, seed=4, zeros=False)[:, :, 0]).astype(np.complex64)
    Nx[0, 1, 2] = 0
    flags = np.zeros(T, np.uint8)
    if sched == "on":
        flags[:] = 1
    elif sched == "stop_mid":
        flags[:T // 2] = 1
    elif sched == "alternate":
        flags[::3] = 1
    floor, beta = cf.f32(1e-3), 1.5
    st = cf.wiener_new_state(S, M)
    Y = cf.wiener_closed_form(Sx, Nx, flags, cf.f32(alpha), floor, beta, st)
    for s in range(S):
        node = _Wiener(M, alpha, floor, beta)
        for t in range(T):
            node.update = bool(flags[t] & 1)             # start/stop_updating_noise_PSD() between two next() calls
            out = node.next(_mirror(Sx[s, :, t], M), _mirror(Nx[s, :, t], M))
            assert np.allclose(Y[s, :, t], out[:K], rtol=1e-13, atol=0, equal_nan=True)
        assert np.allclose(st["psd_s"][s, 1:], node.ps[1:], rtol=1e-13, atol=0)
        assert np.allclose(st["psd_n"][s, 1:], node.pn[1:], rtol=1e-13, atol=0)
        assert st["psd_s"][s, 0] == 0 and st["psd_n"][s, 0] == 0 and node.ps[0] == 0          # bin 0: no state
    assert np.array_equal(Y[:, 0], Sx[:, 0])                                                  # bin 0 of the target, untouched
    if sched == "never":                                  # update stopped before any frame: PSDn = 0, H = 1
        assert not st["psd_n"].any() and np.allclose(Y, Sx)


def test_wiener_first_two_frames_have_no_memory():
    M, K = 8, 5
    Sx = np.ones((1, K, 4), np.complex64) * np.array([1, 2, 3, 4])
    Nx = np.ones((1, K, 4), np.complex64)
    st = cf.wiener_new_state(1, M)
    cf.wiener_closed_form(Sx[..., :2], Nx[..., :2], np.ones(2, np.uint8), 0.5, 1e-3, 1.0, st)
    assert np.all(st["psd_s"][0, 1:] == 4.0)              # frame 1 alone: alpha was 0 for both
    cf.wiener_closed_form(Sx[..., 2:], Nx[..., 2:], np.ones(2, np.uint8), 0.5, 1e-3, 1.0, st)
    assert np.all(st["psd_s"][0, 1:] == 0.5 * (0.5 * 4 + 0.5 * 9) + 0.5 * 16) and st["frames_done"] == 4


def test_highpass_cutoffs():
    M, K = 8, 5
    X = cf.make_input(2, K, 1, 3, seed=9, zeros=False)[:, :, 0]
    assert np.array_equal(cf.highpass_closed_form(X, 0), X)                                   # documented: copies all K bins
    Y = cf.highpass_closed_form(X, 1)
    assert not Y[:, 0].any() and np.array_equal(Y[:, 1:], X[:, 1:])                           # the reference never writes bin 0
    Y = cf.highpass_closed_form(X, M // 2)
    assert not Y[:, :M // 2].any() and np.array_equal(Y[:, M // 2], X[:, M // 2])
    # the restated loop (cutoff >= 1): zero 1 .. cutoff-1, copy cutoff .. M/2, bin 0 never written (it stays 0)
    for cutoff in (1, 2, 4):
        out = [0j] * M
        for k in range(cutoff, M // 2 + 1):
            out[k] = complex(X[0, k, 0])
        assert np.array_equal(cf.highpass_closed_form(X, cutoff)[0, :, 0], np.array(out[:K]))
    # cutoff_fbinX_ = (unsigned)(fftLen * cutOffFreq / (float)sampleRate), float32 arithmetic
    assert cf.highpass_cutoff_bin(512, 150, 16000) == 4 and cf.highpass_cutoff_bin(256, 100, 44100) == 0
    assert cf.highpass_cutoff_bin(512, 8000, 16000) == 256


def test_noise_file_round_trip_and_its_six_decimals(tmp_path):
    from distant_speech_recognition_amd import engine as eng
    psd = np.array([0.0, 1.0, 0.1234564, 0.1234566, 123456.789, 3e-7, 7e-7, 1.0 / 3.0])
    fn = str(tmp_path / "noise.txt")
    assert eng.write_noise_psd_file(fn, psd)
    lines = open(fn).read().split("\n")
    assert lines[-1] == "" and lines[:-1] == ["0.000000", "1.000000", "0.123456", "0.123457", "123456.789000", "0.000000", "0.000001",
                                              "0.333333"]
    back = eng.read_noise_psd_file(fn, len(psd))
    assert back.dtype == np.float64 and np.max(np.abs(back - psd)) <= 5e-7 and back[5] == 0.0
    # reading is idempotent from there on: what the format holds survives another trip bit for bit
    assert eng.write_noise_psd_file(fn, back) and np.array_equal(eng.read_noise_psd_file(fn, len(psd)), back)
    assert eng.read_noise_psd_file(str(tmp_path / "missing.txt"), 4) is None
    assert not eng.write_noise_psd_file(str(tmp_path / "no" / "such" / "dir.txt"), psd)
    short = eng.read_noise_psd_file(fn, len(psd) + 2)              # fewer lines than bins: only the bins the file names
    assert short.shape == (len(psd),) and np.array_equal(short, back)


def test_abi_declares_and_exports_the_entry_points():
    from distant_speech_recognition_amd import _lib
    names = {"btk_ss_max_channels", "btk_ss_process", "btk_ss_finish_training", "btk_ss_clear", "btk_wiener_process",
             "btk_spec_highpass"}
    txt = open(os.path.join(ROOT, "include", "btkhip.h")).read()
    declared = set(re.findall(r"\b(btk_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", txt, flags=re.S)))
    assert names <= declared and names <= set(_lib.SIGNATURES)
    L = _lib.lib()
    assert L.btk_ss_max_channels() == 64
    assert (_lib.BTK_SS_TRAIN, _lib.BTK_SS_SUBTRACT, _lib.BTK_WIENER_UPDATE_NOISE) == (cf.TRAIN, cf.SUBTRACT, cf.UPDATE_NOISE)
    for macro, val in (("BTK_SS_TRAIN", 1), ("BTK_SS_SUBTRACT", 2), ("BTK_WIENER_UPDATE_NOISE", 1), ("BTK_SS_FORM_ROWS", 1)):
        assert re.search(r"#define %s %d\b" % (macro, val), txt)
    # the limits are refused on the host, before anything is launched: no device needed
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.btk_ss_process(p, p, 1, 4096, 1, 4, 4, None, 2, 1.0, 0.001, p, 0, p, p, p, p, 0, None) == _lib.BTK_ERR_DIMENSION
    assert L.btk_ss_process(p, p, 1, 8, 65, 4, 4, None, 2, 1.0, 0.001, p, 0, p, p, p, p, 0, None) == _lib.BTK_ERR_DIMENSION
    assert b"64" in L.btk_last_error()
    assert L.btk_wiener_process(p, p, p, 1, 10, 3, 4, None, 1, 0.5, 0.001, 1.0, 0, p, p, None) == _lib.BTK_ERR_DIMENSION
    assert L.btk_spec_highpass(p, p, 1, 8, 6, 4, 4, None) == _lib.BTK_ERR_DIMENSION
    assert L.btk_spec_highpass(p, None, 1, 8, 1, 4, 4, None) == _lib.BTK_ERR_PARAMETER
