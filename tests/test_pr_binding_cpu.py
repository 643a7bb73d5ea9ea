"""CPU: the PR bank nodes, the windowed FFT bank node, DelayFeature and get_window under the reference's import names
(btk20.modulated, modulated/modulated.i): they import, accept the .i file's keywords and the legacy spellings, refuse what the
reference refuses, and DelayFeature -- a host node -- computes the reference's arithmetic.  Construction touches no device (plans
are made with the first launch), so the nodes are built over Python sources, as tests/test_ss_binding_cpu.py builds its own."""
import numpy as np
import pytest

import pr_closed_form as pcf

NAMES = ("PerfectReconstructionFFTAnalysisBank", "PerfectReconstructionFFTSynthesisBank", "NormalFFTAnalysisBank", "DelayFeature")


class _Src:
    def __init__(self, rows):
        self.rows, self.t = np.asarray(rows), 0

    def size(self):
        return self.rows.shape[1]

    def __iter__(self):
        self.t = 0
        return self

    def next(self, frame_no=-5):
        if self.t >= len(self.rows):
            raise StopIteration
        self.t += 1
        return self.rows[self.t - 1]

    __next__ = next

    def reset(self):
        self.t = 0


def _f(D, T=0):
    return _Src(np.zeros((T, D), np.float32))


def test_names_import_from_btk20_modulated():
    import btk20.modulated as mod
    import distant_speech_recognition_amd.btk20.modulated as mod2
    import distant_speech_recognition_amd.btk20cpp as cpp
    ns = {}
    exec("from btk20.modulated import *", ns)
    for name in NAMES:
        for n in (name, name + "Ptr"):
            assert n in ns and n in mod.__all__ and hasattr(cpp, n) and n in cpp.__all__, n
        assert ns[name] is ns[name + "Ptr"]
    assert "get_window" in ns and mod is mod2
    assert "OverSampledDFTAnalysisBankPtr" in ns                                   # what was there stays
    from distant_speech_recognition_amd.btk20cpp import _signatures as S
    assert {n + "Ptr" for n in NAMES} <= set(S.CTORS)


def test_constructors_accept_the_interface_keywords_and_legacy_spellings():
    from btk20.modulated import (PerfectReconstructionFFTAnalysisBankPtr, PerfectReconstructionFFTSynthesisBankPtr,
                                 NormalFFTAnalysisBankPtr, DelayFeaturePtr)
    from btk20.stream import PyVectorComplexFeatureStreamPtr
    M, m, r = 16, 2, 1
    h = pcf.random_prototype(M, m)
    a = PerfectReconstructionFFTAnalysisBankPtr(samp=_f(8), prototype=h, M=M, m=m, r=r, nm="ana")
    assert a.size() == 2 * M and a.name() == "ana"
    assert PerfectReconstructionFFTAnalysisBankPtr(_f(8), h, M, m, r).size() == 2 * M
    assert a.polyphase(m=3, n=1) == h[3 + 2 * M] and a.polyphase(5, 0) == h[5]
    assert (a.fftLen(), a.nBlocks(), a.subSampRate()) == (2 * M, 4, 2)              # the reference's constants (modulated.h:372-376)
    s = PerfectReconstructionFFTSynthesisBankPtr(samp=a, prototype=h, M=M, m=m, r=r, nm="syn")
    assert s.size() == M >> r and s.polyphase(m=3, n=1) == h[3 + 2 * M]
    # a Python-wrapped C++ node as the source, as the reference's tool passes it
    assert PerfectReconstructionFFTSynthesisBankPtr(PyVectorComplexFeatureStreamPtr(a), h, M, m, r).size() == M >> r
    bare = PerfectReconstructionFFTSynthesisBankPtr(prototype=h, M=M, m=m, r=r)     # the source-less constructor
    from distant_speech_recognition_amd.btk20cpp import j_error
    with pytest.raises(j_error, match="no source"):
        bare.next()
    n = NormalFFTAnalysisBankPtr(samp=_f(4), fftLen=8, r=1, window_type=2)
    assert (n.size(), n.fftlen(), n.fftLen()) == (8, 8, 8)
    assert NormalFFTAnalysisBankPtr(_f(4), 8).size() == 8                           # r = 1, Hamming by default
    assert NormalFFTAnalysisBankPtr(_f(8), fftLen=8, r=0, windowType=0).size() == 8  # the class's own spelling
    d = DelayFeaturePtr(samp=a, time_delay=0.5, nm="delay")
    assert d.size() == 2 * M
    with pytest.raises(TypeError):
        NormalFFTAnalysisBankPtr(_f(4), 8, no_such_keyword=1)


def test_refusals():
    from btk20.modulated import (PerfectReconstructionFFTAnalysisBankPtr, PerfectReconstructionFFTSynthesisBankPtr,
                                 NormalFFTAnalysisBankPtr)
    from distant_speech_recognition_amd.btk20cpp import jconsistency_error, jdimension_error, jparameter_error
    h = pcf.random_prototype(16, 2)
    with pytest.raises(jconsistency_error, match=r"Prototype sizes do not match \(63 vs. 64\)\."):
        PerfectReconstructionFFTAnalysisBankPtr(_f(16), h[:-1], 16, 2, 0)
    with pytest.raises(jconsistency_error, match=r"Prototype sizes do not match \(64 vs. 96\)\."):
        PerfectReconstructionFFTSynthesisBankPtr(h, 16, 3, 0)
    with pytest.raises(jdimension_error, match="Input block length"):
        PerfectReconstructionFFTAnalysisBankPtr(_f(16), h, 16, 2, 1)                # D = 8
    with pytest.raises(jdimension_error, match="Input block length"):
        NormalFFTAnalysisBankPtr(_f(8), 8, 1)                                       # D = 4
    with pytest.raises(jparameter_error):
        PerfectReconstructionFFTAnalysisBankPtr(_f(12), np.zeros(48), 12, 2, 0)     # no power of two
    with pytest.raises(jparameter_error):
        PerfectReconstructionFFTAnalysisBankPtr(_f(2), h, 16, 2, 3)                 # r beyond the engine's range


def test_get_window_matches_the_closed_form():
    from btk20.modulated import get_window
    for wt in (0, 1, 2, 5):
        for n in (8, 33):
            w = get_window(wt, n)
            assert w.dtype == np.float64 and w.shape == (n,)
            assert np.max(np.abs(w - pcf.get_window_cf(wt, n))) <= 2.0 ** -52         # one float64 ulp of 1: libm's cosine against numpy's
    assert np.array_equal(get_window(winType=0, winLen=4), np.ones(4))


def test_delay_feature_is_one_phase_for_all_bins():
    from btk20.modulated import DelayFeaturePtr
    rng = np.random.default_rng(3)
    x = rng.normal(size=(5, 6)) + 1j * rng.normal(size=(5, 6))
    tau = 0.3
    d = DelayFeaturePtr(_Src(x), tau)

    def want(t, row):
        a = np.exp(1j * float(np.float32(t)))                # time_delay is a float; polar(1, .) and the product are complex128
        return np.array([complex(a.real * v.real - a.imag * v.imag, a.real * v.imag + a.imag * v.real) for v in row])

    y0 = np.array(d.next())
    assert y0.dtype == np.complex128 and np.array_equal(y0, want(tau, x[0]))
    assert np.array_equal(np.array(d.next(0)), y0)           # the same frame again: served from the cache, the source is not pulled
    assert np.array_equal(np.array(d.next(1)), want(tau, x[1]))
    d.set_time_delay(time_delay=-1.25)                       # mid-stream
    assert np.array_equal(np.array(d.next()), want(-1.25, x[2]))
    d.reset()
    assert d.frame_no() == -1
    got = np.stack([np.array(v) for v in d])
    assert got.shape == x.shape and np.array_equal(got[4], want(-1.25, x[4]))
    with pytest.raises(StopIteration):
        d.next()
