"""GPU: the echo-canceller nodes (host/include/aec/aec.h, btk20.aec) and tools/subband_aec.py against the float64 closed form of
tests/aec_closed_form.py, within the tolerances of tests/test_gpu_aec.py after the nodes' complex128 widening."""
import json
import os
import wave

import numpy as np
import pytest

from tests import aec_closed_form as cf
from tests import closed_forms as fbcf

pytestmark = pytest.mark.gpu

TOL_E, TOL_R, TOL_K, TOL_S = 1e-4, 1e-4, 1e-3, 1e-5
FS = 16000


class _Src:
    """a Python source node: frames [T][M] complex128 (bins 0..M/2 given, the rest mirrored), as an analysis bank delivers them"""

    def __init__(self, Xh, M):
        self.F = fbcf.hermitian(np.asarray(Xh, np.complex128), M)
        self.M, self.t = M, 0

    def size(self):
        return self.M

    def __iter__(self):
        self.t = 0
        return self

    def next(self, frame_no=-5):
        if self.t >= len(self.F):
            raise StopIteration
        self.t += 1
        return self.F[self.t - 1]

    __next__ = next

    def reset(self):
        self.t = 0


def _case(name):
    return [c for c in cf.CASES if c[0] == name][0]


def _node(case, V, A, block_frames=50):
    import distant_speech_recognition_amd.btk20.aec as aec
    name, kind, S, M, P, T, ts, fn0, kw = case
    v, a = _Src(V, M), _Src(A, M)
    if kind == 0:
        n = aec.NLMSAcousticEchoCancellationFeaturePtr(v, a, **kw)
    elif kind == 1:
        n = aec.KalmanFilterEchoCancellationFeaturePtr(v, a, **kw)
    elif kind == 2:
        n = aec.BlockKalmanFilterEchoCancellationFeaturePtr(v, a, sample_num=P, **kw)
    else:
        n = aec.DTDBlockKalmanFilterEchoCancellationFeaturePtr(v, a, sample_num=P, **kw)
    n.set_block_frames(block_frames)
    return n


def _check_state(node, sr, kind, K):
    for k in (0, 1, K // 2, K - 1):
        R = node.filter_coefficients(k)
        assert np.max(np.abs(R - sr["R"][k])) <= TOL_R * np.max(np.abs(sr["R"])), k
        if kind:
            Km = node.state_covariance(k)
            assert np.max(np.abs(Km - sr["K"][k])) <= TOL_K * np.max(np.abs(sr["K"])), k
            assert abs(node.observation_noise_variance(k) - sr["sig"][k]) <= TOL_S * sr["sig"][k], k


@pytest.mark.parametrize("name", ["nlms", "kalman", "bk_p5", "dtd_p5", "dtd_p5_neg"])
def test_nodes_pulled_with_next_match_closed_form(dev, name):
    """each reference class over two sources that are drained through next(), in blocks of 50 frames: explicit frame numbers
    (or, for the last case, next()'s default -5 on every frame), mirror bins conjugate, state within the tolerances"""
    case = _case(name)
    _, kind, S, M, P, T, ts, fn0, kw = case
    V, A = cf.case_inputs(case)
    Er, flr, mg, sr = cf.case_reference(case)[0]
    node = _node(case, V[0], A[0])
    K = M // 2 + 1
    out = np.zeros((T, M), np.complex128)
    for t in range(T):
        f = node.next(t) if fn0 is None else node.next()
        assert f.dtype == np.complex128 and f.shape == (M,)
        if t == 3:
            assert node.next(node.frame_no()) is not None and node.frame_no() == 3      # same-frame caching: nothing is pulled
        out[t] = f
    with pytest.raises(StopIteration):
        node.next(T) if fn0 is None else node.next()
    assert node.is_end()
    err = np.max(np.abs(out[:, :K].T - Er)) / np.max(np.abs(Er))
    print("aec node %s: E error %.2g of max|E|" % (name, err))
    assert err <= TOL_E
    assert np.array_equal(out[:, K:], np.conj(out[:, M // 2 - 1:0:-1]))
    _check_state(node, sr, kind, K)


def test_iter_twice_continues_or_restarts(dev):
    """__iter__ = reset(): a block Kalman node goes on from its adapted weights, covariances and played history (aec.h:111-114);
    an NLMS node restarts from a zero filter (aec.h:41)"""
    case = _case("bk_p5")
    _, kind, S, M, P, T, ts, fn0, kw = case
    K = M // 2 + 1
    V, A = cf.case_inputs(case)
    node = _node(case, V[0], A[0], block_frames=64)
    first = np.array([np.array(f) for f in node])
    second = np.array([np.array(f) for f in node])
    st = cf.new_state(kind, K, P, **kw)
    E1, _, _ = cf.run(kind, V[0], A[0], st)
    E2, _, _ = cf.run(kind, V[0], A[0], st)                      # the same state: nothing but the sources was reset
    sc = np.max(np.abs(E1))
    assert first.shape == second.shape == (T, M)
    assert np.max(np.abs(first[:, :K].T - E1)) <= TOL_E * sc and np.max(np.abs(second[:, :K].T - E2)) <= TOL_E * sc
    assert np.max(np.abs(E2[:, :20] - E1[:, :20])) > 0.05 * sc   # (the second pass starts converged: it IS another signal)
    case0 = _case("nlms")
    V0, A0 = cf.case_inputs(case0)
    n0 = _node(case0, V0[0], A0[0], block_frames=64)
    a = np.array([np.array(f) for f in n0])
    assert np.max(np.abs(n0.filter_coefficients(3))) > 0
    b = np.array([np.array(f) for f in n0])
    assert a.shape == (case0[5], case0[3]) and np.array_equal(a, b)


def test_frame_number_and_length_contract(dev):
    import distant_speech_recognition_amd.btk20 as b20
    case = _case("bk_p2")
    _, kind, S, M, P, T, ts, fn0, kw = case
    V, A = cf.case_inputs(case)
    node = _node(case, V[0], A[0])
    node.next(0)
    with pytest.raises(b20.jindex_error):
        node.next(2)                                             # aec.cc:248-250
    assert node.frame_no() == 0
    node.next(1)
    # unequal source lengths end at the shorter one
    short = _node(case, V[0][:, :70], A[0][:, :40], block_frames=32)
    frames = [np.array(f) for f in short]
    assert len(frames) == 40
    st = cf.new_state(kind, M // 2 + 1, P, **kw)
    E, _, _ = cf.run(kind, V[0][:, :40], A[0][:, :40], st)
    assert np.max(np.abs(np.array(frames)[:, :M // 2 + 1].T - E)) <= TOL_E * np.max(np.abs(E))
    # a double-talk node computes a block for ONE way of calling next(): mixing them inside a block is refused, not guessed
    dcase = _case("dtd_p5")
    Vd, Ad = cf.case_inputs(dcase)
    dn = _node(dcase, Vd[0], Ad[0])
    dn.next(0)
    with pytest.raises(b20.jconsistency_error):
        dn.next()
    # limits are errors at construction
    with pytest.raises(b20.jdimension_error):
        _node(("x", 2, 1, M, 65, T, T, None, {}), V[0], A[0])


def _write_wav(path, x):
    w = wave.open(str(path), "wb")
    w.setnchannels(1); w.setsampwidth(2); w.setframerate(FS)
    w.writeframes(np.asarray(x, np.int16).tobytes())
    w.close()


def _echo_pcm(seed, L, delays=(0, 37, 150, 300), gains=(0.5, 0.3, -0.2, 0.1), near_from=None, near=300.0):
    """played: white noise at 3000; recorded: a sparse echo of it (up to 300 samples late) + weak noise, + near-end noise from near_from on"""
    rng = np.random.default_rng(seed)
    played = np.round(rng.normal(size=L) * 3000.0).clip(-32000, 32000)
    rec = np.zeros(L)
    for d, g in zip(delays, gains):
        rec[d:] += g * played[:L - d]
    rec += rng.normal(size=L) * 3.0
    if near_from is not None:
        rec[near_from:] += rng.normal(size=L - near_from) * near
    return played.astype(np.int16), np.round(rec).clip(-32000, 32000).astype(np.int16)


def _chain(h, g, M, m, r, played, rec, kind, P, frame_no0, Xv=None, Xa=None, **kw):
    """float64 chain: analysis closed form of both signals -> AEC closed form -> synthesis closed form"""
    K = M // 2 + 1
    Xv = fbcf.analysis_cf(h, M, m, r, 2, played.astype(np.float64))[:, :K].T if Xv is None else Xv
    Xa = fbcf.analysis_cf(h, M, m, r, 2, rec.astype(np.float64))[:, :K].T if Xa is None else Xa
    st = cf.new_state(kind, K, P, **kw)
    E, fl, mg = cf.run(kind, Xv, Xa, st, frame_no0=frame_no0)
    return fbcf.synthesis_cf(g, M, m, r, 2, fbcf.hermitian(E, M)), E, fl, mg, Xa


def test_banks_node_synthesis_m64(dev, tmp_path):
    """two analysis banks at M = 64 -> each node class -> pulled by a synthesis bank, which takes the node's device block and, like
    a reference consumer calling next() without an argument, makes the double-talk detector see frame number -5 throughout; then
    fresh graphs of the same kind pulled from the node with next(): E against the closed form, mirror bins conjugate"""
    from tests.util import design_prototype
    from distant_speech_recognition_amd.btk20 import SampleFeaturePtr, OverSampledDFTAnalysisBankPtr, OverSampledDFTSynthesisBankPtr
    import distant_speech_recognition_amd.btk20.aec as aec
    M, m, r, D = 64, 4, 1, 32
    h, g = design_prototype(M, m), design_prototype(M, m, "g")
    played, rec = _echo_pcm(5, 150 * D, delays=(0, 9, 40, 70))
    _write_wav(tmp_path / "p.wav", played); _write_wav(tmp_path / "r.wav", rec)
    makers = [
        (0, 1, dict(), lambda v, a: aec.NLMSAcousticEchoCancellationFeaturePtr(v, a)),
        (1, 1, dict(), lambda v, a: aec.KalmanFilterEchoCancellationFeaturePtr(v, a)),
        (2, 3, dict(amp4play=0.5), lambda v, a: aec.BlockKalmanFilterEchoCancellationFeaturePtr(v, a, sample_num=3, amp4play=0.5)),
        (3, 3, dict(), lambda v, a: aec.DTDBlockKalmanFilterEchoCancellationFeaturePtr(v, a, sample_num=3)),
    ]
    paths = [str(tmp_path / "p.wav"), str(tmp_path / "r.wav")]
    K = M // 2 + 1

    def graph(make):
        """a fresh banks -> node graph; the recordings are read after the graph is built, as the reference script does"""
        feats, banks = [], []
        for _ in paths:
            sf = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
            afb = OverSampledDFTAnalysisBankPtr(sf, prototype=h, M=M, m=m, r=r, delay_compensation_type=2)
            afb.set_block_frames(64)
            feats.append(sf); banks.append(afb)
        return feats, make(banks[0], banks[1])

    def read(feats):
        for sf, path in zip(feats, paths):
            sf.read(path, FS)

    for kind, P, kw, make in makers:
        feats, node = graph(make)
        sfb = OverSampledDFTSynthesisBankPtr(node, prototype=g, M=M, m=m, r=r, delay_compensation_type=2)
        read(feats)
        out = np.concatenate([np.array(b, np.float64) for b in sfb])
        ref, E, fl, mg, _ = _chain(h, g, M, m, r, played, rec, kind, P, -5, **kw)
        # the banks' float32 frames differ from the float64 closed form by ~1e-6 relative: decisions must sit well clear of that
        assert mg.smallest() >= 1e-4, (kind, mg.smallest())
        n = min(len(out), len(ref))
        assert n >= 140 * D and abs(len(out) - len(ref)) <= D
        err = np.max(np.abs(out[:n] - ref[:n]))
        print("aec node kind %d over banks -> synthesis: max |pcm error| %.3g LSB, %d updates skipped" % (kind, err, fl.size - fl.sum()))
        assert err <= 0.5
        # fresh graphs pulled frame by frame from the node (the banks hand their windows over, the frames come from the host
        # mirror): explicit frame numbers for every class, for the double-talk node next()'s default argument as well
        modes = [("explicit", 0)] + ([("default", -5)] if kind == 3 else [])
        for mode, fn0 in modes:
            _, Em, flm, mgm, _ = _chain(h, g, M, m, r, played, rec, kind, P, fn0, **kw)
            assert mgm.smallest() >= 1e-4, (kind, mode, mgm.smallest())
            T = Em.shape[1]
            feats, node = graph(make)
            read(feats)
            frames = np.zeros((T, M), np.complex128)
            for t in range(T):
                frames[t] = node.next(t) if mode == "explicit" else node.next()
            with pytest.raises(StopIteration):
                node.next(T) if mode == "explicit" else node.next()
            errE = np.max(np.abs(frames[:, :K].T - Em)) / np.max(np.abs(Em))
            print("aec node kind %d over banks, next() with %s frame numbers: E error %.2g of max|E|, %d updates skipped"
                  % (kind, mode, errE, flm.size - flm.sum()))
            assert errE <= TOL_E
            assert np.array_equal(frames[:, K:], np.conj(frames[:, M // 2 - 1:0:-1]))
            if kind == 3 and mode == "explicit":
                assert np.max(np.abs(Em - E)) > 1e-3 * np.max(np.abs(E))    # (the two ways of calling ARE different signals)


def test_tool_subband_aec(dev, proto256, tmp_path):
    """tools/subband_aec.py on two synthetic 2 s recordings, M = 256, filter_length 4, against the float64 chain; the chain itself
    attenuates the echo-only segment by >= 10 dB (a condition on the input, checked on the CPU side)"""
    from tools import subband_aec
    M, m, r, D = 256, 4, 1, 128
    h, g = proto256
    L = 2 * FS
    played, rec = _echo_pcm(9, L, near_from=L * 3 // 4)
    _write_wav(tmp_path / "played.wav", played); _write_wav(tmp_path / "rec.wav", rec)
    conf = dict(subband_aec.DEFAULT_CONF, filter_length=4)
    json.dump(conf, open(tmp_path / "aec.json", "w"))
    kw = dict(beta=conf["beta"], sigmau2=conf["sigmau2"], sigmak2=conf["sigmak2"], snr_threshold=conf["snr_threshold"],
              energy_threshold=conf["energy_threshold"], smooth=conf["smooth"], amp4play=conf["amp4play"])
    ref, E, fl, mg, Xa = _chain(h, g, M, m, r, played, rec, 3, 4, -5, **kw)
    assert mg.smallest() >= 1e-4, mg.smallest()
    seg = slice(int(0.5 * FS), int(1.4 * FS))                   # echo only: after convergence, before the near end sets in
    delay = len(rec) - len(ref) if len(ref) < len(rec) else 0
    att = 10 * np.log10(np.sum(rec[seg].astype(np.float64) ** 2) / np.sum(ref[seg] ** 2))
    print("aec tool: closed-form chain attenuates the echo-only segment by %.1f dB (margin %.3g, %d of %d updates skipped, %d samples shorter)"
          % (att, mg.smallest(), fl.size - fl.sum(), fl.size, delay))
    assert att >= 10.0
    opath = str(tmp_path / "out" / "aec.wav")
    assert subband_aec.main(["-q", "-i", str(tmp_path / "rec.wav"), "-p", str(tmp_path / "played.wav"), "-o", opath,
                             "-c", str(tmp_path / "aec.json")]) == 0
    w = wave.open(opath, "rb"); pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.float64); w.close()
    blocks = subband_aec.cancel_echo(h, g, M, m, r, str(tmp_path / "rec.wav"), str(tmp_path / "played.wav"), opath, conf, verbose=False)
    out = blocks.reshape(-1).astype(np.float64)
    n = min(len(out), len(ref))
    assert n >= L - 8 * D and abs(len(out) - len(ref)) <= D
    err = np.max(np.abs(out[:n] - ref[:n]))
    print("aec tool: max |pcm error| %.3g LSB against the float64 chain" % err)
    assert err <= 0.5
    # the file holds the same blocks as 16-bit integers (numpy.array(b, numpy.int16), as the reference script writes them)
    assert len(pcm) == len(out) and np.array_equal(pcm, np.array(out, np.int16).astype(np.float64))
