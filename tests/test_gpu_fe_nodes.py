"""GPU: the front-end nodes of btk20.feature (PreemphasisFeaturePtr, SpectralPowerFeaturePtr, VTLNFeaturePtr, MelFeaturePtr,
LogFeaturePtr, CepstralFeaturePtr, StorageFeaturePtr) and the tools built from them, on a 3 000-sample int16 WAV the test writes.

The node chains launch the kernel engine.fe_process launches, on the same samples, so their frames are compared with it bit for
bit; what fe_process computes is held to its bounds in tests/test_gpu_fe.py.  A MelFeature over a Python source is held to
2u sum |w| |in| against the closed form (float64 accumulation, one output rounding), u = 2^-24."""
import importlib.util
import os
import pickle
import wave

import numpy as np
import pytest

from tests import fe_closed_form as cf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
N, D, L = 3000, 160, 256
POWN = L // 2 + 1


@pytest.fixture(scope="module")
def wav(tmp_path_factory):
    rng = np.random.default_rng(7)
    x = np.round(rng.normal(scale=3000.0, size=N)).clip(-32768, 32767).astype(np.int16)
    x[320:480] = 0                                                   # one silent frame
    path = str(tmp_path_factory.mktemp("fe") / "utt.wav")
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(x.tobytes())
    return path, x.astype(np.float32)


@pytest.fixture(scope="module")
def expected(dev, wav):
    """engine.fe_process on the same samples, computed once: the two script chains and the chain the MFCC script meant"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    xd = torch.from_numpy(wav[1]).to(dev).view(1, 1, -1)
    kw = dict(D=D, shift=D, L=L, pad_zeros=False)
    out = {"T": eng.fe_frames(N, D, D, False)}
    o = eng.fe_process(xd, "pcm", ("power", "log", "cep"), dct=eng.fe_dct_table(1, 13, POWN), **kw)
    out["power"], out["log_power"], out["cep_power"] = (o[k][0, 0].cpu().numpy() for k in ("power", "log", "cep"))
    for ratio in (1.0, 0.9):
        o = eng.fe_process(xd, "pcm", ("vtln", "mel", "log", "cep"), vtln=eng.fe_vtln_table(POWN, ratio, 0.8, 2),
                           mel=eng.fe_mel_table(POWN, 16000, 100, 6800, 30, 2), dct=eng.fe_dct_table(1, 13, 30), **kw)
        out["vtln_%g" % ratio] = o["vtln"][0, 0].cpu().numpy()
        if ratio == 1.0:
            out["mel"], out["cep_mel"] = o["mel"][0, 0].cpu().numpy(), o["cep"][0, 0].cpu().numpy()
    return out


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def drain(node):
    return np.stack([np.array(v) for v in node])


def sample_count(path):
    from btk20.feature import SampleFeaturePtr
    s = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=False)
    s.read(path)
    return sum(1 for _ in s)


def test_log_power_chain_is_fe_process(wav, expected):
    samplefe, logfe = load_tool("log_power_extractor").build_chain(block_frames=7)
    samplefe.read(wav[0])
    got = drain(logfe)
    T = expected["T"]
    assert got.dtype == np.float32 and got.shape == (T, POWN) and T == sample_count(wav[0]) == 18
    assert np.array_equal(got, expected["log_power"])
    assert np.all(got[2] == 0)                                       # the silent frame: log10(0 + 1)
    assert logfe.launches() == -(-T // 7) and logfe.block_frames() == 7


@pytest.mark.parametrize("log_input", ["power", "mel"])
def test_mfcc_chain_is_fe_process(wav, expected, log_input):
    samplefe, cepfe, cep_storage = load_tool("mfcc_extractor").build_chain(log_input, block_frames=7)
    samplefe.read(wav[0])
    got = drain(cep_storage)
    assert got.dtype == np.float32 and got.shape == (expected["T"], 13)
    assert np.array_equal(got, expected["cep_" + log_input])
    assert cepfe.launches() == -(-expected["T"] // 7)
    # StorageFeature: random access into what it has served, for the cepstra and for the sample blocks below the window
    for j in (0, 5, 17):
        assert np.array_equal(np.array(cep_storage.next(j)), got[j])
    assert cep_storage.frame_no() == 17
    samplefe.read(wav[0])                                            # a SampleFeature drops its samples at its end
    assert cep_storage.evaluate() == 17
    assert np.array_equal(np.array(cep_storage.next(9)), got[9])


def test_block_size_does_not_change_the_bits(wav, expected):
    for bf in (1, 64):
        samplefe, logfe = load_tool("log_power_extractor").build_chain(block_frames=bf)
        samplefe.read(wav[0])
        assert np.array_equal(drain(logfe), expected["log_power"])
        assert logfe.launches() == -(-expected["T"] // bf)


def test_stream_protocol(wav, expected):
    from distant_speech_recognition_amd.btk20cpp import jindex_error
    samplefe, logfe = load_tool("log_power_extractor").build_chain(block_frames=7)
    samplefe.read(wav[0])
    a = logfe.next()
    b = logfe.next(0)
    assert logfe.frame_no() == 0 and np.shares_memory(a, b) and np.array_equal(b, expected["log_power"][0])
    c = logfe.next(1)
    assert np.array_equal(c, expected["log_power"][1])
    with pytest.raises(jindex_error):
        logfe.next(3)
    assert logfe.frame_no() == 1
    rest = [np.array(logfe.next()) for _ in range(expected["T"] - 2)]
    assert np.array_equal(np.stack(rest), expected["log_power"][2:])
    with pytest.raises(StopIteration):
        logfe.next()
    samplefe.read(wav[0])
    assert np.array_equal(drain(logfe), expected["log_power"])       # __iter__ resets every node of the chain


def test_overlapping_blocks_with_preemphasis(dev, wav):
    """SampleFeature blocks that overlap go up back to back; the kernel's pre-emphasis carries the last sample of the block before"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    from btk20.feature import (SampleFeaturePtr, PreemphasisFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr,
                               LogFeaturePtr)
    Dw, shift, Lw = 400, 160, 512
    s = SampleFeaturePtr(block_len=Dw, shift_len=shift, pad_zeros=True)
    pre = PreemphasisFeaturePtr(s, mu=0.95)
    logfe = LogFeaturePtr(SpectralPowerFeaturePtr(FFTFeaturePtr(HammingFeaturePtr(pre), fft_len=Lw), pow_num=Lw // 2 + 1))
    logfe.set_block_frames(7)
    s.read(wav[0])
    got = drain(logfe)
    xd = torch.from_numpy(wav[1]).to(dev).view(1, 1, -1)
    want = eng.fe_process(xd, "pcm", "log", D=Dw, shift=shift, L=Lw, preemph=0.95)["log"][0, 0].cpu().numpy()
    assert got.shape == want.shape == (eng.fe_frames(N, Dw, shift), Lw // 2 + 1) and np.array_equal(got, want)
    assert logfe.launches() == -(-got.shape[0] // 7)
    # the host node on its own gives the closed form's frames
    s.read(wav[0])
    pre.reset()
    fr = np.stack([np.array(pre.next()) for _ in range(5)])
    assert np.array_equal(fr, cf.frames(wav[1], Dw, shift, 5, 0.95, 0.0, window=False))


class PowerSource:
    """a Python source of power vectors"""

    def __init__(self, P):
        self.P, self.t = P, 0

    def size(self):
        return self.P.shape[1]

    def __iter__(self):
        return self

    def __next__(self):
        if self.t >= len(self.P):
            raise StopIteration
        self.t += 1
        return self.P[self.t - 1]

    next = __next__

    def reset(self):
        self.t = 0


def test_mel_over_a_python_source(dev):
    from btk20.feature import MelFeaturePtr
    rng = np.random.default_rng(3)
    P = rng.uniform(0.0, 4.0e9, size=(5, POWN)).astype(np.float32).astype(np.float64)
    P[2] = 0.0
    mel = MelFeaturePtr(PowerSource(P), pow_num=POWN, filter_num=30, rate=16000.0, low=100.0, up=6800.0, version=2)
    got = drain(mel)
    assert got.dtype == np.float64 and got.shape == (5, 30) and mel.launches() == 5
    off, cnt, rows = cf.mel_table(POWN, 16000, 100, 6800, 30, 2)
    want, scale = cf.mel_apply(P, off, cnt, rows), cf.mel_abs(P, off, cnt, rows)
    err = np.abs(got - want)
    print("MelFeature over a Python source: error/bound %.3f" % float(np.max(err / np.where(scale > 0, 2 * U * scale, 1.0))))
    assert np.all(err <= 2 * U * scale) and np.all(got[2] == 0)
    assert np.array_equal(mel.matrix(), np.stack([np.pad(r.astype(np.float64), (o, POWN - o - c)) for o, c, r in zip(off, cnt, rows)]))


def test_vtln_warp_changes_later_frames_only(wav, expected):
    from btk20.feature import SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr, VTLNFeaturePtr
    s = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=False)
    powerfe = SpectralPowerFeaturePtr(FFTFeaturePtr(HammingFeaturePtr(s), fft_len=L), pow_num=POWN)
    v = VTLNFeaturePtr(powerfe, coeff_num=POWN, edge=0.8, version=2)
    v.set_block_frames(7)
    s.read(wav[0])
    first = [np.array(v.next()) for _ in range(7)]
    v.warp(0.9)
    later = [np.array(v.next()) for _ in range(expected["T"] - 7)]
    assert np.array_equal(np.stack(first), expected["vtln_1"][:7])
    assert np.array_equal(np.stack(later), expected["vtln_0.9"][7:]) and not np.array_equal(np.stack(later), expected["vtln_1"][7:])
    from distant_speech_recognition_amd import engine as eng
    assert np.array_equal(v.matrix(), eng.fe_vtln_table(POWN, 0.9, 0.8, 2).matrix())


def _pickles(path):
    out = []
    with open(path, "rb") as fp:
        while True:
            try:
                out.append(pickle.load(fp))
            except EOFError:
                return np.stack(out)


def test_tools_write_the_node_outputs(wav, expected, tmp_path):
    lp = str(tmp_path / "log_power.pickle")
    assert load_tool("log_power_extractor").main([wav[0], lp, "-q", "--block-frames", "7"]) == expected["T"]
    assert np.array_equal(_pickles(lp), expected["log_power"])
    for mode in ("power", "mel"):
        mp = str(tmp_path / ("mfcc_%s.pickle" % mode))
        assert load_tool("mfcc_extractor").main([wav[0], mp, "-q", "--log-input", mode]) == expected["T"]
        got = _pickles(mp)
        assert got.dtype == np.float32 and np.array_equal(got, expected["cep_" + mode])
