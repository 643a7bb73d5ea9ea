"""GPU: the nodes SpectralSubtractor, WienerFilter (host/include/postfilter/spectralsubtraction.h) and HighPassFilter
(postfilter/postfilter.h) against the engine functions they launch (engine.spectral_subtract / wiener_filter / spec_highpass),
and tools/spectral_subtraction.py.

Where the node and the comparison scan the same 64-frame chunks the comparison is bit for bit: a switch cuts the stream into
segments of one constant mode (postfilter/enhancement_node.h), so `train the frames up to the mark, finish_training, subtract the
rest` is two engine launches with the state's frame counter carried along, and the node's blocks end on multiples of 64 of that
counter.  That holds for the flow of src/ss.cc (samples and model) and for a switch inside a block.  The Wiener test compares a
replayed segment (a cut at frame 40, inside a chunk) with one engine launch driven by per-frame flags: there the recursive scans
round elsewhere (tests/test_gpu_ss.py: (25 + 6n) 2^-24 relative on a PSD, (2 eps + 9u)|Y| on the output, below 1e-5 for the
shapes here), and that comparison alone is held to TOL = 1e-5 max|reference|.
The noise file keeps six decimals: a bin read back is within d = 5e-7, S2 = p - ft est moves by ft d, and with both roots
>= sqrt(floor) a subband magnitude moves by at most ft d / (2 sqrt(floor)); a synthesis sample is a sum over at most M bins and
the prototype's taps, so a PCM sample moves by at most  M sum|g| ft d / (2 sqrt(floor))  (+ TOL for the float32 roundings that
fall elsewhere)."""
import os

import numpy as np
import pytest

from tests import ss_closed_form as cf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, m, r, DCT = 256, 4, 1, 2
D, K = M >> r, M // 2 + 1
TOL = 1e-5
FT, FLOOR, NTRAIN = 1.5, 0.1, 80


def _protos():
    from distant_speech_recognition_amd import prototypes
    return prototypes.load(M, m, r)


def _pcm(T, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(T * D)
    return (300.0 * rng.normal(size=T * D) + 2000.0 * np.sin(2 * np.pi * 440.0 * t / 16000.0) * (t > 100 * D)).astype(np.float32)


def _bank(pcm, block_frames):
    from distant_speech_recognition_amd.btk20 import SampleFeaturePtr, OverSampledDFTAnalysisBankPtr
    sf = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
    sf.set_samples(np.ascontiguousarray(pcm, np.float32))
    a = OverSampledDFTAnalysisBankPtr(sf, prototype=_protos()[0], M=M, m=m, r=r, delay_compensation_type=DCT)
    a.set_block_frames(block_frames)
    return sf, a


class _Wrap:
    """a Python object in front of a node: whatever sits behind it is drained through next()"""

    def __init__(self, node):
        self.node = node

    def size(self):
        return self.node.size()

    def __iter__(self):
        self.node.reset()
        return self

    def next(self, frame_no=-5):
        return self.node.next(frame_no)

    __next__ = next

    def reset(self):
        self.node.reset()


class _Src:
    """frames [T][K] complex -> a Python source of M-bin vectors"""

    def __init__(self, X):
        self.F = np.zeros((X.shape[0], M), np.complex128)
        self.F[:, :K] = X
        self.F[:, K:] = np.conj(X[:, 1:M // 2][:, ::-1])
        self.t = 0

    def size(self):
        return M

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


def _drain(node):
    out = []
    while True:
        try:
            out.append(np.array(node.next()))
        except StopIteration:
            return out


def _ss_flow(pcm, block_frames, drained=False):
    """the flow of src/ss.cc: N + 1 synthesis outputs while training, stopTraining, startNoiseSubtraction, the rest"""
    from distant_speech_recognition_amd.btk20 import OverSampledDFTSynthesisBankPtr
    from distant_speech_recognition_amd.btk20.postfilter import SpectralSubtractorPtr
    sf, afb = _bank(pcm, block_frames)
    ss = SpectralSubtractorPtr(M, False, FT, FLOOR)
    if drained:
        ss.set_channel(_Wrap(afb))
        ss.set_block_frames(block_frames)
    else:
        ss.setChannel(afb)
    sfb = OverSampledDFTSynthesisBankPtr(ss, prototype=_protos()[1], M=M, m=m, r=r, delay_compensation_type=DCT)
    out = [np.array(sfb.next()) for _ in range(NTRAIN + 1)]
    v0 = ss.block_version()
    ss.stop_training()
    ss.start_noise_subtraction()
    assert ss.block_version() > v0
    psd = ss.noise_psd()
    out += _drain(sfb)
    return np.concatenate(out), psd, (sf, afb, ss, sfb)


@pytest.fixture(scope="module")
def flow_reference(dev):
    """the same flow from engine calls: the frames a per-frame graph has pulled after N + 1 outputs are 0 .. pd + N"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    T = 230
    pcm = _pcm(T, 5)
    h, g = _protos()
    afb = eng.FilterBank(h, M, m, r, DCT)
    sfb = eng.FilterBank(g, M, m, r, DCT, synthesis=True)
    X = afb.analysis(torch.from_numpy(pcm).to(dev).reshape(1, 1, -1))          # [1][K][1][T]
    mark = sfb.processing_delay + NTRAIN
    st = eng.SpectralSubtractionState(1, 1, M, [-1.0], device=dev)
    Y = torch.empty((1, K, X.shape[-1]), dtype=torch.complex64, device=dev)
    eng.spectral_subtract(X[..., :mark + 1], st, ft=FT, floor=FLOOR, train=True, subtract=False, out=Y[..., :mark + 1])
    st.finish_training()
    eng.spectral_subtract(X[..., mark + 1:], st, ft=FT, floor=FLOOR, train=False, subtract=True, out=Y[..., mark + 1:])
    ref = sfb.synthesize(Y).cpu().numpy()[0]
    return pcm, ref, st.est.cpu().numpy()[0, 0], int(st.count.cpu().numpy()[0, 0]), mark


def test_ss_cc_flow_over_block_sizes(dev, flow_reference, tmp_path):
    pcm, ref, est_ref, count, mark = flow_reference
    assert count == mark + 1 and mark + 1 > 64                   # training crosses a scan chunk and, with 64-frame blocks, a block
    outs = {}
    for name, bf, drained in (("64", 64, False), ("128", 128, False), ("0", 0, False), ("drained", 64, True)):
        y, psd, keep = _ss_flow(pcm, bf, drained)
        outs[name] = y
        n = min(len(y), len(ref))
        assert n >= len(ref) - D and n > (mark + 40) * D
        # the same launches in the same chunks: training chunks sit on multiples of 64 of the frame counter (the banks' blocks end
        # there too), the replayed segment ends at the mark as the engine's first launch does, and the model is float64 sums in
        # one order -- so the samples and the model are the engine's, bit for bit
        assert np.array_equal(y[:n].view(np.uint32), ref[:n].view(np.uint32)), name
        assert np.array_equal(psd.view(np.uint64), est_ref.view(np.uint64)), name
    for name in ("128", "0", "drained"):
        assert outs[name].shape == outs["64"].shape and np.array_equal(outs[name], outs["64"]), name
    # write_noise_file -> a fresh node -> read_noise_file: the output to the six decimals the format keeps
    y, psd, (sf, afb, ss, sfb) = _ss_flow(pcm, 64)
    fn = str(tmp_path / "noise.txt")
    assert ss.write_noise_file(fn) and len(open(fn).read().split()) == K
    from distant_speech_recognition_amd.btk20 import OverSampledDFTSynthesisBankPtr
    from distant_speech_recognition_amd.btk20.postfilter import SpectralSubtractorPtr
    sf2, afb2 = _bank(pcm, 64)
    ss2 = SpectralSubtractorPtr(M, False, FT, FLOOR)
    ss2.set_channel(afb2)
    assert ss2.read_noise_file(fn) and not ss2.read_noise_file(str(tmp_path / "missing.txt"))
    assert np.max(np.abs(ss2.noise_psd() - psd)) <= 5e-7
    ss2.start_noise_subtraction()
    sfb2 = OverSampledDFTSynthesisBankPtr(ss2, prototype=_protos()[1], M=M, m=m, r=r, delay_compensation_type=DCT)
    y2 = np.concatenate(_drain(sfb2))
    first = (NTRAIN + 1 + m * (1 << r) + (1 << r) + 2) * D        # blocks that no longer reach back into the training frames
    n = min(len(y), len(y2))
    bound = M * float(np.sum(np.abs(_protos()[1]))) * FT * 5e-7 / (2 * np.sqrt(FLOOR)) + TOL * float(np.max(np.abs(y)))
    d = float(np.max(np.abs(y[first:n] - y2[first:n])))
    print("noise file round trip: max |difference| %.3g, bound %.3g" % (d, bound))
    assert n - first > 50 * D and d <= bound and bound <= 0.01 * float(np.max(np.abs(y)))


def test_switch_in_the_middle_of_a_block_keeps_what_was_served(dev):
    import torch
    from distant_speech_recognition_amd import engine as eng
    from distant_speech_recognition_amd.btk20.postfilter import SpectralSubtractorPtr
    T, n0 = 150, 70
    X = (cf.make_input(1, K, 2, T, seed=21, zeros=False)[0] * 50).astype(np.complex64)       # [K][C][T]
    ss = SpectralSubtractorPtr(M, False, FT, FLOOR)
    ss.set_channel(_Src(X[:, 0].T)); ss.set_channel(_Src(X[:, 1].T), alpha=0.75)
    ss.set_block_frames(0)                                         # one block: the switch falls inside it
    served = [np.array(ss.next()) for _ in range(n0)]
    b0 = np.array(ss.block())[0]
    assert b0.shape == (K, T)
    ss.stop_training()
    ss.start_noise_subtraction()
    ss.set_noise_over_estimation_factor(2.0)
    b1 = np.array(ss.block())[0]
    assert np.array_equal(b1[:, :n0].view(np.uint32), b0[:, :n0].view(np.uint32))
    assert not np.array_equal(b1[:, n0:], b0[:, n0:])
    rest = _drain(ss)
    assert len(rest) == T - n0
    with pytest.raises(StopIteration):
        ss.next()
    # the same launches from the engine: frames 0 .. n0-1 train, average(), the rest is subtracted with the new factor
    Xd = torch.from_numpy(X).to(dev).unsqueeze(0)
    st = eng.SpectralSubtractionState(1, 2, M, [-1.0, 0.75], device=dev)
    Y = torch.empty((1, K, T), dtype=torch.complex64, device=dev)
    eng.spectral_subtract(Xd[..., :n0], st, ft=FT, floor=FLOOR, train=True, subtract=False, out=Y[..., :n0])
    st.finish_training()
    eng.spectral_subtract(Xd[..., n0:], st, ft=2.0, floor=FLOOR, train=False, subtract=True, out=Y[..., n0:])
    Yh = Y.cpu().numpy()[0]
    assert np.array_equal(b1.view(np.uint32), Yh.view(np.uint32))
    got = np.array(served + rest)                                  # [T][M]: bins 0..M/2 and their Hermitian mirror
    assert np.array_equal(got[:, :K].astype(np.complex64), Yh.T)
    assert np.array_equal(got[:, K:], np.conj(got[:, 1:M // 2][:, ::-1]))
    # the iterator protocol: __iter__ resets, the estimators live on, every frame comes once
    assert sum(1 for _ in ss) == T


def test_wiener_over_two_banks_stop_updating_and_reset(dev):
    import torch
    from distant_speech_recognition_amd import engine as eng
    from distant_speech_recognition_amd.btk20.postfilter import WienerFilterPtr
    T, n0, alpha, beta = 150, 40, 0.75, 1.5
    p1, p2 = _pcm(T, 7), (0.3 * _pcm(T, 8)).astype(np.float32)
    k1, k2 = _bank(p1, 64), _bank(p2, 64)
    w = WienerFilterPtr(k1[1], k2[1], False, alpha, FLOOR, beta)
    a = [np.array(w.next()) for _ in range(n0)]
    w.stop_updating_noise_PSD()
    a += _drain(w)
    got = np.array(a)[:, :K].T.astype(np.complex64)                # [K][T']
    h = _protos()[0]
    fb = eng.FilterBank(h, M, m, r, DCT)
    S1 = fb.analysis(torch.from_numpy(p1).to(dev).reshape(1, 1, -1))[:, :, 0].contiguous()
    S2 = fb.analysis(torch.from_numpy(p2).to(dev).reshape(1, 1, -1))[:, :, 0].contiguous()
    Tn = got.shape[1]
    assert Tn == S1.shape[-1]
    flags = np.zeros(Tn, np.uint8)
    flags[:n0] = 1
    st = eng.WienerState(1, M, device=dev)
    Y = eng.wiener_filter(S1, S2, st, alpha=alpha, floor=FLOOR, beta=beta, flags=flags).cpu().numpy()[0]
    assert np.max(np.abs(got - Y)) <= TOL * np.max(np.abs(Y))
    ps, pn = w.target_psd(), w.noise_psd()
    assert np.allclose(ps, st.psd_s.cpu().numpy()[0], rtol=1e-5, atol=0) and np.allclose(pn, st.psd_n.cpu().numpy()[0], rtol=1e-5, atol=0)
    # reset(): the sources restart, PSDs and frame counter live on (the first frame after it HAS memory)
    w.reset()
    assert np.array_equal(w.target_psd(), ps) and np.array_equal(w.noise_psd(), pn)
    k1[0].set_samples(p1); k2[0].set_samples(p2)
    f0 = np.array(w.next())[:K].astype(np.complex64)
    Y2 = eng.wiener_filter(S1[..., :1].contiguous(), S2[..., :1].contiguous(), st, alpha=alpha, floor=FLOOR, beta=beta,
                           update_noise=False).cpu().numpy()[0, :, 0]
    assert st.frames_done == Tn + 1 and np.max(np.abs(f0 - Y2)) <= TOL * np.max(np.abs(Y2))


def test_highpass_behind_a_beamformer(dev):
    """The high-pass takes the beamformer's block on the device and passes the synthesis bank's mark on to it, so a new look
    direction between two next() calls of the synthesis bank keeps its per-frame meaning: blocks of 64 frames give the samples of
    blocks of one frame (a per-frame graph), and they differ from the samples without the change."""
    from distant_speech_recognition_amd.btk20 import SubbandDSPtr, OverSampledDFTSynthesisBankPtr
    from distant_speech_recognition_amd.btk20.postfilter import HighPassFilterPtr
    from tests.util import la_delays, ula_positions
    T, N = 100, 4

    def beamformer(block_frames):
        bf, keep = SubbandDSPtr(fftlen=M, half_band_shift=False), []
        for c in range(N):
            keep.append(_bank(_pcm(T, 30 + c), block_frames))
            bf.set_channel(keep[-1][1])
        bf.calc_array_manifold_vectors(16000.0, la_delays(ula_positions(N), 0.3))
        return bf, keep
    bf1, k1 = beamformer(64)
    bf2, k2 = beamformer(64)
    hp = HighPassFilterPtr(bf1, cut_off_freq=150, samplerate=16000)
    cut = hp.cutoff_bin()
    assert cut == 2
    a, b = np.array(_drain(hp)), np.array(_drain(bf2))
    assert a.shape == b.shape and a.shape[0] >= T - 1
    ref = b.astype(np.complex64)
    ref[:, :cut] = 0
    ref[:, M - cut + 1:] = 0                                       # the mirror of the bins that were cut
    assert np.array_equal(a.astype(np.complex64), ref)

    def run(block_frames, change):
        bf, keep = beamformer(block_frames)
        h = HighPassFilterPtr(bf, cut_off_freq=150, samplerate=16000)
        sfb = OverSampledDFTSynthesisBankPtr(h, prototype=_protos()[1], M=M, m=m, r=r, delay_compensation_type=DCT)
        out = [np.array(sfb.next()) for _ in range(20)]
        if change:
            bf.calc_array_manifold_vectors(16000.0, la_delays(ula_positions(N), -1.0))
        return np.concatenate(out + _drain(sfb))
    y64, y1, y0 = run(64, True), run(1, True), run(64, False)
    assert y64.shape == y1.shape == y0.shape
    assert np.array_equal(y64.view(np.uint32), y1.view(np.uint32))
    assert np.array_equal(y64[:20 * D], y0[:20 * D]) and not np.array_equal(y64, y0)


def test_tool_runs_the_flow(dev, flow_reference, tmp_path):
    import wave
    from tools import spectral_subtraction as tool
    pcm, ref, est_ref, count, mark = flow_reference
    wav, out, nf = str(tmp_path / "in.wav"), str(tmp_path / "out.wav"), str(tmp_path / "model.txt")
    with wave.open(wav, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.round(pcm).astype(np.int16).tobytes())
    assert tool.main(["-A", wav, "-O", out, "-M", str(M), "-a", str(FT), "-f", str(FLOOR), "-N", str(NTRAIN), "-W", nf]) == 0
    with wave.open(out, "rb") as w:
        y = np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.float64)
    model = np.array(open(nf).read().split(), np.float64)
    assert model.shape == (K,) and len(y) >= len(ref) - D
    # the tool reads 16-bit samples (the reference's rounded here): its model is the engine's on those samples to the format's
    # six decimals only if the samples agree, so it is compared with the flow on the SAME rounded samples
    blocks, ss = tool.spectral_subtraction(np.round(pcm), *_protos(), M, m, r, FT, FLOOR, NTRAIN, "", "", DCT, verbose=False)
    assert np.max(np.abs(model - ss.noise_psd())) <= 5e-7
    n = min(len(y), blocks.size)
    assert np.max(np.abs(y[:n] - np.clip(np.trunc(blocks.reshape(-1)[:n]), -32768, 32767))) == 0
