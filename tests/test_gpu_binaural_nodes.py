"""GPU: the nodes BinaryMaskFilter, KimBinaryMaskFilter, IIDBinaryMaskFilter, KimITDThresholdEstimator, IIDThresholdEstimator and
FDIIDThresholdEstimator (host/include/postfilter/binauralprocessing.h) against the engine functions they launch
(engine.binaural_mask / binaural_stats / binaural_threshold), and tools/binaural_mask.py.

A node computes blocks; over analysis banks its blocks end on multiples of 64 of the frame counter, where the mask recursion's
scan chunks end too, so the mask filters give the bits of ONE engine launch at every block size.  An estimator adds one launch
per block to its float64 sums: its cost function has the bits of engine.binaural_stats called block by block, and the threshold
is the candidate the float64 closed form picks (tests/binaural_closed_form.py).  calc_threshold() mid-stream reads the sums at
the frame a per-frame graph has reached: the blocks before the current one and the current one up to that frame."""
import numpy as np
import pytest

from tests import binaural_closed_form as cf

pytestmark = pytest.mark.gpu

M, m, r, DCT = 256, 4, 1, 2
D, K = M >> r, M // 2 + 1
T = 150
ETA = 0.01
KINDS = {cf.KIM: "kim", cf.IID: "iid", cf.FDIID: "fdiid"}


def _protos():
    from distant_speech_recognition_amd import prototypes
    return prototypes.load(M, m, r)


def _pcm(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    t = np.arange(T * D)
    return (scale * (300.0 * rng.normal(size=T * D) + 2000.0 * np.sin(2 * np.pi * (440.0 + 100 * seed) * t / 16000.0) * (t > 60 * D))).astype(np.float32)


PCM = (_pcm(1), _pcm(2, 0.8))


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


def _drain(node):
    out = []
    while True:
        try:
            out.append(np.array(node.next()))
        except StopIteration:
            return out


def _drain_blocks(node, limit=None, splits=None):
    """next() until the end (or `limit` times): the frames, and the frames per block the node computed them in (read off block());
    a second call with the first's `splits` goes on where that one stopped"""
    out = []
    left = 0 if splits is None else splits.pop()
    splits = [] if splits is None else splits
    while limit is None or len(out) < limit:
        try:
            out.append(np.array(node.next()))
        except StopIteration:
            break
        if left == 0:
            left = np.array(node.block()).shape[-1]
            splits.append(left)
        left -= 1
    return out, (splits + [left] if limit is not None else splits)


CONFIGS = (("64", 64, False), ("128", 128, False), ("0", 0, False), ("drained", 64, True))


def _sources(block_frames, drained):
    """the two analysis banks (and what keeps them alive), as the node's sources"""
    k1, k2 = _bank(PCM[0], block_frames), _bank(PCM[1], block_frames)
    if drained:
        return (_Wrap(k1[1]), _Wrap(k2[1])), (k1, k2)
    return (k1[1], k2[1]), (k1, k2)


@pytest.fixture(scope="module")
def spectra(dev):
    """the subband frames of the two sources, complex64 [1][K][T'] on the device and on the host"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    fb = eng.FilterBank(_protos()[0], M, m, r, DCT)
    S = [fb.analysis(torch.from_numpy(p).to(dev).reshape(1, 1, -1))[:, :, 0].contiguous() for p in PCM]
    return S, [s.cpu().numpy() for s in S]


def _frames(out):
    """frames served by next() [T][M] -> complex64 [K][T], after checking the Hermitian upper half"""
    a = np.array(out)
    assert np.array_equal(a[:, K:], np.conj(a[:, 1:M // 2][:, ::-1]))
    return np.ascontiguousarray(a[:, :K].T.astype(np.complex64))


@pytest.mark.parametrize("kind,chan,thr,alpha", [(cf.KIM, 0, 0.8, 0.6), (cf.KIM, 1, 0.8, 0.0), (cf.IID, 0, 50.0, 0.6), (cf.IID, 1, -20.0, 0.6)])
def test_mask_filters_over_block_sizes(dev, spectra, kind, chan, thr, alpha):
    from distant_speech_recognition_amd import engine as eng
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    S, _ = spectra
    st = eng.binaural_mask_state(1, M, dev)
    Y = eng.binaural_mask(S[0], S[1], KINDS[kind], chan, thr, alpha, ETA, state=st).cpu().numpy()[0]
    cls = pf.KimBinaryMaskFilterPtr if kind == cf.KIM else pf.IIDBinaryMaskFilterPtr
    for name, bf, drained in CONFIGS:
        (a, b), keep = _sources(bf, drained)
        node = cls(chan, a, b, M, thr, alpha, ETA)
        if drained:
            node.set_block_frames(bf)
        got = _frames(_drain(node))
        assert got.shape == Y.shape, name
        assert np.array_equal(got.view(np.uint32), Y.view(np.uint32)), name
        assert np.array_equal(node.prev_mu(), st.cpu().numpy()[0]), name
        assert node.threshold() == np.float32(thr)


def test_set_threshold_and_set_thresholds_mid_stream(dev, spectra):
    from distant_speech_recognition_amd import engine as eng
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    S, _ = spectra
    Tn, n0, n1 = S[0].shape[-1], 40, 90
    thrs = np.linspace(-100.0, 100.0, K)

    def run(alpha, bf, drained):
        (a, b), keep = _sources(bf, drained)
        node = pf.IIDBinaryMaskFilterPtr(0, a, b, M, 50.0, alpha, ETA)
        if drained:
            node.set_block_frames(bf)
        out = [np.array(node.next()) for _ in range(n0)]
        v0 = node.block_version()
        node.set_threshold(-30.0)
        assert node.block_version() > v0 and node.threshold() == -30.0 and node.thresholds() is None
        out += [np.array(node.next()) for _ in range(n1 - n0)]
        node.set_thresholds(thrs)
        out += _drain(node)
        assert np.array_equal(node.thresholds()[1:], thrs[1:]) and node.threshold() == np.float32(thrs[-1])
        return _frames(out), node.prev_mu()

    # the same launches from the engine: three segments of one constant mode, the frame counter carried along
    for alpha in (0.6, 0.0):
        st = eng.binaural_mask_state(1, M, dev)
        parts = [eng.binaural_mask(S[0][..., :n0], S[1][..., :n0], "iid", 0, 50.0, alpha, ETA, state=st, frames_done=0),
                 eng.binaural_mask(S[0][..., n0:n1], S[1][..., n0:n1], "iid", 0, -30.0, alpha, ETA, state=st, frames_done=n0),
                 eng.binaural_mask(S[0][..., n1:], S[1][..., n1:], "iid", 0, 0.0, alpha, ETA, state=st, thresholds=thrs, frames_done=n1)]
        Y = np.concatenate([p.cpu().numpy()[0] for p in parts], axis=1)
        got, mu = run(alpha, 64, False)
        assert got.shape == (K, Tn) and np.array_equal(got.view(np.uint32), Y.view(np.uint32)), alpha
        assert np.array_equal(mu, st.cpu().numpy()[0])
        if alpha == 0.0:
            # without memory a block of one frame is a launch of one frame: a per-frame graph, bit for bit
            one, _ = run(alpha, 1, True)
            assert np.array_equal(one.view(np.uint32), got.view(np.uint32))
    # it does change the frames behind the mark, and only those
    st = eng.binaural_mask_state(1, M, dev)
    same = eng.binaural_mask(S[0], S[1], "iid", 0, 50.0, 0.0, ETA, state=st).cpu().numpy()[0]
    assert np.array_equal(got[:, :n0], same[:, :n0]) and not np.array_equal(got[:, n0:n1], same[:, n0:n1])


EST = {cf.KIM: ("KimITDThresholdEstimatorPtr", dict(), (float(np.float32(-0.2 * 16000 / 340)), float(np.float32(0.2 * 16000 / 340)), 0.02), 1 / 15.0),
       cf.IID: ("IIDThresholdEstimatorPtr", dict(minThreshold=-1000.0, maxThreshold=1000.0, width=50.0), (-1000.0, 1000.0, 50.0), 0.5),
       cf.FDIID: ("FDIIDThresholdEstimatorPtr", dict(min_threshold=-2000.0, max_threshold=2000.0, width=125.0), (-2000.0, 2000.0, 125.0), 1 / 15.0)}


def _engine_sums(eng, S, kind, cands, pc, splits, k0=1, k1=K):
    st, t0 = None, 0
    for n in splits:
        st = eng.binaural_stats(S[0][..., t0:t0 + n], S[1][..., t0:t0 + n], KINDS[kind], cands, ETA, pc, k0, k1, state=st)
        t0 += n
    return st


def _cost(est, kind):
    return np.stack([est.cost_function(k) for k in range(K)]) if kind == cf.FDIID else est.cost_function()


@pytest.mark.parametrize("kind", [cf.KIM, cf.IID, cf.FDIID], ids=["kim", "iid", "fdiid"])
def test_estimators_over_block_sizes_and_mid_stream(dev, spectra, kind):
    from distant_speech_recognition_amd import engine as eng
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    S, Sh = spectra
    Tn = S[0].shape[-1]
    cname, kw, rng_, pc = EST[kind]
    cands = eng.binaural_candidates(*rng_)
    sums, _ = cf.stats_closed_form(Sh[0], Sh[1], kind, cands[0], cands[1], ETA, pc)
    ref = cf.threshold_closed_form(kind, sums[0], Tn, *cands)
    for name, bf, drained in CONFIGS:
        (a, b), keep = _sources(bf, drained)
        est = getattr(pf, cname)(a, b, M, **kw)
        if drained:
            est.set_block_frames(bf)
        assert est.num_candidates() == cands[1] and np.array_equal(est.candidates(), cands[0])
        out, splits = _drain_blocks(est)
        out = np.array(out)
        assert out.shape == (Tn, M) and not out.any(), "an estimator's next() returns its own zero vector"
        assert sum(splits) == Tn and (bf == 0 or max(splits) <= max(bf, 128)) and (bf != 0 or splits == [Tn]), (name, splits)
        thr = est.calc_threshold()
        want = eng.binaural_threshold(KINDS[kind], _engine_sums(eng, S, kind, cands, pc, splits), cands)
        assert thr == want[0] == ref[0], (name, thr, want[0], ref[0])
        assert np.array_equal(_cost(est, kind), want[1]), name
        assert est.threshold() == np.float32(thr)
        if kind == cf.FDIID:
            assert np.array_equal(est.thresholds()[1:], want[2][1:]) and np.array_equal(want[2], ref[2])
        else:
            assert est.num_samples() == Tn
        assert est.calc_threshold() == thr and np.array_equal(_cost(est, kind), want[1]), "calc_threshold() is idempotent"
    # mid-stream: after n0 frames the sums are those of the frames a per-frame graph has pulled
    n0 = 100
    (a, b), keep = _sources(64, False)
    est = getattr(pf, cname)(a, b, M, **kw)
    _, state = _drain_blocks(est, n0)                              # the blocks so far, and what is left of the last
    splits = state[:-1]
    assert sum(splits) > n0 and len(splits) >= 2, "the mark lies inside a block, behind the first"
    thr = est.calc_threshold()
    upto = splits[:-1] + [n0 - sum(splits[:-1])]
    want = eng.binaural_threshold(KINDS[kind], _engine_sums(eng, S, kind, cands, pc, upto), cands)
    sums0, _ = cf.stats_closed_form(Sh[0][..., :n0], Sh[1][..., :n0], kind, cands[0], cands[1], ETA, pc)
    assert thr == want[0] == cf.threshold_closed_form(kind, sums0[0], n0, *cands)[0]
    assert np.array_equal(_cost(est, kind), want[1])
    # ... and accumulation goes on after it, to the same end
    _, splits = _drain_blocks(est, None, state)
    assert sum(splits) == Tn
    want = eng.binaural_threshold(KINDS[kind], _engine_sums(eng, S, kind, cands, pc, splits), cands)
    assert est.calc_threshold() == want[0] == ref[0] and np.array_equal(_cost(est, kind), want[1])
    # reset() clears the sums (and restarts the sources)
    est.reset()
    if kind != cf.FDIID:
        assert est.num_samples() == 0
    keep[0][0].set_samples(PCM[0]); keep[1][0].set_samples(PCM[1])
    _, again = _drain_blocks(est)
    want = eng.binaural_threshold(KINDS[kind], _engine_sums(eng, S, kind, cands, pc, again), cands)
    assert est.calc_threshold() == ref[0] and np.array_equal(_cost(est, kind), want[1])


def test_kim_estimator_bin_range_in_float(dev, spectra):
    from distant_speech_recognition_amd import engine as eng
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    S, _ = spectra
    (a, b), keep = _sources(64, False)
    est = pf.KimITDThresholdEstimatorPtr(a, b, M, 0.0, 2.0, 0.1, minFreq=0.0, maxFreq=3000.0, sampleRate=16000)
    k0, k1 = int(np.float32(M) * np.float32(0.0) / np.float32(16000)), int(np.float32(M) * np.float32(3000.0) / np.float32(16000))
    assert (est.min_fbin(), est.max_fbin()) == (k0, k1) == (0, 48)
    assert est.num_candidates() == 21 and len(est.candidates()) == 20
    _, splits = _drain_blocks(est)
    cands = eng.binaural_candidates(0.0, 2.0, 0.1)
    want = eng.binaural_threshold("kim", _engine_sums(eng, S, cf.KIM, cands, 1 / 15.0, splits, k0, k1), cands)
    assert est.calc_threshold() == want[0] and np.array_equal(est.cost_function(), want[1]) and est.cost_function()[20] == 0


def test_reset_of_a_mask_filter_leaves_prev_mu(dev, spectra):
    from distant_speech_recognition_amd import engine as eng
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    S, _ = spectra
    Tn = S[0].shape[-1]
    (a, b), keep = _sources(64, False)
    node = pf.KimBinaryMaskFilterPtr(0, a, b, M, 0.8, 0.6, ETA)
    _drain(node)
    mu = node.prev_mu()
    assert mu[0] == 1.0 and np.any(mu[1:] != 1.0)
    node.reset()
    assert np.array_equal(node.prev_mu(), mu)
    keep[0][0].set_samples(PCM[0]); keep[1][0].set_samples(PCM[1])
    f0 = np.array(node.next())[:K].astype(np.complex64)
    st = eng.binaural_mask_state(1, M, dev)
    st.copy_(__import__("torch").from_numpy(mu)[None])
    want = eng.binaural_mask(S[0][..., :1].contiguous(), S[1][..., :1].contiguous(), "kim", 0, 0.8, 0.6, ETA, state=st, frames_done=Tn)
    assert np.array_equal(f0, want.cpu().numpy()[0, :, 0]), "the first frame after reset() has the memory of the stream before"


def test_base_class_only_counts_frames(dev):
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    (a, b), keep = _sources(64, False)
    node = pf.BinaryMaskFilterPtr(0, a, b, M, 0.5, 0.0)
    for i in range(3):
        v = np.array(node.next())
        assert v.shape == (M,) and not v.any() and node.frame_no() == i
    assert a.frame_no() == -1, "the base class pulls nothing"
    node.setThreshold(0.25)
    assert node.getThreshold() == 0.25 and node.getThresholds() is None


def test_two_beams_estimator_filter_synthesis(dev, kinect_pcm):
    """two SubbandDS beams at two look directions -> IID estimator -> the filter with its threshold -> synthesis, device to device"""
    import torch
    from distant_speech_recognition_amd import btk20cpp, engine as eng
    from distant_speech_recognition_amd.btk20 import SubbandDSPtr, OverSampledDFTSynthesisBankPtr
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    from tests.util import la_delays, ula_positions
    N = 4
    pcm = np.ascontiguousarray(kinect_pcm[:N, :T * D], np.float32)

    def beams():
        out, keep = [], []
        for look in (0.3, -1.0):
            bf = SubbandDSPtr(fftlen=M, half_band_shift=False)
            for c in range(N):
                keep.append(_bank(pcm[c], 64))
                bf.set_channel(keep[-1][1])
            bf.calc_array_manifold_vectors(16000.0, la_delays(ula_positions(N), look))
            out.append(bf)
        return out, keep
    (bt, bi), keep = beams()
    B = [_frames(_drain(x)) for x in beams()[0]]                          # the beams' frames, through the host
    Bd = [torch.from_numpy(x).to(dev)[None] for x in B]
    rng_ = (-1000.0, 1000.0, 50.0)
    est = pf.IIDThresholdEstimatorPtr(bt, bi, M, *rng_)
    _, splits = _drain_blocks(est)
    thr = est.calc_threshold()
    cands = eng.binaural_candidates(*rng_)
    Tn = B[0].shape[1]
    assert sum(splits) == Tn
    want = eng.binaural_threshold("iid", _engine_sums(eng, Bd, cf.IID, cands, 0.5, splits), cands)
    assert thr == want[0] and np.array_equal(est.cost_function(), want[1]) and np.ptp(want[1]) > 0
    (bt, bi), keep2 = beams()
    filt = pf.IIDBinaryMaskFilterPtr(0, bt, bi, M, thr, 0.6, ETA)
    sfb = OverSampledDFTSynthesisBankPtr(filt, prototype=_protos()[1], M=M, m=m, r=r, delay_compensation_type=DCT)
    b0 = btk20cpp.node_d2h_bytes()
    y = np.concatenate(_drain(sfb))
    back = btk20cpp.node_d2h_bytes() - b0
    assert back < 8 * K * Tn, "%d bytes came back to the host: a spectrum [K][T] is %d" % (back, 8 * K * Tn)
    # the filter's frames are the engine's, launched in the blocks the beams deliver (read off a third graph, through next())
    (bt, bi), keep3 = beams()
    got, splits = _drain_blocks(pf.IIDBinaryMaskFilterPtr(0, bt, bi, M, thr, 0.6, ETA))
    assert sum(splits) == Tn
    st, Y, t0 = eng.binaural_mask_state(1, M, dev), torch.empty_like(Bd[0]), 0
    for n in splits:
        eng.binaural_mask(Bd[0][..., t0:t0 + n], Bd[1][..., t0:t0 + n], "iid", 0, thr, 0.6, ETA, state=st, frames_done=t0, out=Y[..., t0:t0 + n])
        t0 += n
    assert np.array_equal(_frames(got).view(np.uint32), Y.cpu().numpy()[0].view(np.uint32)), splits
    ref = eng.FilterBank(_protos()[1], M, m, r, DCT, synthesis=True).synthesize(Y).cpu().numpy()[0]
    n = min(len(y), len(ref))
    assert n >= len(ref) - D and np.array_equal(y[:n].view(np.uint32), ref[:n].view(np.uint32))


def test_constructor_errors(dev):
    from distant_speech_recognition_amd import btk20cpp
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    (a, b), keep = _sources(64, False)
    err = btk20cpp.jdimension_error
    for make in (lambda: pf.BinaryMaskFilterPtr(0, a, b, M // 2, 0.0, 0.0),
                 lambda: pf.KimBinaryMaskFilterPtr(0, a, b, 2 * M, 0.0, 0.0),
                 lambda: pf.IIDBinaryMaskFilterPtr(2, a, b, M, 0.0, 0.0),
                 lambda: pf.KimITDThresholdEstimatorPtr(a, b, M // 2),
                 lambda: pf.IIDThresholdEstimatorPtr(a, b, M, minFreq=0.0, maxFreq=9000.0, sampleRate=16000),
                 lambda: pf.KimITDThresholdEstimatorPtr(a, b, M, -1e6, 1e6, 0.5),
                 lambda: pf.FDIIDThresholdEstimatorPtr(a, b, M // 2)):
        with pytest.raises(err):
            make()
    node = pf.IIDBinaryMaskFilterPtr(0, a, b, M, 0.0, 0.0)
    with pytest.raises(err):
        node.set_thresholds(np.zeros(K - 1))


def test_names_keywords_and_defaults(dev):
    from distant_speech_recognition_amd import btk20, btk20cpp
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    for n in ("BinaryMaskFilter", "KimBinaryMaskFilter", "KimITDThresholdEstimator", "IIDBinaryMaskFilter", "IIDThresholdEstimator",
              "FDIIDThresholdEstimator"):
        assert getattr(pf, n) is getattr(pf, n + "Ptr") is getattr(btk20cpp, n) and n in pf.__all__ and n + "Ptr" in pf.__all__
    (a, b), keep = _sources(64, False)
    k = pf.KimBinaryMaskFilter(chanX=1, srcL=a, srcR=b, M=M, threshold=0.5, alpha=0.25, dEta=0.1, dPowerCoeff=0.2, nm="kim")
    assert k.name() == "kim" and k.getThreshold() == 0.5
    i = pf.IIDBinaryMaskFilter(chanX=0, srcL=a, srcR=b, M=M, threshold=2.0, alpha=0.0)
    assert i.threshold() == 2.0
    e = pf.KimITDThresholdEstimator(srcL=a, srcR=b, M=M, minThreshold=0.0, maxThreshold=1.0, width=0.1, dEta=0.01)
    assert (e.num_candidates(), len(e.candidates())) == (11, 10) and (e.min_fbin(), e.max_fbin()) == (1, K)
    e = pf.KimITDThresholdEstimator(a, b, M)                       # the default range: +-0.2 x 16000 / 340 whatever the sample rate
    assert e.num_candidates() == 942 and e.candidates()[0] == np.float32(-0.2 * 16000 / 340)
    e = pf.IIDThresholdEstimator(srcL=a, srcR=b, M=M, minThreshold=-1.0, maxThreshold=1.0, width=0.5, minFreq=100.0, maxFreq=4000.0, sampleRate=16000)
    assert (e.min_fbin(), e.max_fbin()) == (1, 64) and e.num_candidates() == 5
    f = pf.FDIIDThresholdEstimator(src_left=a, src_right=b, M=M, min_threshold=-1.0, max_threshold=1.0, width=0.5, deta=0.1, dpowercoeff=0.3)
    assert f.num_candidates() == 5
    f = pf.FDIIDThresholdEstimator(srcL=a, srcR=b, M=M, minThreshold=-1.0, maxThreshold=1.0, width=0.25, dEta=0.1)
    assert f.num_candidates() == 9
    f = pf.FDIIDThresholdEstimator(a, b, M)                        # +-100000 in steps of 1000
    assert f.num_candidates() == 201 and f.candidates()[0] == -100000.0
    for obj, names in ((k, ("setThreshold", "setThresholds", "getThreshold", "getThresholds")),
                       (e, ("calcThreshold", "getCostFunction")), (f, ("calcThreshold", "getCostFunction"))):
        for nme in names:
            assert callable(getattr(obj, nme))
    assert btk20.postfilter is pf


@pytest.mark.parametrize("kind", ["iid", "fdiid", "kim"])
def test_tool_runs_the_two_passes(dev, kinect_pcm, tmp_path, kind):
    import wave
    from tools import binaural_mask as tool
    out = str(tmp_path / "out.wav")
    assert tool.main(["-O", out, "-k", kind, "-M", str(M)]) == 0
    with wave.open(out, "rb") as w:
        assert (w.getnchannels(), w.getsampwidth(), w.getframerate()) == (1, 2, 16000)
        y = np.frombuffer(w.readframes(w.getnframes()), np.int16)
    blocks, thr, est = tool.binaural_mask(kinect_pcm, 16000, *_protos(), M, m, r, kind, verbose=False)
    assert len(y) == blocks.size >= kinect_pcm.shape[1] - D and np.any(y != 0)
    assert np.array_equal(y, np.clip(np.trunc(blocks.reshape(-1)), -32768, 32767).astype(np.int16))
    assert thr in est.candidates() and np.isfinite(blocks).all()
