"""GPU: the TDOA node chain (SampleFeaturePtr -> HammingFeaturePtr -> FFTFeaturePtr), btk20.pytdoa's front end and
tools/tdoa_estimator.py, against the float64 closed form (tests/tdoa_closed_form.py) and the reference's own results
(tests/golden/pytdoa_golden.npz).

Bounds: those of tests/test_gpu_tdoa.py (derived in its docstring) -- the spectra bound (log2 L + 1) eta per frame for what
FFTFeature serves, B = (log2 L + 1) eta + 4u for peak heights, lags equal wherever the two largest |g| of the float64
correlation of the golden's spectra are more than 2B apart (at most 1 % of a case left out), positions within 1e-9 on frames
whose contributing lags are all equal (the same float64 arithmetic on the same integers).
Every test prints its largest error / bound ratio and its left-out count.
"""
import json
import math
import os
import wave

import numpy as np
import pytest

from tests import tdoa_closed_form as cf
from tests.test_gpu_tdoa import spectra_bound, gcc_bound

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FS = 16000
SSPEED = 343740.0
KINECT_MPOS = [[-113.0, 0.0, 2.0], [36.0, 0.0, 2.0], [76.0, 0.0, 2.0], [113.0, 0.0, 2.0]]
KINECT_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
KINECT_CONF = dict(energy_threshold=128, minimum_pairs=5, threshold=0.12)
CIRC_CONF = dict(energy_threshold=64, minimum_pairs=3, threshold=0.12)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "pytdoa_golden.npz"))


def chain(x, D, L, block_frames=0):
    from btk20.feature import SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr
    s = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
    s.set_samples(np.ascontiguousarray(x, np.float32))
    return s, FFTFeaturePtr(HammingFeaturePtr(s), L, block_frames=block_frames)


def drain(node):
    return np.stack([np.array(v) for v in node])


@pytest.mark.parametrize("D,L", [(256, 512), (8192, 16384)], ids=["short", "script"])
def test_node_chain_against_closed_form(dev, kinect_pcm, D, L):
    x = kinect_pcm[1]
    T = cf.n_frames(len(x), D)
    s, f = chain(x, D, L)
    assert f.has_sample_chain() and f.size() == L and f.fftLen() == L and f.windowLen() == D
    frames = drain(f)
    assert frames.shape == (T, L) and frames.dtype == np.complex128
    X64 = cf.spectra(x, D, L)[0]
    half = frames[:, :L // 2 + 1]
    num = np.sqrt(np.sum(np.abs(half - X64) ** 2, axis=-1))
    den = np.sqrt(np.sum(np.abs(X64) ** 2, axis=-1))
    print("FFTFeature D=%d L=%d: %d frames, error/bound %.3f, launches %d" % (D, L, T, float(np.max(num / den)) / spectra_bound(L), f.launches()))
    assert np.all(num <= spectra_bound(L) * den)
    # the mirror half is the exact conjugate, bins 0 and L/2 are real, the values are widened float32
    assert np.array_equal(frames[:, L // 2 + 1:], np.conj(frames[:, L // 2 - 1:0:-1]))
    assert np.all(frames[:, 0].imag == 0) and np.all(frames[:, L // 2].imag == 0)
    assert np.array_equal(half, half.astype(np.complex64).astype(np.complex128))
    assert f.launches() == -(-T // f.block_frames())
    with pytest.raises(StopIteration):
        f.next()


def test_node_protocol_and_block_boundaries(dev, kinect_pcm):
    from distant_speech_recognition_amd.btk20cpp import jindex_error
    D, L = 256, 512
    x = kinect_pcm[0][:10 * D + 77]                      # 11 frames, the last one ragged
    s, f = chain(x, D, L)
    ref = drain(f)
    assert ref.shape == (11, L) and f.launches() == 1
    # a block length of 4 frames crosses block boundaries: the same bits
    s4, f4 = chain(x, D, L, block_frames=4)
    assert f4.block_frames() == 4
    a = f4.next(0)
    b = f4.next(0)                                       # the same number returns the cached vector
    assert np.shares_memory(a, b) and np.array_equal(a, ref[0]) and f4.frame_no() == 0
    with pytest.raises(jindex_error):
        f4.next(2)                                       # a skipped frame number
    got = [np.array(a)] + [np.array(f4.next(t)) for t in range(1, 11)]
    assert np.array_equal(np.stack(got), ref) and f4.launches() == 3
    with pytest.raises(StopIteration):
        f4.next(11)
    assert f4.is_end()
    # reset() and a second pass over reloaded samples (the source drops them at its end, as the reference's does)
    s4.set_samples(np.ascontiguousarray(x, np.float32))
    again = drain(f4)                                    # __iter__ resets
    assert np.array_equal(again, ref)
    f4.set_block_frames(5)
    s4.set_samples(np.ascontiguousarray(x, np.float32))
    assert np.array_equal(drain(f4), ref)
    # the HammingFeature alone: the float64 product rounded to float32
    from btk20.feature import SampleFeaturePtr, HammingFeaturePtr
    sh = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
    sh.set_samples(np.ascontiguousarray(x, np.float32))
    hw = drain(HammingFeaturePtr(sh))
    assert hw.dtype == np.float32 and hw.shape == (11, D)
    cfw = cf.windowed_frames(x, D)
    assert np.max(np.abs(hw.astype(np.float64) - cfw)) <= 2.0 ** -23 * np.max(np.abs(cfw))   # one float32 rounding, window to 1 ulp of double


class FloatFrames:
    """a numpy-backed float source: any Python object with size() / __iter__ / next() / reset()"""

    def __init__(self, frames):
        self.frames, self.t = frames, 0

    def size(self):
        return self.frames.shape[1]

    def __iter__(self):
        return self

    def next(self):
        if self.t >= len(self.frames):
            raise StopIteration
        self.t += 1
        return self.frames[self.t - 1]

    __next__ = next

    def reset(self):
        self.t = 0


def test_one_frame_path_gives_the_block_path_bits(dev, kinect_pcm):
    from btk20.feature import SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr
    D, L = 1000, 1024
    x = kinect_pcm[2][:7 * D + 123]
    s, f = chain(x, D, L)
    ref = drain(f)
    sh = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
    sh.set_samples(np.ascontiguousarray(x, np.float32))
    windowed = drain(HammingFeaturePtr(sh))              # what the block path windows inside its kernel
    g = FFTFeaturePtr(FloatFrames(windowed), L)
    assert not g.has_sample_chain()
    one = drain(g)
    assert one.shape == ref.shape == (8, L) and np.array_equal(one, ref) and g.launches() == 8
    # a HammingFeature over a Python source: windowed on the host, one frame per launch, the same bits again
    raw = np.zeros((8, D), np.float32)
    raw.reshape(-1)[:len(x)] = x
    g2 = FFTFeaturePtr(HammingFeaturePtr(FloatFrames(raw)), L)
    assert np.array_equal(drain(g2), ref)


class SpectralFrames:
    """a supplied spectral source: next(frame_no) is the full spectrum of the frame"""

    def __init__(self, Xhalf):
        L = 2 * (Xhalf.shape[1] - 1)
        self.X = np.concatenate([Xhalf, np.conj(Xhalf[:, L // 2 - 1:0:-1])], axis=1)

    def next(self, frame_no):
        if frame_no >= len(self.X):
            raise StopIteration
        return self.X[frame_no]

    def reset(self):
        pass


def compare_with_golden(fe, golden, name, pcm, D, L, pairs, conf, label):
    """Drive the front end frame by frame as the reference's script does and compare with the golden under the rules of the
    module docstring.  Returns the number of frames."""
    peaks = golden[name + "_peaks"]
    T, P = peaks.shape[:2]
    X = cf.spectra(pcm, D, L)[0].astype(np.complex64).astype(np.complex128)
    margin = cf.gcc_peaks(X, cf.energy(X), pairs, conf["energy_threshold"])[2].T          # [T][P]
    B = gcc_bound(L)
    left_out = mismatches = frames = pos_checked = 0
    worst_h = worst_pos = 0.0
    for t, obs in enumerate(fe):
        frames += 1
        got = np.array([[np.nan if d is None else d, h] for d, h in (src.next(t) for src in fe._mic_pair_srcs)])
        none_ref = np.isnan(peaks[t, :, 0])
        assert np.array_equal(np.isnan(got[:, 0]), none_ref)
        dh = np.abs(got[:, 1] - peaks[t, :, 1])
        worst_h = max(worst_h, float(dh.max()) / B)
        assert np.all(dh <= B), (t, dh.max() / B)
        sure = ~none_ref & (margin[t] > 2 * B)
        left_out += int(np.sum(~none_ref & ~sure))
        equal = np.zeros(P, bool)
        equal[~none_ref] = got[~none_ref, 0] == peaks[t, ~none_ref, 0]
        mismatches += int(np.sum(sure & ~equal))
        # the observation list and the keys of mic_pair_tdoa()
        assert (obs is not None) == bool(golden[name + "_has_obs"][t])
        if obs is not None:
            assert sorted(o.pairx for o in obs) == np.nonzero(golden[name + "_observed"][t])[0].tolist()
        buf = fe.mic_pair_tdoa()
        assert sorted((a, b) for a in buf for b in buf[a]) == sorted(pairs)
        assert all((buf[a][b] is None) == bool(none_ref[p]) for p, (a, b) in enumerate(pairs))
        # positions: the same float64 arithmetic on the same integers where every contributing lag is equal
        pos = fe.instantaneous_position(t)
        contributing = peaks[t, :, 1] > conf["threshold"]
        if np.all(equal[contributing]) and np.array_equal(got[:, 1] > conf["threshold"], contributing):
            d = float(np.max(np.abs(pos - golden[name + "_positions"][t])))
            worst_pos = max(worst_pos, d)
            pos_checked += 1
            assert d <= 1e-9, (t, pos, golden[name + "_positions"][t])
    print("%s: %d frames, height error/bound %.3f, left out %d of %d, lag mismatches outside them %d, positions checked %d (max diff %.2e), launches %s"
          % (label, frames, worst_h, left_out, T * P, mismatches, pos_checked, worst_pos, fe.launch_count))
    assert frames == T and mismatches == 0 and left_out <= 0.01 * T * P and pos_checked > 0
    return frames


@pytest.mark.parametrize("D,L,name,block", [(8192, 16384, "kinect_D8192", 4), (256, 512, "kinect_D256", 64)], ids=["script", "short"])
def test_front_end_over_nodes_matches_the_reference(dev, kinect_pcm, golden, D, L, name, block):
    from btk20.pytdoa import make_tdoa_front_end, FarfieldLinearArrayTDOAFeatureVector
    keep = [chain(kinect_pcm[c], D, L) for c in range(4)]
    fe = make_tdoa_front_end(array_type="linear", pair_ids=KINECT_PAIRS, spec_sources=[f for _, f in keep], fftlen=L, samplerate=FS,
                             mpos=np.array(KINECT_MPOS), energy_threshold=KINECT_CONF["energy_threshold"],
                             minimum_pairs=KINECT_CONF["minimum_pairs"], threshold=KINECT_CONF["threshold"], sspeed=SSPEED,
                             block_frames=block)
    assert isinstance(fe, FarfieldLinearArrayTDOAFeatureVector) and fe.launch_count == 0
    T = compare_with_golden(fe, golden, name, kinect_pcm, D, L, KINECT_PAIRS, KINECT_CONF, "front end over nodes D=%d L=%d" % (D, L))
    # two launches per block of frames, whatever the number of pairs; the nodes themselves launched nothing
    assert fe.launch_count == 2 * -(-T // block)
    assert all(f.launches() == 0 for _, f in keep)


def test_front_end_over_supplied_spectra_circular(dev, golden):
    from btk20.pytdoa import make_tdoa_front_end, FarfieldCircularArrayTDOAFeatureVector, PHATFeature, TDOAFeature
    pcm = golden["circ_pcm"].astype(np.float32)
    pairs = [tuple(int(v) for v in p) for p in golden["circ_pairs"]]
    D, L = 256, 512
    X = cf.spectra(pcm, D, L)[0].astype(np.complex64).astype(np.complex128)
    sources = [SpectralFrames(X[c]) for c in range(6)]
    fe = make_tdoa_front_end("circular", pairs, sources, L, FS, golden["circ_mpos"], CIRC_CONF["energy_threshold"],
                             CIRC_CONF["minimum_pairs"], CIRC_CONF["threshold"], SSPEED)
    assert isinstance(fe, FarfieldCircularArrayTDOAFeatureVector)
    T = compare_with_golden(fe, golden, "circ", pcm, D, L, pairs, CIRC_CONF, "front end over supplied spectra (circular)")
    assert fe.launch_count == T                              # one launch per frame for all 15 pairs
    from distant_speech_recognition_amd.btk20cpp import jindex_error
    with pytest.raises(jindex_error):
        fe.next(T + 3)                                       # a skipped frame number, as the nodes refuse it
    # PHATFeature.next: the float64-widened correlation; zeros(1) where gated; the peak TDOAFeature reports is its first largest
    ph = PHATFeature(sources[0], sources[1], L, CIRC_CONF["energy_threshold"])
    g = ph.next(0)
    g64 = cf.gcc(X[0, 0], X[1, 0])
    assert g.dtype == np.float64 and g.shape == (L,) and np.max(np.abs(g - g64)) <= gcc_bound(L)
    d, h = TDOAFeature(PHATFeature(sources[0], sources[1], L, CIRC_CONF["energy_threshold"]), L, FS).next(0)
    n = int(np.argmax(np.abs(g)))
    assert h == abs(g[n]) and d == float(n if n < L // 2 else n - L) * (1.0 / FS)
    quiet = PHATFeature(sources[0], sources[1], L, 1e30).next(0)
    assert quiet.shape == (1,) and quiet[0] == 0
    # microphone 5 is silent in frame 16: a zero bin, every lag NaN (not gated: microphone 0 has energy)
    nan = PHATFeature(SpectralFrames(X[0, 16:]), SpectralFrames(X[5, 16:]), L, CIRC_CONF["energy_threshold"]).next(0)
    assert nan.shape == (L,) and np.all(np.isnan(nan))


def write_wav(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(FS)
        w.writeframes(np.asarray(x, np.int16).tobytes())


def test_tool_writes_the_reference_layout(dev, kinect_pcm, golden, tmp_path):
    from tools import tdoa_estimator as tool
    paths = []
    for c in range(4):
        paths.append(str(tmp_path / ("c%d.wav" % (c + 1))))
        write_wav(paths[-1], kinect_pcm[c])
    prefix = str(tmp_path / "out" / "kinect")
    fe = tool.main(["-i"] + paths + ["-o", prefix, "-r", str(FS)])       # the default configuration: D 8192, L 16384
    assert fe.launch_count == 2                                          # 10 frames, one block
    tdoa = json.load(open(prefix + ".tdoa.json"))
    trj = json.load(open(prefix + ".trj.pos.json"))
    ave = json.load(open(prefix + ".ave.pos.json"))
    name, D, L = "kinect_D8192", 8192, 16384
    pos_ref, peaks = golden[name + "_positions"], golden[name + "_peaks"]
    frames = np.nonzero(pos_ref[:, 0] > -1e10)[0]
    assert fe is not None and list(trj) == ["positions"] and list(ave) == ["positions"]
    assert [r[0] for r in tdoa] == [t * D / FS for t in frames] == [r[0] for r in trj["positions"]]
    X = cf.spectra(kinect_pcm, D, L)[0].astype(np.complex64).astype(np.complex128)
    margin = cf.gcc_peaks(X, cf.energy(X), KINECT_PAIRS, KINECT_CONF["energy_threshold"])[2].T
    B = gcc_bound(L)
    all_equal = True
    for (stamp, buf), (_, pos), t in zip(tdoa, trj["positions"], frames):
        # {"first": {"second": delay}} with string keys, [x, null, null]
        assert sorted((int(a), int(b)) for a in buf for b in buf[a]) == sorted(KINECT_PAIRS)
        assert len(pos) == 3 and pos[1] is None and pos[2] is None
        equal = [buf[str(a)][str(b)] == peaks[t, p, 0] for p, (a, b) in enumerate(KINECT_PAIRS)]
        assert all(e or margin[t, p] <= 2 * B for p, e in enumerate(equal))
        if all(equal):
            assert abs(pos[0] - pos_ref[t, 0]) <= 1e-9
        all_equal &= all(equal)
    p = ave["positions"]
    assert len(p) == 1 and p[0][0] == 0.0 and p[0][1][1:] == [None, None]
    if all_equal:
        assert abs(p[0][1][0] - float(np.mean(pos_ref[frames, 0]))) <= 1e-9
    print("tool: %d of 10 frames with a position, all lags equal to the reference's: %s" % (len(frames), all_equal))
