"""GPU: OverlapAddPtr / OverlapSavePtr of btk20.convolution and tools/correlate.py, on a 3 000-sample int16 WAV the test writes.

Over a SampleFeaturePtr the nodes launch the kernel engine.fir_convolve / engine.conv_blocks launch, with the node's own plan, on
the blocks laid end to end, and every launch ends on a tile boundary: the frames are compared with the engine's bit for bit, for
every block size.  What the engine computes is held to its bound in tests/test_gpu_conv.py; over a Python source (one launch per
block) the frames are held to that bound against the float64 direct sum directly."""
import importlib.util
import os
import struct
import wave

import numpy as np
import pytest

from tests import conv_closed_form as cf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = 3000


def write_wav(path, x):
    with wave.open(path, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.asarray(x, np.int16).tobytes())


@pytest.fixture(scope="module")
def wav(tmp_path_factory):
    rng = np.random.default_rng(21)
    x = np.round(rng.normal(scale=3000.0, size=NS)).clip(-32768, 32767).astype(np.int16)
    path = str(tmp_path_factory.mktemp("conv") / "utt.wav")
    write_wav(path, x)
    return path, x.astype(np.float32)


def served(x, L, shift):
    """the blocks of SampleFeaturePtr(block_len=L, shift_len=shift, pad_zeros=True), [T][L]"""
    out, cur = [], 0
    while cur < len(x):
        b = np.zeros(L, np.float32)
        b[:len(x[cur:cur + L])] = x[cur:cur + L]
        out.append(b)
        cur += shift
    return np.stack(out)


def source(path, L, shift):
    from btk20.feature import SampleFeaturePtr
    s = SampleFeaturePtr(block_len=L, shift_len=shift, pad_zeros=True)
    s.read(path)
    return s


def drain(node):
    return np.stack([np.array(v) for v in node])


def taps(seed, P):
    rng = np.random.default_rng(seed)
    return (rng.normal(size=P) * np.exp(-3.0 * np.arange(P) / P)).astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("L,shift,P", [(100, 100, 157),      # P - 1 > L: the kept tail spans more than a block
                                       (128, 64, 40),        # overlapping source blocks, filtered end to end as served
                                       (500, 500, 9000)])    # two partitions
def test_overlap_add_over_samples_is_fir_convolve(dev, wav, L, shift, P):
    import torch
    from btk20.convolution import OverlapAddPtr
    from distant_speech_recognition_amd import engine as eng
    h = taps(L + P, P)
    blocks = served(wav[1], L, shift)
    T = blocks.shape[0]
    got = {}
    for bf in (1, 7, 64):
        node = OverlapAddPtr(source(wav[0], L, shift), h, block_frames=bf)
        got[bf] = drain(node)
        assert got[bf].dtype == np.float32 and got[bf].shape == (T, L)
        assert node.launches() == -(-T // bf) and node.block_frames() == bf
    filt = eng.conv_filter(torch.from_numpy(h[None]).to(dev), plan=node.plan())
    want = eng.fir_convolve(torch.from_numpy(blocks.reshape(1, -1)).to(dev), filt).cpu().numpy().reshape(T, L)
    for bf in (1, 7, 64):
        assert np.array_equal(got[bf], want), bf


@pytest.mark.parametrize("shift", [256, 100])
def test_overlap_save_over_samples_is_conv_blocks(dev, wav, shift):
    import torch
    from btk20.convolution import OverlapSavePtr
    from distant_speech_recognition_amd import engine as eng
    L, P = 256, 17
    h = taps(3, P)
    blocks = served(wav[1], L, shift)
    T = blocks.shape[0]
    got = {}
    for bf in (1, 7, 64):
        node = OverlapSavePtr(source(wav[0], L, shift), h, block_frames=bf)
        got[bf] = drain(node)
        assert got[bf].shape == (T, L - P) and node.launches() == -(-T // bf)
    x = np.zeros((T - 1) * shift + L, np.float32)
    x[:NS] = wav[1]
    filt = eng.conv_filter(torch.from_numpy(h[None]).to(dev), plan=node.plan())
    want = eng.conv_blocks(torch.from_numpy(x[None]).to(dev), filt, L, shift).cpu().numpy()[0, 0]
    for bf in (1, 7, 64):
        assert np.array_equal(got[bf], want), bf


class PySource:
    """a Python float source: size() / __iter__ / next() / reset()"""

    def __init__(self, blocks):
        self.blocks, self.i = blocks, 0

    def size(self):
        return self.blocks.shape[1]

    def __iter__(self):
        self.i = 0
        return self

    def reset(self):
        self.i = 0

    def next(self):
        if self.i >= len(self.blocks):
            raise StopIteration
        self.i += 1
        return self.blocks[self.i - 1]

    __next__ = next


def test_nodes_over_a_python_source_are_within_the_bound(dev, wav):
    from btk20.convolution import OverlapAddPtr, OverlapSavePtr
    L, P = 256, 157
    h = taps(5, P)
    blocks = served(wav[1], L, 200)
    T = blocks.shape[0]
    node = OverlapAddPtr(PySource(blocks), h)
    got = drain(node)
    assert got.shape == (T, L) and node.launches() == T     # the source hands out one block at a time
    stream = np.concatenate([np.zeros(P - 1, np.float32), blocks.reshape(-1)])
    ref = cf.direct(stream, h, T * L, hist=P - 1)
    worst = 0.0
    for t in range(T):                                       # launch t: the block behind the P - 1 samples kept so far
        call = stream[t * L:t * L + P - 1 + L]
        tiles = cf.apply_tile_bounds(call, h, node.plan(), L, hist=P - 1)
        worst = max(worst, cf.worst_ratio(got[t], ref[t * L:(t + 1) * L], tiles))
    print("OverlapAdd over a Python source: largest tile error / bound = %.2e" % worst)
    assert worst <= 1.0
    # and the reference's own arithmetic is as close to the same sums as its float32 running sum allows
    rest = cf.overlap_add_restated(blocks, h).reshape(-1)
    assert np.all(np.abs(rest - ref) <= cf.running_sum_bound(blocks, stream[P - 1:], h, T * L))

    P = 17
    h = taps(6, P)
    node = OverlapSavePtr(PySource(blocks), h)
    got = drain(node)
    assert got.shape == (T, L - P) and node.launches() == T
    worst = 0.0
    for t in range(T):
        ref = cf.blocks_direct(blocks[t], h, L, L)[0]
        worst = max(worst, float(np.sqrt(np.sum((got[t] - ref) ** 2))) / cf.blocks_tile_bounds(blocks[t], h, L, L)[0])
    print("OverlapSave over a Python source: largest block error / bound = %.2e" % worst)
    assert worst <= 1.0


def test_next_protocol(dev, wav):
    from btk20.convolution import OverlapAddPtr, OverlapSavePtr
    from distant_speech_recognition_amd.btk20cpp import jindex_error
    for cls in (OverlapAddPtr, OverlapSavePtr):
        src = source(wav[0], 256, 256)
        node = cls(src, taps(7, 40), block_frames=5)
        T = -(-NS // 256)
        v0 = np.array(node.next(0))
        assert node.frame_no() == 0 and np.array_equal(np.array(node.next(0)), v0)     # the same number: the cached vector
        assert node.launches() == 1
        with pytest.raises(jindex_error):
            node.next(2)                                     # a skipped number
        v1 = np.array(node.next(1))
        assert node.frame_no() == 1 and not np.array_equal(v0, v1)
        rest = [np.array(node.next()) for _ in range(T - 2)]
        with pytest.raises(StopIteration):
            node.next()
        first = np.stack([v0, v1] + rest)
        src.read(wav[0])                                     # a SampleFeature drops its samples at the end of a pass
        second = drain(node)                                 # __iter__ resets: a second pass, the buffer zeroed
        assert second.shape == first.shape and np.array_equal(first, second)
        assert node.launches() == 2 * -(-T // 5)


def load_tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def read_float_wav(path):
    b = open(path, "rb").read()
    assert b[:4] == b"RIFF" and b[8:12] == b"WAVE" and struct.unpack("<I", b[4:8])[0] == len(b) - 8
    pos, fmt, data = 12, None, None
    while pos < len(b):
        tag, n = b[pos:pos + 4], struct.unpack("<I", b[pos + 4:pos + 8])[0]
        if tag == b"fmt ":
            fmt = struct.unpack("<HHIIHH", b[pos + 8:pos + 24])
        elif tag == b"data":
            data = np.frombuffer(b[pos + 8:pos + 8 + n], "<f4")
        pos += 8 + n + (n & 1)
    assert fmt == (3, 1, 16000, 64000, 4, 32)                # IEEE float, one channel, 16 kHz
    return data


def test_correlate_tool_recovers_a_three_tap_response(dev, tmp_path):
    M = 256
    n = np.arange(M)
    chirp = np.round(8000.0 * np.sin(2 * np.pi * (0.02 * n + 0.5 * (0.4 / M) * n * n))).astype(np.int16)
    delays, gains = (10, 90, 200), (1.0, -0.5, 0.25)
    rec = np.zeros(5 * M + 70)
    for d, g in zip(delays, gains):
        rec[d:d + M] += g * chirp
    rec = np.round(rec).astype(np.int16)
    cpath, rpath, opath = (str(tmp_path / f) for f in ("chirp.wav", "rec.wav", "out.wav"))
    write_wav(cpath, chirp)
    write_wav(rpath, rec)
    tool = load_tool("correlate")
    T = tool.main(["-c", cpath, "-i", rpath, "-o", opath, "-M", str(M)])
    assert T == -(-len(rec) // M) == 6
    y = read_float_wav(opath)
    assert y.shape == (T * M,)
    x = np.zeros(T * M, np.float32)
    x[:len(rec)] = rec
    h = chirp[::-1].astype(np.float64)
    ref = cf.direct(x, h)
    _, node, _ = tool.build_chain(cpath, M)
    worst = cf.worst_ratio(y, ref, cf.apply_tile_bounds(x, h, node.plan(), T * M))
    print("correlate: largest tile error / bound = %.2e" % worst)
    assert worst <= 1.0

    def peaks(v, count=3, guard=8):
        v, found = np.abs(v).copy(), []
        for _ in range(count):
            i = int(np.argmax(v))
            found.append(i)
            v[max(i - guard, 0):i + guard + 1] = 0
        return sorted(found)

    want = [M - 1 + d for d in delays]                       # the correlation is delayed by M - 1
    assert peaks(ref) == want and peaks(y) == want
    e0 = float(np.sum(chirp.astype(np.float64) ** 2))
    for d, g in zip(delays, gains):                          # a tap's height: its gain times the chirp's energy, sidelobes aside
        assert abs(y[M - 1 + d] / e0 - g) < 0.05
    # convolve mode filters with the block as it is
    tool.main(["-c", cpath, "-i", rpath, "-o", opath, "-M", str(M), "--mode", "convolve", "--block-frames", "2"])
    y2 = read_float_wav(opath)
    h2 = chirp.astype(np.float64)
    assert cf.worst_ratio(y2, cf.direct(x, h2), cf.apply_tile_bounds(x, h2, node.plan(), T * M)) <= 1.0
