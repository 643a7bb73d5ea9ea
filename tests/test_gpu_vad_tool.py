"""GPU: tools/vad_segments.py on a synthetic four-channel recording (noise, tone burst, noise) written by the test: one segment
that covers the burst, as a `vad_label` list with which SubbandSMIMVDRBeamformer.accu_stats_from_label counts exactly the
frames outside the segment as noise."""
import json
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M, m, r, D, FS = 256, 4, 1, 128, 16000
FRAMES, BURST = 260, (100, 180)                       # the burst fills frames 100 .. 179


@pytest.fixture(scope="module")
def recording(tmp_path_factory):
    rng = np.random.default_rng(7)
    d = tmp_path_factory.mktemp("vadwav")
    n = FRAMES * D
    t = np.arange(n) / FS
    gate = np.zeros(n)
    gate[BURST[0] * D:BURST[1] * D] = 1.0
    paths = []
    for c in range(4):
        # the tone is loudest on channel 0 (the target's microphone), so that the power metrics see it there
        x = rng.normal(size=n) * 30.0 + gate * (6000.0 if c == 0 else 1500.0) * np.sin(2 * np.pi * 700.0 * t + 0.3 * c)
        p = str(d / ("ch%d.wav" % c))
        with wave.open(p, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(FS)
            w.writeframes(np.round(x).astype(np.int16).tobytes())
        paths.append(p)
    return paths, d


def _noise_frames(paths, proto256, labels):
    from distant_speech_recognition_amd.btk20 import SampleFeaturePtr, OverSampledDFTAnalysisBankPtr
    from distant_speech_recognition_amd.pybeamformer import SubbandSMIMVDRBeamformer
    afbs = []
    for p in paths:
        sf = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
        sf.read(p, FS)
        afbs.append(OverSampledDFTAnalysisBankPtr(sf, prototype=proto256[0], M=M, m=m, r=r, delay_compensation_type=2))
    bf = SubbandSMIMVDRBeamformer(afbs, Nc=1)
    bf.accu_stats_from_label(FS, target_labs=labels, energy_threshold=-1.0)     # every frame passes the energy gate
    return int(round(float(bf._noise_frame_num.item())))


@pytest.mark.parametrize("metric", [["energy"], ["normalized"], ["energy", "normalized", "tsps"]])
def test_tool_finds_the_burst_and_the_beamformer_counts_the_rest(dev, proto256, recording, metric):
    from tools import vad_segments as tool
    paths, d = recording
    out = str(d / ("label_%s.json" % "_".join(metric)))
    # energy: the window starts at 1e6, between the noise's frame energy (1.2e5) and the burst's (2e9), and with threshold 0.95
    # the 191st smallest entry decides: it stays 1e6 for the 260 frames (171 shifts).  E0 = 1.6: a normalised-energy share above
    # 0.4 (noise: about 0.25, below 0.35; burst: 6000 / 10500 = 0.57)
    argv = ["-i"] + paths + ["-o", out, "-M", str(M), "-r", str(r), "--metric"] + metric + [
        "-q", "--initial-energy", "1e6", "--energy-threshold", "0.95", "--e0", "1.6"]
    conf = tool.main(argv)
    with open(out) as fp:
        assert json.load(fp) == json.loads(json.dumps(conf))
    segs, labels = conf["segments"], conf["target"]["vad_label"]
    assert conf["frames"] == FRAMES and len(segs) == 1 and len(labels) == 1
    a, b = segs[0]
    # the onset is the burst's first frame; the hangover tail (10 misses) closes it at most a frame after the burst's last + 10
    assert a <= BURST[0] and a >= BURST[0] - 1 and BURST[1] <= b <= BURST[1] + 11
    total = _noise_frames(paths, proto256, [])
    assert total >= FRAMES
    assert _noise_frames(paths, proto256, labels) == total - (b - a)
