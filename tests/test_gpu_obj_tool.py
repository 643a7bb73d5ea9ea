"""GPU: tools/quality_assessment.py on a tone-plus-noise recording and two degraded copies written by the test: the values are
the classes' values, the noisier copy scores a lower SNR and a larger Itakura-Saito distance, and -n, -b / -e and --segmental
reach the measures."""
import wave

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS, N = 16000, 16000


@pytest.fixture(scope="module")
def recordings(tmp_path_factory):
    rng = np.random.default_rng(3)
    d = tmp_path_factory.mktemp("qawav")
    t = np.arange(N) / FS
    clean = 5000 * np.sin(2 * np.pi * 500 * t) * (1 + 0.5 * np.sin(2 * np.pi * 3 * t)) + rng.normal(size=N) * 100 + 40
    noise = rng.normal(size=N)
    out = {}
    for name, x in (("clean", clean), ("good", clean + 150 * noise), ("bad", clean + 1500 * noise)):
        p = str(d / (name + ".wav"))
        with wave.open(p, "wb") as w:
            w.setnchannels(1)
            w.setsampwidth(2)
            w.setframerate(FS)
            w.writeframes(np.round(x).astype(np.int16).tobytes())
        out[name] = p
    return out


def test_values_are_the_classes_values(dev, recordings, capsys):
    from btk20.objective_measure import SNRPtr, ItakuraSaitoMeasurePSPtr
    from tools import quality_assessment as tool
    out = tool.main(["-1", recordings["clean"], "-2", recordings["bad"]])
    printed = capsys.readouterr().out.split("\n")
    assert printed[0] == "SNR %f" % out["snr"] and printed[1] == "IS  %f" % out["is"]
    assert out["snr"] == SNRPtr().getSNR(recordings["clean"], recordings["bad"], 0, 1, 16000, 0, -1)
    assert out["is"] == ItakuraSaitoMeasurePSPtr(64, 1, 1).getDistance(recordings["clean"], recordings["bad"], 1, 16000, 0, -1)
    assert "segmental" not in out


def test_noisier_copy_scores_worse(dev, recordings):
    from tools import quality_assessment as tool
    good = tool.main(["-1", recordings["clean"], "-2", recordings["good"], "-q", "--segmental", "256"])
    bad = tool.main(["-1", recordings["clean"], "-2", recordings["bad"], "-q", "--segmental", "256"])
    assert bad["snr"] < good["snr"] - 15 and bad["is"] > good["is"] > 0
    assert -10.0 <= bad["segmental"] < good["segmental"] <= 35.0
    # 150 against 1500 noise on the same signal: 20 dB apart
    assert abs((good["snr"] - bad["snr"]) - 20.0) < 0.5


def test_options_reach_the_measures(dev, recordings):
    from btk20.objective_measure import SNRPtr, ItakuraSaitoMeasurePSPtr
    from tools import quality_assessment as tool
    c, b = recordings["clean"], recordings["bad"]
    base = tool.main(["-1", c, "-2", b, "-q"])
    n1 = tool.main(["-1", c, "-2", b, "-q", "-n", "1"])
    assert n1["snr"] == SNRPtr().getSNR(c, b, 1, 1, 16000, 0, -1) and n1["snr"] != base["snr"] and n1["is"] == base["is"]
    cut = tool.main(["-1", c, "-2", b, "-q", "-b", "2048", "-e", "8191", "-M", "256", "-r", "2", "-w", "2", "--segmental", "100"])
    assert cut["snr"] == SNRPtr().getSNR(c, b, 0, 1, 16000, 2048, 8191)
    assert cut["is"] == ItakuraSaitoMeasurePSPtr(256, 2, 2).getDistance(c, b, 1, 16000, 2048 // 64, 8191 // 64)
    assert cut["snr"] != base["snr"] and cut["is"] != base["is"]
    assert tool.main(["-1", c, "-2", b, "-q", "-b", "0", "-e", "-1"]) == base                # -e below 0: to the end, for both
    whole = tool.main(["-1", c, "-2", b, "-q", "-M", "256", "-r", "2", "-w", "2", "--segmental", "100", "--seg-hi", "5"])
    assert whole["segmental"] != cut["segmental"] and whole["segmental"] <= 5.0
