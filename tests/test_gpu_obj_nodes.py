"""GPU: SNR and ItakuraSaitoMeasurePS of the C++ node layer (host/src/obj_nodes.cc, bound as btk20.objective_measure) on WAV
files the test writes: getSNR / getSNR2 against engine.snr on the decoded samples with ==, getDistance against the node chain
SampleFeature -> NormalFFTAnalysisBank iterated in Python with the closed form on its frames (bound (a) of
tests/test_gpu_obj.py), and every exception case."""
import wave

import numpy as np
import pytest

from tests import obj_closed_form as cf

pytestmark = pytest.mark.gpu

FS = 16000
N1, N2 = 5003, 4211


def _write(path, x, rate=FS):
    x = np.asarray(x, np.int16)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1 if x.ndim == 1 else x.shape[1])
        w.setsampwidth(2)
        w.setframerate(rate)
        w.writeframes(np.ascontiguousarray(x).tobytes())
    return str(path)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    rng = np.random.default_rng(11)
    d = tmp_path_factory.mktemp("objwav")
    t = np.arange(N1) / FS
    clean = np.round(6000 * np.sin(2 * np.pi * 440 * t) + rng.normal(size=N1) * 200 + 50).astype(np.int16)
    noisy = np.round(clean[:N2] * 0.8 + rng.normal(size=N2) * 900 - 30).astype(np.int16)
    other = np.round(rng.normal(size=N1) * 3000).astype(np.int16)
    return {
        "clean": _write(d / "clean.wav", clean), "noisy": _write(d / "noisy.wav", noisy),
        "stereo1": _write(d / "stereo1.wav", np.stack([other, clean], axis=1)),
        "stereo2": _write(d / "stereo2.wav", np.stack([other[:N2], noisy], axis=1)),
        "rate8k": _write(d / "rate8k.wav", noisy, 8000),
        "missing": str(d / "nothing.wav"),
        "x1": clean.astype(np.float32), "x2": noisy.astype(np.float32), "dir": d,
    }


@pytest.fixture(scope="module")
def eng(dev):
    from distant_speech_recognition_amd import engine
    return engine


def _engine_snr(eng, dev, a, b, option):
    import torch
    db, st = eng.snr(torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev), option=option)
    return db[0], st[0]


def test_names_import():
    import btk20.objective_measure as om
    ns = {}
    exec("from btk20.objective_measure import *", ns)
    assert ns["SNRPtr"] is om.SNRPtr and ns["ItakuraSaitoMeasurePSPtr"] is om.ItakuraSaitoMeasurePSPtr
    from distant_speech_recognition_amd.btk20.objective_measure import SNR, ItakuraSaitoMeasurePS
    assert SNR is om.SNRPtr and ItakuraSaitoMeasurePS is om.ItakuraSaitoMeasurePSPtr


# cfrom / to of objective_measure.cc:233-247: cfrom < 0 is 0; `to` < 0 or behind the end of either file: each file to its end
@pytest.mark.parametrize("cfrom,to", [(-1, -1), (0, -1), (100, -1), (-5, 999), (100, 4210), (100, 4211), (100, 5002), (100, 10 ** 6),
                                      (4000, 4000), (N2 - 1, -1)])
@pytest.mark.parametrize("option", [0, 5])
def test_get_snr_ranges(eng, dev, files, cfrom, to, option):
    from btk20.objective_measure import SNRPtr
    snr = SNRPtr()
    got = snr.getSNR(files["clean"], files["noisy"], option, 1, FS, cfrom, to)
    c = max(cfrom, 0)
    if to < 0 or to >= N1 or to >= N2:
        n1, n2 = N1 - c, N2 - c
    else:
        n1 = n2 = to - c + 1
    s = np.float32(1.0 / 32768.0)
    a, b = (files["x1"] * s)[c:c + n1], (files["x2"] * s)[c:c + n2]
    assert len(a) == n1 and len(b) == n2
    db, st = _engine_snr(eng, dev, a, b, option)
    assert np.float32(got) == db and np.array_equal(snr.stats(), st, equal_nan=True)


def test_get_snr_channel_and_keywords(eng, dev, files):
    from btk20.objective_measure import SNRPtr
    snr = SNRPtr()
    want = snr.getSNR(files["clean"], files["noisy"], 1)
    assert snr.getSNR(fn1=files["stereo1"], fn2=files["stereo2"], normalizationOption=1, chX=2) == want
    assert snr.getSNR(files["stereo1"], files["stereo2"], 1, chX=1) != want
    assert snr.getSNR(files["clean"], files["clean"], 0) == np.finfo(np.float32).max


@pytest.mark.parametrize("option", [0, 1, 2, 4, 8, 9])
def test_get_snr2(eng, dev, files, option):
    from btk20.objective_measure import SNRPtr
    snr = SNRPtr()
    a, b = files["x1"], files["x2"]
    keep = a.copy()
    got = snr.getSNR2(a, b, option)
    db, st = _engine_snr(eng, dev, a, b, option)
    assert np.float32(got) == db and np.array_equal(snr.stats(), st, equal_nan=True)
    assert np.array_equal(a, keep)                                   # the inputs stay as they are
    assert snr.getSNR2(original=a, enhanced=b, normalizationOption=option) == got
    want = cf.snr(a, b, option)[0]
    assert abs(float(got) - float(want)) <= 1e-4


def test_snr_exceptions(files):
    import btk20
    from btk20.objective_measure import SNRPtr
    snr = SNRPtr()
    with pytest.raises(btk20.jio_error):
        snr.getSNR(files["missing"], files["noisy"], 0)
    with pytest.raises(btk20.jio_error):
        snr.getSNR(files["clean"], files["missing"], 0)
    with pytest.raises(btk20.jconsistency_error, match="Multi-channel read is not yet supported"):
        snr.getSNR(files["clean"], files["noisy"], 0, 0)
    for chX in (2, -1):
        with pytest.raises(btk20.jconsistency_error, match="out of range"):
            snr.getSNR(files["clean"], files["noisy"], 0, chX)
    with pytest.raises(btk20.jconsistency_error):
        snr.getSNR(files["stereo1"], files["noisy"], 0, 2)           # the second file has one channel
    with pytest.raises(btk20.jio_error, match="Sampling rates"):
        snr.getSNR(files["clean"], files["rate8k"], 0)
    with pytest.raises(btk20.jio_error, match="Cannot load samples"):
        snr.getSNR(files["clean"], files["noisy"], 0, 1, FS, N2 + 1, -1)
    with pytest.raises(btk20.jdimension_error):
        snr.getSNR(files["clean"], files["noisy"], 0, 1, FS, N2, -1)  # nothing is left of the second signal
    with pytest.raises(btk20.jdimension_error):
        snr.getSNR2(files["x2"], files["x1"], 8)                      # option 8 with a shorter first signal
    with pytest.raises(btk20.jparameter_error):
        snr.getSNR2(files["x1"], files["x2"], 16)
    with pytest.raises(btk20.jdimension_error):
        snr.getSNR2(np.zeros(0, np.float32), files["x2"], 0)


@pytest.mark.parametrize("M,r,w", [(64, 1, 1), (8, 3, 0), (512, 2, 2)])
@pytest.mark.parametrize("bframe,eframe", [(0, -1), (3, 9), (5, 2)])
def test_get_distance_against_the_node_chain(files, M, r, w, bframe, eframe):
    from btk20.feature import SampleFeaturePtr
    from btk20.modulated import NormalFFTAnalysisBankPtr
    from btk20.objective_measure import ItakuraSaitoMeasurePSPtr
    isd = ItakuraSaitoMeasurePSPtr(M, r, w)
    D = M >> r
    assert isd.frameShiftLength() == D
    got = isd.getDistance(files["clean"], files["noisy"], 1, FS, bframe, eframe)
    spectra = []
    for fn in (files["clean"], files["noisy"]):
        sf = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=False)
        sf.read(fn, 0, FS, 1)
        bank = NormalFFTAnalysisBankPtr(sf, M, r, w)
        spectra.append(np.array([np.array(f) for f in bank]))
    eis, bound = cf.eis_rows(spectra[0], spectra[1])
    F = len(eis)
    assert F == len(spectra[1]) < len(spectra[0])
    lo, hi = cf.frame_range(F, bframe, eframe)
    assert isd.frames() == hi - lo
    if hi == lo:
        assert np.isnan(got) and np.isnan(isd.distance())
        return
    want = cf.is_distance(eis, bframe, eframe)
    tol = cf.fsum(bound[lo:hi]) / (hi - lo) + (-(-(hi - lo) // 256) + 12) * 2.0 ** -53 * want
    assert abs(isd.distance() - want) <= tol
    assert got == np.float32(isd.distance())
    assert isd.getDistance(fn1=files["clean"], fn2=files["noisy"], bframe=bframe, eframe=eframe) == got


def test_distance_exceptions(files):
    import btk20
    from btk20.objective_measure import ItakuraSaitoMeasurePSPtr
    isd = ItakuraSaitoMeasurePSPtr(fftLen=64, r=1, windowType=1)
    with pytest.raises(btk20.jio_error):
        isd.getDistance(files["missing"], files["noisy"])
    with pytest.raises(btk20.jconsistency_error):
        isd.getDistance(files["clean"], files["noisy"], 2)
    with pytest.raises(btk20.jconsistency_error):
        isd.getDistance(files["clean"], files["noisy"], 0)
    for M, r in ((48, 1), (4096, 1), (64, 7)):
        with pytest.raises(btk20.jparameter_error):
            ItakuraSaitoMeasurePSPtr(M, r).getDistance(files["clean"], files["noisy"])
    assert isd.getDistance(files["clean"], files["clean"]) == 0.0
