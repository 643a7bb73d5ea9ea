"""CPU: the closed forms of the objective measures (tests/obj_closed_form.py) against themselves.

Stated deviation: the reference adds its sums in running floats, the engine in float64.  On channels 0 and 1 of
tests/golden/kinect_4ch_16k.npz (78064 and 70000 samples) the reference's own arithmetic, restated loop for loop in float32,
lies this far from the closed form -- measured on the build machine, asserted with the project's margin of 4:
    SNR, all 16 options:            at most 4.28e-4 dB   (options 3, 7, 11, 15)
    Itakura-Saito distance:         at most 8.21e-7 relative (M = 64, r = 1; M = 512, r = 1; whole signal and frames 10 .. 200)"""
import numpy as np
import pytest

from tests import obj_closed_form as cf

SNR_DEVIATION_DB = 4.28e-4
IS_DEVIATION_REL = 8.21e-7
F32 = np.float32


@pytest.fixture(scope="module")
def two_channels(kinect_pcm):
    return kinect_pcm[0].copy(), kinect_pcm[1][:70000].copy()


def test_float32_restatement_of_the_snr_lies_within_the_stated_deviation(two_channels):
    x1, x2 = two_channels
    worst = 0.0
    for option in range(16):
        ref, want = cf.calc_snr_f32(x1, x2, option), cf.snr(x1, x2, option)[0]
        d = abs(float(ref) - float(want))
        print("option %2d: float32 restatement %.6f dB, closed form %.6f dB, apart %.3e dB" % (option, ref, want, d))
        worst = max(worst, d)
    print("largest: %.3e dB" % worst)
    assert worst <= 4 * SNR_DEVIATION_DB


def test_float32_restatement_of_the_distance_lies_within_the_stated_deviation(two_channels):
    x1, x2 = two_channels
    worst = 0.0
    for M, r in ((64, 1), (512, 1)):
        X1, X2 = cf.stft64(x1, M, r), cf.stft64(x2, M, r)
        eis, _ = cf.eis_rows(X1, X2)
        for b, e in ((0, -1), (10, 200)):
            ref, want = cf.calc_is_f32(X1, X2, b, e), cf.is_distance(eis, b, e)
            d = abs(float(ref) - want) / want
            print("M=%d r=%d frames %d..%d: float32 restatement %.6f, closed form %.6f, apart %.3e" % (M, r, b, e, ref, want, d))
            worst = max(worst, d)
    print("largest: %.3e" % worst)
    assert worst <= 4 * IS_DEVIATION_REL


def test_option_precedence():
    rng = np.random.default_rng(0)
    x1 = (rng.normal(size=500) * 1000 + 300).astype(F32)
    x2 = (0.5 * x1 + rng.normal(size=400 + 100) * 100 - 200).astype(F32)[:400]
    base = {o: cf.snr_scales(x1, x2, o) for o in range(16)}
    for o in range(16):
        mu1, mu2, a1, a2 = base[o]
        # bit 1 decides the means alone
        assert (mu1 != 0 and mu2 != 0) == bool(o & 1)
        # 2 over 4 over 8
        eff = 2 if o & 2 else 4 if o & 4 else 8 if o & 8 else 0
        assert (a1, a2) == base[eff | (o & 1)][2:]
        assert (a1 != 1) == (eff == 2)
        assert (a2 != 1) == (eff != 0)
        assert cf.calc_snr_f32(x1, x2, o) == cf.calc_snr_f32(x1, x2, eff | (o & 1))
    assert len({base[o][3] for o in (2, 4, 8)}) == 3
    with pytest.raises(ValueError):
        cf.snr_scales(x2, x1, 8)


def test_both_tail_rules():
    x1 = np.array([3, -4, 5, 6, 7], F32)
    x2 = np.array([1, -4, 2], F32)
    # the clean signal is the longer one: its tail goes into both sums
    s, e = cf.snr_sums(x1, x2, 0, 0, 1, 1)
    assert s == 9 + 16 + 25 + 36 + 49 and e == 4 + 0 + 9 + 36 + 49
    # the enhanced signal is the longer one: ITS tail goes into both sums, into `sum` too
    s, e = cf.snr_sums(x2, x1, 0, 0, 1, 1)
    assert s == 1 + 16 + 4 + 36 + 49 and e == 4 + 0 + 9 + 36 + 49
    assert cf.calc_snr_f32(x2, x1, 0) == F32(10) * np.log10(F32(106) / F32(98))
    # the tail is scaled like the rest
    s, e = cf.snr_sums(x2, x1, 0, 0, 1, 2)
    assert s == 1 + 16 + 4 + 4 * (36 + 49) and e == (1 - 6) ** 2 + (-4 + 8) ** 2 + (2 - 10) ** 2 + 4 * (36 + 49)


def test_signed_maximum():
    x1 = np.array([-5, -20000, -7, -3], F32)
    x2 = np.array([100, -30000, 50], F32)
    _, _, a1, a2 = cf.snr_scales(x1, x2, 2)
    assert a1 == F32(1) / F32(-3) and a2 == F32(1) / F32(100)            # not 1 / 20000, not 1 / 30000
    assert cf.snr_scales(np.full(3, -20000, F32), x2, 2)[2] == F32(1) / F32(-10000)      # the initial value stays
    # after the mean went: the maximum of the centred samples
    mu1, _, a1, _ = cf.snr_scales(x1, x2, 3)
    assert a1 == F32(1) / (x1 - mu1).astype(F32).max()


def test_identical_signals_and_segments():
    x = np.arange(1, 301, dtype=F32)
    assert cf.snr(x, x, 5)[0] == cf.FLT_MAX and cf.calc_snr_f32(x, x, 0) == cf.FLT_MAX
    y = x.copy()
    y[100:200] = 0
    rows = cf.segment_rows(x, y, 0, 0, 1, 1, 100)
    assert rows.shape == (3, 2) and rows[0, 1] == 0 and rows[1, 0] == rows[1, 1]
    assert cf.segmental_snr(rows) == (35.0 + 0.0 + 35.0) / 3
    assert cf.segmental_snr(cf.segment_rows(y, x, 0, 0, 1, 1, 100)) == (35.0 - 10.0 + 35.0) / 3      # sum_b = 0: lo
    assert np.isnan(cf.segmental_snr(cf.segment_rows(x, y, 0, 0, 1, 1, 301)))
    assert cf.segment_rows(x, y[:250], 0, 0, 1, 1, 100).shape == (2, 2)                              # whole segments below nmin


def test_frame_range_logic():
    eis = np.arange(10, dtype=np.float64)
    assert cf.is_distance(eis, 0, -1) == 4.5
    assert cf.is_distance(eis, 3, 3) == 3.0
    assert np.isnan(cf.is_distance(eis, 5, 2))
    assert cf.is_distance(eis, 7, 1000) == 8.0
    assert np.isnan(cf.is_distance(eis, 10, -1))
    assert cf.frame_range(10, 2, 5) == (2, 6)
    X = cf.stft64(np.arange(1, 100, dtype=F32), 16, 1)
    Y = cf.stft64(np.arange(1, 60, dtype=F32) * 2, 16, 1)
    assert len(X) == cf.num_frames(99, 8) == 14 and len(Y) == 9
    e, bound = cf.eis_rows(X, Y)
    assert len(e) == 9                                                   # the shorter stream ends the loop
    for b, en in ((0, -1), (3, 3), (2, 100)):
        assert abs(float(cf.calc_is_f32(X, Y, b, en)) - cf.is_distance(e, b, en)) <= 1e-5 * cf.is_distance(e, b, en)
    assert np.isnan(cf.calc_is_f32(X, Y, 5, 2))
    # a skipped bin stays in the divisor
    Z = Y.copy()
    Z[4, 1:4] = 0
    ez, _ = cf.eis_rows(X, Z)
    r = (np.abs(X[4, 4:9]) ** 2).astype(F32) / (np.abs(Y[4, 4:9]) ** 2).astype(F32)
    assert abs(ez[4] - float(np.sum(r.astype(np.float64) - np.log(r.astype(np.float64)) - 1)) / 8) <= 1e-12 * ez[4]


def test_keyword_table_has_the_objective_measures():
    from distant_speech_recognition_amd.btk20cpp import _signatures as S
    assert S.CTORS["SNRPtr"] == []
    assert S.CTORS["ItakuraSaitoMeasurePSPtr"] == [("fftLen", "required"), ("r", 1), ("windowType", 1), ("nm", "ItakuraSaitoMeasurePS")]
    assert S.METHODS["SNRPtr"]["getSNR"] == [("fn1", "required"), ("fn2", "required"), ("normalizationOption", "required"), ("chX", 1),
                                             ("samplerate", 16000), ("cfrom", -1), ("to", -1)]
    assert [p for p, _ in S.METHODS["SNRPtr"]["getSNR2"]] == ["original", "enhanced", "normalizationOption"]
    assert S.METHODS["ItakuraSaitoMeasurePSPtr"]["getDistance"] == [("fn1", "required"), ("fn2", "required"), ("chX", 1),
                                                                    ("samplerate", 16000), ("bframe", 0), ("eframe", -1)]
