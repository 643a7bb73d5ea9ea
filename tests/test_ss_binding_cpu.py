"""CPU: the three single-channel enhancement nodes under the reference's import names (btk20.postfilter, postfilter/postfilter.i):
they import, accept the .i file's keywords and the legacy aliases, and refuse what the reference refuses.  Construction touches no
device (state is allocated with the first block), so the nodes are built over Python sources, as
tests/test_reference_conv_callers_resolve.py builds its chain."""
import numpy as np
import pytest


class _Src:
    def __init__(self, M, T=0):
        self.M, self.T, self.t = M, T, 0

    def size(self):
        return self.M

    def __iter__(self):
        self.t = 0
        return self

    def next(self, frame_no=-5):
        if self.t >= self.T:
            raise StopIteration
        self.t += 1
        return np.zeros(self.M, np.complex128)

    __next__ = next

    def reset(self):
        self.t = 0


def test_names_import_from_btk20_postfilter():
    import btk20.postfilter as pf
    ns = {}
    exec("from btk20.postfilter import *", ns)
    for name in ("SpectralSubtractorPtr", "WienerFilterPtr", "HighPassFilterPtr", "SpectralSubtractor", "WienerFilter", "HighPassFilter"):
        assert name in ns and name in pf.__all__, name
    assert ns["SpectralSubtractor"] is ns["SpectralSubtractorPtr"]
    from distant_speech_recognition_amd.btk20cpp import _signatures as S
    assert {"SpectralSubtractorPtr", "WienerFilterPtr", "HighPassFilterPtr"} <= set(S.CTORS)


def test_spectral_subtractor_keywords_and_aliases():
    from btk20.postfilter import SpectralSubtractorPtr
    ss = SpectralSubtractorPtr(fftLen=8, halfBandShift=False, ft=2.0, flooringV=0.01, nm="ss")
    assert ss.size() == 8 and SpectralSubtractorPtr(8).size() == 8
    ss.set_channel(chan=_Src(8), alpha=0.5)
    ss.setChannel(_Src(8))
    for snake, legacy in (("start_training", "startTraining"), ("stop_noise_subtraction", "stopNoiseSubtraction"),
                          ("start_noise_subtraction", "startNoiseSubtraction"), ("clear_noise_samples", "clearNoiseSamples"),
                          ("stop_training", "stopTraining"), ("read_noise_file", "readNoiseFile"), ("write_noise_file", "writeNoiseFile"),
                          ("set_noise_over_estimation_factor", "setNoiseOverEstimationFactor"), ("clear", "clear")):
        assert callable(getattr(ss, snake)) and callable(getattr(ss, legacy))
    from distant_speech_recognition_amd.btk20cpp import jdimension_error
    with pytest.raises(jdimension_error):
        ss.set_channel(_Src(16))                                  # a channel of another size
    with pytest.raises(jdimension_error):
        SpectralSubtractorPtr(fftLen=4096)                        # beyond the engine's M
    with pytest.raises(TypeError):
        SpectralSubtractorPtr(8, no_such_keyword=1)


def test_wiener_filter_keywords_and_refusals():
    from btk20.postfilter import WienerFilterPtr
    from distant_speech_recognition_amd.btk20cpp import jdimension_error, j_error
    w = WienerFilterPtr(targetSignal=_Src(8), noiseSignal=_Src(8), halfBandShift=False, alpha=0.5, flooringV=0.001, beta=2.0)
    assert w.size() == 8
    # postfilter.i declares the setters under their legacy names only; the class has both
    w.setNoiseAmplificationFactor(beta=1.5)
    w.startUpdatingNoisePSD(); w.stopUpdatingNoisePSD()
    w.set_noise_amplification_factor(beta=1.0); w.start_updating_noise_PSD(); w.stop_updating_noise_PSD()
    with pytest.raises(jdimension_error, match="Input block length"):
        WienerFilterPtr(_Src(8), _Src(16))
    hb = WienerFilterPtr(_Src(8, 3), _Src(8, 3), halfBandShift=True)          # accepted at construction, a j_error in next()
    with pytest.raises(j_error, match="half band shift"):
        hb.next()


def test_highpass_keywords():
    from btk20.postfilter import HighPassFilterPtr
    h = HighPassFilterPtr(output=_Src(512), cut_off_freq=150, samplerate=16000)            # the .i file's keywords
    assert h.size() == 512 and h.cutoff_bin() == 4
    assert HighPassFilterPtr(_Src(512), cutOffFreq=300.0, sampleRate=16000).cutoff_bin() == 9      # the class's own
    assert HighPassFilterPtr(_Src(512), 150, 16000, "hp").cutoff_bin() == 4
    assert HighPassFilterPtr(_Src(256), 100, 44100).cutoff_bin() == 0
    with pytest.raises(TypeError):
        HighPassFilterPtr(_Src(512), cut_off_freq=150)                                     # samplerate has no default
