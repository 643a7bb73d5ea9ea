#!/usr/bin/env python
"""Subband acoustic echo cancellation of a WAV file through the MI355X engine -- the application-level counterpart of the
reference's unit_test/test_subband_aec.py on this repo's mirror.

Same command line (-a -s -M -m -r -i observed -p played -o output -c JSON) and JSON keys: type, filter_length, beta, sigmau2,
sigmak2, snr_threshold, energy_threshold, smooth, amp4play (block filters), delta, epsilon, energy_threshold (nlms).
Types: nlms, block_kalman_filter, dtd_block_kalman_filter (the default, filter_length 36).  information_filter and
square_root_information_filter are not supported by this engine and are refused by name.
"""
import argparse
import json
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.online_beamforming import load_prototype      # noqa: E402

UNSUPPORTED = ("information_filter", "square_root_information_filter")
DEFAULT_CONF = {"type": "dtd_block_kalman_filter", "filter_length": 36, "loading": 10e-4, "sigmau2": 10e-6, "sigmak2": 5.0,
                "beta": 0.95, "snr_threshold": 0.01, "energy_threshold": 1.0E+01, "smooth": 0.95, "amp4play": 1.0}


def make_canceller(reference_afb, input_afb, aec_conf):
    """the reference script's constructor calls, keyword by keyword (unit_test/test_subband_aec.py:47-89)"""
    from distant_speech_recognition_amd.btk20.aec import (NLMSAcousticEchoCancellationFeaturePtr,
                                                          BlockKalmanFilterEchoCancellationFeaturePtr,
                                                          DTDBlockKalmanFilterEchoCancellationFeaturePtr)
    kind = aec_conf["type"].lower()
    if kind in UNSUPPORTED:
        raise KeyError("AEC type %r is not supported by this engine (supported: nlms, block_kalman_filter, "
                       "dtd_block_kalman_filter; unsupported: %s)" % (aec_conf["type"], ", ".join(UNSUPPORTED)))
    if kind == "dtd_block_kalman_filter":
        return DTDBlockKalmanFilterEchoCancellationFeaturePtr(reference_afb, input_afb,
                                                              sample_num=aec_conf.get("filter_length", 2),
                                                              beta=aec_conf.get("beta", 0.95),
                                                              sigmau2=aec_conf.get("sigmau2", 10E-4),
                                                              sigmak2=aec_conf.get("sigmak2", 5.0),
                                                              snr_threshold=aec_conf.get("snr_threshold", 0.01),
                                                              energy_threshold=aec_conf.get("energy_threshold", 100),
                                                              smooth=aec_conf.get("smooth", 0.9),
                                                              amp4play=aec_conf.get("amp4play", 1.0))
    if kind == "block_kalman_filter":
        return BlockKalmanFilterEchoCancellationFeaturePtr(reference_afb, input_afb,
                                                           sample_num=aec_conf.get("filter_length", 2),
                                                           beta=aec_conf.get("beta", 0.95),
                                                           sigmau2=aec_conf.get("sigmau2", 10E-4),
                                                           sigmak2=aec_conf.get("sigmak2", 5.0),
                                                           threshold=aec_conf.get("energy_threshold", 100.0),
                                                           amp4play=aec_conf.get("amp4play", 1.0))
    if kind == "nlms":
        return NLMSAcousticEchoCancellationFeaturePtr(reference_afb, input_afb,
                                                      delta=aec_conf.get("delta", 100.0),
                                                      epsilon=aec_conf.get("epsilon", 1.0E-04),
                                                      threshold=aec_conf.get("energy_threshold", 100.0))
    raise KeyError("Invalid AEC type {}".format(aec_conf["type"]))


def cancel_echo(h_fb, g_fb, M, m, r, input_audio_path, reference_audio_path, out_path, aec_conf, samplerate=16000, verbose=True):
    """Runs the graph of the reference script; returns the synthesis bank's output blocks as float32 [blocks][D] (what the WAV
    file holds after the conversion to 16-bit integers)."""
    from distant_speech_recognition_amd.btk20 import SampleFeaturePtr, OverSampledDFTAnalysisBankPtr, OverSampledDFTSynthesisBankPtr
    D = M // 2 ** r
    input_sample_feat = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
    reference_sample_feat = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
    input_afb = OverSampledDFTAnalysisBankPtr(input_sample_feat, prototype=h_fb, M=M, m=m, r=r, delay_compensation_type=2)
    reference_afb = OverSampledDFTAnalysisBankPtr(reference_sample_feat, prototype=h_fb, M=M, m=m, r=r, delay_compensation_type=2)
    aec = make_canceller(reference_afb, input_afb, aec_conf)
    sfb = OverSampledDFTSynthesisBankPtr(aec, prototype=g_fb, M=M, m=m, r=r, delay_compensation_type=2)
    input_sample_feat.read(input_audio_path, samplerate)
    reference_sample_feat.read(reference_audio_path, samplerate)
    d = os.path.dirname(out_path)
    if d:
        os.makedirs(d, exist_ok=True)
    wavefile = wave.open(out_path, "w")
    wavefile.setnchannels(1)
    wavefile.setsampwidth(2)
    wavefile.setframerate(int(samplerate))
    blocks = []
    for frame_no, b in enumerate(sfb):
        if verbose and frame_no % 128 == 0:
            print("%0.2f sec. processed" % (frame_no * D / samplerate))
        blk = np.array(b, np.float32)
        blocks.append(blk)
        wavefile.writeframes(np.array(blk, np.int16).tobytes())
    wavefile.close()
    return np.stack(blocks) if blocks else np.zeros((0, D), np.float32)


def main(argv=None):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proto = os.path.join(here, "tests", "golden", "prototype_M256_m4_r1.npz")
    p = argparse.ArgumentParser(description="subband acoustic echo cancellation on the MI355X engine")
    p.add_argument("-a", dest="analysis_filter_path", default=proto, help="analysis filter prototype file")
    p.add_argument("-s", dest="synthesis_filter_path", default=proto, help="synthesis filter prototype file")
    p.add_argument("-M", dest="M", default=256, type=int, help="no. of subbands")
    p.add_argument("-m", dest="m", default=4, type=int, help="Prototype filter length factor")
    p.add_argument("-r", dest="r", default=1, type=int, help="Decimation factor")
    p.add_argument("-i", dest="input_audio_path", default="data/speech_and_reverb_lt.wav", help="observation audio file")
    p.add_argument("-o", dest="out_path", default="out/aec_output.wav", help="output audio file")
    p.add_argument("-p", dest="reference_audio_path", default="data/lt.wav", help="reference audio file")
    p.add_argument("-c", dest="aec_conf_path", default=None, help="JSON path for AEC configuration")
    p.add_argument("-q", dest="quiet", action="store_true")
    args = p.parse_args(argv)
    aec_conf = dict(DEFAULT_CONF)
    if args.aec_conf_path is not None:
        with open(args.aec_conf_path) as fp:
            aec_conf = json.load(fp)
    if not args.quiet:
        print("AEC config.")
        print(json.dumps(aec_conf, indent=4))
        print("")
    if aec_conf.get("type", "").lower() in UNSUPPORTED:
        print("error: AEC type %r is not supported by this engine (unsupported: %s)" % (aec_conf["type"], ", ".join(UNSUPPORTED)), file=sys.stderr)
        return 2
    blocks = cancel_echo(load_prototype(args.analysis_filter_path, "h"), load_prototype(args.synthesis_filter_path, "g"),
                         args.M, args.m, args.r, args.input_audio_path, args.reference_audio_path, args.out_path, aec_conf,
                         samplerate=16000, verbose=not args.quiet)
    print("No. blocks written: %d" % len(blocks))
    return 0


if __name__ == "__main__":
    sys.exit(main())
