#!/usr/bin/env python
"""Batch maximum-kurtosis beamforming (MEK / NMEK) on WAV files through the MI355X engine.

The reference has the classes (lib/pybeamformer.py:1331-1860) but no script that runs them; this one follows the command line
(-a -s -M -m -r -i -o -c) and JSON conventions of tools/sos_batch_beamforming.py:
  array_type, microphone_positions, target.positions[0][1] (look direction), target.vad_label [[start, end], ...],
  beamformer.type in {mek, nmek}; beamformer.upper in {ds, sd} (delay-and-sum or super-directive upper branch, sd takes mu);
  alpha, beta, gamma, Nc, energy_threshold, R; maxiter, gtol, mindelta, max_halvings, armijo_c1 of the optimiser;
  module in {device, scipy}; input_scale: one factor on the samples before analysis, taken out again after synthesis (alpha, gtol
  and mindelta mean something only when the beamformer output power is of order 1).
--report FILE.npz stores ||g0|| per bin and the upper-branch and final outputs on the adaptation frames.
"""
import argparse
import json
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.online_beamforming import load_prototype, SSPEED      # noqa: E402


def read_wav(path):
    w = wave.open(path, "rb")
    assert w.getnchannels() == 1 and w.getsampwidth() == 2, "%s: one channel of 16-bit PCM expected" % path
    x = np.frombuffer(w.readframes(w.getnframes()), np.int16).astype(np.float64)
    rate = w.getframerate()
    w.close()
    return x, rate


def hos_batch_beamforming(h_fb, g_fb, D, M, m, r, input_audio_paths, out_path, ap_conf, samplerate, verbose=True, report=None):
    from distant_speech_recognition_amd.btk20 import (SampleFeaturePtr, OverSampledDFTAnalysisBankPtr,
                                                      OverSampledDFTSynthesisBankPtr, PyVectorComplexFeatureStreamPtr)
    from distant_speech_recognition_amd import pybeamformer as pb
    bf_conf = ap_conf["beamformer"]
    scale = float(bf_conf.get("input_scale", 1.0))
    samples = [read_wav(p)[0] * scale for p in input_audio_paths]
    sample_feats, afbs = [], []
    for x in samples:
        sf = SampleFeaturePtr(block_len=D, shift_len=D, pad_zeros=True)
        sf.setSamples(x, int(samplerate))
        afbs.append(OverSampledDFTAnalysisBankPtr(sf, prototype=h_fb, M=M, m=m, r=r, delay_compensation_type=2))
        sample_feats.append(sf)

    delays = pb.calc_delays(ap_conf["array_type"], ap_conf["microphone_positions"], ap_conf["target"]["positions"][0][1], sspeed=SSPEED)
    upper_type = bf_conf.get("upper", "ds")
    if upper_type == "ds":
        upper = pb.SubbandGSCBeamformer(afbs, Nc=1)
        upper._wqH = np.conjugate(np.stack([pb.calc_array_manifold_f(k, M, samplerate, delays, False) for k in range(M // 2 + 1)]))
    elif upper_type == "sd":
        upper = pb.SubbandMVDRBeamformer(afbs, Nc=1)
        upper.calc_sd_beamformer_weights(samplerate, delays, ap_conf["microphone_positions"], sspeed=SSPEED, mu=bf_conf.get("mu", 0.01),
                                         update_active_weights=False)
    else:
        raise KeyError("Invalid upper beamformer type: {}".format(upper_type))

    kw = dict(Nc=bf_conf.get("Nc", 1), alpha=bf_conf.get("alpha", 0.01), beta=bf_conf.get("beta", 3.0))
    if bf_conf["type"] == "nmek":
        beamformer = pb.SubbandNMEKBeamformer([upper], gamma=bf_conf.get("gamma", -1.0), **kw)
    elif bf_conf["type"] == "mek":
        beamformer = pb.SubbandMEKBeamformer([upper], **kw)
    else:
        raise KeyError("Invalid HOS beamformer type: {}".format(bf_conf["type"]))

    obs = beamformer.accum_observations(samplerate, target_labs=[tuple(l) for l in ap_conf["target"]["vad_label"]],
                                        energy_threshold=bf_conf.get("energy_threshold", 10) * scale ** 2, R=bf_conf.get("R", 1))
    if verbose:
        print("%d frames accumulated" % len(obs))
    options = {key: bf_conf[key] for key in ("maxiter", "gtol", "mindelta", "max_halvings", "armijo_c1", "tolerance", "eps") if key in bf_conf}
    module = bf_conf.get("module", "device")
    if report:
        beamformer.calc_upper_beamformer_weights()
        _, g0, _ = beamformer._eval(None)
        g0norm = np.linalg.norm(g0.cpu().numpy(), axis=1)
    beamformer.estimate_active_weights(module=module, solver=bf_conf.get("solver", "CG"), options=options)
    if report:
        src = beamformer._srcX
        np.savez(report, g0norm=g0norm, Y_upper=np.einsum("kn,tkn->tk", beamformer._wuH[src][: M // 2 + 1], obs),
                 Y_hos=np.einsum("kn,tkn->tk", beamformer._woH[src], obs), selected=beamformer._selected_frames)

    for sf, x in zip(sample_feats, samples):                      # reload the data (reset the feature pointer)
        sf.setSamples(x, int(samplerate))
    sfb = OverSampledDFTSynthesisBankPtr(PyVectorComplexFeatureStreamPtr(beamformer), prototype=g_fb, M=M, m=m, r=r,
                                         delay_compensation_type=2)
    out_dir = os.path.dirname(out_path)
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)
    wavefile = wave.open(out_path, "w")
    wavefile.setnchannels(1)
    wavefile.setsampwidth(2)
    wavefile.setframerate(int(samplerate))
    total_energy, frame_no = 0.0, -1
    for frame_no, buf in enumerate(sfb):
        buf = np.array(buf) / scale
        if verbose and frame_no % 128 == 0:
            print("%0.2f sec. processed" % (frame_no * D / float(samplerate)))
        total_energy += float(np.inner(buf, buf))
        wavefile.writeframes(np.clip(buf, -32768, 32767).astype(np.int16).tobytes())
    wavefile.close()
    return total_energy, frame_no


def main(argv=None):
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    proto = os.path.join(here, "tests", "golden", "prototype_M256_m4_r1.npz")
    p = argparse.ArgumentParser(description="batch maximum-kurtosis beamforming (MEK, NMEK) on the MI355X engine")
    p.add_argument("-a", dest="analysis_filter_path", default=proto)
    p.add_argument("-s", dest="synthesis_filter_path", default=proto)
    p.add_argument("-M", dest="M", default=256, type=int)
    p.add_argument("-m", dest="m", default=4, type=int)
    p.add_argument("-r", dest="r", default=1, type=int)
    p.add_argument("-i", dest="input_audio_paths", nargs="+", required=True)
    p.add_argument("-o", dest="out_path", default="out/beamformed.wav")
    p.add_argument("-c", dest="ap_conf_path", required=True)
    p.add_argument("-q", dest="quiet", action="store_true")
    p.add_argument("--report", dest="report", default=None)
    args = p.parse_args(argv)
    with open(args.ap_conf_path) as fp:
        ap_conf = json.load(fp)
    D = args.M // 2 ** args.r
    total_energy, frame_no = hos_batch_beamforming(load_prototype(args.analysis_filter_path, "h"),
                                                   load_prototype(args.synthesis_filter_path, "g"), D, args.M, args.m, args.r,
                                                   args.input_audio_paths, args.out_path, ap_conf, 16000, verbose=not args.quiet,
                                                   report=args.report)
    print("Avg. output power: %f" % (total_energy / max(frame_no + 1, 1)))
    print("No. frames processed: %d" % (frame_no + 1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
