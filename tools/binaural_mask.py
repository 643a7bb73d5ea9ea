#!/usr/bin/env python
"""Binary masking of two beams through the MI355X engine: two delay-and-sum beamformers steered at a target and at an
interferer, a threshold estimator over their outputs, then the mask filter with the estimated threshold into the synthesis bank.

  -A multi-channel audio: a 16-bit WAV or an .npz with `pcm` [N][L] (default: the 4-channel recording under tests/golden)
  -O output WAV
  -M subbands (256)   -m (4)   -r (1)   -d delay compensation type (2)
  -t / -i look directions of the target and of the interferer in radians, azimuth of a linear array (0.3, -1.0)
  -p microphone pitch in mm (20)
  -k kind: `iid` (level difference, IIDThresholdEstimator + IIDBinaryMaskFilter), `kim` (time delay, KimITDThresholdEstimator +
     KimBinaryMaskFilter) or `fdiid` (per-bin level thresholds, FDIIDThresholdEstimator + IIDBinaryMaskFilter.set_thresholds)
  --min / --max / --width the candidate thresholds (the classes' defaults where min == max; the level kinds need a range on the
     scale of the subband magnitudes: -1000 .. 1000 in steps of 50 here)
  -a forgetting factor of the mask (0.6)   -e flooring value (0.01)   -n factor the output samples are multiplied by (1.0)
Two passes over the recording, each on a fresh graph: the estimator pulls both beams to the end and calc_threshold() picks the
threshold; the filter then runs beams -> mask -> synthesis with the blocks handed over on the device.  The output is 16-bit
PCM, the samples truncated as `(short)` does."""
import argparse
import os
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SSPEED = 343740.0                    # mm/s, beamformer/beamformer.h:26


def linear_array_delays(N, pitch_mm, azimuth):
    """far-field delays of a uniform linear array relative to its middle microphone (lib/pybeamformer.py:41-64)"""
    x = (np.arange(N) - (N - 1) / 2.0) * pitch_mm
    d = -x * np.cos(azimuth) / SSPEED
    return d - d[N // 2]


def load_channels(path):
    if path.endswith(".npz"):
        return np.asarray(np.load(path)["pcm"], np.float32), 16000
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise SystemExit("binaural_mask: %s is not 16-bit PCM" % path)
        pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels()).T.astype(np.float32)
        return np.ascontiguousarray(pcm), w.getframerate()


def two_beams(pcm, rate, h, M, m, r, dct, looks, pitch_mm, block_frames=None):
    """two SubbandDS beamformers over their own analysis banks; returns (target beam, interferer beam, what keeps them alive)"""
    from distant_speech_recognition_amd.btk20 import SampleFeaturePtr, OverSampledDFTAnalysisBankPtr, SubbandDSPtr
    D = M >> r
    beams, keep = [], []
    for look in looks:
        bf = SubbandDSPtr(M, False)
        for c in range(pcm.shape[0]):
            samp = SampleFeaturePtr("", D, D, True)
            samp.set_samples(np.ascontiguousarray(pcm[c], np.float32))
            afb = OverSampledDFTAnalysisBankPtr(samp, h, M, m, r, dct)
            if block_frames is not None:
                afb.set_block_frames(block_frames)
            bf.set_channel(afb)
            keep.append((samp, afb))
        bf.calc_array_manifold_vectors(float(rate), linear_array_delays(pcm.shape[0], pitch_mm, look))
        beams.append(bf)
    return beams[0], beams[1], keep


def binaural_mask(pcm, rate, h, g, M, m, r, kind="iid", looks=(0.3, -1.0), pitch_mm=20.0, lo=0.0, hi=0.0, width=0.0, alpha=0.6,
                  eta=0.01, dct=2, block_frames=None, verbose=True):
    """pcm float32 [N][L], int16 scale.  Returns (the output blocks float32 [n][D], the threshold, the estimator node)."""
    from distant_speech_recognition_amd.btk20 import OverSampledDFTSynthesisBankPtr
    from distant_speech_recognition_amd.btk20 import postfilter as pf
    if kind not in ("iid", "kim", "fdiid"):
        raise ValueError("kind %r: iid, kim or fdiid" % (kind,))
    if lo == hi and kind != "kim":
        lo, hi, width = -1000.0, 1000.0, 50.0
    if width <= 0:
        width = 0.02 if kind == "kim" else 50.0
    # pass 1: the estimator pulls both beams to the end
    bt, bi, keep = two_beams(pcm, rate, h, M, m, r, dct, looks, pitch_mm, block_frames)
    if kind == "kim":
        est = pf.KimITDThresholdEstimatorPtr(bt, bi, M, lo, hi, width, dEta=eta)
    elif kind == "iid":
        est = pf.IIDThresholdEstimatorPtr(bt, bi, M, lo, hi, width, dEta=eta)
    else:
        est = pf.FDIIDThresholdEstimatorPtr(bt, bi, M, lo, hi, width, eta)
    frames = sum(1 for _ in est)
    thr = est.calc_threshold()
    if verbose:
        print("%s threshold %g from %d frames and %d candidates" % (kind, thr, frames, len(est.candidates())), file=sys.stderr)
    # pass 2: beams -> mask filter -> synthesis, on a fresh graph
    bt, bi, keep2 = two_beams(pcm, rate, h, M, m, r, dct, looks, pitch_mm, block_frames)
    if kind == "kim":
        filt = pf.KimBinaryMaskFilterPtr(0, bt, bi, M, thr, alpha, eta)
    else:
        filt = pf.IIDBinaryMaskFilterPtr(0, bt, bi, M, thr, alpha, eta)
        if kind == "fdiid":
            filt.set_thresholds(est.thresholds())
    sfb = OverSampledDFTSynthesisBankPtr(filt, g, M, m, r, dct)
    out = [np.array(b, np.float32) for b in sfb]
    return (np.stack(out) if out else np.zeros((0, M >> r), np.float32)), thr, est


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-A", dest="audio", default=os.path.join(ROOT, "tests", "golden", "kinect_4ch_16k.npz"))
    p.add_argument("-O", dest="output", default="")
    p.add_argument("-M", dest="M", type=int, default=256)
    p.add_argument("-m", dest="m", type=int, default=4)
    p.add_argument("-r", dest="r", type=int, default=1)
    p.add_argument("-d", dest="dct", type=int, default=2)
    p.add_argument("-t", dest="target", type=float, default=0.3)
    p.add_argument("-i", dest="interferer", type=float, default=-1.0)
    p.add_argument("-p", dest="pitch", type=float, default=20.0)
    p.add_argument("-k", dest="kind", default="iid")
    p.add_argument("--min", dest="lo", type=float, default=0.0)
    p.add_argument("--max", dest="hi", type=float, default=0.0)
    p.add_argument("--width", dest="width", type=float, default=0.0)
    p.add_argument("-a", dest="alpha", type=float, default=0.6)
    p.add_argument("-e", dest="eta", type=float, default=0.01)
    p.add_argument("-n", dest="norm", type=float, default=1.0)
    args = p.parse_args(argv)
    from distant_speech_recognition_amd import prototypes
    pcm, rate = load_channels(args.audio)
    h, g = prototypes.load(args.M, args.m, args.r)
    blocks, thr, _ = binaural_mask(pcm, rate, h, g, args.M, args.m, args.r, args.kind, (args.target, args.interferer), args.pitch,
                                   args.lo, args.hi, args.width, args.alpha, args.eta, args.dct)
    y = np.clip(np.trunc(blocks.reshape(-1) * args.norm), -32768, 32767).astype(np.int16)
    print("MAX %e" % (float(np.max(np.abs(blocks))) if blocks.size else 0.0), file=sys.stderr)
    if args.output:
        with wave.open(args.output, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
            w.writeframes(y.tobytes())
    return 0


if __name__ == "__main__":
    sys.exit(main())
