#!/usr/bin/env python
"""Spectral subtraction of a WAV file through the MI355X engine -- the application-level counterpart of the reference's C++ main
src/ss.cc on this repository's nodes: analysis bank -> SpectralSubtractor -> synthesis bank.

The options are those of src/ss.cc, with its defaults:
  -A audio file        -O output WAV          -C prototype file (.npz with h and g, or the reference's text format: analysis
  -M subbands (256)    -m (4)   -r (1)           coefficients, then synthesis coefficients); without it the shipped design for M
  -a noise over-estimation factor (1.5)       -f flooring value (0.1)
  -N frames the noise model is trained on (100; <= 0: the whole file)
  -s noise model to read instead of training  -W noise model to write (outNoiseModel.txt)
  -n factor the output samples are multiplied by (1.0)      -d delay compensation type (2)
Flow, as there: without -s, N + 1 outputs of the SYNTHESIS bank are pulled while the subtractor trains (the bank runs its
processing delay ahead, so the model sees that many more frames), then stop_training() and the model is written; with -s the model
is read.  Then the rest of the file is pulled.  One deviation, stated: src/ss.cc never calls startNoiseSubtraction(), so its
second loop hands the input through unchanged; the real-time twin rt_ss.cc does (rt_ss.cc:406), and so does this tool, right
after the model is complete.  The output is 16-bit PCM, the samples truncated as `(short)` does."""
import argparse
import os
import sys
import wave

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_coefficients(path, M, m, r):
    """(h, g) from -C, or the shipped design"""
    if not path:
        from distant_speech_recognition_amd import prototypes
        return prototypes.load(M, m, r)
    if path.endswith(".npz"):
        z = np.load(path)
        return np.asarray(z["h"], np.float64), np.asarray(z["g"], np.float64)
    v = np.array(open(path).read().split(), np.float64)       # ss.cc readFilterCoeffs: first half analysis, second half synthesis
    return v[: len(v) // 2].copy(), v[len(v) // 2:].copy()


def spectral_subtraction(samples, h, g, M, m, r, ft=1.5, floor=0.1, frames=100, noise_in="", noise_out="outNoiseModel.txt",
                         dct=2, block_frames=None, verbose=True):
    """samples: float32, int16 scale.  Returns (the output blocks float32 [n][D], the subtractor node)."""
    from distant_speech_recognition_amd.btk20 import SampleFeaturePtr, OverSampledDFTAnalysisBankPtr, OverSampledDFTSynthesisBankPtr
    from distant_speech_recognition_amd.btk20.postfilter import SpectralSubtractorPtr
    D = M >> r
    samp = SampleFeaturePtr("", D, D, True)
    samp.set_samples(np.ascontiguousarray(samples, np.float32))
    afb = OverSampledDFTAnalysisBankPtr(samp, h, M, m, r, dct)
    if block_frames is not None:
        afb.set_block_frames(block_frames)
    ss = SpectralSubtractorPtr(M, False, ft, floor)
    sfb = OverSampledDFTSynthesisBankPtr(ss, g, M, m, r, dct)
    ss.setChannel(afb)
    out = []

    def pull(limit):
        n = 0
        while True:
            try:
                out.append(np.array(sfb.next(), np.float32))
            except StopIteration:
                return False
            if limit > 0 and n >= limit:
                return True
            n += 1

    if noise_in:
        if not ss.readNoiseFile(noise_in, 0):
            raise IOError("could not read the noise model %s" % noise_in)
        more = True
    else:
        more = pull(frames)
        ss.stopTraining()
        if noise_out and not ss.writeNoiseFile(noise_out, 0):
            raise IOError("could not write the noise model %s" % noise_out)
        if verbose:
            print("trained a noise model with %d outputs" % len(out), file=sys.stderr)
    ss.startNoiseSubtraction()
    if more:
        pull(0)
    return (np.stack(out) if out else np.zeros((0, D), np.float32)), ss


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-A", dest="audio", default="test.wav")
    p.add_argument("-O", dest="output", default="")
    p.add_argument("-C", dest="coeff", default="")
    p.add_argument("-M", dest="M", type=int, default=256)
    p.add_argument("-m", dest="m", type=int, default=4)
    p.add_argument("-r", dest="r", type=int, default=1)
    p.add_argument("-a", dest="ft", type=float, default=1.5)
    p.add_argument("-f", dest="floor", type=float, default=0.1)
    p.add_argument("-N", dest="frames", type=int, default=100)
    p.add_argument("-n", dest="norm", type=float, default=1.0)
    p.add_argument("-s", dest="noise_in", default="")
    p.add_argument("-W", dest="noise_out", default="outNoiseModel.txt")
    p.add_argument("-d", dest="dct", type=int, default=2)
    args = p.parse_args(argv)
    with wave.open(args.audio, "rb") as w:
        if w.getsampwidth() != 2:
            raise SystemExit("spectral_subtraction: %s is not 16-bit PCM" % args.audio)
        pcm = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels())[:, 0].astype(np.float32)
        rate = w.getframerate()
    h, g = load_coefficients(args.coeff, args.M, args.m, args.r)
    blocks, _ = spectral_subtraction(pcm, h, g, args.M, args.m, args.r, args.ft, args.floor, args.frames, args.noise_in,
                                     args.noise_out, args.dct)
    y = np.clip(np.trunc(blocks.reshape(-1) * args.norm), -32768, 32767).astype(np.int16)
    print("MAX %e" % (float(np.max(np.abs(blocks))) if blocks.size else 0.0), file=sys.stderr)
    if args.output:
        with wave.open(args.output, "wb") as w:
            w.setnchannels(1); w.setsampwidth(2); w.setframerate(rate)
            w.writeframes(y.tobytes())
    return 0


if __name__ == "__main__":
    sys.exit(main())
