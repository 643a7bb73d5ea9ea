#!/usr/bin/env python
"""Pass a recording through the cosine-modulated perfect-reconstruction filter bank, analysis then synthesis, on the MI355X engine.

The flow of the reference's PR prototype check on Python 3: a SampleFeaturePtr hands out blocks of D = M / 2^r samples, a
PerfectReconstructionFFTAnalysisBankPtr turns them into frames of 2 M subbands, and a PerfectReconstructionFFTSynthesisBankPtr
over PyVectorComplexFeatureStreamPtr(analysis bank) turns the frames back into blocks, which are written as a 16-bit WAV.  With a
perfect-reconstruction prototype the output is the input (delayed by the prototype's reach, and without the first 2R - 1 blocks'
overlap partners); whatever else comes out is the prototype's reconstruction error.

The prototype (length 2 M m) comes from a pickle or .npy file, or is the sine window sin(pi (n + 1/2) / 2M) with --sine (m = 1):
the prototype designers are not part of the engine.
"""
import argparse
import os
import pickle
import sys
import wave

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def load_prototype(path):
    if path.endswith(".npy"):
        return numpy.asarray(numpy.load(path), numpy.float64).reshape(-1)
    with open(path, "rb") as fp:
        return numpy.asarray(pickle.load(fp, encoding="latin1"), numpy.float64).reshape(-1)


def sine_prototype(M):
    return numpy.sin(numpy.pi * (numpy.arange(2 * M) + 0.5) / (2 * M))


def build_chain(prototype, M, m, r=0, block_frames=0):
    from btk20.feature import SampleFeaturePtr
    from btk20.modulated import PerfectReconstructionFFTAnalysisBankPtr, PerfectReconstructionFFTSynthesisBankPtr
    from btk20.stream import PyVectorComplexFeatureStreamPtr
    D = M // 2 ** r
    sample_feature = SampleFeaturePtr(blockLen=D, shiftLen=D, padZeros=True)
    analysis = PerfectReconstructionFFTAnalysisBankPtr(sample_feature, prototype, M, m, r)
    synthesis = PerfectReconstructionFFTSynthesisBankPtr(PyVectorComplexFeatureStreamPtr(analysis), prototype, M, m, r)
    if block_frames:
        analysis.set_block_frames(block_frames)
        synthesis.set_block_frames(block_frames)
    return sample_feature, analysis, synthesis


def write_wav16(path, samples, samplerate):
    pcm = numpy.clip(numpy.rint(samples), -32768, 32767).astype("<i2")
    with wave.open(path, "wb") as w:
        w.setnchannels(1)
        w.setsampwidth(2)
        w.setframerate(int(samplerate))
        w.writeframes(pcm.tobytes())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-i", "--input", required=True, help="the recording (16-bit PCM WAV, one channel)")
    ap.add_argument("-o", "--output", default="pr-filter-bank.wav", help="output WAV (16-bit PCM, one channel)")
    ap.add_argument("-M", type=int, default=256, help="number of subbands / 2: frames hold 2 M bins")
    ap.add_argument("-m", type=int, default=None, help="prototype length factor (default: the prototype's length / 2M)")
    ap.add_argument("-r", type=int, default=0, help="decimation exponent: the frame shift is M / 2^r")
    ap.add_argument("-p", "--prototype", default=None, help="prototype of length 2 M m: a pickle or a .npy file")
    ap.add_argument("--sine", action="store_true", help="use the sine window (m = 1) instead of a prototype file")
    ap.add_argument("--block-frames", type=int, default=0, help="frames per kernel launch (0: the nodes' default)")
    args = ap.parse_args(argv)
    if args.sine == (args.prototype is not None):
        ap.error("give exactly one of --prototype and --sine")
    prototype = sine_prototype(args.M) if args.sine else load_prototype(args.prototype)
    m = args.m if args.m is not None else max(1, len(prototype) // (2 * args.M))
    sample_feature, analysis, synthesis = build_chain(prototype, args.M, m, args.r, args.block_frames)
    sample_feature.read(args.input)
    samplerate = sample_feature.samplerate()
    blocks = [numpy.array(b) for b in synthesis]
    out = numpy.concatenate(blocks) if blocks else numpy.zeros(0, numpy.float32)
    write_wav16(args.output, out, samplerate)
    print("%d blocks of %d samples written to %s (%d analysis, %d synthesis launches)"
          % (len(blocks), args.M // 2 ** args.r, args.output, analysis.launches(), synthesis.launches()))
    return len(blocks)


if __name__ == "__main__":
    main()
