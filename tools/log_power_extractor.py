#!/usr/bin/env python
"""Log power features of a WAV file, frame by frame, on the MI355X engine.

The chain of the reference's log-power script: SampleFeaturePtr -> HammingFeaturePtr -> FFTFeaturePtr -> SpectralPowerFeaturePtr
-> LogFeaturePtr, with that script's constants as defaults (160-sample frames without overlap, 256-point transform, 129 power
values).  The chain serves blocks: one kernel launch per --block-frames frames.  Every frame's vector (float32 [pow_num]) is
pickled to the output file one after the other, in binary mode.
"""
import argparse
import os
import pickle
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_chain(frame_len=160, fft_len=256, block_frames=0):
    from btk20.feature import SampleFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr, LogFeaturePtr
    pow_num = fft_len // 2 + 1
    samplefe = SampleFeaturePtr(block_len=frame_len, shift_len=frame_len, pad_zeros=False)
    hammingfe = HammingFeaturePtr(samplefe)
    fftfe = FFTFeaturePtr(hammingfe, fft_len=fft_len)
    powerfe = SpectralPowerFeaturePtr(fftfe, pow_num=pow_num)
    logfe = LogFeaturePtr(powerfe)
    if block_frames:
        logfe.set_block_frames(block_frames)
    return samplefe, logfe


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("input", help="input WAV file (16-bit PCM, one channel)")
    ap.add_argument("output", nargs="?", default="log_power.pickle", help="output pickle, one vector per frame")
    ap.add_argument("--frame-len", type=int, default=160, help="samples per frame: 10 ms at 16 kHz")
    ap.add_argument("--fft-len", type=int, default=256)
    ap.add_argument("--block-frames", type=int, default=0, help="frames per kernel launch (0: the node's default)")
    ap.add_argument("-q", "--quiet", action="store_true", help="do not print the first ten values of every frame")
    args = ap.parse_args(argv)
    samplefe, logfe = build_chain(args.frame_len, args.fft_len, args.block_frames)
    samplefe.read(args.input)
    frame_no = 0
    with open(args.output, "wb") as ofp:
        for log_vector in logfe:
            if not args.quiet:
                print("fr. {}: {}..".format(frame_no, numpy.array2string(log_vector[0:10], formatter={"float_kind": lambda x: "%.2f" % x})))
            pickle.dump(numpy.array(log_vector), ofp, True)
            frame_no += 1
    print("%d frames written to %s (%d launches)" % (frame_no, args.output, logfe.launches()))
    return frame_no


if __name__ == "__main__":
    main()
