#!/usr/bin/env python
"""Mel frequency cepstral coefficients (MFCC) of a WAV file, frame by frame, on the MI355X engine.

The chain of the reference's MFCC script with that script's constants as defaults: SampleFeaturePtr -> StorageFeaturePtr ->
HammingFeaturePtr -> FFTFeaturePtr -> SpectralPowerFeaturePtr -> [VTLNFeaturePtr -> MelFeaturePtr] -> LogFeaturePtr ->
CepstralFeaturePtr -> StorageFeaturePtr.  The chain serves blocks: one kernel launch per --block-frames frames.  Every frame's
cepstra (float32 [ncep]) are pickled to the output file one after the other, in binary mode.
"""
import argparse
import os
import pickle
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build_chain(log_input="power", frame_len=160, fft_len=256, samplerate=16000.0, mel_num=30, lower=100.0, upper=6800.0, ncep=13,
                block_frames=0):
    from btk20.feature import (SampleFeaturePtr, StorageFeaturePtr, HammingFeaturePtr, FFTFeaturePtr, SpectralPowerFeaturePtr,
                               VTLNFeaturePtr, MelFeaturePtr, LogFeaturePtr, CepstralFeaturePtr)
    pow_num = fft_len // 2 + 1
    samplefe = SampleFeaturePtr(block_len=frame_len, shift_len=frame_len, pad_zeros=False)
    sample_storage = StorageFeaturePtr(samplefe)
    hammingfe = HammingFeaturePtr(sample_storage)
    fftfe = FFTFeaturePtr(hammingfe, fft_len=fft_len)
    powerfe = SpectralPowerFeaturePtr(fftfe, pow_num=pow_num)
    vtlnfe = VTLNFeaturePtr(powerfe, coeff_num=pow_num, edge=0.8, version=2)
    melfe = MelFeaturePtr(vtlnfe, pow_num=pow_num, filter_num=mel_num, rate=samplerate, low=lower, up=upper, version=2)
    logfe = LogFeaturePtr(melfe if log_input == "mel" else powerfe)
    cepfe = CepstralFeaturePtr(logfe, ncep=ncep)
    if block_frames:
        cepfe.set_block_frames(block_frames)
    cep_storage = StorageFeaturePtr(cepfe)
    return samplefe, cepfe, cep_storage


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("input", help="input WAV file (16-bit PCM, one channel)")
    ap.add_argument("output", nargs="?", default="mfcc.pickle", help="output pickle, one vector per frame")
    ap.add_argument("--log-input", choices=("power", "mel"), default="power",
                    help="what the log is taken of.  power (default): the reference script's wiring as it stands -- it builds the VTLN "
                         "and the mel node and then takes the log of the POWER node, so the cepstra come from fft_len/2+1 log-power "
                         "values and the two nodes are unused; mel: the chain the script evidently meant, the log of the mel bands "
                         "of the VTLN-warped power spectrum")
    ap.add_argument("--frame-len", type=int, default=160, help="samples per frame: 10 ms at 16 kHz")
    ap.add_argument("--fft-len", type=int, default=256)
    ap.add_argument("--samplerate", type=float, default=16000.0)
    ap.add_argument("--mel-num", type=int, default=30, help="mel filter-bank outputs")
    ap.add_argument("--lower", type=float, default=100.0, help="lower frequency of the mel filter bank")
    ap.add_argument("--upper", type=float, default=6800.0, help="upper frequency of the mel filter bank")
    ap.add_argument("--ncep", type=int, default=13, help="cepstral coefficients")
    ap.add_argument("--block-frames", type=int, default=0, help="frames per kernel launch (0: the node's default)")
    ap.add_argument("-q", "--quiet", action="store_true", help="do not print every frame")
    args = ap.parse_args(argv)
    samplefe, cepfe, cep_storage = build_chain(args.log_input, args.frame_len, args.fft_len, args.samplerate, args.mel_num, args.lower,
                                               args.upper, args.ncep, args.block_frames)
    samplefe.read(args.input)
    frame_no = 0
    with open(args.output, "wb") as ofp:
        for cep_vector in cep_storage:
            if not args.quiet:
                print("fr. {}: {}".format(frame_no, numpy.array2string(cep_vector, formatter={"float_kind": lambda x: "%.2f" % x})))
            pickle.dump(numpy.array(cep_vector), ofp, True)
            frame_no += 1
    print("%d frames written to %s (%d launches)" % (frame_no, args.output, cepfe.launches()))
    return frame_no


if __name__ == "__main__":
    main()
