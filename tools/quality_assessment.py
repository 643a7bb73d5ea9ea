#!/usr/bin/env python
"""SNR and Itakura-Saito distance of an enhanced recording against the original through the MI355X engine: the options of the
reference's src/quality_assessment.cc.

  -1 / -2  the original and the enhanced speech, 16-bit WAV files (channel 1 is compared)
  -M / -r / -w  transform length, decimation exponent and window type of the distance's spectra (64, 1, 1: Hamming)
  -b / -e  first and last sample of the comparison (0, -1); -e below 0 means "to the end" for both measures.  The distance takes
      them divided by the frame shift M >> r as its first and last frame
  -n  normalisation of the SNR: 1 mean, then the first of 2 signed-maximum, 4 power, 8 projection scaling (0)
  --segmental L  also the segmental SNR over segments of L samples, clamped to [--seg-lo, --seg-hi] dB (-10, 35); this measure
      is the project's own (the reference's segmentalSNR class is empty)
Prints `SNR <dB>` and `IS  <distance>` like the reference (and `SEG <dB>`); main(argv) returns the values as a dict."""
import argparse
import os
import re
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def read_channel(path, chX=1):
    """Channel chX of a 16-bit WAV file as sf_readf_float hands it out: x / 32768, float32."""
    with wave.open(path, "rb") as w:
        if w.getsampwidth() != 2:
            raise SystemExit("quality_assessment: %s is not 16-bit PCM" % path)
        x = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels())
    return (x[:, chX - 1].astype(np.float32) * np.float32(1.0 / 32768.0)).astype(np.float32)


def sample_range(f1, f2, cfrom, to):
    """SNR::getSNR's range rule (objective_measure.cc:233-242) -> (cfrom, n1, n2)."""
    cfrom = max(cfrom, 0)
    if to < 0 or to >= f1 or to >= f2:
        return cfrom, f1 - cfrom, f2 - cfrom
    return cfrom, to - cfrom + 1, to - cfrom + 1


def segmental(fn1, fn2, L, option=0, begin=0, end=-1, lo=-10.0, hi=35.0):
    import torch
    from distant_speech_recognition_amd import engine as eng
    x1, x2 = read_channel(fn1), read_channel(fn2)
    cfrom, n1, n2 = sample_range(len(x1), len(x2), begin, end)
    if n1 < 1 or n2 < 1:
        raise SystemExit("quality_assessment: no samples from %d to %d" % (begin, end))
    dev = torch.device("cuda:0")
    a = torch.from_numpy(np.ascontiguousarray(x1[cfrom:cfrom + n1])).to(dev)
    b = torch.from_numpy(np.ascontiguousarray(x2[cfrom:cfrom + n2])).to(dev)
    return float(eng.segmental_snr(a, b, L, option=option, lo=lo, hi=hi)[0][0])


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-M", "--M", dest="M", type=int, default=64)
    p.add_argument("-r", "--r", dest="r", type=int, default=1)
    p.add_argument("-w", "--w", dest="w", type=int, default=1)
    p.add_argument("-b", "--b", dest="begin", type=int, default=0)
    p.add_argument("-e", "--e", dest="end", type=int, default=-1)
    p.add_argument("-n", "--normalization", dest="option", type=int, default=0)
    p.add_argument("-1", "--1", dest="original", required=True)
    p.add_argument("-2", "--2", dest="enhanced", required=True)
    p.add_argument("--segmental", type=int, default=None, metavar="L")
    p.add_argument("--seg-lo", type=float, default=-10.0)
    p.add_argument("--seg-hi", type=float, default=35.0)
    p.add_argument("-q", dest="quiet", action="store_true")
    # `-e -1`: with options named -1 and -2 the parser would take the value for an option
    argv, merged = list(sys.argv[1:] if argv is None else argv), []
    while argv:
        tok = argv.pop(0)
        if tok in ("-b", "--b", "-e", "--e") and argv and re.fullmatch(r"-\d+", argv[0]):
            tok += "=" + argv.pop(0)
        merged.append(tok)
    a = p.parse_args(merged)
    from btk20.objective_measure import SNRPtr, ItakuraSaitoMeasurePSPtr
    out = {}
    out["snr"] = SNRPtr().getSNR(a.original, a.enhanced, a.option, 1, 16000, a.begin, a.end)
    isd = ItakuraSaitoMeasurePSPtr(a.M, a.r, a.w)
    shift = max(isd.frameShiftLength(), 1)                    # 0 for an r that leaves no shift: getDistance raises for it
    out["is"] = isd.getDistance(a.original, a.enhanced, 1, 16000, a.begin // shift, a.end // shift if a.end >= 0 else -1)
    if a.segmental is not None:
        out["segmental"] = segmental(a.original, a.enhanced, a.segmental, a.option, a.begin, a.end, a.seg_lo, a.seg_hi)
    if not a.quiet:
        print("SNR %f" % out["snr"])
        print("IS  %f" % out["is"])
        if "segmental" in out:
            print("SEG %f" % out["segmental"])
    return out


if __name__ == "__main__":
    main()
