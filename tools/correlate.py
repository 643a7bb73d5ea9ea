#!/usr/bin/env python
"""Correlate a recorded chirp with the original chirp to extract the impulse response of the room + beamformer, on the MI355X engine.

The reference's correlation script made to run: a SampleFeaturePtr over the chirp hands out its first M-sample block, which becomes
the impulse response of an OverlapAddPtr over a SampleFeaturePtr over the recording.  In `correlate` mode (the default, and the
script's stated purpose) the block is time-reversed, so the output is the cross-correlation of the recording with the chirp,
delayed by M - 1 samples: a chirp's autocorrelation is a narrow pulse, so the output shows the response the chirp went through.
`convolve` mode filters with the block as it is.

Where the script cannot run as written, this tool deviates: the filter is the chirp block the script reads (it names an undefined
`chirpSignal`), the transform length is left to the node (the script's fftLen = M is shorter than L + P - 1 and refused), and the
frames are written to the output file (the script prints them and never writes).  The output is a 32-bit float WAV: correlation
values leave the 16-bit range, which the 16-bit writers of the other tools cannot hold.
"""
import argparse
import os
import struct
import sys

import numpy

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_float_wav(path, samples, samplerate):
    """One channel of float32 samples as a RIFF/WAVE file of format 3 (IEEE float), with the `fact` chunk that format asks for."""
    data = numpy.ascontiguousarray(samples, dtype="<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 1, int(samplerate), int(samplerate) * 4, 4, 32)
    fact = struct.pack("<I", len(data) // 4)
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"fact" + struct.pack("<I", len(fact)) + fact \
        + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as fp:
        fp.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def build_chain(chirp_path, M=2048, shift=None, mode="correlate", block_frames=0):
    from btk20.feature import SampleFeaturePtr
    from btk20.convolution import OverlapAddPtr
    if mode not in ("correlate", "convolve"):
        raise ValueError("mode must be correlate or convolve, not %r" % (mode,))
    chirp_feature = SampleFeaturePtr(blockLen=M, shiftLen=M, padZeros=True)
    chirp_feature.read(chirp_path)
    impulse_response = numpy.array(chirp_feature.next(0), dtype=numpy.float64)
    if mode == "correlate":
        impulse_response = impulse_response[::-1].copy()
    sample_feature = SampleFeaturePtr(blockLen=M, shiftLen=M if shift is None else int(shift), padZeros=True)
    overlap_add = OverlapAddPtr(sample_feature, impulse_response, fftLen=0)
    if block_frames:
        overlap_add.set_block_frames(block_frames)
    return sample_feature, overlap_add, impulse_response


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("-c", "--chirp", required=True, help="the original chirp (16-bit PCM WAV, one channel)")
    ap.add_argument("-i", "--input", required=True, help="the recording, e.g. a beamformer's output (16-bit PCM WAV)")
    ap.add_argument("-o", "--output", default="impulse-response.wav", help="output WAV (32-bit float, one channel)")
    ap.add_argument("-M", type=int, default=2048, help="block length; the first M samples of the chirp are the filter")
    ap.add_argument("--shift", type=int, default=None, help="shift of the recording's blocks (default M; the blocks are filtered "
                    "laid end to end as served, so a shift below M repeats samples)")
    ap.add_argument("--mode", choices=("correlate", "convolve"), default="correlate")
    ap.add_argument("--block-frames", type=int, default=0, help="blocks per kernel launch (0: the node's default)")
    args = ap.parse_args(argv)
    sample_feature, overlap_add, _ = build_chain(args.chirp, args.M, args.shift, args.mode, args.block_frames)
    sample_feature.read(args.input)
    frames = [numpy.array(fc) for fc in overlap_add]
    out = numpy.concatenate(frames) if frames else numpy.zeros(0, numpy.float32)
    write_float_wav(args.output, out, sample_feature.samplerate())
    print("%d blocks of %d samples written to %s (%d launches)" % (len(frames), args.M, args.output, overlap_add.launches()))
    return len(frames)


if __name__ == "__main__":
    main()
