#!/usr/bin/env python
"""Direction of a source from a linear microphone array by multichannel cross-correlation, block by block, through the MI355X
engine (btk20.localization.MCCLocalizerPtr over csrc/mcc_kernels.hip).  The reference ships the classes
(localization/mcc_localizer.{h,cc}) but no script for this localiser; the options are this project's.

  inputs           16-bit WAV files, one per channel (channel 1 of each), or one .npz whose `pcm` array is [channels][samples]
  --spacing MM     equally spaced microphones MM millimetres apart, or
  --positions ...  the microphones' places along the array in millimetres, one per channel
  --block L        samples per block (4096); the last, shorter block is dropped
  --nbest K        candidates kept per block (1)
  --rate HZ        sampling rate of an .npz input (16000); WAV files carry theirs
Prints JSON: the grid size, the largest sample delay D and, per block, the azimuth (radian, the reference's far-field
convention: 0 .. pi/2 and 3 pi/2 .. 2 pi), the MCCC = 1 - det of the normalised correlation matrix, the sample delays and the
N-best list.  main(argv) returns the same as a dict."""
import argparse
import json
import os
import sys
import wave

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class ArraySource:
    """One channel cut into blocks of L samples: size() / __iter__ / next() / reset(), what the node layer pulls from."""

    def __init__(self, x, L):
        self.x, self.L, self.at = np.ascontiguousarray(x, np.float32), int(L), 0

    def size(self):
        return self.L

    def reset(self):
        self.at = 0

    def __iter__(self):
        return self

    def __next__(self):
        if self.at + self.L > len(self.x):
            raise StopIteration
        self.at += self.L
        return self.x[self.at - self.L:self.at]

    next = __next__


def read_inputs(paths, rate):
    if len(paths) == 1 and paths[0].endswith(".npz"):
        return np.load(paths[0])["pcm"].astype(np.float32), rate
    chans, rates = [], set()
    for p in paths:
        with wave.open(p, "rb") as w:
            if w.getsampwidth() != 2:
                raise SystemExit("mcc_localizer: %s is not 16-bit PCM" % p)
            x = np.frombuffer(w.readframes(w.getnframes()), np.int16).reshape(-1, w.getnchannels())
            rates.add(w.getframerate())
        chans.append(x[:, 0].astype(np.float32))
    if len(rates) != 1:
        raise SystemExit("mcc_localizer: the files have different sampling rates %s" % sorted(rates))
    n = min(len(c) for c in chans)
    return np.stack([c[:n] for c in chans]), rates.pop()


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("inputs", nargs="+")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--spacing", type=float)
    g.add_argument("--positions", type=float, nargs="+")
    p.add_argument("--block", type=int, default=4096)
    p.add_argument("--nbest", type=int, default=1)
    p.add_argument("--rate", type=int, default=16000)
    p.add_argument("-q", "--quiet", action="store_true")
    a = p.parse_args(argv)
    from btk20.localization import SGB4LinearArrayPtr, MCCLocalizerPtr
    pcm, fs = read_inputs(a.inputs, a.rate)
    N = pcm.shape[0]
    grid = SGB4LinearArrayPtr(N, True, fs)
    if a.positions is not None:
        if len(a.positions) != N:
            raise SystemExit("mcc_localizer: %d positions for %d channels" % (len(a.positions), N))
        grid.setPositionsOfMicrophones(np.array([[0.0, y, 0.0] for y in a.positions]))
    else:
        grid.setDistanceBtwMicrophones(a.spacing)
    points = 1
    while grid.nextSearchGrid():
        points += 1
    loc = MCCLocalizerPtr(grid, a.nbest)
    for c in range(N):
        loc.setChannel(ArraySource(pcm[c], a.block))
    blocks = []
    for b, pos in enumerate(loc):
        nbest = [dict(azimuth=float(loc.getNthBestPosition(j)[1]), mccc=float(loc.getNthBestMCCC(j)),
                      delays=[int(loc.getNthBestDelayedSample(j, c)) for c in range(N)]) for j in range(a.nbest)]
        blocks.append(dict(block=b, azimuth=float(pos[1]), mccc=float(loc.getMaxMCCC()), delays=nbest[0]["delays"], nbest=nbest))
    out = dict(rate=int(fs), channels=int(N), block=int(a.block), grid_points=points,
               D=int(np.float32(fs) * np.float32(grid.maxTimeDelay())), blocks=blocks)
    if not a.quiet:
        print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
