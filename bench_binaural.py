#!/usr/bin/env python
"""Binaural binary-mask filters and threshold estimators: binaural_mask / binaural_stats (csrc/binaural_kernels.hip).

Mask filters (Kim, IID): M = 512 (257 bins), 4096 frames in padded rows, alpha = 0.6, and as many streams as make a launch move at
least 1 GB of algorithmic bytes: two inputs read once and one output written once, 24 B per bin-frame.  The yardstick, measured
in the same run, is the fixed-model spectral subtraction of bench_ss.py with one channel (16 B per bin-frame, the same kind of
rows).  Figures: ms per GB moved and the share of the HBM peak.
Estimators (Kim, IID, FD-IID): M = 512, one stream, `--est-frames` frames, the default candidate lists of the node classes (942
for Kim and IID: +-0.2 x 16000 / 340 in steps of 0.02; 201 for FD-IID: +-100000 in steps of 1000).  Figure: ns per
(frame x candidate x bin).  The timed call is engine.binaural_stats as a caller uses it, the upload of the candidate list and
the scratch allocation included.
Every launch is timed with its own pair of HIP events after a warm-up; the figure is the median, with min and max.  Prints one
JSON line and writes it to --out."""
import argparse
import json
import os

import numpy as np
import torch

from bench_srp import median_ms
from bench_ss import rand_rows, streams_for
from bench_stages import HBM
from distant_speech_recognition_amd import engine as eng

ALPHA, ETA = 0.6, 0.01


def ms(t):
    return {"median": t[0], "min": t[1], "max": t[2]}


def moved(name, S, K, T, bytes_per_binframe, t):
    nbytes = float(bytes_per_binframe) * S * K * T
    return {"case": name, "S": S, "K": K, "T": T, "algorithmic_bytes": nbytes, "kernel_ms": ms(t),
            "ms_per_GB": t[0] / (nbytes / 1e9), "algorithmic_GBps": nbytes / (t[0] * 1e-3) / 1e9,
            "hbm_roofline_share": nbytes / (t[0] * 1e-3) / HBM}


def run_masks(M, T, launches, target, dev):
    K = M // 2 + 1
    res = []
    S = streams_for(K, T, 24, target)
    XL, XR = rand_rows((S, K, T), dev, seed=1), rand_rows((S, K, T), dev, seed=2)
    Y = eng.rows_like(XL, (S, K, T))
    for kind, thr in (("kim", 0.9), ("iid", 0.3)):
        st = eng.binaural_mask_state(S, M, dev)
        t = median_ms(lambda: eng.binaural_mask(XL, XR, kind, 0, thr, ALPHA, ETA, state=st, out=Y), launches)
        res.append(moved("mask_" + kind, S, K, T, 24, t))
    # the yardstick: fixed-model spectral subtraction, one channel
    S1 = streams_for(K, T, 16, target)
    X = rand_rows((S1, K, 1, T), dev, seed=3)
    Y1 = eng.rows_like(X, (S1, K, T))
    ss = eng.SpectralSubtractionState(S1, 1, M, [0.9375], device=dev)
    ss.set_noise_psd(torch.rand((S1, 1, K), dtype=torch.float64, device=dev) + 0.5)
    t = median_ms(lambda: eng.spectral_subtract(X, ss, ft=1.5, floor=0.001, train=False, subtract=True, out=Y1), launches)
    res.append(moved("ss_subtract_fixed_yardstick", S1, K, T, 16, t))
    for e in res[:-1]:
        e["time_per_GB_vs_yardstick"] = e["ms_per_GB"] / res[-1]["ms_per_GB"]
    return res


def run_estimators(M, T, launches, dev):
    K = M // 2 + 1
    XL, XR = rand_rows((1, K, T), dev, seed=4), rand_rows((1, K, T), dev, seed=5)
    lim = float(np.float32(0.2 * 16000 / 340))
    res = []
    for kind, rng_, pc, nb in (("kim", (-lim, lim, 0.02), 1 / 15.0, K - 1), ("iid", (-lim, lim, 0.02), 0.5, K - 1),
                               ("fdiid", (-1e5, 1e5, 1e3), 1 / 15.0, K - 1)):
        cands = eng.binaural_candidates(*rng_)
        st = eng.BinauralStatsState(kind, 1, M, cands[1], dev)
        t = median_ms(lambda: eng.binaural_stats(XL, XR, kind, cands, ETA, pc, 1, K, state=st), launches)
        cells = float(T) * len(cands[0]) * nb
        res.append({"case": "stats_" + kind, "S": 1, "K": K, "T": T, "candidates": len(cands[0]), "slots": cands[1], "bins": nb,
                    "kernel_ms": ms(t), "ns_per_frame_candidate_bin": t[0] * 1e6 / cells})
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fftlen", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--est-frames", type=int, default=1024)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--bytes", type=float, default=1.0e9, help="algorithmic bytes a mask launch moves at least")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "bench_binaural_mi355x.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = run_masks(args.fftlen, args.frames, args.launches, args.bytes, dev) + run_estimators(args.fftlen, args.est_frames, args.launches, dev)
    line = json.dumps({"bench": "binaural", "device": torch.cuda.get_device_name(0),
                       "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "M": args.fftlen,
                       "hbm_peak_Bps": HBM, "results": res})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
