#!/usr/bin/env python
"""The PR filter banks and the windowed FFT bank (csrc/fb_pr_kernels.hip): PRFilterBank.analysis / .synthesis and STFTBank.analysis,
with the oversampled bank's FilterBank.analysis at DFT length M2 = 2 M, the same m and the same frame shift (r = 1) timed beside
them in the same run as the yardstick.

Cases: M = 256 and 512, m = 4, r = 0, N = 8 and 64 channels, `--frames` frames per channel (2048: 1024 .. 16384 analysis workgroups on
256 compute units).  The synthesis bank runs N streams of the analysis bank's own output.  Algorithmic bytes: PR analysis 4 D + 8 M2
per channel-frame, PR synthesis 8 M2 + 4 D per frame, STFT 4 D + 8 M, oversampled analysis 4 D + 8 (M2/2 + 1); the roofline is the HBM
peak over these.  Every launch is timed with its own pair of HIP events after a warm-up; the figure is the median, with min and
max.  No threshold: the figures are a record.  Prints one JSON line."""
import argparse
import json

import numpy as np
import torch

from bench_srp import median_ms
from bench_stages import HBM
from distant_speech_recognition_amd import engine as eng


def entry(stage, M, m, r, N, T, nbytes, t):
    return {"stage": stage, "M": M, "m": m, "r": r, "N": N, "T": T, "algorithmic_bytes": float(nbytes),
            "ms": {"median": t[0], "min": t[1], "max": t[2]}, "algorithmic_GBps": nbytes / (t[0] * 1e-3) / 1e9,
            "hbm_roofline_share": nbytes / (t[0] * 1e-3) / HBM}


def run(M, m, r, N, T, launches, dev):
    M2, D = 2 * M, M >> r
    rng = np.random.default_rng(M + N)
    h = rng.uniform(-1.0, 1.0, M2 * m)
    L = (T - (2 * m - 1)) * D
    g = torch.Generator(device=dev).manual_seed(N)
    pcm = torch.round(torch.randn((1, N, L), dtype=torch.float32, device=dev, generator=g) * 3000.0)
    afb, sfb = eng.PRFilterBank(h, M, m, r), eng.PRFilterBank(h, M, m, r, synthesis=True)
    assert afb.num_frames(L) == T
    X = torch.empty((1, M2, N, T), dtype=torch.complex64, device=dev)
    res = [entry("pr_analysis", M, m, r, N, T, (4 * D + 8 * M2) * N * T, median_ms(lambda: afb.analysis(pcm, out=X), launches))]
    Y = X[0].permute(1, 0, 2).contiguous()                       # N streams [N][M2][T]
    B = sfb.num_blocks(T)
    out = torch.empty((N, B * D), dtype=torch.float32, device=dev)
    res.append(entry("pr_synthesis", M, m, r, N, T, (8 * M2 + 4 * D) * N * T, median_ms(lambda: sfb.synthesis(Y, out=out), launches)))
    del Y, out
    stft = eng.STFTBank(M, 1, 1)
    Ts = stft.num_frames(L)
    Xs = torch.empty((1, M, N, Ts), dtype=torch.complex64, device=dev)
    res.append(entry("stft", M, 1, 1, N, Ts, (4 * (M // 2) + 8 * M) * N * Ts, median_ms(lambda: stft.analysis(pcm, out=Xs), launches)))
    del Xs
    # the yardstick: the oversampled bank at DFT length M2 with the same prototype length and the same frame shift D = M2 / 2
    ofb = eng.FilterBank(h, M2, m, 1)
    To = ofb.num_frames(L)
    Xo = torch.empty((1, ofb.K, N, To), dtype=torch.complex64, device=dev)
    res.append(entry("oversampled_analysis_M2", M2, m, 1, N, To, (4 * M + 8 * ofb.K) * N * To,
                     median_ms(lambda: ofb.analysis(pcm, out=Xo), launches)))
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fftlens", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--channels", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--m", type=int, default=4)
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = []
    for M in args.fftlens:
        for N in args.channels:
            res += run(M, args.m, 0, N, args.frames, args.launches, dev)
    print(json.dumps({"bench": "prfb", "device": torch.cuda.get_device_name(0),
                      "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "hbm_peak_Bps": HBM, "results": res}))


if __name__ == "__main__":
    main()
