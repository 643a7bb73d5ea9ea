#!/usr/bin/env python
"""GCC-PHAT time delay of arrival: btk_tdoa_spectra + btk_tdoa_gcc_peaks against the same computation composed from
torch.fft.rfft / irfft and torch reductions, timed in the same run.

Shape: 64 channels, all 2016 pairs, window 8192, transform 16384 (the setting of the reference's TDOA script), --streams x
--frames frames per launch (default 1 x 1024: 2 million correlations, about a second of GPU time for the two paths together).  The composition runs frame by frame (the correlations of one frame's 2016 pairs are 132 MB in
float32, its normalised cross spectra as much again) and is timed over the same frames.  Every timed call is bracketed by its
own pair of HIP events after a warm-up of back-to-back calls; the figure is the median.  Prints one JSON line and writes it to
--out (default profiles/bench_tdoa_mi355x.json).
"""
import argparse
import json
import os

import numpy as np
import torch

from bench_srp import median_ms
from distant_speech_recognition_amd import engine as eng


def run(S, C, D, L, T, reps, reps_composition, threshold=128.0):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    pcm = torch.randn((S, C, T * D), dtype=torch.float32, device=dev, generator=g) * 1000.0
    pairs = [(a, b) for a in range(C) for b in range(a + 1, C)]
    P = len(pairs)
    pd = eng.tdoa_pairs(pairs, C, dev)
    ia = torch.tensor([a for a, _ in pairs], device=dev)
    ib = torch.tensor([b for _, b in pairs], device=dev)
    win = (0.54 - 0.46 * torch.cos(2.0 * np.pi * torch.arange(D, dtype=torch.float64, device=dev) / (D - 1)))

    def k_spectra():
        return eng.tdoa_spectra(pcm, D, L)

    X, energy = k_spectra()

    def k_gcc():
        return eng.tdoa_gcc_peaks(X, energy, pd, threshold)

    def k_both():
        Xk, ek = eng.tdoa_spectra(pcm, D, L)
        return eng.tdoa_gcc_peaks(Xk, ek, pd, threshold)

    def t_spectra():
        fr = (pcm.view(S, C, T, D).to(torch.float64) * win).to(torch.float32)
        Xt = torch.fft.rfft(fr, n=L, dim=-1)
        return Xt, 2.0 * (Xt.real ** 2 + Xt.imag ** 2).sum(dim=-1)

    Xt, et = t_spectra()
    lag_t = torch.empty((S, P, T), dtype=torch.int64, device=dev)
    h_t = torch.empty((S, P, T), dtype=torch.float32, device=dev)

    def t_gcc():
        for s in range(S):
            for t in range(T):
                Xf = Xt[s, :, t]
                c = Xf[ia] * torch.conj(Xf[ib])
                gc = torch.fft.irfft(c / c.abs(), n=L, dim=-1).abs()
                h, n = gc.max(dim=-1)
                gate = (et[s, ia, t] <= threshold) & (et[s, ib, t] <= threshold)
                lag_t[s, :, t] = torch.where(gate, torch.full_like(n, eng.TDOA_NO_PEAK), torch.where(n < L // 2, n, n - L))
                h_t[s, :, t] = torch.where(gate, torch.zeros_like(h), h)
        return lag_t, h_t

    def t_both():
        nonlocal Xt, et
        Xt, et = t_spectra()
        return t_gcc()

    ks, kg, kb = median_ms(k_spectra, reps), median_ms(k_gcc, reps), median_ms(k_both, reps)
    ts, tg, tb = median_ms(t_spectra, reps_composition), median_ms(t_gcc, reps_composition), median_ms(t_both, reps_composition)
    lag, h = k_both()
    lt, ht = t_both()
    return {"S": S, "C": C, "pairs": P, "D": D, "L": L, "T": T,
            "kernels_ms": {"spectra": ks[0], "gcc_peaks": kg[0], "both": kb[0], "both_min": kb[1], "both_max": kb[2], "calls": reps},
            "torch_ms": {"spectra": ts[0], "gcc_peaks": tg[0], "both": tb[0], "both_min": tb[1], "both_max": tb[2], "calls": reps_composition},
            "torch_over_kernels": tb[0] / kb[0], "correlations_per_s": S * P * T / (kb[0] * 1e-3),
            "lags_equal_frac": float((lag.to(torch.int64) == lt).float().mean()), "max_height_diff": float((h - ht).abs().max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=1)
    ap.add_argument("--channels", type=int, default=64)
    ap.add_argument("--window", type=int, default=8192)
    ap.add_argument("--fftlen", type=int, default=16384)
    ap.add_argument("--frames", type=int, default=1024, help="frames per call: 1024 makes kernels plus composition about a second of GPU time")
    ap.add_argument("--calls", type=int, default=20, help="timed calls of the kernels (>= 20 for a figure to quote)")
    ap.add_argument("--calls-composition", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "bench_tdoa_mi355x.json"))
    args = ap.parse_args()
    out = {"bench": "tdoa", "device": torch.cuda.get_device_name(0)}
    out["result"] = run(args.streams, args.channels, args.window, args.fftlen, args.frames, args.calls, args.calls_composition)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
