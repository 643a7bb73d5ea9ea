#!/usr/bin/env python
"""FFT block convolution: fir_convolve against the same outputs composed from torch.fft.rfft / irfft over the whole row, timed in
the same run.

Shape: 32 streams x 64 impulse responses x 262 144 samples, with P = 8000 taps (one partition at N = 16384) and P = 32 000
(four partitions: five transforms a tile).  Every call is timed with its own pair of HIP events after a warm-up of back-to-back
calls (the shader clock needs ~0.3 s of load to settle); the figure is the median of the timed calls, with min and max.  The
filter spectra are computed once, outside the timed region, on both sides.  Sweeps over the transform length at P = 500 and P = 2000 show
what the planning rule's choice of N gives up or gains against its neighbours.  Prints one JSON line.
"""
import argparse
import json

import torch

from bench_srp import median_ms
from distant_speech_recognition_amd import engine as eng


def composition_setup(h, n):
    """the row-long transform: next power of two >= n + P - 1; -> (nfft, H)"""
    P = h.shape[-1]
    nfft = 1
    while nfft < n + P - 1:
        nfft *= 2
    return nfft, torch.fft.rfft(h, nfft)                   # [C][nfft/2+1]


def run(S, Cn, n, P, reps, reps_composition, n_max=16384):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((S, n), dtype=torch.float32, device=dev, generator=g)
    h = torch.randn((Cn, P), dtype=torch.float32, device=dev, generator=g) * torch.exp(-3.0 * torch.arange(P, device=dev) / P)
    filt = eng.conv_filter(h, n_max=n_max)
    out = torch.empty((S, Cn, n), dtype=torch.float32, device=dev)
    nfft, Hrow = composition_setup(h, n)

    def ours():
        return eng.fir_convolve(x, filt, out=out)

    def composition():
        X = torch.fft.rfft(x, nfft)                         # [S][K]
        return torch.fft.irfft(X[:, None, :] * Hrow[None], nfft)[..., :n]

    t_o = median_ms(ours, reps)
    t_c = median_ms(composition, reps_composition)
    y, ref = ours(), composition()
    rel = float((y - ref).abs().max() / ref.abs().max())
    del ref
    tiles = -(-n // filt.Lk)
    return {"S": S, "C": Cn, "len": n, "P": P, "N": filt.N, "Lk": filt.Lk, "Bp": filt.Bp, "Q": filt.Q, "tiles_per_row": tiles,
            "transforms_per_tile": filt.Q + 1,
            "fir_convolve_ms": {"median": t_o[0], "min": t_o[1], "max": t_o[2], "calls": reps},
            "composition_ms": {"median": t_c[0], "min": t_c[1], "max": t_c[2], "calls": reps_composition, "nfft": nfft},
            "speedup": t_c[0] / t_o[0], "output_samples_per_s": S * Cn * n / (t_o[0] * 1e-3),
            "output_bytes_per_s": 4.0 * S * Cn * n / (t_o[0] * 1e-3), "max_rel_diff_vs_composition": rel}


def plan_sweep(S, Cn, n, P, reps):
    """the same filter at every transform length that holds it in one partition, and the rule's own choice"""
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(2)
    x = torch.randn((S, n), dtype=torch.float32, device=dev, generator=g)
    h = torch.randn((Cn, P), dtype=torch.float32, device=dev, generator=g)
    out = torch.empty((S, Cn, n), dtype=torch.float32, device=dev)
    rows = []
    N = 256
    while N <= 16384:
        if P <= N // 2 + 1:
            filt = eng.conv_filter(h, plan=(N, N - P + 1, P, 1))
            t = median_ms(lambda: eng.fir_convolve(x, filt, out=out), reps)
            rows.append({"N": N, "Lk": N - P + 1, "ms": t[0], "min": t[1], "max": t[2]})
        N *= 2
    return {"P": P, "rule_N": eng.conv_plan(P)[0], "plans": rows}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--responses", type=int, default=64)
    ap.add_argument("--samples", type=int, default=262144)
    ap.add_argument("--calls", type=int, default=20, help="timed calls of fir_convolve (>= 20 for a figure to quote)")
    ap.add_argument("--calls-composition", type=int, default=10)
    ap.add_argument("--no-sweep", action="store_true")
    args = ap.parse_args()
    out = {"bench": "conv", "device": torch.cuda.get_device_name(0), "counters_collected": False}
    out["P8000_Q1"] = run(args.streams, args.responses, args.samples, 8000, args.calls, args.calls_composition)
    out["P32000_Q4"] = run(args.streams, args.responses, args.samples, 32000, args.calls, args.calls_composition)
    if not args.no_sweep:
        for P in (500, 2000):
            out["plan_sweep_P%d" % P] = plan_sweep(args.streams, args.responses, args.samples, P, max(args.calls // 2, 5))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
