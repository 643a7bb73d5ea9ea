#!/usr/bin/env python
"""Multichannel cross-correlation localisation: mcc_costs + mcc_select (csrc/mcc_kernels.hip) against the composition one would
otherwise write in torch (gather of the shifted samples, batched float64 matmul, torch.linalg.cholesky, log sums, argmin),
timed in the same run; the two are checked against each other.

Shapes: 64 microphones 20 mm apart (D = 58, 120 grid points at 16 kHz) and 8 microphones (D = 6, 15 points), 32 streams x 64
blocks of 4096 samples.  Every launch is timed with its own pair of HIP events after a warm-up of back-to-back launches; the
figure is the median of the timed launches, with the fastest and the slowest next to it.  The matrix work is
N (N + 1) nS flop per (stream, block, grid point) on the lower triangle (what the kernel issues: 16 x 16 tiles, 2 x 16 x 16 x 4
flop per instruction), set against the FP64 matrix peak AMD publishes for the MI355X (78.6 TFLOP/s).  Prints one JSON line.
"""
import argparse
import json

import numpy as np
import torch

from distant_speech_recognition_amd import engine as eng

FP64_MATRIX = 78.6e12


def median_ms(fn, reps, warm_ms=300.0):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record()
    torch.cuda.synchronize()
    t1 = max(e0.elapsed_time(e1), 1e-3)
    for _ in range(int(min(max(warm_ms / t1, 1), 200))):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record(); fn(); b.record()
    torch.cuda.synchronize()
    ts = sorted(a.elapsed_time(b) for a, b in ev)
    return ts[len(ts) // 2], ts[0], ts[-1]


def run(S, N, B, L, spacing, reps, reps_composition, nbest=1):
    dev = torch.device("cuda:0")
    grid = eng.mcc_linear_grid(16000, N, spacing=spacing)
    tau, D = grid["tau"], grid["D"]
    G, nS = len(tau), L - D
    g = torch.Generator(device=dev).manual_seed(1)
    # a common source plus independent noise 10 dB down, integers at PCM scale
    src = torch.randn((S, 1, B * L), device=dev, generator=g) * 3000.0
    x = torch.round(src + torch.randn((S, N, B * L), device=dev, generator=g) * 950.0).to(torch.float32).contiguous()
    del src

    def fused():
        cost, flag = eng.mcc_costs(x, tau, L, D)
        return cost, eng.mcc_select(cost, nbest)

    def costs_only():
        return eng.mcc_costs(x, tau, L, D)

    f = torch.arange(nS, device=dev)
    tau_d = torch.from_numpy(tau.astype(np.int64)).to(dev)
    xb = x.view(S, N, B, L).permute(0, 2, 1, 3)                             # [S][B][N][L]
    out = torch.empty((S, B, G), dtype=torch.float64, device=dev)

    def composition():
        for c in range(G):
            idx = f[None, :] + tau_d[c][:, None]                            # [N][nS]
            idx = torch.where(idx < 0, idx + L, idx)
            xt = torch.gather(xb, 3, idx.expand(S, B, N, nS)).to(torch.float64)
            R = torch.matmul(xt, xt.transpose(-1, -2)) * (1.0 / nS)
            ch = torch.linalg.cholesky(R)
            out[:, :, c] = 2.0 * torch.log(torch.diagonal(ch, dim1=-2, dim2=-1)).sum(-1) - torch.log(torch.diagonal(R, dim1=-2, dim2=-1)).sum(-1)
        return out, torch.argmin(out, dim=-1)

    t_f = median_ms(fused, reps)
    t_c = median_ms(costs_only, reps)
    cost0 = costs_only()[0]
    t_s = median_ms(lambda: eng.mcc_select(cost0, nbest), reps)
    t_o = median_ms(composition, reps_composition, warm_ms=0.0)
    cost, (nbc, nbi) = fused()
    ref, best = composition()
    diff = float((cost - ref).abs().max())
    same = float((nbi[..., 0].long() == best).double().mean())
    flop = float(N) * (N + 1) * nS * S * B * G
    tiles = ((N + 15) // 16) * ((N + 15) // 16 + 1) // 2
    issued = 2048.0 * tiles * ((nS + 3) // 4) * S * B * G
    return {"S": S, "N": N, "B": B, "L": L, "D": D, "G": G,
            "fused_ms": {"median": t_f[0], "min": t_f[1], "max": t_f[2], "launches": reps},
            "mcc_costs_only_ms": t_c[0], "mcc_select_only_ms": t_s[0],
            "composition_ms": {"median": t_o[0], "min": t_o[1], "max": t_o[2], "launches": reps_composition},
            "speedup": t_o[0] / t_f[0], "blocks_per_s": S * B / (t_f[0] * 1e-3),
            "fp64_matrix_frac_useful": flop / (t_c[0] * 1e-3) / FP64_MATRIX,
            "fp64_matrix_frac_issued": issued / (t_c[0] * 1e-3) / FP64_MATRIX,
            "max_abs_cost_diff_vs_composition": diff, "best_index_agreement": same}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=64)
    ap.add_argument("--block", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20, help="timed launches of the fused path (>= 20 for a figure to quote)")
    ap.add_argument("--launches-composition", type=int, default=3)
    args = ap.parse_args()
    out = {"bench": "mcc", "device": torch.cuda.get_device_name(0)}
    out["mics_64"] = run(args.streams, 64, args.blocks, args.block, 20.0, args.launches, args.launches_composition)
    out["mics_8"] = run(args.streams, 8, args.blocks, args.block, 20.0, args.launches, args.launches_composition)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
