#!/usr/bin/env python
"""Steered-response-power DOA estimation: srp_power + srp_select against the only composition the other entry points offer
(one bf_apply per grid direction plus the torch reduction sum_k c_k |Y|^2), timed in the same run.

Shape: 64 microphones x 512-point banks x 32 streams x 4096 frames, the default 31-direction grid and a 1-degree grid (0..pi).
Every launch is timed with its own pair of HIP events after a warm-up of back-to-back launches (the shader clock needs ~0.3 s of
load to settle, bench_util.gpu_time); the figure is the median of the timed launches.  Rooflines: fp32 matrix peak over
8 U N nb T S flop, HBM peak over X read once + rp written once.  Prints one JSON line.
"""
import argparse
import json

import numpy as np
import torch

from bench_stages import HBM, FP32             # the peaks the per-stage benchmark measures against: 8 TB/s, 157.3 TFLOP/s fp32
from distant_speech_recognition_amd import engine as eng


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


def run(S, N, M, T, thetas, reps, reps_composition, nbest=3):
    dev = torch.device("cuda:0")
    K, nb, U = M // 2 + 1, M // 2, len(thetas)
    pos = np.arange(N) * 20.0 / 343740.0
    tbl = eng.srp_table(M, N, 16000.0, pos, thetas)
    table = eng.SRPTable(tbl, dev)
    g = torch.Generator(device=dev).manual_seed(1)
    X = torch.view_as_complex(torch.randn((S, K, N, T, 2), dtype=torch.float32, device=dev, generator=g))
    acc = torch.zeros((S, U), dtype=torch.float64, device=dev)

    def fused():
        rp, en = eng.srp_power(X, table, M)
        return rp, eng.srp_select(rp, en, nbest, 0.0, acc)

    def power_only():
        return eng.srp_power(X, table, M)

    W = torch.from_numpy(tbl.astype(np.complex64)).to(dev)                 # [U][K][N]
    W[:, 0] = 0
    c = torch.full((K,), 2.0, device=dev); c[0] = 0.0; c[K - 1] = 1.0
    Y = torch.empty((S, K, T), dtype=torch.complex64, device=dev)
    P = torch.empty((S, U, T), dtype=torch.float32, device=dev)

    def composition():
        for u in range(U):
            eng.bf_apply(W[u], X, out=Y)
            Yr = torch.view_as_real(Y)
            P[:, u] = torch.einsum("k,skt->st", c, Yr[..., 0] ** 2 + Yr[..., 1] ** 2) / nb
        return P

    t_f = median_ms(fused, reps)
    t_p = median_ms(power_only, reps)
    rp0, en0 = power_only()
    t_s = median_ms(lambda: eng.srp_select(rp0, en0, nbest, 0.0, acc), reps)
    t_c = median_ms(composition, reps_composition)
    rp = fused()[0]
    ref = composition()
    rel = float((rp - ref).abs().max() / ref.abs().max())
    flop = 8.0 * U * N * nb * T * S
    byts = 8.0 * S * nb * N * T + 4.0 * S * U * T
    return {"S": S, "N": N, "M": M, "T": T, "U": U,
            "fused_ms": {"median": t_f[0], "min": t_f[1], "max": t_f[2], "launches": reps},
            "srp_power_only_ms": t_p[0], "srp_select_only_ms": t_s[0],
            "composition_ms": {"median": t_c[0], "min": t_c[1], "max": t_c[2], "launches": reps_composition},
            "speedup": t_c[0] / t_f[0], "frames_per_s": S * T / (t_f[0] * 1e-3),
            "fp32_mfma_frac": flop / (t_f[0] * 1e-3) / FP32, "hbm_frac": byts / (t_f[0] * 1e-3) / HBM,
            "max_rel_diff_vs_composition": rel}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=32)
    ap.add_argument("--mics", type=int, default=64)
    ap.add_argument("--fftlen", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20, help="timed launches of the fused path (>= 20 for a figure to quote)")
    ap.add_argument("--launches-composition", type=int, default=20)
    args = ap.parse_args()
    out = {"bench": "srp", "device": torch.cuda.get_device_name(0)}
    out["grid_31"] = run(args.streams, args.mics, args.fftlen, args.frames, eng.srp_grid(), args.launches, args.launches_composition)
    out["grid_1deg"] = run(args.streams, args.mics, args.fftlen, args.frames, eng.srp_grid(0.0, np.pi, 0.0174533), args.launches,
                           args.launches_composition)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
