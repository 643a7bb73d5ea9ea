#!/usr/bin/env python
"""Objective measures (csrc/obj_kernels.hip), timed call by call: 64 pairs of 30 s at 16 kHz, M = 512, r = 1.

Cases:
  snr option 0 / 1 / 5   btk_obj_snr without the download of the result: one, two and three passes over the samples.  Bytes
                         that must move once: 8 n per pair (both signals, float32); their share of the HBM peak is reported
                         against the whole call, passes and finish included
  snr segments L = 256   the same with the optional segment rows (a fourth read of the samples)
  is_distance fused      btk_obj_is_distance: both transforms, the terms and the mean, 8 bytes written per frame
  is_distance unfused    the same numbers by two STFTBank.analysis launches (all M bins of every frame to HBM as complex64) and
                         a torch pass over the spectra
Recorded numbers, no threshold.  Timing: bench_util.gpu_time (HIP events around back-to-back calls after a pre-warm).  Prints
one JSON line (kept as profiles/bench_obj_mi355x.json)."""
import argparse
import ctypes as C
import json

import numpy as np
import torch

from bench_stages import HBM
from bench_util import gpu_time
from distant_speech_recognition_amd import _lib, engine as eng


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=30.0)
    ap.add_argument("--fftlen", type=int, default=512)
    ap.add_argument("--r", type=int, default=1)
    ap.add_argument("--segment", type=int, default=256)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    S, n, M, r, L = args.pairs, int(args.seconds * 16000), args.fftlen, args.r, args.segment
    g = torch.Generator(device=dev).manual_seed(1)
    x1 = torch.round(torch.randn((S, n), device=dev, generator=g) * 3000)
    x2 = x1 + torch.round(torch.randn((S, n), device=dev, generator=g) * 950)
    lens = np.full(S, n, np.int64)
    lp = lens.ctypes.data_as(C.c_void_p)
    lib = _lib.lib()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws = torch.empty(lib.btk_obj_snr_workspace_bytes(S, n) // 8, dtype=torch.float64, device=dev)
    stats = torch.empty((S, 6), dtype=torch.float64, device=dev)
    seg = torch.empty((S, n // L, 2), dtype=torch.float64, device=dev)
    res = []

    def snr(option, rows):
        eng.check(lib.btk_obj_snr(x1.data_ptr(), n, x2.data_ptr(), n, S, lp, lp, option, stats.data_ptr(), L if rows else 0,
                                  seg.data_ptr() if rows else None, n // L, ws.data_ptr(), stream))
    nbytes = 8.0 * n * S
    for name, option, rows in (("snr option 0", 0, False), ("snr option 1", 1, False), ("snr option 5", 5, False),
                               ("snr option 5, segments L=%d" % L, 5, True)):
        t, _ = gpu_time(torch, lambda: snr(option, rows))
        res.append(dict(case=name, S=S, n=n, must_move_bytes=nbytes, ms=t * 1e3, GBps=nbytes / t / 1e9, hbm_roofline_share=nbytes / t / HBM))

    bank = eng.STFTBank(M, r, 1)
    T = bank.num_frames(n)
    H = M // 2
    eis = torch.empty((S, T), dtype=torch.float64, device=dev)
    dist = torch.empty(S, dtype=torch.float64, device=dev)
    count = torch.empty(S, dtype=torch.int64, device=dev)

    def fused():
        eng.check(lib.btk_obj_is_distance(bank._h, x1.data_ptr(), n, x2.data_ptr(), n, S, lp, lp, 0, -1, dist.data_ptr(),
                                          count.data_ptr(), eis.data_ptr(), T, stream))
        return dist

    X1 = torch.empty((S, M, 1, T), dtype=torch.complex64, device=dev)
    X2 = torch.empty((S, M, 1, T), dtype=torch.complex64, device=dev)

    def power(X):
        a = X[:, 1:H + 1, 0, :]
        return (a.real.double() ** 2 + a.imag.double() ** 2).float()

    def unfused():
        bank.analysis(x1.view(S, 1, n), out=X1)
        bank.analysis(x2.view(S, 1, n), out=X2)
        P1, P2 = power(X1), power(X2)
        ratio = (P1 / P2).double()
        term = torch.where((P1 > 0) & (P2 > 0), ratio - torch.log(ratio) - 1.0, torch.zeros((), dtype=torch.float64, device=dev))
        return (term.sum(dim=1) / H).mean(dim=1)

    def analyses():
        bank.analysis(x1.view(S, 1, n), out=X1)
        bank.analysis(x2.view(S, 1, n), out=X2)

    tf, df = gpu_time(torch, fused)
    df = df.clone()
    tu, du = gpu_time(torch, unfused)
    ta, _ = gpu_time(torch, analyses)
    apart = float(((df - du).abs() / du.abs()).max())
    res.append(dict(case="is_distance fused", S=S, n=n, M=M, r=r, frames=T, ms=tf * 1e3, must_move_bytes=nbytes,
                    hbm_roofline_share=nbytes / tf / HBM))
    res.append(dict(case="is_distance unfused (2 x STFTBank.analysis + torch)", S=S, n=n, M=M, r=r, frames=T, ms=tu * 1e3,
                    analyses_ms=ta * 1e3, spectra_bytes=2.0 * 8 * M * T * S, largest_relative_difference_to_fused=apart))
    print(json.dumps({"bench": "obj", "device": torch.cuda.get_device_name(0),
                      "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "hbm_peak_Bps": HBM, "results": res}))


if __name__ == "__main__":
    main()
