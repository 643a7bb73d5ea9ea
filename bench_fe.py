#!/usr/bin/env python
"""ASR front end: btk_fe_process PCM -> cepstra against the same computation composed from torch.fft.rfft and torch operations,
timed in the same run.

Shape: the MFCC chain of the reference's mfcc_extractor.py as that script evidently meant it -- 25 ms Hamming window, 10 ms
shift, pre-emphasis 0.95, 512-point transform, 257 power values, VTLN (version 2), 30 mel bands (version 2), log, 13 cepstra
(type 1) -- over --streams x --channels rows of --frames frames per launch (default 16 x 8 x 4096: half a million frames,
84 MB of PCM).  The composition uses the same tables as dense float64 matrices.  Every timed call is bracketed by its own pair
of HIP events after a warm-up of back-to-back calls; the figure is the median.  hbm_frac is the HBM peak's share taken by the
algorithmic bytes: 4 shift bytes of PCM read plus the requested outputs written per frame (the cepstra alone here; overlapping
frames re-read their samples from L2).  Prints one JSON line and writes it to --out (default profiles/bench_fe_mi355x.json).
"""
import argparse
import json
import os

import numpy as np
import torch

from bench_srp import median_ms
from bench_stages import HBM
from distant_speech_recognition_amd import engine as eng


def run(S, C, D, shift, L, T, reps, reps_composition, mu=0.95):
    dev = torch.device("cuda:0")
    n = (T - 1) * shift + D
    g = torch.Generator(device=dev).manual_seed(1)
    pcm = torch.round(torch.randn((S, C, n), dtype=torch.float32, device=dev, generator=g) * 3000.0)
    powN = L // 2 + 1
    vtln = eng.fe_vtln_table(powN, 0.94, 0.8, 2)
    mel = eng.fe_mel_table(powN, 16000, 100, 6800, 30, 2)
    dct = eng.fe_dct_table(1, 13, 30)
    kw = dict(D=D, shift=shift, L=L, T=T, preemph=mu, vtln=vtln, mel=mel, dct=dct)

    def k_cep():
        return eng.fe_process(pcm, "pcm", "cep", **kw)["cep"]

    def k_all():
        return eng.fe_process(pcm, "pcm", ("spectrum", "power", "vtln", "mel", "log", "cep"), **kw)

    win = 0.54 - 0.46 * torch.cos(2.0 * np.pi * torch.arange(D, dtype=torch.float64, device=dev) / (D - 1))
    Vt = torch.from_numpy(vtln.matrix().T.copy()).to(dev)
    Mt = torch.from_numpy(mel.matrix().T.copy()).to(dev)
    Dt = torch.from_numpy(dct.matrix().T.copy()).to(dev)

    def t_cep():
        fr = pcm.unfold(-1, D, shift)[:, :, :T]
        prior = torch.empty_like(fr)
        prior[..., 1:] = fr[..., :-1]
        prior[:, :, 1:, 0] = fr[:, :, :-1, -1]
        prior[:, :, 0, 0] = 0.0
        pe = (fr.to(torch.float64) - mu * prior.to(torch.float64)).to(torch.float32)
        w = (pe.to(torch.float64) * win).to(torch.float32)
        X = torch.fft.rfft(w, n=L, dim=-1)
        P = X.real * X.real + X.imag * X.imag
        v = (P.to(torch.float64) @ Vt).to(torch.float32)
        m = (v.to(torch.float64) @ Mt).to(torch.float32)
        val = m.to(torch.float64) + 1.0
        lg = torch.log10(torch.where(val <= 0.0, torch.ones_like(val), val)).to(torch.float32)
        return (lg.to(torch.float64) @ Dt).to(torch.float32)

    kc, ka, tc = median_ms(k_cep, reps), median_ms(k_all, reps), median_ms(t_cep, reps_composition)
    a, b = k_cep(), t_cep()
    frames = S * C * T
    byts = frames * (4 * shift + 4 * 13)
    return {"S": S, "C": C, "D": D, "shift": shift, "L": L, "T": T, "frames": frames,
            "kernel_ms": {"cep_only": kc[0], "cep_only_min": kc[1], "cep_only_max": kc[2], "all_stages": ka[0], "calls": reps},
            "torch_ms": {"cep": tc[0], "min": tc[1], "max": tc[2], "calls": reps_composition},
            "torch_over_kernel": tc[0] / kc[0], "frames_per_s": frames / (kc[0] * 1e-3),
            "algorithmic_bytes": byts, "hbm_frac": byts / (kc[0] * 1e-3) / HBM,
            "max_cep_diff": float((a - b).abs().max()), "max_cep": float(b.abs().max())}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=16)
    ap.add_argument("--channels", type=int, default=8)
    ap.add_argument("--window", type=int, default=400)
    ap.add_argument("--shift", type=int, default=160)
    ap.add_argument("--fftlen", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4096, help="frames per row and call")
    ap.add_argument("--calls", type=int, default=20, help="timed calls of the kernel (>= 20 for a figure to quote)")
    ap.add_argument("--calls-composition", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "bench_fe_mi355x.json"))
    args = ap.parse_args()
    out = {"bench": "fe", "device": torch.cuda.get_device_name(0)}
    out["result"] = run(args.streams, args.channels, args.window, args.shift, args.fftlen, args.frames, args.calls,
                        args.calls_composition)
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
