#!/usr/bin/env python
"""Subband echo cancellation: aec_process (block Kalman and double-talk detecting block Kalman) against the same recursion
composed from batched torch complex128 operations, one frame at a time, timed in the same run.

Shapes: M = 256 and M = 512, sample_num P = 36 (the reference script's default), 4096 frames, with as many streams as fill the
chip: the block Kalman kernel runs one 256-thread workgroup per (stream, bin), so S = 2 streams x 129 bins is one workgroup per
compute unit; the double-talk kernel runs ONE workgroup per stream (the detector's scalars pass from bin to bin), so S = 256.
Every launch is timed with its own pair of HIP events after a warm-up; the figure is the median, with min and max.  The torch
composition is timed over `--composition-frames` frames from the same state and scaled to the block (its cost per frame does not
depend on the frame).  Prints one JSON line.
"""
import argparse
import json

import numpy as np
import torch

from bench_srp import median_ms
from distant_speech_recognition_amd import engine as eng


def inputs(S, K, T, P, dev, seed=1):
    g = torch.Generator(device=dev).manual_seed(seed)
    V = torch.randn((S, K, T), dtype=torch.complex64, device=dev, generator=g) * 3000.0
    h = torch.randn((S, K, P + 2), dtype=torch.complex64, device=dev, generator=g) * (0.6 ** torch.arange(P + 2, device=dev)) * 0.5
    A = torch.randn((S, K, T), dtype=torch.complex64, device=dev, generator=g) * 300.0
    for i in range(P + 2):
        A[..., i:] += h[..., i:i + 1] * V[..., :T - i]
    return V, A


class TorchAEC:
    """kind 2 / kind 3 of csrc/aec_kernels.hip, frame by frame, every bin and stream of a frame in one batched operation"""

    def __init__(self, kind, S, K, P, dev, p):
        self.kind, self.p, self.P = kind, p, P
        c = torch.complex128
        self.R = torch.zeros((S, K, P), dtype=c, device=dev)
        self.K = torch.eye(P, dtype=c, device=dev).repeat(S, K, 1, 1) * p["sigmak2"]
        self.sig = torch.full((S, K), p["sigmau2"], dtype=torch.float64, device=dev)
        self.hist = torch.zeros((S, K, P), dtype=c, device=dev)
        self.dtd = torch.zeros((3, S), dtype=torch.float64, device=dev)
        self.eye = torch.eye(P, dtype=c, device=dev)

    def frame(self, v0, a, fn):
        p = self.p
        self.hist = torch.cat([(v0 * p["amp4play"]).unsqueeze(-1), self.hist[..., :-1]], dim=-1)
        v = self.hist
        e = a - (self.R * v).sum(-1)
        e2 = e.real ** 2 + e.imag ** 2
        if self.kind == 2:
            upd = (v[..., 0].real ** 2 + v[..., 0].imag ** 2) > p["threshold"]
            sf = torch.ones_like(e2)
        else:
            smth = 1.0 - fn * (1.0 - p["smooth"]) / 100.0 if fn < 100 else p["smooth"]
            sk = a - e
            s2 = sk.real ** 2 + sk.imag ** 2
            snr_in = s2 / (e2 + 1.0e-15) * smth
            ek, skE, snr = self.dtd[0], self.dtd[1], self.dtd[2]
            sfs = []
            for m in range(e.shape[1]):                          # the ordered walk over the bins, all streams at once
                ek = e2[:, m] * smth + ek * (1.0 - smth)
                skE = s2[:, m] * smth + skE * (1.0 - smth)
                snr = snr_in[:, m] + snr * (1.0 - smth)
                s = 2.0 / (1.0 + torch.exp(-snr)) - 1.0
                if fn >= 100:
                    s = torch.where((snr > p["snr_threshold"]) & (skE > p["energy_threshold"]), s, torch.full_like(s, -1.0))
                sfs.append(s)
            self.dtd = torch.stack([ek, skE, snr])
            sf = torch.stack(sfs, dim=1)
            upd = sf >= 0
        svn = p["beta"] * self.sig + (1.0 - p["beta"]) * e2
        Kp = self.K + self.eye * (sf * p["sigmau2"]).unsqueeze(-1).unsqueeze(-1)
        s = (Kp @ v.conj().unsqueeze(-1)).squeeze(-1)
        u = (v.unsqueeze(-2) @ Kp).squeeze(-2)
        g = s / ((v * s).sum(-1).real + svn).unsqueeze(-1)
        m1, m2 = upd.unsqueeze(-1), upd.unsqueeze(-1).unsqueeze(-1)
        self.R = torch.where(m1, self.R + e.unsqueeze(-1) * g, self.R)
        self.K = torch.where(m2, Kp - g.unsqueeze(-1) * u.unsqueeze(-2), self.K)
        self.sig = torch.where(upd, svn, self.sig)
        return e


def run(kind, M, P, T, S, launches, comp_frames, dev):
    K = M // 2 + 1
    V, A = inputs(S, K, T, P, dev)
    kw = dict(beta=0.95, sigmau2=10e-6, sigmak2=5.0, amp4play=1.0)
    if kind == 2:
        kw["threshold"] = 100.0
    else:
        kw.update(snr_threshold=0.01, energy_threshold=10.0, smooth=0.95)
    st = eng.AECState(kind, S, M, P, device=dev, **kw)
    E = torch.empty_like(V)
    # agreement with the composition on the first frames of a fresh state (explicit frame numbers from 0)
    ref = TorchAEC(kind, S, K, P, dev, st.p)
    n = min(comp_frames, T)
    Er = torch.stack([ref.frame(V[..., t].to(torch.complex128), A[..., t].to(torch.complex128), t) for t in range(n)], dim=-1)
    En = eng.aec_process(V[..., :n].contiguous(), A[..., :n].contiguous(), eng.AECState(kind, S, M, P, device=dev, **kw), frame_no0=0)
    diff = float((En.to(torch.complex128) - Er).abs().max() / Er.abs().max())
    # E leaves the kernel as complex64 (2^-24 = 6e-8 relative); the composition sums in another order in float64.  1e-5 is two
    # orders above that and an order below the tolerance of the tests: beyond it the two are not the same recursion
    if not diff <= 1.0e-5:
        raise SystemExit("bench_aec: kind %d M=%d: aec_process and the torch composition differ by %.3g of max|E| on the first %d frames"
                         % (kind, M, diff, n))
    t_k = median_ms(lambda: eng.aec_process(V, A, st, out=E, frame_no0=200), launches)
    # the share of (stream, bin, frame) updates the gates let through in a launch like the timed ones (one more, with the map)
    fl = torch.zeros(V.shape, dtype=torch.uint8, device=dev)
    eng.aec_process(V, A, st, out=E, frame_no0=200, adapted=fl)
    share = float(fl.to(torch.float32).mean())
    finite = bool(torch.isfinite(torch.view_as_real(E)).all())

    def comp():
        for t in range(n):
            ref.frame(V[..., t].to(torch.complex128), A[..., t].to(torch.complex128), 200 + t)
    t_c = median_ms(comp, max(3, launches // 4))
    scale = T / float(n)
    # one complex multiply-add of the update = 8 flops; per adapting (stream, bin, frame): two P x P products and the rank-one update
    flops = 8.0 * 3 * P * P * S * K * T * share
    return {"kind": kind, "M": M, "K": K, "P": P, "T": T, "S": S, "dtd_state_in_lds": bool(st.dtd_state_in_lds()) if kind == 3 else None,
            "aec_process_ms": {"median": t_k[0], "min": t_k[1], "max": t_k[2], "launches": launches},
            "composition_ms_scaled_to_block": {"median": t_c[0] * scale, "min": t_c[1] * scale, "max": t_c[2] * scale, "frames_timed": n},
            "speedup_vs_composition": t_c[0] * scale / t_k[0], "updates_run_share": share, "output_finite": finite,
            "fp64_update_flops_per_s": flops / (t_k[0] * 1e-3),
            "stream_frames_per_s": S * T / (t_k[0] * 1e-3), "max_rel_diff_vs_composition": diff}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--filter-length", type=int, default=36)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--composition-frames", type=int, default=8)
    ap.add_argument("--fftlens", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--kinds", type=int, nargs="+", default=[2, 3])
    ap.add_argument("--streams-dtd", type=int, default=256, help="streams of the double-talk kernel: one workgroup each")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    res = []
    for M in args.fftlens:
        for kind in args.kinds:
            K = M // 2 + 1
            S = max(1, int(np.ceil(cus / K))) if kind == 2 else args.streams_dtd
            res.append(run(kind, M, args.filter_length, args.frames, S, args.launches, args.composition_frames, dev))
    print(json.dumps({"bench": "aec", "device": torch.cuda.get_device_name(0), "compute_units": cus, "results": res}))


if __name__ == "__main__":
    main()
