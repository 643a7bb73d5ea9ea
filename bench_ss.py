#!/usr/bin/env python
"""Spectral subtraction and Wiener filter: spectral_subtract / wiener_filter (csrc/ss_kernels.hip) against the same outputs
composed from torch elementwise operations, timed in the same run.

Shapes: M = 512 (257 bins), 4096 frames in padded rows, C = 1 and C = 4 channels, and as many streams as make a launch move at
least 1 GB of algorithmic bytes: every input bin-frame read once and every output bin-frame written once, (C + 1) x 8 B per
bin-frame (the Wiener filter reads target and noise: 24 B).  Cases:
  subtract_fixed    a fixed noise model, subtraction only: the frame-parallel kernel (the production case)
  train_subtract    recursive training and subtraction in the same pass: the row-scan kernel
  wiener            the Wiener filter with the noise PSD updated in every frame: the row-scan kernel
subtract_fixed is compared with, and timed against, the torch composition of the whole block.  The two recursions are compared
with a per-frame torch float64 loop over the first `--composition-frames` frames of a fresh state; that loop's time is scaled to
the block (its cost per frame does not depend on the frame).  The timed launches of the two recursions run on a state that the
launches before them have trained further (the arithmetic per frame is the same); agreement is checked on the fresh prefix
only, not on the timed configuration.  Every launch is timed with its own pair of HIP events after a
warm-up; the figure is the median, with min and max.  The roofline is the HBM peak over the algorithmic bytes.  Prints one JSON
line."""
import argparse
import json

import torch

from bench_srp import median_ms
from bench_stages import HBM
from distant_speech_recognition_amd import engine as eng

ALPHA, FT, FLOOR, BETA = 0.9375, 1.5, 0.001, 1.0


def rand_rows(shape, dev, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    X = eng.padded_rows(shape, torch.complex64, dev)
    X.copy_(torch.randn(shape, dtype=torch.complex64, device=dev, generator=g))
    return X


def torch_subtract(X, est, ft, floor):
    """the fixed-model subtraction from elementwise torch operations, float32: X [S][K][C][T], est [S][C][K]"""
    p = X.real * X.real + X.imag * X.imag
    s2 = torch.clamp_min(p - ft * est.permute(0, 2, 1).unsqueeze(-1).to(torch.float32), floor)
    g = torch.sqrt(s2) / torch.sqrt(p)
    return (X * g).mean(dim=2)


def torch_train_subtract_frames(X, n, alpha, ft, floor):
    """recursive training + subtraction, one frame at a time, float64; a fresh state: the first frame is copied"""
    est, out = None, []
    for t in range(n):
        x = X[..., t].to(torch.complex128)
        p = x.real ** 2 + x.imag ** 2
        est = p if est is None else alpha * est + (1.0 - alpha) * p
        s2 = torch.clamp_min(p - ft * est, floor)
        out.append((x * (torch.sqrt(s2) / torch.sqrt(p))).mean(dim=2))
    return torch.stack(out, dim=-1)


def torch_wiener_frames(Sx, Nx, n, alpha, floor, beta, f0=0, ps=None, pn=None):
    out = []
    for t in range(n):
        s, nn = Sx[..., t].to(torch.complex128), Nx[..., t].to(torch.complex128)
        a = alpha if f0 + t >= 2 else 0.0
        cs = s.real ** 2 + s.imag ** 2
        cn = torch.clamp_min(nn.real ** 2 + nn.imag ** 2, floor)
        ps = cs if ps is None else a * ps + (1.0 - a) * cs
        pn = cn if pn is None else a * pn + (1.0 - a) * cn
        y = s * (ps / (ps + beta * pn))
        y[:, 0] = s[:, 0]
        out.append(y)
    return torch.stack(out, dim=-1), ps, pn


def rel_diff(a, b):
    return float((a.to(torch.complex128) - b.to(torch.complex128)).abs().max() / b.abs().max())


def entry(name, C, S, K, T, bytes_per_binframe, t_k, t_c, comp_frames, diff, form):
    nbytes = float(bytes_per_binframe) * S * K * T
    return {"case": name, "C": C, "S": S, "K": K, "T": T, "kernel_form": form, "algorithmic_bytes": nbytes,
            "kernel_ms": {"median": t_k[0], "min": t_k[1], "max": t_k[2]},
            "composition_ms": {"median": t_c[0], "min": t_c[1], "max": t_c[2], "frames_timed": comp_frames,
                               "scaled_to_block": comp_frames != T},
            "speedup_vs_composition": t_c[0] / t_k[0], "algorithmic_GBps": nbytes / (t_k[0] * 1e-3) / 1e9,
            "hbm_roofline_share": nbytes / (t_k[0] * 1e-3) / HBM, "max_rel_diff_vs_composition": diff}


def check(diff, what):
    # complex64 outputs (2^-24 = 6e-8 relative) of float32 arithmetic against float32 / float64 compositions that round elsewhere;
    # beyond 1e-4 of the largest output the two are not the same computation (the tests hold the kernels to derived bounds)
    if not diff <= 1.0e-4:
        raise SystemExit("bench_ss: %s: kernel and torch composition differ by %.3g of max|Y|" % (what, diff))


def run(M, T, C, S, launches, n, dev):
    K = M // 2 + 1
    res = []
    X = rand_rows((S, K, C, T), dev, seed=C)
    Y = eng.rows_like(X, (S, K, T))
    # (a) fixed model
    st = eng.SpectralSubtractionState(S, C, M, [ALPHA] * C, device=dev)
    st.set_noise_psd(torch.rand((S, C, K), dtype=torch.float64, device=dev) + 0.5)
    eng.spectral_subtract(X, st, ft=FT, floor=FLOOR, train=False, subtract=True, out=Y)
    diff = rel_diff(Y, torch_subtract(X, st.est, FT, FLOOR))
    check(diff, "subtract_fixed C=%d" % C)
    t_k = median_ms(lambda: eng.spectral_subtract(X, st, ft=FT, floor=FLOOR, train=False, subtract=True, out=Y), launches)
    t_c = median_ms(lambda: torch_subtract(X, st.est, FT, FLOOR), max(3, launches // 4))
    res.append(entry("subtract_fixed", C, S, K, T, (C + 1) * 8, t_k, t_c, T, diff, "frames"))
    # (b) recursive training and subtraction in one pass
    fresh = eng.SpectralSubtractionState(S, C, M, [ALPHA] * C, device=dev)
    Yn = eng.spectral_subtract(X[..., :n], fresh, ft=FT, floor=FLOOR, train=True, subtract=True)
    diff = rel_diff(Yn, torch_train_subtract_frames(X, n, ALPHA, FT, FLOOR))
    check(diff, "train_subtract C=%d" % C)
    t_k = median_ms(lambda: eng.spectral_subtract(X, st, ft=FT, floor=FLOOR, train=True, subtract=True, out=Y), launches)
    t_c = median_ms(lambda: torch_train_subtract_frames(X, n, ALPHA, FT, FLOOR), max(3, launches // 4))
    scale = T / float(n)
    res.append(entry("train_subtract", C, S, K, T, (C + 1) * 8, t_k, tuple(v * scale for v in t_c), n, diff, "rows"))
    return res


def run_wiener(M, T, S, launches, n, dev):
    K = M // 2 + 1
    Sx, Nx = rand_rows((S, K, T), dev, seed=11), rand_rows((S, K, T), dev, seed=12)
    Y = eng.rows_like(Sx, (S, K, T))
    fresh = eng.WienerState(S, M, device=dev)
    Yn = eng.wiener_filter(Sx[..., :n], Nx[..., :n], fresh, alpha=ALPHA, floor=FLOOR, beta=BETA)
    diff = rel_diff(Yn, torch_wiener_frames(Sx, Nx, n, ALPHA, FLOOR, BETA)[0])
    check(diff, "wiener")
    st = eng.WienerState(S, M, device=dev)
    t_k = median_ms(lambda: eng.wiener_filter(Sx, Nx, st, alpha=ALPHA, floor=FLOOR, beta=BETA, out=Y), launches)
    t_c = median_ms(lambda: torch_wiener_frames(Sx, Nx, n, ALPHA, FLOOR, BETA), max(3, launches // 4))
    scale = T / float(n)
    return entry("wiener", 2, S, K, T, 24, t_k, tuple(v * scale for v in t_c), n, diff, "rows")


def streams_for(K, T, bytes_per_binframe, target_bytes):
    return max(1, -(-int(target_bytes) // (bytes_per_binframe * K * T)))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fftlen", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--channels", type=int, nargs="+", default=[1, 4])
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--composition-frames", type=int, default=16)
    ap.add_argument("--bytes", type=float, default=1.0e9, help="algorithmic bytes a launch moves at least")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K = args.fftlen // 2 + 1
    res = []
    for C in args.channels:
        S = streams_for(K, args.frames, (C + 1) * 8, args.bytes)
        res += run(args.fftlen, args.frames, C, S, args.launches, args.composition_frames, dev)
    res.append(run_wiener(args.fftlen, args.frames, streams_for(K, args.frames, 24, args.bytes), args.launches,
                          args.composition_frames, dev))
    print(json.dumps({"bench": "ss", "device": torch.cuda.get_device_name(0),
                      "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "M": args.fftlen,
                      "hbm_peak_Bps": HBM, "results": res}))


if __name__ == "__main__":
    main()
