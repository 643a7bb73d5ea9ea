#!/usr/bin/env python
"""Maximum-kurtosis beamformers: hos_eval against the same objective and gradient composed from the other entry points (bf_apply
plus torch reductions), and hos_minimize against the reference's scipy flow served by hos_eval, timed in the same run.

Shape: 64 microphones x 257 bins x 4096 observation frames, NS = 1, Nc = 1, NMEK.  The snapshots are a super-Gaussian target in
the look direction plus a super-Gaussian interferer and Gaussian noise, scaled so that the upper-branch output power is about 1
(only there do alpha, gtol and mindelta mean anything).  Every launch is timed with its own pair of HIP events after a warm-up
of back-to-back launches; the figure is the median of the timed launches, with min and max.  The scipy flow is host code around
one launch per evaluation and is timed by the wall clock on 8 bins, then scaled to 257.  Effective bytes/s count 8 N T K bytes
per evaluation pass (the snapshots of every bin once); an evaluation with the gradient reads every tile twice (phase 1, phase 2).
Prints one JSON line.
"""
import argparse
import json
import time

import numpy as np
import torch

from bench_srp import median_ms
from distant_speech_recognition_amd import engine as eng


def problem(K, N, T, dev, seed=1):
    rng = np.random.default_rng(seed)
    k = np.arange(K)[:, None]
    n = np.arange(N)[None, :]
    a_t = np.ones((K, N), complex)                                          # look direction: broadside
    a_j = np.exp(-2j * np.pi * k * n * 0.37 / K)                            # interferer
    def lap(shape):
        return rng.laplace(size=shape) * np.exp(2j * np.pi * rng.random(shape))
    s, j = lap((K, 1, T)), 0.7 * lap((K, 1, T))
    noise = 0.3 * (rng.normal(size=(K, N, T)) + 1j * rng.normal(size=(K, N, T)))
    X = (a_t[:, :, None] * s + a_j[:, :, None] * j + noise).astype(np.complex64)
    wuH = (np.conjugate(a_t) / N)[None]                                     # [1][K][N]
    # a stack of transposes comes out in the transposes' memory order: hos_eval wants the rows of BmH contiguous
    BmH = np.ascontiguousarray(np.stack([eng.weights_blocking_matrix(np.conjugate(wuH[0, kk]), 1).T for kk in range(K)])[None])
    pw = np.mean(np.abs(np.einsum("kn,knt->kt", wuH[0], X[:, :, :256])) ** 2)
    X = (X / np.sqrt(pw)).astype(np.complex64)
    return torch.from_numpy(X).to(dev), torch.from_numpy(wuH).to(dev), torch.from_numpy(BmH).to(dev)


def composition(X, Xd, wuH, BmH, x, alpha, beta):
    """fun and grad of MEK (no clamp, zero previous statistics) from bf_apply and torch reductions; Xd: X widened beforehand"""
    K, N, T = X.shape
    wa = torch.view_as_complex(x.reshape(K, N - 1, 2).contiguous())
    woH = wuH[0] - torch.einsum("kj,kjn->kn", wa.conj(), BmH[0])
    Y = eng.bf_apply(woH.conj().to(torch.complex64), X[None])[0].to(torch.complex128)
    y2 = Y.real ** 2 + Y.imag ** 2
    s2, s4 = y2.sum(-1), (y2 * y2).sum(-1)
    fun = -(s4 / T - beta * (s2 / T) ** 2 - 1.0e6) + alpha * (wa.real ** 2 + wa.imag ** 2).sum(-1)
    c2 = Y.conj()
    v2 = torch.einsum("kt,knt->kn", c2, Xd)
    v4 = torch.einsum("kt,knt->kn", 2 * y2 * c2, Xd)
    d2 = -torch.einsum("kjn,kn->kj", BmH[0], v2) / T
    d4 = -torch.einsum("kjn,kn->kj", BmH[0], v4) / T
    g = -(d4 - 2 * beta * (s2 / T)[:, None] * d2) + alpha * wa
    return fun, torch.view_as_real(g).reshape(K, -1)


def scipy_flow(X, wuH, BmH, bins, alpha, beta, gamma, solver="CG"):
    """estimate_wa_f_scipy (lib/pybeamformer.py:1767-1787) on the given bins, fun and jac served by hos_eval on that bin"""
    import scipy.optimize
    D = 2 * (X.shape[1] - 1)
    evals = 0
    t0 = time.perf_counter()
    for k in bins:
        Xk, wk, Bk = X[k:k + 1], wuH[:, k:k + 1].contiguous(), BmH[:, k:k + 1].contiguous()

        def both(x):
            f, g, _ = eng.hos_eval(Xk, wk, Bk, torch.from_numpy(x[None].copy()).to(X.device), alpha=alpha, beta=beta, gamma=gamma,
                                   normalize=True)
            return float(f.item()), g[0].cpu().numpy()
        calls = [0]

        def fun(x):
            calls[0] += 1
            return both(x)[0]
        scipy.optimize.minimize(fun, np.zeros(D), method=solver, jac=lambda x: both(x)[1], options={"maxiter": 40, "gtol": 1.0e-2})
        evals += calls[0]
    torch.cuda.synchronize()
    return time.perf_counter() - t0, evals


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mics", type=int, default=64)
    ap.add_argument("--fftlen", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=20, help="timed launches (>= 20 for a figure to quote)")
    ap.add_argument("--scipy-bins", type=int, default=8)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    K, N, T = args.fftlen // 2 + 1, args.mics, args.frames
    alpha, beta, gamma = 0.01, 3.0, -1.0
    X, wuH, BmH = problem(K, N, T, dev)
    D = 2 * (N - 1)
    g = torch.Generator(device=dev).manual_seed(2)
    x = 0.01 * torch.randn((K, D), dtype=torch.float64, device=dev, generator=g)
    Xd = X.to(torch.complex128)
    pass_bytes = 8.0 * N * T * K

    def ms(t):
        return {"median": t[0], "min": t[1], "max": t[2], "launches": args.launches}

    t_fg = median_ms(lambda: eng.hos_eval(X, wuH, BmH, x, alpha=alpha, beta=beta, gamma=gamma, normalize=False), args.launches)
    t_f = median_ms(lambda: eng.hos_eval(X, wuH, BmH, x, alpha=alpha, beta=beta, gamma=gamma, normalize=False, grad=False), args.launches)
    t_c = median_ms(lambda: composition(X, Xd, wuH, BmH, x, alpha, beta), args.launches)
    f1, g1, _ = eng.hos_eval(X, wuH, BmH, x, alpha=alpha, beta=beta, gamma=gamma, normalize=False)
    f2, g2 = composition(X, Xd, wuH, BmH, x, alpha, beta)
    out = {"bench": "hos", "device": torch.cuda.get_device_name(0), "N": N, "K": K, "T": T, "NS": 1, "Nc": 1,
           "hos_eval_fun_grad_ms": ms(t_fg), "hos_eval_fun_only_ms": ms(t_f), "composition_fun_grad_ms": ms(t_c),
           "eval_speedup_vs_composition": t_c[0] / t_fg[0],
           "eval_effective_bytes_per_s": pass_bytes / (t_fg[0] * 1e-3), "fun_only_effective_bytes_per_s": pass_bytes / (t_f[0] * 1e-3),
           "max_rel_diff_vs_composition": {"fun": float(((f1 - f2).abs() / f2.abs()).max()),
                                           "grad": float((g1 - g2).abs().max() / g2.abs().max())}}

    t_m = median_ms(lambda: eng.hos_minimize(X, wuH, BmH, alpha=alpha, beta=beta, gamma=gamma, normalize=True), args.launches)
    res = eng.hos_minimize(X, wuH, BmH, alpha=alpha, beta=beta, gamma=gamma, normalize=True)
    iters, halv = res.iters.cpu().numpy(), res.trace_halvings.cpu().numpy()
    trials = np.where(halv >= 0, halv + 1, np.where(halv == -1, 31, 0)).sum(1)          # objective-only passes
    grads = 1 + iters                                                                   # passes with the gradient
    f0, _, _ = eng.hos_eval(X, wuH, BmH, None, alpha=alpha, beta=beta, gamma=gamma, normalize=True, grad=False)
    out["hos_minimize_ms"] = ms(t_m)
    out["hos_minimize"] = {"iterations_min_median_max": [int(iters.min()), float(np.median(iters)), int(iters.max())],
                           "evaluations_per_bin_max": int((trials + grads).max()), "evaluations_total": int((trials + grads).sum()),
                           "objective_decrease_median": float(np.median((f0 - res.f).cpu().numpy())),
                           "effective_bytes_per_s": float((trials + grads).sum()) * 8.0 * N * T / (t_m[0] * 1e-3)}
    bins = np.linspace(1, K - 2, args.scipy_bins).astype(int)
    sec, evals = scipy_flow(X, wuH, BmH, bins, alpha, beta, gamma)
    out["scipy_flow"] = {"bins": [int(b) for b in bins], "seconds": sec, "fun_calls": evals, "seconds_scaled_to_all_bins": sec * K / len(bins)}
    out["minimize_speedup_vs_scipy_flow"] = sec * K / len(bins) / (t_m[0] * 1e-3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
