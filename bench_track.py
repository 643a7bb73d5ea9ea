#!/usr/bin/env python
"""EKF / IEKF speaker tracking: btk_ekf_track for many streams against btk20.pykalman's host classes (the reference's float64
numpy arithmetic, frame by frame) on the same lag / height tables, in the same run.

Shape: --streams independent trackers (default 4096) over a circular array of --mics microphones with all pairs (default 8:
28 pairs), --frames frames per launch (default 256), IEKF with three rounds.  The kernel is LATENCY-bound by construction -- one
wavefront per stream walks the frames in order, a few hundred dependent float64 operations per frame -- so the figure to read
is frames per second over all streams and what it removes (the per-frame host work and the nobs x nobs inverse of the
reference), not a fraction of a roofline.  The host classes are timed with the wall clock on --host-streams of the streams
(default 4) and compared with the kernel's result on those.  Every timed launch is bracketed by its own pair of HIP events
after a warm-up of back-to-back launches; the figure is the median.  Prints one JSON line and writes it to --out (default
profiles/bench_track_mi355x.json).
"""
import argparse
import contextlib
import io
import json
import os
import time

import numpy as np
import torch

from bench_srp import median_ms
from distant_speech_recognition_amd import engine as eng
from distant_speech_recognition_amd import pykalman, pytdoa

FS, SSPEED, THRESHOLD, MIN_PAIRS = 16000, 343740.0, 0.11, 3
NO_PEAK = eng.TDOA_NO_PEAK


class TableSource:
    """[delay, height] of one pair from stored rows, where a TDOAFeature stands"""

    def __init__(self, lag, height):
        self.lag, self.height = lag, height

    def next(self, frame_no):
        lg = int(self.lag[frame_no])
        return [None, 0.0] if lg == NO_PEAK else [float(lg) * (1.0 / FS), float(self.height[frame_no])]

    def reset(self):
        pass


def tables(S, mpos, pairs, T, seed=1):
    """integer lags of sources that drift in azimuth at a fixed polar angle, one frame in 16 without a detection"""
    rng = np.random.default_rng(seed)
    off = np.array([mpos[b] - mpos[a] for a, b in pairs])                      # [P][3]
    theta = rng.uniform(0.8, 1.4, size=(S, 1))
    phi = rng.uniform(-2.5, 2.5, size=(S, 1)) + 0.002 * np.arange(T)[None, :]
    u = np.stack([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta) * np.ones_like(phi)], axis=-1)   # [S][T][3]
    lag = np.rint(np.einsum("stk,pk->spt", u, off) / SSPEED * FS).astype(np.int32)
    height = (0.3 + 0.4 * rng.random(lag.shape)).astype(np.float32)
    height[:, :, 15::16] = 0.01
    return lag, height, np.concatenate([theta, phi[:, :1]], axis=1)


def host_track(lag, height, mpos, pairs, F, U, sigmaV2, sigmaK2, frame_s, x0):
    """-> (seconds, x [T][2], flags [T]) of the host classes over one stream's tables"""
    T = lag.shape[1]
    srcs = [pytdoa.MicrophonePairSource(p, a, b, TableSource(lag[p], height[p])) for p, (a, b) in enumerate(pairs)]
    vec = pytdoa.FarfieldCircularArrayTDOAFeatureVector(srcs, mpos, MIN_PAIRS, THRESHOLD, SSPEED)
    trk = pykalman.IteratedExtendedKalmanFilter(vec, F, U, sigmaV2, sigmaK2, frame_s, initialXk=x0.copy(), gate_prob=0.95,
                                                num_iterations=3, iteration_threshold=1e-4)
    trk.set_time(0)
    xs, fl = np.zeros((T, 2)), np.zeros(T, np.int32)
    with contextlib.redirect_stdout(io.StringIO()):
        t0 = time.perf_counter()
        for t in range(T):
            xs[t] = trk.next(t)
            fl[t] = eng.EKF_TRACKED | (eng.EKF_OBSERVED if trk.observed else 0) | \
                ((eng.EKF_UPDATED | (trk.rounds << eng.EKF_ROUNDS_SHIFT)) if trk.updated else 0)
        seconds = time.perf_counter() - t0
    return seconds, xs, fl


def run(S, mics, T, reps, host_streams, sigmaK2=1e2, sigmaV2=4e-4):
    dev = torch.device("cuda:0")
    ang = 2 * np.pi * np.arange(mics) / mics
    mpos = np.stack([100.0 * np.cos(ang), 100.0 * np.sin(ang), np.zeros(mics)], axis=1)
    mpos[-1, 2] = 30.0
    pairs = [(a, b) for a in range(mics) for b in range(a + 1, mics)]
    lag, height, x0 = tables(S, mpos, pairs, T)
    frame_s = 256.0 / FS
    F, U = np.identity(2), 10.0 * np.identity(2)
    prm = eng.ekf_params("circular", "iekf", F, U, sigmaV2, frame_s, gate_prob=0.95, num_iterations=3, iteration_threshold=1e-4,
                         threshold=THRESHOLD, minimum_pairs=MIN_PAIRS, Ts=1.0 / FS, c=SSPEED)
    geom = np.zeros((len(pairs), 6))
    geom[:, :3] = [mpos[b] - mpos[a] for a, b in pairs]
    lag_d, height_d, geom_d = torch.from_numpy(lag).to(dev), torch.from_numpy(height).to(dev), torch.from_numpy(geom).to(dev)

    rec = np.zeros((S, 16))                      # x, K_filter (3 x 3 row-major), time, lastUpdateT
    rec[:, :2], rec[:, 3], rec[:, 7], rec[:, 13] = x0, sigmaK2, sigmaK2, -1.0
    state0 = torch.from_numpy(rec).to(dev)
    state = state0.clone()

    def k_track():
        state.copy_(state0)
        return eng.ekf_track(lag_d, height_d, geom_d, prm, state)

    med, lo, hi = median_ms(k_track, reps)
    xk, Kf, flags = (t.cpu().numpy() for t in k_track())

    # the host classes on the first host_streams streams (scipy's incomplete gamma function loaded before the clock starts)
    pykalman._chi_cdf(1.0, 2)
    t_host, dx, flags_equal = 0.0, 0.0, True
    for s in range(host_streams):
        seconds, xs, fl = host_track(lag[s], height[s], mpos, pairs, F, U, sigmaV2, sigmaK2, frame_s, x0[s])
        t_host += seconds
        dx = max(dx, float(np.abs(xs - xk[s, :, :2]).max()))
        flags_equal = flags_equal and bool(np.array_equal(fl, flags[s]))
    host_us = t_host / (host_streams * T) * 1e6
    kernel_us = med * 1e3 / (S * T)
    return {"S": S, "mics": mics, "pairs": len(pairs), "T": T, "type": "iekf", "sigmaK2": sigmaK2, "sigmaV2": sigmaV2,
            "kernel_ms": med, "kernel_ms_min": lo, "kernel_ms_max": hi, "calls": reps,
            "stream_frames_per_s": S * T / (med * 1e-3), "kernel_us_per_stream_frame": kernel_us,
            "frame_latency_us": med * 1e3 / T,
            "host_us_per_stream_frame": host_us, "host_streams": host_streams, "host_over_kernel": host_us / kernel_us,
            "observed_frac": float(((flags & eng.EKF_OBSERVED) != 0).mean()), "updated_frac": float(((flags & eng.EKF_UPDATED) != 0).mean()),
            "flags_equal_host": flags_equal, "max_x_diff_host": dx}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--mics", type=int, default=8)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--calls", type=int, default=20, help="timed launches (>= 20 for a figure to quote)")
    ap.add_argument("--host-streams", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "bench_track_mi355x.json"))
    args = ap.parse_args()
    out = {"bench": "track", "device": torch.cuda.get_device_name(0)}
    out["result"] = run(args.streams, args.mics, args.frames, args.calls, min(args.host_streams, args.streams))
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as fp:
            fp.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
