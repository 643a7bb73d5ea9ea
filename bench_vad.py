#!/usr/bin/env python
"""Voice activity detection kernels (csrc/vad_kernels.hip), timed launch by launch.

Cases (M = 512, 4096 frames):
  energy_rows     vad_frame_energy over complex64 snapshot rows [40][512][4096]: all fftLen bins of a frame, frame-minor rows
  energy_frames   vad_frame_energy over float32 feature rows [40][4096][512]: one lane walks one contiguous frame
  band_power      vad_band_power (power, normalised energy, TSPS) over float32 power spectra [40][4][4096][257], bins 0 .. 256
  energy_metric   vad_energy_metric, energiesN = 200, for 1, 64 and 1024 streams: one wavefront per stream, sequential in time
Yardstick in the same run: btk_frame_energy (engine.frame_energy), the covariance gate's float32 frame energy over complex64
snapshots [40][257][1][4096].  The frame-parallel cases report algorithmic bytes (every input value read once, every output
written once) over the median time and its share of the HBM peak; the sequential metric reports nanoseconds per frame of one
stream (its chain) and per (frame, stream).  Every launch is timed with its own pair of HIP events after a warm-up: median of
--launches with min and max.  Prints one JSON line (kept as profiles/bench_vad_mi355x.json)."""
import argparse
import json

import torch

from bench_srp import median_ms
from bench_stages import HBM
from distant_speech_recognition_amd import engine as eng


def stat(t):
    return {"median": t[0], "min": t[1], "max": t[2]}


def bytes_entry(name, nbytes, t, **kw):
    return dict(case=name, algorithmic_bytes=float(nbytes), kernel_ms=stat(t), algorithmic_GBps=nbytes / (t[0] * 1e-3) / 1e9,
                hbm_roofline_share=nbytes / (t[0] * 1e-3) / HBM, **kw)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--fftlen", type=int, default=512)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--streams", type=int, default=40)
    ap.add_argument("--channels", type=int, default=4)
    ap.add_argument("--energies", type=int, default=200)
    ap.add_argument("--metric-streams", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--launches", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    M, T, S, Cn, n = args.fftlen, args.frames, args.streams, args.channels, args.launches
    K = M // 2 + 1
    g = torch.Generator(device=dev).manual_seed(1)
    res = []
    # yardstick: the covariance gate's frame energy
    X = torch.randn((S, K, 1, T), dtype=torch.complex64, device=dev, generator=g)
    res.append(bytes_entry("btk_frame_energy (yardstick)", S * K * T * 8 + S * T * 4, median_ms(lambda: eng.frame_energy(X, M), n),
                           S=S, K=K, T=T))
    Z = torch.randn((S, M, T), dtype=torch.complex64, device=dev, generator=g)
    res.append(bytes_entry("energy_rows", S * M * T * 8 + S * T * 8, median_ms(lambda: eng.vad_frame_energy(Z), n), S=S, D=M, T=T))
    del Z
    F = torch.randn((S, T, M), dtype=torch.float32, device=dev, generator=g)
    res.append(bytes_entry("energy_frames", S * M * T * 4 + S * T * 8, median_ms(lambda: eng.vad_frame_energy(F), n), S=S, D=M, T=T))
    del F
    spec = torch.randn((S, Cn, T, K), dtype=torch.float32, device=dev, generator=g) ** 2
    lowX, highX, _ = eng.vad_band_limits(M, 16000.0)
    for kind in ("power", "normalized", "tsps"):
        nbytes = S * Cn * T * (highX - lowX + 1) * 4 + S * Cn * T * 8 + 2 * S * T * 8
        res.append(bytes_entry("band_power " + kind, nbytes, median_ms(lambda: eng.vad_band_power(spec, kind, M, lowX, highX), n),
                               S=S, C=Cn, T=T, bins=highX - lowX + 1))
    del spec
    for Sm in args.metric_streams:
        energy = torch.rand((Sm, T), dtype=torch.float64, device=dev, generator=g) + 0.5
        st = eng.EnergyVADState(Sm, args.energies, 1.0, dev)
        t = median_ms(lambda: eng.vad_energy_metric(energy, st, 0.5, 4, 10), n)
        res.append(dict(case="energy_metric", S=Sm, T=T, energiesN=args.energies, kernel_ms=stat(t),
                        ns_per_frame_of_a_stream=t[0] * 1e6 / T, ns_per_frame_and_stream=t[0] * 1e6 / (T * Sm)))
    print(json.dumps({"bench": "vad", "device": torch.cuda.get_device_name(0),
                      "compute_units": torch.cuda.get_device_properties(0).multi_processor_count, "M": M, "hbm_peak_Bps": HBM,
                      "launches": n, "results": res}))


if __name__ == "__main__":
    main()
