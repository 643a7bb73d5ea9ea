#!/usr/bin/env python
"""What the edge tiles of the fused M = 512 kernel cost (profiles/r07_fused512_edge_tiles.txt).

One process, warm clocks, the launches below taken in rotation; every launch has 32 streams x 64 channels x 4096 frames = 256 tiles
per stream on the same grid, and differs only in which tiles' spans leave the recording:
   bench  the bench.py launch itself (its own buffer: t0 = 0, nsamples = 4092 * 256)
   both   the same on the long buffer (row pitch 4116 * 256): first and last tile of every stream are edge tiles
   first  t0 = 0, the recording longer than the last span: only the first tile
   last   t0 = 16, the recording ends inside the last span: only the last tile
   none   t0 = 16, the recording longer than the last span: no edge tile
   cut    the issue's form: the bench buffer with t0 = 16, tcount = 4064 (254 tiles per stream, no edge tile); per-frame figure
Prints one JSON line: medians, and per round the differences to `none` (their spread is the noise the prize is set against).
BTK_FUSED512_NEW=0 in the environment selects the parent's kernel (the switch is read once per process); BTK_LIB_PATH = another
build of libbtkhip.so times that build."""
import os, sys, json, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from distant_speech_recognition_amd import engine as eng, prototypes
from distant_speech_recognition_amd.pybeamformer import calc_la_delays
from bench_util import ula_positions

dev = torch.device("cuda:0")
N, M, S, T = 64, 512, 32, 4096
D, K = M // 2, M // 2 + 1
ROUNDS = int(os.environ.get("EDGE_AB_ROUNDS", "10"))
REPS = int(os.environ.get("EDGE_AB_REPS", "20"))
h, _ = prototypes.load(M, 4, 1)
afb = eng.FilterBank(h, M, 4, 1, 2)
L = (T - afb.processing_delay + afb.lookahead) * D
assert afb.num_frames(L) == T and L == 4092 * 256
LL = 4116 * 256
g = torch.Generator(device=dev).manual_seed(7)
pcm_long = (torch.randn((S, N, LL), device=dev, generator=g) * 1000.0).round_()
pcm = pcm_long[:, :, :L].contiguous()
delays = calc_la_delays(ula_positions(N), -1.306379)
wq = eng.weights_mainlobe(M, N, 16000.0, delays)
rng = np.random.default_rng(0)
wl = np.zeros((M, N), np.complex128)
for k in range(1, K):
    wl[k] = eng.weights_sidelobe(eng.weights_blocking_matrix(wq[k], 1), (rng.normal(size=N - 1) + 1j * rng.normal(size=N - 1)) * 0.01)
W = torch.from_numpy(eng.weights_gsc_effective(wq, wl, M)).to(dev)
Y = eng.padded_rows((S, K, T), torch.complex64, dev)

cases = {
    "bench": (lambda: afb.analysis_beamform(pcm, W, out=Y), T),
    "both":  (lambda: afb.analysis_beamform(pcm_long, W, nsamples=L, t0=0, tcount=T, out=Y), T),
    "first": (lambda: afb.analysis_beamform(pcm_long, W, nsamples=LL, t0=0, tcount=T, out=Y), T),
    "last":  (lambda: afb.analysis_beamform(pcm_long, W, nsamples=4108 * 256, t0=16, tcount=T, out=Y), T),
    "none":  (lambda: afb.analysis_beamform(pcm_long, W, nsamples=LL, t0=16, tcount=T, out=Y), T),
    "cut":   (lambda: afb.analysis_beamform(pcm, W, t0=16, tcount=T - 32, out=Y), T - 32),
}
names = list(cases)
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
import time
t = time.perf_counter()
while time.perf_counter() - t < 1.0:                     # warm clocks: back-to-back launches, no host synchronisation between them
    for n in names:
        for _ in range(4):
            cases[n][0]()
    torch.cuda.synchronize()
ms = {n: [] for n in names}
for rnd in range(ROUNDS):
    order = names if rnd % 2 == 0 else names[::-1]       # alternate the order: no case always follows the same neighbour
    for n in order:
        fn = cases[n][0]
        fn()
        e0.record()
        for _ in range(REPS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ms[n].append(e0.elapsed_time(e1) / REPS)
res = {"BTK_FUSED512_NEW": os.environ.get("BTK_FUSED512_NEW"), "BTK_LIB_PATH": os.environ.get("BTK_LIB_PATH"), "rounds": ROUNDS, "launches_per_round": REPS,
       "median_ms": {n: round(statistics.median(v), 5) for n, v in ms.items()},
       "min_ms": {n: round(min(v), 5) for n, v in ms.items()},
       "max_ms": {n: round(max(v), 5) for n, v in ms.items()},
       "ns_per_frame_median": {n: round(statistics.median(v) * 1e6 / (S * cases[n][1]), 4) for n, v in ms.items()}}
res["diff_to_none_us"] = {n: {"median": round(statistics.median([a - b for a, b in zip(ms[n], ms["none"])]) * 1e3, 2),
                              "min": round(min(a - b for a, b in zip(ms[n], ms["none"])) * 1e3, 2),
                              "max": round(max(a - b for a, b in zip(ms[n], ms["none"])) * 1e3, 2)}
                          for n in names if n not in ("none", "cut")}
print(json.dumps(res), flush=True)
