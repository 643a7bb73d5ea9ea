#!/usr/bin/env python
"""Two launches of the fused M = 512 kernel at the bench.py shape (32 streams x 64 mics x 4096 frames, float32 PCM, shared weights,
padded Y rows) for rocprofv3 --pmc passes (counters only, one group per run; profiles/r08_fused512_rows_once.txt).
BTK_LIB_PATH = another build of libbtkhip.so profiles that build.  With a directory of rocprofv3 CSVs as argument it prints the
mean counter values per dispatch of fused512_kernel instead."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

if len(sys.argv) > 1:
    import csv, glob
    from collections import defaultdict
    vals = defaultdict(list)
    for f in sorted(glob.glob(os.path.join(sys.argv[1], "**", "*counter_collection.csv"), recursive=True)):
        for r in csv.DictReader(open(f)):
            if "fused512_kernel" in r["Kernel_Name"]:
                vals[r["Counter_Name"]].append(float(r["Counter_Value"]))
    for c, v in sorted(vals.items()):
        print("%-28s %18.1f  (n=%d)" % (c, sum(v) / len(v), len(v)))
    sys.exit(0)

import torch
from distant_speech_recognition_amd import engine as eng, prototypes

dev = torch.device("cuda:0")
N, M, S, T = 64, 512, 32, 4096
h, _ = prototypes.load(M, 4, 1)
afb = eng.FilterBank(h, M, 4, 1, 2)
L = (T - afb.processing_delay + afb.lookahead) * (M // 2)
pcm = (torch.randn((S, N, L), device=dev) * 1000.0).round_()
W = torch.randn((M // 2 + 1, N), dtype=torch.complex64, device=dev) / N
Y = eng.padded_rows((S, M // 2 + 1, T), torch.complex64, dev)
for _ in range(2):
    afb.analysis_beamform(pcm, W, out=Y)
torch.cuda.synchronize()
print("fused launch: algorithmic bytes %d, window bytes %d" % ((4 * 256 * N + 8 * 257) * S * T, 4 * 256 * N * S * T))
