"""GPU: fused512_kernel (fb_fused512.hip: edge tiles dispatched first and served by the direct window loads) against the kernel it
replaces on the production launch, analysis512_bfz_kernel<2, 33231> (fb_analysis512.hip) -- the same bits -- and against the
float64 closed form of tests/closed_forms.py.

BTK_FUSED512_NEW is read once per process, so every launch below runs in two child processes, one with BTK_FUSED512_NEW=0 (the
parent kernel) and one with the switch unset; the two Y are compared on their int32 view.

Fixed: M = 512, m = 4, r = 1, dct = 2 (look-ahead 3 frames: the span of tile i of a launch at t0 is
[(t0 + 16 i - 4) 256, (t0 + 16 i + 19) 256)).  Varied: N in {1, 3, 64}; S = 1, S = 3 with shared and with per-stream W; float32 and
int16 PCM; and the (t0, tcount, nsamples) of GEOMETRIES, chosen so that every way a tile can meet the recording's boundaries
occurs: only the first tile an edge tile, only the last, both, every tile (tcount <= 16 and 17), a recording that is no multiple of
256 samples long with an odd length (the end cuts an 8-byte window row) and an even one, a recording that ends inside the first
window row of its tile, t0 > 0, and a launch with no edge tile at all.  The rows are a multiple of 4 samples apart and 16-byte
aligned with nsamples < pitch, the samples behind nsamples are 12345 (must not be read as signal); the MISALIGNED launches
repeat every geometry with the base pointer 4 bytes past a 16-byte boundary and an odd pitch, which the register-staged loop serves.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from tests import closed_forms as cf
from tests.util import design_prototype

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, m, r, DCT, K, D = 512, 4, 1, 2, 257, 256

# (label, t0, tcount, nsamples)
GEOMETRIES = [
    ("first tile only", 0, 33, 60 * D),
    ("last tile only, t0 = 4", 4, 48, 50 * D),
    ("first and last", 0, 48, 44 * D),
    ("one tile, 1 frame", 0, 1, 12 * D),
    ("one tile, 15 frames", 0, 15, 12 * D),
    ("one tile, 16 frames", 0, 16, 12 * D),
    ("two tiles, both edge", 0, 17, 13 * D),
    ("odd length: a cut row", 0, 48, 43 * D + 101),
    ("even length, no multiple of 256", 0, 48, 43 * D + 100),
    ("ends inside the first row", 12, 1, 8 * D + 57),
    ("ends inside the first row, odd, whole recording", 0, 7, 2 * D + 57),
    ("no edge tile, t0 = 5", 5, 33, 70 * D),
    ("t0 = 16, both tiles cut by an odd end", 16, 17, 30 * D + 1),
]
LMAX = max(g[3] for g in GEOMETRIES)
STREAMS = [(1, False), (3, False), (3, True)]                       # S, per-stream W
CASES = [(gi, N, S, ps, i16, False) for gi in range(len(GEOMETRIES)) for N in (1, 3, 64) for (S, ps) in STREAMS for i16 in (False, True)]
CASES += [(gi, 3, 3, True, i16, True) for gi in range(len(GEOMETRIES)) for i16 in (False, True)]      # misaligned: the staged loop
CF_PROTOS = ("dense", "shipped")
CF_N, CF_T, CF_S = 3, 33, 2


def _proto(name):
    return cf.dense_prototype(M, m) if name == "dense" else design_prototype(M, m, "h")


def _cf_inputs():
    L = cf.num_samples(CF_T, M, m, r, DCT)
    return cf.int_pcm(CF_S, CF_N, L, seed=512), cf.unit_weights(CF_S, K, CF_N, seed=33), L


def _key(case):
    gi, N, S, ps, i16, mis = case
    return "g%d_N%d_S%d_%s_%s_%s" % (gi, N, S, "own" if ps else "shared", "i16" if i16 else "f32", "mis" if mis else "al")


def _child_main(out_path):
    """Every launch of CASES and the closed-form launches, in this process's setting of the switch."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    dev = torch.device("cuda", 0)
    fb = eng.FilterBank(design_prototype(M, m, "h"), M, m, r, DCT)
    pool = cf.int_pcm(3, 64, LMAX, seed=77)
    pool_d = {False: torch.from_numpy(pool).to(dev), True: torch.from_numpy(pool.astype(np.int16)).to(dev)}
    Wall = cf.unit_weights(3, K, 64, seed=3)
    out = {}
    for case in CASES:
        gi, N, S, ps, i16, mis = case
        _, t0, tcount, ns = GEOMETRIES[gi]
        assert t0 + tcount <= fb.num_frames(ns)
        pitch = (ns + 3) // 4 * 4 + 4 + (1 if mis else 0)
        off = (2 if i16 else 1) if mis else 0
        flat = torch.full((S * N * pitch + off + 64,), 12345, dtype=torch.int16 if i16 else torch.float32, device=dev)
        rows = flat[off: off + S * N * pitch].view(S, N, pitch)
        rows[..., :ns] = pool_d[i16][:S, :N, :ns]
        assert rows.data_ptr() % 16 == (4 if mis else 0) and pitch % 4 == (1 if mis else 0)
        W = torch.from_numpy(np.ascontiguousarray(Wall[:S if ps else 1, :, :N])).to(dev)
        Y = fb.analysis_beamform(rows, W, nsamples=ns, t0=t0, tcount=tcount)
        assert Y.shape == (S, K, tcount)
        out[_key(case)] = Y.cpu().numpy()
    pcm, W, L = _cf_inputs()
    for name in CF_PROTOS:
        fbn = eng.FilterBank(_proto(name), M, m, r, DCT)
        assert fbn.num_frames(L) == CF_T
        out["cf_" + name] = fbn.analysis_beamform(torch.from_numpy(pcm).to(dev), torch.from_numpy(W).to(dev)).cpu().numpy()
    np.savez(out_path, **out)


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); from tests import test_gpu_fused512_new as t; t._child_main(sys.argv[2])"


@pytest.fixture(scope="module")
def both(dev):
    """{"old": arrays with BTK_FUSED512_NEW=0, "new": arrays with the switch unset}; the second child only after the first succeeded."""
    got = {}
    with tempfile.TemporaryDirectory() as tmp:
        for side in ("old", "new"):
            env = {k: v for k, v in os.environ.items() if k not in ("BTK_FUSED512_NEW", "BTK_FUSED_VAR", "BTK_DISABLE_FUSED")}
            if side == "old":
                env["BTK_FUSED512_NEW"] = "0"
            path = os.path.join(tmp, side + ".npz")
            res = subprocess.run([sys.executable, "-c", _CHILD, ROOT, path], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
            assert res.returncode == 0, (side, res.stdout[-800:], res.stderr[-1500:])
            with np.load(path) as z:
                got[side] = {k: z[k] for k in z.files}
    return got


def test_new_kernel_gives_the_parent_kernels_bits(both):
    assert len(CASES) == len(GEOMETRIES) * (3 * 3 * 2 + 2)
    bad = []
    for case in CASES:
        k = _key(case)
        a, b = both["old"][k], both["new"][k]
        assert a.shape == b.shape and a.dtype == np.complex64 and np.all(np.isfinite(a.view(np.float32)))
        assert np.any(a != 0), k
        if not np.array_equal(a.view(np.int32), b.view(np.int32)):
            bad.append((k, GEOMETRIES[case[0]][0], int(np.count_nonzero(a.view(np.int32) != b.view(np.int32)))))
    assert not bad, bad
    for name in CF_PROTOS:
        assert np.array_equal(both["old"]["cf_" + name].view(np.int32), both["new"]["cf_" + name].view(np.int32)), name


def test_float32_and_int16_entries_agree_on_the_new_kernel(both):
    """(tests/test_gpu_fused_i16.py asks the same of the default path; here on every geometry above, integer PCM in the int16 range)"""
    for case in CASES:
        if not case[4]:
            k16 = _key(case[:4] + (True,) + case[5:])
            assert np.array_equal(both["new"][_key(case)].view(np.int32), both["new"][k16].view(np.int32)), k16


@pytest.mark.parametrize("name", CF_PROTOS)
def test_new_kernel_against_closed_form(both, name):
    """N = 3, T = 33 (a whole recording: all three tiles are edge tiles), every stream, under the rule of closed_forms.accept:
    e_max and the worst bin's e_bin <= 4 x the figure of a plain float32 evaluation of the same inputs."""
    pcm, W, L = _cf_inputs()
    Y = both["new"]["cf_" + name]
    assert Y.shape == (CF_S, K, CF_T)
    h = _proto(name)
    for s in range(CF_S):
        Ycf, Y32 = cf.fused_cf(h, M, m, r, DCT, pcm[s], W[s]), cf.plain_f32(h, M, m, r, DCT, pcm[s], W[s])
        ok, fig = cf.accept(Y[s], Y32, Ycf)
        print("CFRATIO fused512 new N=%d T=%d %s s=%d ratio %.3f e_max %.3e (f32 %.3e) e_bin %.3e (f32 %.3e)" %
              (CF_N, CF_T, name, s, fig["ratio"], fig["e_max"], fig["y_max"], fig["e_bin"], fig["y_bin"]))
        assert ok, (name, s, fig)
