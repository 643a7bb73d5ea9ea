"""GPU: fused512_kernel with every window row loaded once per tile (the workgroup split by row parity: threads 0..127 take the 12
even rows of a tile's 23-row span, threads 128..255 the 11 odd ones) against the kernel it descends from,
analysis512_bfz_kernel<2, 33231> (fb_analysis512.hip): the same bits; and once against the float64 closed form of
tests/closed_forms.py, so that the two kernels are not only compared where they could be wrong together.  (The cases also cover
what a change of the weight table's layout could break: see the weights below.)

BTK_FUSED512_NEW is read once per process, so every launch runs in two child processes, one with BTK_FUSED512_NEW=0 (the parent
kernel) and one with the switch unset; the two Y are compared on their int32 view.

Fixed: M = 512, m = 4, r = 1, dct = 2 (7 frames of delay, 3 of look-ahead: the span of tile i of a launch at t0 is the 23 rows
[(t0 + 16 i - 4) 256, (t0 + 16 i + 19) 256)), S = 2 streams, recordings of at most 96 frames = 92 rows: at t0 = 0 tile 0 is a
first-edge tile (4 rows in front of the recording), tiles 1..4 are interior and tile 5 (rows 76..98) is a last-edge tile.
Varied: N in {1, 3, 64}; float32 and int16 PCM; per-stream and shared weights; and the (t0, tcount, nsamples) of GEOMETRIES: the
recording's end on a row boundary, inside a row at an even and at an odd length (the odd one cuts an 8-byte row in two), inside an
even row (10) and inside an odd row (11) of the last tile's span, each at both parities of the length; t0 = 5 (no first-edge
tile; the tiles start on other rows) and tcount no multiple of 16.  The staged loop (same parity map, rows from LDS) is reached
by a base pointer 4 bytes past a 16-byte boundary and by an odd row pitch.

The weights are independent random complex numbers per (stream, bin, channel), magnitudes U(0.5, 1.5) / N: |w[q]| and
|w[256 - q]| differ everywhere (asserted), so a swapped or shifted pair of the table cannot cancel.  The samples behind nsamples
are 12345 and must not be read as signal.
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
S, T = 2, 96
ROWS = T - 7 + 3                                                       # 92 rows of D samples give 96 frames

# (label, t0, tcount, nsamples)
GEOMETRIES = [
    ("whole recording, even length on a row boundary", 0, 96, ROWS * D),
    ("even length inside the last row", 0, 96, ROWS * D - 156),
    ("odd length: a cut row", 0, 96, ROWS * D - 155),
    ("ends inside even row 10 of the last span, odd length", 0, 91, 86 * D + 57),
    ("ends inside even row 10 of the last span, even length", 0, 91, 86 * D + 58),
    ("ends inside odd row 11 of the last span, odd length", 0, 92, 87 * D + 57),
    ("ends inside odd row 11 of the last span, even length", 0, 92, 87 * D + 58),
    ("t0 = 5, tcount = 87", 5, 87, ROWS * D),
    ("t0 = 5, tcount = 83, odd length inside a row", 5, 83, 86 * D + 201),
    ("t0 = 0, tcount = 37: interior last tile, not full", 0, 37, ROWS * D),
]
LMAX = ROWS * D
CASES = [(gi, N, ps, i16, 0) for gi in range(len(GEOMETRIES)) for N in (1, 3, 64) for ps in (False, True) for i16 in (False, True)]
# the staged loop: 1 = base pointer 4 bytes past a 16-byte boundary (pitch a multiple of 4), 2 = odd row pitch
CASES += [(gi, 3, True, i16, mis) for gi in (0, 2, 5, 8) for i16 in (False, True) for mis in (1, 2)]
CF_N, CF_T = 3, 48


def rand_weights(Sw, N, seed):
    """complex64 [Sw][K][N], independent per entry, magnitudes U(0.5, 1.5) / N."""
    rng = np.random.default_rng(seed)
    W = (rng.uniform(0.5, 1.5, (Sw, K, N)) * np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, (Sw, K, N))) / N).astype(np.complex64)
    q = np.arange(1, 128)                                              # (bins 0 and 128 are their own partners)
    assert np.all(np.abs(W[:, q, :]) != np.abs(W[:, 256 - q, :]))
    return W


def _cf_inputs():
    L = cf.num_samples(CF_T, M, m, r, DCT)
    return cf.int_pcm(S, CF_N, L, seed=812), rand_weights(S, CF_N, seed=48), L


def _key(case):
    gi, N, ps, i16, mis = case
    return "g%d_N%d_%s_%s_%s" % (gi, N, "own" if ps else "shared", "i16" if i16 else "f32", ("al", "ptr", "pitch")[mis])


def _child_main(out_path):
    """Every launch of CASES and the closed-form launch, in this process's setting of the switch."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    dev = torch.device("cuda", 0)
    fb = eng.FilterBank(design_prototype(M, m, "h"), M, m, r, DCT)
    pool = cf.int_pcm(S, 64, LMAX, seed=96)
    pool_d = {False: torch.from_numpy(pool).to(dev), True: torch.from_numpy(pool.astype(np.int16)).to(dev)}
    Wall = {N: rand_weights(S, N, seed=N) for N in (1, 3, 64)}
    out = {}
    for case in CASES:
        gi, N, ps, i16, mis = case
        _, t0, tcount, ns = GEOMETRIES[gi]
        assert t0 + tcount <= fb.num_frames(ns)
        pitch = (ns + 3) // 4 * 4 + 4 + (1 if mis == 2 else 0)
        off = (2 if i16 else 1) if mis == 1 else 0
        flat = torch.full((S * N * pitch + off + 64,), 12345, dtype=torch.int16 if i16 else torch.float32, device=dev)
        rows = flat[off: off + S * N * pitch].view(S, N, pitch)
        rows[..., :ns] = pool_d[i16][:, :N, :ns]
        assert rows.data_ptr() % 16 == (4 if mis == 1 else 0) and pitch % 4 == (1 if mis == 2 else 0)
        W = torch.from_numpy(np.ascontiguousarray(Wall[N][:S if ps else 1])).to(dev)
        Y = fb.analysis_beamform(rows, W, nsamples=ns, t0=t0, tcount=tcount)
        assert Y.shape == (S, K, tcount)
        out[_key(case)] = Y.cpu().numpy()
    pcm, W, L = _cf_inputs()
    assert fb.num_frames(L) == CF_T
    out["cf"] = fb.analysis_beamform(torch.from_numpy(pcm).to(dev), torch.from_numpy(W).to(dev)).cpu().numpy()
    np.savez(out_path, **out)


_CHILD = "import sys; sys.path.insert(0, sys.argv[1]); from tests import test_gpu_fused512_rows_once as t; t._child_main(sys.argv[2])"


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


def test_rows_once_kernel_gives_the_parent_kernels_bits(both):
    assert len(CASES) == len(GEOMETRIES) * 3 * 2 * 2 + 4 * 2 * 2
    bad = []
    for case in CASES:
        k = _key(case)
        a, b = both["old"][k], both["new"][k]
        assert a.shape == b.shape and a.dtype == np.complex64 and np.all(np.isfinite(a.view(np.float32)))
        assert np.all(np.any(a != 0, axis=(1, 2))), k                  # every stream carries signal
        if not np.array_equal(a.view(np.int32), b.view(np.int32)):
            bad.append((k, GEOMETRIES[case[0]][0], int(np.count_nonzero(a.view(np.int32) != b.view(np.int32)))))
    assert not bad, bad
    assert np.array_equal(both["old"]["cf"].view(np.int32), both["new"]["cf"].view(np.int32))


def test_float32_and_int16_entries_agree(both):
    """Integer samples in the int16 range: the typed loads of the int16 entry deliver the floats of the float32 entry."""
    for case in CASES:
        if not case[3]:
            k16 = _key(case[:3] + (True,) + case[4:])
            assert np.array_equal(both["new"][_key(case)].view(np.int32), both["new"][k16].view(np.int32)), k16


def test_rows_once_kernel_against_closed_form(both):
    """N = 3, T = 48 (a whole recording: first-edge, interior and last-edge tile), both streams, under the rule of
    closed_forms.accept as tests/test_gpu_fused_closed_form.py applies it: e_max and the worst bin's e_bin <= 4 x the figure of a
    plain float32 evaluation of the same inputs."""
    pcm, W, L = _cf_inputs()
    Y = both["new"]["cf"]
    assert Y.shape == (S, K, CF_T)
    h = design_prototype(M, m, "h")
    for s in range(S):
        Ycf, Y32 = cf.fused_cf(h, M, m, r, DCT, pcm[s], W[s]), cf.plain_f32(h, M, m, r, DCT, pcm[s], W[s])
        cf.judge("fused512 rows once N=%d T=%d s=%d" % (CF_N, CF_T, s), Y[s], Y32, Ycf)
