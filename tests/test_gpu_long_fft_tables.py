"""GPU: the twiddle table and the Hamming windows behind rfft_long.h are one copy per process, created by whichever module
launches a long transform first.  A fresh child process calls convolution, then the front end, then TDOA; this process calls
them in the opposite order (and inside the suite long after other tests created the tables in theirs).  Both must hand out the
same bytes.  L = 256 and 512: with and without the radix-2 tail pass, NF/4 below and at the workgroup's 64 threads."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (256, 512)
D, SHIFT, FRAMES = 200, 80, 3


def _inputs():
    """Generated on the host from a fixed seed: both processes hold the same samples."""
    rng = np.random.default_rng(20384)
    noise = lambda *shape: np.round(rng.normal(scale=3000.0, size=shape)).astype(np.float32)
    return {"taps": rng.normal(size=(1, 5)).astype(np.float32), "conv": noise(1, 300),
            "fe": noise(1, 1, (FRAMES - 1) * SHIFT + SHIFT // 2), "tdoa": noise(1, 2, FRAMES * D - 40)}


def _conv(eng, dev, x, L):
    import torch
    filt = eng.conv_filter(torch.from_numpy(x["taps"]).to(dev), n_max=L)
    assert filt.N == L
    y = eng.fir_convolve(torch.from_numpy(x["conv"]).to(dev), filt)
    return {"conv_H": filt.H, "conv_y": y}


def _fe(eng, dev, x, L):
    import torch
    pcm = torch.from_numpy(x["fe"]).to(dev)
    assert eng.fe_frames(pcm.shape[-1], D, SHIFT) == FRAMES
    o = eng.fe_process(pcm, "pcm", ("spectrum", "power"), D=D, shift=SHIFT, L=L)
    return {"fe_spectrum": o["spectrum"], "fe_power": o["power"]}


def _tdoa(eng, dev, x, L):
    import torch
    pcm = torch.from_numpy(x["tdoa"]).to(dev)
    assert eng.tdoa_frames(pcm.shape[-1], D) == FRAMES
    X, energy = eng.tdoa_spectra(pcm, D, L)
    lag, height, gcc = eng.tdoa_gcc_peaks(X, energy, [(0, 1)], 0.0, want_gcc=True)
    return {"tdoa_X": X, "tdoa_energy": energy, "tdoa_lag": lag, "tdoa_height": height, "tdoa_gcc": gcc}


def _run(modules):
    """{name_L: raw bytes as uint8} of the modules' outputs, called in the order given."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    dev = torch.device("cuda", 0)
    x = _inputs()
    out = {}
    for fn in modules:
        for L in LENGTHS:
            for k, v in fn(eng, dev, x, L).items():
                v = v.cpu().contiguous()
                out["%s_%d" % (k, L)] = (torch.view_as_real(v) if v.is_complex() else v).numpy().view(np.uint8)
    return out


def test_tables_do_not_depend_on_the_module_that_creates_them(dev):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "child.npz")
        # the child is this file run by its path (the hook at the bottom), not an import of a package named tests
        res = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert res.returncode == 0, (res.stdout[-800:], res.stderr[-1500:])
        with np.load(path) as z:
            child = {k: z[k] for k in z.files}
    here = _run((_tdoa, _fe, _conv))
    assert sorted(child) == sorted(here) and len(here) == 9 * len(LENGTHS)
    for k in sorted(here):
        assert here[k].size > 0 and (np.any(here[k] != 0) or k.startswith("tdoa_lag")), k   # (lag 0 is a lag)
        assert child[k].shape == here[k].shape and np.array_equal(child[k], here[k]), k
    # the correlation really was computed: a peak in every frame
    for L in LENGTHS:
        assert np.all(here["tdoa_height_%d" % L].view(np.float32) > 0)


if __name__ == "__main__":                    # the child process: convolution, then the front end, then TDOA
    sys.path.insert(0, ROOT)
    np.savez(sys.argv[1], **_run((_conv, _fe, _tdoa)))
