"""Inputs of the maximum-empirical-kurtosis tests: the snapshots the golden generator (tests/golden/gen_golden_pybeamformer_hos.py)
fed to the reference, rebuilt from the committed fixtures."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
M, FS, N = 256, 16000, 4
K = M // 2 + 1
ENERGY_THRESHOLD = 10
VARIANTS = (("mek", False, -1.0), ("nmek_gneg", True, -1.0), ("nmek_gpos", True, 0.3))     # tag, normalize, gamma


def golden():
    return np.load(os.path.join(GOLDEN, "pybeamformer_hos_golden.npz"))


def frames(orc, proto256, kinect_pcm, T, factor=1.0):
    """oracle analysis frames scaled by `factor`, rounded to complex64 and widened back: complex128 [T][N][M]"""
    h, _ = proto256
    X = np.stack([orc.analysis(h, M, 4, 1, 2, kinect_pcm[c][: (T + 8) * 128])[:T] for c in range(N)], axis=1)
    return (X * factor).astype(np.complex64).astype(np.complex128)


def energies(X):
    """what update_snapshot_array(chan_no = 0) / fftlen is for every frame (lib/pybeamformer.py:263-277, :1409)"""
    return np.array([abs(np.dot(np.conjugate(x[0]), x[0])) for x in X]) / M


def observations(X, sel):
    """[T][N][M] -> the kernel's layout [K][N][Tobs] of the selected frames"""
    return np.ascontiguousarray(X[sel][:, :, :K].transpose(2, 1, 0))
