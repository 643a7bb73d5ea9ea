"""Golden vectors for btk20.pytdoa from the REFERENCE's own Python arithmetic (dev container only; same mechanism as
gen_golden_pybeamformer.py -- nothing of the reference is written here).

The reference's lib/pytdoa.py is loaded IN MEMORY without its `from btk20.feature import *` line (the SWIG module cannot be
built here; pytdoa itself is pure numpy) and with the numpy.float alias it uses restored.  Its own classes -- PHATFeature,
TDOAFeature, MicrophonePairSource and the array-specific TDOAFeatureVector from make_tdoa_front_end -- are driven with numpy
spectral sources that serve the closed-form spectra (tests/tdoa_closed_form.py) ROUNDED TO complex64 AND WIDENED BACK, so that
the reference and the GPU see identical inputs.

Stored per case: peaks [T][P][2] = [delay, height] per pair and frame (NaN delay = None), observed [T][P] (the pair is in the
observation list), has_obs [T] (next() returned a list, not None), tdoa [T][P] (mic_pair_tdoa(), NaN = None) and
positions [T][dim] (instantaneous_position).
Cases: the Kinect linear array with the six pairs and the configuration of unit_test/test_tdoa_estimator.py at (D 8192, L 16384)
and (D 256, L 512); a synthetic circular array (6 microphones, radius 50 mm, microphone 5 lifted 20 mm) with plane-wave noise
from two directions, a silent stretch of the lifted microphone (its pairs have zero bins: no peak, and only pairs parallel to
the xy-plane remain) -- its int16 PCM is stored too.

Run:  python tests/golden/gen_golden_pytdoa.py  -> tests/golden/pytdoa_golden.npz
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF_PY = "/root/reference/btk20_src/lib/pytdoa.py"

SSPEED = 343740.0
KINECT_MPOS = [[-113.0, 0.0, 2.0], [36.0, 0.0, 2.0], [76.0, 0.0, 2.0], [113.0, 0.0, 2.0]]
KINECT_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
KINECT_CONF = dict(energy_threshold=128, minimum_pairs=5, threshold=0.12)
CIRC_CONF = dict(energy_threshold=64, minimum_pairs=3, threshold=0.12)
CIRC_D, CIRC_L, CIRC_T, FS = 256, 512, 48, 16000


def load_reference_module():
    src = open(REF_PY).read()
    src = "\n".join(l for l in src.splitlines() if l.strip() != "from btk20.feature import *") + "\n"
    if not hasattr(np, "float"):
        np.float = float
    mod = types.ModuleType("ref_pytdoa")
    exec(compile(src, REF_PY, "exec"), mod.__dict__)
    return mod


class NumpySpectralSource:
    """Stands where an FFTFeature stands: next(frame_no) is the full spectrum of the frame (half plus conjugate mirror)."""

    def __init__(self, Xhalf):
        L = 2 * (Xhalf.shape[1] - 1)
        self.X = np.concatenate([Xhalf, np.conj(Xhalf[:, L // 2 - 1:0:-1])], axis=1)

    def next(self, frame_no):
        if frame_no >= self.X.shape[0]:
            raise StopIteration
        return self.X[frame_no]

    def reset(self):
        pass


def circular_mpos():
    ang = 2 * np.pi * np.arange(6) / 6
    mpos = np.stack([50.0 * np.cos(ang), 50.0 * np.sin(ang), np.zeros(6)], axis=1)
    mpos[5, 2] = 20.0
    return mpos


def circular_pcm():
    """Plane-wave white noise from direction 1 (above the array) in the first half and direction 2 (below it) in the second, a
    little sensor noise, microphone 5 silent in frames 16..23 and 40..47; int16."""
    rng = np.random.default_rng(2024)
    mpos = circular_mpos()
    n = CIRC_D * CIRC_T
    out = np.zeros((6, n))
    for half, (theta, phi) in enumerate([(1.1, 0.7), (2.2, 1.9)]):
        u = np.array([np.sin(theta) * np.cos(phi), np.sin(theta) * np.sin(phi), np.cos(theta)])
        s = rng.normal(size=n // 2) * 3000
        S = np.fft.rfft(s)
        f = np.arange(len(S)) / (n // 2)
        for c in range(6):
            # a source in direction u reaches a microphone at p earlier by u.p / c: pair delays are u.(p_second - p_first) / c
            # with the sign convention of FarfieldCircularArrayTDOAFeatureVector.tdoa once the correlation lag is taken as is
            delay = np.dot(u, mpos[c]) / SSPEED * FS
            out[c, half * (n // 2):(half + 1) * (n // 2)] = np.fft.irfft(S * np.exp(-2j * np.pi * f * delay), n // 2)
    out += rng.normal(size=out.shape) * 30
    for a, b in ((16, 24), (40, 48)):
        out[5, a * CIRC_D:b * CIRC_D] = 0
    return np.clip(np.rint(out), -32768, 32767).astype(np.int16)


def run_case(ref, array_type, X64, pairs, mpos, L, conf):
    """X64 complex128 [C][T][K] (already complex64-rounded)."""
    C, T, K = X64.shape
    sources = [NumpySpectralSource(X64[c]) for c in range(C)]
    fe = ref.make_tdoa_front_end(array_type=array_type, pair_ids=pairs, spec_sources=sources, fftlen=L, samplerate=FS,
                                 mpos=np.array(mpos), energy_threshold=conf["energy_threshold"],
                                 minimum_pairs=conf["minimum_pairs"], threshold=conf["threshold"], sspeed=SSPEED)
    P = len(pairs)
    peaks = np.zeros((T, P, 2))
    observed = np.zeros((T, P), bool)
    has_obs = np.zeros(T, bool)
    tdoa = np.zeros((T, P))
    positions = []
    for t in range(T):
        obs = fe.next(t)
        has_obs[t] = obs is not None
        for o in (obs or []):
            observed[t, o.pairx] = True
        buf = fe.mic_pair_tdoa()
        for p, (a, b) in enumerate(pairs):
            d = buf[a][b]
            tdoa[t, p] = np.nan if d is None else d
            delay, height = fe._mic_pair_srcs[p].next(t)
            peaks[t, p] = (np.nan if delay is None else delay, height)
        positions.append(np.array(fe.instantaneous_position(t), np.float64))
    return dict(peaks=peaks, observed=observed, has_obs=has_obs, tdoa=tdoa, positions=np.stack(positions))


def main():
    from tests import tdoa_closed_form as cf
    ref = load_reference_module()
    out = {}
    pcm = np.load(os.path.join(HERE, "kinect_4ch_16k.npz"))["pcm"].astype(np.float32)
    for D, L in ((8192, 16384), (256, 512)):
        X = cf.spectra(pcm, D, L)[0].astype(np.complex64).astype(np.complex128)
        res = run_case(ref, "linear", X, KINECT_PAIRS, KINECT_MPOS, L, KINECT_CONF)
        for k, v in res.items():
            out["kinect_D%d_%s" % (D, k)] = v
        print("kinect D=%d: %d frames, %d with observations, %d positions, %d peaks without delay" % (
            D, X.shape[1], res["has_obs"].sum(), (res["positions"][:, 0] > -1e10).sum(), np.isnan(res["peaks"][..., 0]).sum()))
    cp = circular_pcm()
    pairs = [(a, b) for a in range(6) for b in range(a + 1, 6)]
    X = cf.spectra(cp.astype(np.float32), CIRC_D, CIRC_L)[0].astype(np.complex64).astype(np.complex128)
    res = run_case(ref, "circular", X, pairs, circular_mpos(), CIRC_L, CIRC_CONF)
    for k, v in res.items():
        out["circ_" + k] = v
    out["circ_pcm"] = cp
    out["circ_mpos"] = circular_mpos()
    out["circ_pairs"] = np.array(pairs)
    pos = res["positions"]
    print("circular: %d frames, %d with observations, %d positions, %d peaks without delay" % (
        X.shape[1], res["has_obs"].sum(), (pos[:, 0] > -1e10).sum(), np.isnan(res["peaks"][..., 0]).sum()))
    print(np.round(pos, 3))
    np.savez_compressed(os.path.join(HERE, "pytdoa_golden.npz"), **out)
    print({k: v.shape for k, v in out.items()}, os.path.getsize(os.path.join(HERE, "pytdoa_golden.npz")))


if __name__ == "__main__":
    main()
