"""Golden vectors of the reference's maximum-empirical-kurtosis beamformers (dev container only).

Same mechanism as gen_golden_pybeamformer.py: the reference's lib/pybeamformer.py is translated to Python 3 and exec'd IN
MEMORY (nothing of it is written to this repository), its classes are driven with their SWIG-dependent __init__ bypassed and a
numpy snapshot source that serves the oracle's analysis frames of the committed Kinect fixture, ROUNDED TO COMPLEX64 AND WIDENED
BACK so that the reference and the GPU see identical inputs.  Two input scales: (a) raw PCM scale, (b) one global factor that
makes the median bin's delay-and-sum output power 1 (only there do alpha, gtol and mindelta mean anything; the energy threshold is
scaled along, so both scales select the same frames).

Pinned (tests/golden/pybeamformer_hos_golden.npz): the frames accum_observations selects for two label sets with R = 1 and 2;
_BmH; fun_hos_bf, dfun_hos_bf and calc_obj_func of SubbandMEKBeamformer / SubbandNMEKBeamformer (gamma < 0 and > 0) at zero, inside
and outside the clamp, for NS = 1, 2 and Nc = 1, 2, with zero previous statistics and with those the reference's store_stats left
after an earlier segment; those statistics; _woH right after finalize_wa_f; and, at scale (b) for every bin, f0, ||g0|| and the
objective the reference's estimate_wa_f_scipy reaches with CG and with BFGS (maxiter = 40).

The observation segment is an input choice: of the segments tried (0.2-0.9 s and all of 192 frames, 0.1-1.5 s of 256, all of
320) this one and all of 320 frames are those on which the Armijo conjugate-gradient iteration of DESIGN.md 3.15 ends at or below
the reference's scipy result on EVERY bin that moves; on the shorter ones two bins of 129 ended above it (a failed line search
at the clamp, a mindelta stop).

Run:  python tests/golden/gen_golden_pybeamformer_hos.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from gen_golden_pybeamformer import load_reference_module, NumpySnapshotSource      # noqa: E402

M, FS, T = 256, 16000, 320
K = M // 2 + 1
MPOS = np.array([[-113.0, 0.0, 2.0], [36.0, 0.0, 2.0], [76.0, 0.0, 2.0], [113.0, 0.0, 2.0]])
AZIMUTHS = (-1.306379, 0.6)                  # target of confs/ds.json and a second source
LABELS_A = [(0.3, 2.0)]                      # the observations of the pinned evaluations (213 frames)
LABELS_B = [(0.1, 0.45), (0.5, 0.7), (1.0, -1)]
LABELS_PREV = [(2.1, 2.5)]                   # the earlier segment whose statistics become the previous ones
BINS = np.arange(0, K, 8)                    # bins of the large arrays
ENERGY_THRESHOLD = 10


def frames(orc):
    """oracle analysis frames of the Kinect fixture, complex64-rounded: [T][N][M]"""
    proto = np.load(os.path.join(HERE, "prototype_M256_m4_r1.npz"))
    pcm = np.load(os.path.join(HERE, "kinect_4ch_16k.npz"))["pcm"].astype(np.float32)
    X = np.stack([orc.analysis(proto["h"], M, 4, 1, 2, pcm[c][: (T + 8) * 128])[:T] for c in range(4)], axis=1)
    return X


def round64(X):
    return X.astype(np.complex64).astype(np.complex128)


class Upper:
    """stands where an upper-branch beamformer stands: calc_entire_weights() -> wqH [K][N]"""

    def __init__(self, wqH):
        self.wqH = wqH

    def calc_entire_weights(self):
        return self.wqH


def upper_weights(ref, NS):
    out = []
    for az in AZIMUTHS[:NS]:
        d = ref.calc_la_delays(MPOS, az)
        out.append(np.conjugate(np.stack([ref.calc_array_manifold_f(m, M, FS, d, False) for m in range(K)])))
    return out


def make(ref, cls_name, X, NS, Nc, alpha=0.01, beta=3.0, gamma=None):
    cls = getattr(ref, cls_name)
    bf = cls.__new__(cls)
    bf._array_source = NumpySnapshotSource(X)
    bf._chan_num, bf._fftlen, bf._fftlen2, bf._shiftlen = 4, M, M // 2, 128
    bf._upper_beamformers = [Upper(w) for w in upper_weights(ref, NS)]
    bf._num_sources, bf._Nc, bf._srcX, bf._isamp, bf._alpha, bf._beta = NS, Nc, 0, 0, alpha, beta
    if gamma is not None:
        bf._gamma = gamma
    bf._half_band_shift, bf._logfp, bf._observations, bf._wuH, bf._BmH = False, None, None, None, None
    bf._woH = np.zeros((NS, K, 4), complex)
    # reset_stats (:1613-1616) with its Python-2 integer division written out
    bf._prevAvgY4, bf._prevAvgY2 = np.zeros((K, NS)), np.zeros((K, NS))
    bf._prevFrameN = np.zeros((K, NS), int)
    return bf


def test_points(NS, dim, seed):
    """packed weights [3][K][D]: zero, inside the clamp (norm << ||wuH|| = 0.5), outside it"""
    rng = np.random.default_rng(seed)
    r = rng.normal(size=(K, 2 * NS * dim))
    return np.stack([np.zeros_like(r), 0.05 * r, 2.0 * r])


VARIANTS = (("mek", "SubbandMEKBeamformer", None), ("nmek_gneg", "SubbandNMEKBeamformer", -1.0),
            ("nmek_gpos", "SubbandNMEKBeamformer", 0.3))


def main():
    from oracle import oracle as orc
    ref = load_reference_module()
    Xraw = frames(orc)
    out = {"meta_T": np.array([T]), "bins": BINS}

    # ---- selection logic
    Xa = round64(Xraw)
    for tag, labs in (("A", LABELS_A), ("B", LABELS_B)):
        for R in (1, 2):
            bf = make(ref, "SubbandMEKBeamformer", Xa, 1, 1)
            obs = bf.accum_observations(FS, target_labs=labs, energy_threshold=ENERGY_THRESHOLD, R=R)
            # recover the stream indices from the snapshots themselves
            idx = [int(np.where((Xa[:, :, 5] == o[5]).all(axis=1))[0][0]) for o in obs]
            out["sel_%s_R%d" % (tag, R)] = np.array(idx, np.int64)
    out["labels_A"], out["labels_B"], out["labels_prev"] = np.array(LABELS_A), np.array(LABELS_B), np.array(LABELS_PREV)

    # ---- scale (b): the median bin's delay-and-sum output power over the observations A becomes 1
    selA = out["sel_A_R1"]
    wu = upper_weights(ref, 1)[0]
    pw = np.mean(np.abs(np.einsum("kn,tnk->tk", wu, Xa[selA][:, :, :K])) ** 2, axis=0)
    scale_b = 1.0 / np.sqrt(np.median(pw))
    out["scale_b"] = np.array([scale_b])
    scales = {"a": 1.0, "b": scale_b}

    for sc, factor in scales.items():
        X = round64(Xraw * factor)
        thr = ENERGY_THRESHOLD * factor ** 2          # the same frames are selected at both scales
        for NS in (1, 2):
            for Nc in (1, 2):
                if sc == "a" and (NS, Nc) != (1, 1):
                    continue
                dim = 4 - Nc
                pts = test_points(NS, dim, 100 * NS + Nc)
                if sc == "b":
                    out["x_ns%d_nc%d" % (NS, Nc)] = pts
                for vtag, cls_name, gamma in VARIANTS:
                    bf = make(ref, cls_name, X, NS, Nc, gamma=gamma)
                    bf.calc_upper_beamformer_weights()
                    if sc == "b" and vtag == "mek":
                        out["BmH_ns%d_nc%d" % (NS, Nc)] = bf._BmH.copy()
                        out["wuH_ns%d_nc%d" % (NS, Nc)] = bf._wuH.copy()
                    for prev in (0, 1):
                        if prev:
                            # previous statistics: the reference's store_stats on an earlier segment at the inside-clamp point
                            obs = bf.accum_observations(FS, target_labs=LABELS_PREV, energy_threshold=thr, R=1)
                            out["sel_prev"] = np.array([int(np.where((X[:, :, 5] == o[5]).all(axis=1))[0][0]) for o in obs], np.int64)
                            bf._array_source.reset()
                            for m in range(K):
                                wa = bf.norm_active_weight_vectors(m, ref.unpack_weights(pts[1][m], NS, dim))
                                for srcX in range(NS):
                                    bf.store_stats(srcX, m, wa)
                            key = "%s_%s_ns%d_nc%d" % (sc, vtag, NS, Nc)
                            out[key + "_prevY2"], out[key + "_prevY4"] = bf._prevAvgY2.copy(), bf._prevAvgY4.copy()
                            out[key + "_prevN"] = bf._prevFrameN.astype(np.int64)
                        obs = bf.accum_observations(FS, target_labs=LABELS_A, energy_threshold=thr, R=1)
                        assert len(obs) == len(selA)
                        bf._array_source.reset()
                        for p in range(3):
                            key = "%s_%s_ns%d_nc%d_prev%d_x%d" % (sc, vtag, NS, Nc, prev, p)
                            out[key + "_fun"] = np.array([ref.fun_hos_bf(pts[p][m], m, bf) for m in BINS])
                            out[key + "_dfun"] = np.array([ref.dfun_hos_bf(pts[p][m], m, bf) for m in BINS])
                            out[key + "_obj"] = np.array([bf.calc_obj_func(m, bf.norm_active_weight_vectors(
                                m, ref.unpack_weights(pts[p][m], NS, dim))) for m in BINS])
                    # finalize_wa_f on two bins: _woH[.][m] right after, and the statistics it stored there
                    if sc == "b":
                        key = "%s_%s_ns%d_nc%d" % (sc, vtag, NS, Nc)
                        fin = []
                        for m in (8, 72):
                            bf.finalize_wa_f(m, pts[2][m])
                            fin.append(bf._woH[:, m].copy())
                        out[key + "_fin_woH"] = np.array(fin)
                        out[key + "_fin_prevY2"] = bf._prevAvgY2[[8, 72]].copy()
                        out[key + "_fin_prevY4"] = bf._prevAvgY4[[8, 72]].copy()
                        out[key + "_fin_prevN"] = bf._prevFrameN[[8, 72]].astype(np.int64)
                print("done", sc, NS, Nc, flush=True)

    # ---- the reference's scipy flow at scale (b), every bin: NMEK, NS = 1, Nc = 1, gamma < 0, zero previous statistics
    import contextlib
    import io
    import warnings
    X = round64(Xraw * scale_b)
    bf = make(ref, "SubbandNMEKBeamformer", X, 1, 1, gamma=-1.0)
    bf.calc_upper_beamformer_weights()
    bf.accum_observations(FS, target_labs=LABELS_A, energy_threshold=ENERGY_THRESHOLD * scale_b ** 2, R=1)
    assert len(bf._observations) == len(selA)
    x0 = np.zeros(2 * 3)
    f0 = np.array([ref.fun_hos_bf(x0, m, bf) for m in range(K)])
    g0 = np.array([np.linalg.norm(ref.dfun_hos_bf(x0, m, bf)) for m in range(K)])
    fs = {}
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        for solver in ("CG", "BFGS"):
            fs[solver] = np.array([ref.fun_hos_bf(bf.estimate_wa_f_scipy(m, x0.copy(), 1.0e-3, solver,
                                                                         options={"maxiter": 40, "gtol": 1.0e-2}), m, bf)
                                   for m in range(K)])
    out["opt_f0"], out["opt_g0norm"] = f0, g0
    out["opt_f_cg"], out["opt_f_bfgs"] = fs["CG"], fs["BFGS"]
    out["opt_f_ref"] = np.minimum(fs["CG"], fs["BFGS"])
    out["opt_spread"] = np.abs(fs["CG"] - fs["BFGS"])

    path = os.path.join(HERE, "pybeamformer_hos_golden.npz")
    np.savez_compressed(path, **out)
    print(len(out), "arrays,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
