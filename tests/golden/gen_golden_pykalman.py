"""Golden vectors for btk20.pykalman from the REFERENCE's own Python arithmetic (dev container only; same mechanism as
gen_golden_pytdoa.py -- nothing of the reference is written here).

The reference's lib/pykalman.py is loaded IN MEMORY without its `from pytdoa import *` line and with the numpy.float alias it
uses restored; its ExtendedKalmanFilter / IteratedExtendedKalmanFilter run over the reference's own feature vector classes
(lib/pytdoa.py, loaded as gen_golden_pytdoa.py loads it), which are fed by synthetic pair sources serving stored [delay, height]
tables (tests/track_closed_form.py: TablePairSource; delay = float(lag) / samplerate as TDOAFeature.next forms it).

Stored per case: the inputs -- lag int32 [P][T] (NO_PEAK = -2^31: no peak), height float32 [P][T], mpos, pairs, and a JSON record
(model, type, n, x0, t_begin, params) -- and per frame x [T][n], K [T][n][n] (K_filter), observed [T], updated [T] (observed and
not gated) and rounds [T] (IEKF rounds of an update, 0 otherwise; the reference keeps no count: one calc_innovation call per round).
Frames before t_begin are not tracked: the tracker is started with set_time(t_begin), as unit_test/test_source_tracking.py does.

The tables: integer lags of a moving far-field source (or a near-field position for the Cartesian model), heights well above
the threshold; OUTLIER frames with every lag sign-flipped (the gate filters them: that needs sigmaV2 far below the script's
4e-4, next to which delays of 1e-4 s never leave the gate; the reference's arithmetic is conditioned like sigmaK2 / sigmaV2, so
the gated cases have sigmaK2 = 1e2 and the sigmaK2 = 1e6 cases the script's sigmaV2); UNOBSERVED stretches of 1 and 5 frames (heights below the
threshold, some pairs without a peak); jumps of the source that carry the update across theta < 0, theta > pi and phi beyond
+- pi (every branch of adjust_boundaries).

Run:  python tests/golden/gen_golden_pykalman.py  -> tests/golden/pykalman_golden.npz
"""
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF_KALMAN = "/root/reference/btk20_src/lib/pykalman.py"

FS, SSPEED, THRESHOLD = 16000, 343740.0, 0.11
TIME_DELTA = 256.0 / FS
NO_PEAK = -(1 << 31)
KINECT_MPOS = [[-113.0, 0.0, 2.0], [36.0, 0.0, 2.0], [76.0, 0.0, 2.0], [113.0, 0.0, 2.0]]
KINECT_PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]


def load_reference_kalman():
    src = open(REF_KALMAN).read()
    src = "\n".join(l for l in src.splitlines() if l.strip() != "from pytdoa import *") + "\n"
    if not hasattr(np, "float"):
        np.float = float
    mod = types.ModuleType("ref_pykalman")
    exec(compile(src, REF_KALMAN, "exec"), mod.__dict__)
    return mod


def circular_mpos():
    ang = 2 * np.pi * np.arange(6) / 6
    mpos = np.stack([50.0 * np.cos(ang), 50.0 * np.sin(ang), np.zeros(6)], axis=1)
    mpos[5, 2] = 20.0
    return mpos


def all_pairs(n):
    return [(a, b) for a in range(n) for b in range(a + 1, n)]


ARRAYS = {
    "linear": (KINECT_MPOS, KINECT_PAIRS),
    "circular": (circular_mpos().tolist(), all_pairs(6)),
    # four microphones not in a plane
    "cartesian": ([[0.0, 0.0, 0.0], [200.0, 0.0, 0.0], [0.0, 200.0, 0.0], [0.0, 0.0, 200.0]], all_pairs(4)),
}


def trajectory(model, T, rng):
    """true states [T][n]: a slow drift with a few jumps (the jumps carry the linearised update over the boundaries)"""
    t = np.arange(T)
    if model == "linear":
        th = 0.9 + 0.02 * t
        th[8:14] = 0.15          # from 1.06 towards endfire: the step overshoots below 0
        th[14:22] = 2.2
        th[22:] = 2.95 - 0.01 * (t[22:] - 22)
        th[30:] = 0.4            # from 2.9 to 0.4: overshoots (cos grows, sin small) -- beyond pi the other way at 14
        return th[:, None]
    if model == "circular":
        th = 1.1 + 0.01 * t
        ph = 2.6 + 0.05 * t      # crosses +pi upwards
        ph = np.where(ph > np.pi, ph - 2 * np.pi, ph)
        th[20:] = 0.25           # a jump towards the pole: theta may overshoot below 0
        ph[26:] = -2.9 - 0.04 * (t[26:] - 26)   # crosses -pi downwards
        ph = np.where(ph < -np.pi, ph + 2 * np.pi, ph)
        return np.stack([th, ph], axis=1)
    # adjust_boundaries folds the first two Cartesian coordinates like angles (the reference applies it to every model): a
    # source that stays above the array, within that fold, and rises
    return np.stack([1.5 + 0.02 * t, 0.5 - 0.03 * t, 900.0 + 4.0 * t], axis=1)


def tables(model, mpos, pairs, T, seed, outliers=(), unobserved=()):
    from tests import track_closed_form as cf
    rng = np.random.default_rng(seed)
    g = cf.pair_geometry(model, mpos, pairs)
    traj = trajectory(model, T, rng)
    P = len(pairs)
    lag = np.zeros((P, T), np.int32)
    height = (0.3 + 0.4 * rng.random((P, T))).astype(np.float32)
    for t in range(T):
        lag[:, t] = np.rint(cf.model_rows(model, g, traj[t], SSPEED)[0] * FS).astype(np.int32)
    for t in outliers:
        lag[:, t] = -lag[:, t] - 3
    for t in unobserved:
        height[:, t] = (0.01 + 0.05 * rng.random(P)).astype(np.float32)
        height[0, t] = np.float32(0.5)                     # one pair above the threshold: fewer than minimum_pairs
        lag[P - 1, t], height[P - 1, t] = NO_PEAK, 0.0       # and one without a peak
    return lag, height


def params(n, sigmaK2, sigmaV2, gate_prob=0.95, sigmaU2=10.0, minimum_pairs=3, F=None, U=None, num_iterations=3,
           iteration_threshold=1e-4):
    return dict(F=(np.identity(n) if F is None else np.array(F)).tolist(), U=(sigmaU2 * np.identity(n) if U is None else np.array(U)).tolist(),
                sigmaV2=sigmaV2, sigmaK2=sigmaK2, time_delta=TIME_DELTA, gate_prob=gate_prob, num_iterations=num_iterations,
                iteration_threshold=iteration_threshold, threshold=THRESHOLD, minimum_pairs=minimum_pairs, Ts=1.0 / FS, c=SSPEED)


X0 = {"linear": [0.9], "circular": [1.1, 2.6], "cartesian": [1.5, 0.5, 900.0]}
OUTLIERS, UNOBSERVED = (5, 17, 18), (3, 24, 25, 26, 27, 28)


def build_cases():
    cases = []

    def add(name, model, type, prm, T=37, seed=1, t_begin=0, mpos=None, pairs=None, x0=None, outliers=OUTLIERS,
            unobserved=UNOBSERVED):
        m, p = ARRAYS[model]
        mpos, pairs = (m if mpos is None else mpos), (p if pairs is None else pairs)
        out = [t for t in outliers if t < T]
        un = [t for t in unobserved if t < T]
        lag, height = tables(model, mpos, pairs, T, seed, out, un)
        cases.append(dict(name=name, model=model, type=type, n=len(X0[model]), x0=X0[model] if x0 is None else x0, t_begin=t_begin,
                          params=prm, lag=lag, height=height, mpos=np.array(mpos, np.float64), pairs=np.array(pairs, np.int32)))

    SV = 2e-8                                      # the gate decides on residuals of a fraction of a sample: see the module text
    for model, n in (("linear", 1), ("circular", 2), ("cartesian", 3)):
        add(model + "_ekf_k2", model, "ekf", params(n, 1e2, SV))
        add(model + "_iekf_k6", model, "iekf", params(n, 1e6, 4e-4, iteration_threshold=1e-3))
        add(model + "_default", model, "iekf", params(n, 1e10, 4e-4))
    # a non-identity F and a non-diagonal U
    add("circular_iekf_FU", "circular", "iekf",
        params(2, 1e2, SV, F=[[1.0, 0.01], [-0.02, 0.995]], U=[[10.0, 2.0], [2.0, 6.0]], num_iterations=4, iteration_threshold=1e-6))
    # IEKF that stops in round 1 (a wide threshold) and one that uses all rounds (a threshold never met)
    add("linear_iekf_round1", "linear", "iekf", params(1, 1e2, SV, iteration_threshold=1e3))
    add("linear_iekf_allrounds", "linear", "iekf", params(1, 1e6, 4e-4, num_iterations=5, iteration_threshold=1e-30))
    add("linear_ekf_gate0", "linear", "ekf", params(1, 1e2, 1e-11, gate_prob=0.0))
    add("linear_ekf_T1", "linear", "ekf", params(1, 1e2, SV), T=1)
    # one pair, minimum_pairs 2: never observed
    add("linear_P1_never", "linear", "ekf", params(1, 1e2, SV, minimum_pairs=2), T=9, mpos=KINECT_MPOS[:2], pairs=[(0, 1)], unobserved=())
    # more pairs than lanes: a line of 12 microphones 40 mm apart has 66 pairs a < b; four reversed ones make 70
    line = [[40.0 * i, 0.0, 0.0] for i in range(12)]
    add("linear_P70", "linear", "iekf", params(1, 1e2, SV, minimum_pairs=40), mpos=line, pairs=all_pairs(12) + [(1, 0), (5, 2), (11, 0), (7, 6)])
    # three streams of one configuration: different tables, different first frames
    for i, tb in enumerate((0, 3, 7)):
        add("stream%d" % i, "circular", "iekf", params(2, 1e2, SV), seed=10 + i, t_begin=tb,
            outliers=(5 + i, 17), unobserved=(9 + 2 * i, 24, 25, 26, 27, 28))
    return cases


def main():
    from tests import track_closed_form as cf
    from tests.golden.gen_golden_pytdoa import load_reference_module
    ref_tdoa, ref_kalman = load_reference_module(), load_reference_kalman()
    out, names = {}, []
    for case in build_cases():
        src = cf.table_front_end(ref_tdoa, case)
        trk = cf.make_tracker(ref_kalman, case, src)
        res = cf.drive(trk, case, count_rounds=True)
        name = case["name"]
        names.append(name)
        for k in ("lag", "height", "mpos", "pairs"):
            out["%s_%s" % (name, k)] = case[k]
        out[name + "_meta"] = np.array(json.dumps({k: case[k] for k in ("model", "type", "n", "x0", "t_begin", "params")}))
        for k in ("x", "K", "observed", "updated", "rounds"):
            out["%s_%s" % (name, k)] = res[k]
        r = res["rounds"][res["updated"]]
        print("%-22s T=%2d P=%2d observed %2d updated %2d gated %2d ('Filtering' lines %d) rounds %s last x %s" % (
            name, case["lag"].shape[1], len(case["pairs"]), res["observed"].sum(), res["updated"].sum(),
            (res["observed"] & ~res["updated"]).sum(), res["filtered_lines"], np.bincount(r).tolist() if len(r) else [],
            np.array_str(res["x"][-1], precision=4)))
    out["names"] = np.array(json.dumps(names))
    path = os.path.join(HERE, "pykalman_golden.npz")
    np.savez_compressed(path, **out)
    print(len(names), "cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
