"""Float64 restatements for the tracker tests (no test in here; imported by test_track_cpu.py and test_gpu_track.py).

  * gammainc_restated: the regularised lower incomplete gamma function the way track_kernels.hip computes it (series below
    a + 1, modified Lentz continued fraction from there on).
  * track_form: the tracker in the O(P) form of the kernel -- per frame only A = H^T H, H^T s and s^T s of the observed pairs
    and algebra in n <= 3 dimensions -- in numpy.
  * TablePairSource / table_front_end / run_host: this package's pytdoa feature vectors over stored lag / height tables, and the
    package's host tracker classes run over them.
  * load_cases: the cases of tests/golden/pykalman_golden.npz.
"""
import contextlib
import io
import json
import math
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "pykalman_golden.npz")
NO_PEAK = -(1 << 31)
MODEL_OF = {"linear": 0, "circular": 1, "cartesian": 2}


def gammainc_restated(a, x, itmax=20000):
    if not x > 0.0:
        return 0.0
    if math.isinf(x):
        return 1.0
    EPS, FPMIN = 1.0e-16, 1.0e-300
    e = -x + a * math.log(x) - math.lgamma(a)
    front = math.exp(e) if e > -745.0 else 0.0
    if x < a + 1.0:
        ap, dl = a, 1.0 / a
        total = dl
        for _ in range(itmax):
            ap += 1.0
            dl *= x / ap
            total += dl
            if abs(dl) < abs(total) * EPS:
                break
        return total * front
    b = x + 1.0 - a
    c, d = 1.0 / FPMIN, 1.0 / b
    h = d
    for i in range(1, itmax + 1):
        an = -float(i) * (float(i) - a)
        b += 2.0
        d = an * d + b
        if abs(d) < FPMIN:
            d = FPMIN
        c = b + an / c
        if abs(c) < FPMIN:
            c = FPMIN
        d = 1.0 / d
        dl = d * c
        h *= dl
        if abs(dl - 1.0) < EPS:
            break
    return 1.0 - front * h


# ---- the observation models (pytdoa.py of this repository: tdoa / linearize of the three feature vectors) -------------------
def pair_geometry(model, mpos, pairs):
    """float64 [P][6] as engine.ekf_track reads it."""
    mpos = np.asarray(mpos, np.float64)
    g = np.zeros((len(pairs), 6))
    for p, (a, b) in enumerate(pairs):
        if model == "linear":
            d = [math.sqrt(np.dot(mpos[i] - mpos[0], mpos[i] - mpos[0])) if i else 0.0 for i in (a, b)]
            g[p, 0] = d[1] - d[0]
        elif model == "circular":
            g[p, :3] = mpos[b] - mpos[a]
        else:
            g[p, :3], g[p, 3:] = mpos[a], mpos[b]
    return g


def model_rows(model, g, xp, c):
    """tau [P], H [P][n] of every pair at the predicted state."""
    if model == "linear":
        return g[:, 0] * math.cos(xp[0]) / c, (-g[:, 0] * math.sin(xp[0]) / c)[:, None]
    if model == "circular":
        st, ct, sp, cp = math.sin(xp[0]), math.cos(xp[0]), math.sin(xp[1]), math.cos(xp[1])
        off = g[:, :3]
        tau = off @ np.array([st * cp, st * sp, ct]) / c
        H = np.stack([off @ np.array([ct * cp, ct * sp, -st]) / c, off @ np.array([-st * sp, st * cp, 0.0]) / c], axis=1)
        return tau, H
    d1, d2 = xp[None, :] - g[:, :3], xp[None, :] - g[:, 3:]
    r1, r2 = np.sqrt(np.sum(d1 * d1, axis=1)), np.sqrt(np.sum(d2 * d2, axis=1))
    return (r1 - r2) / c, (d1 / r1[:, None] - d2 / r2[:, None]) / c


BRANCH_HITS = set()          # the branches of adjust_boundaries that track_form has taken (the fixtures must reach all four)


def adjust_boundaries(x):
    theta, phi = x[0], (x[1] if len(x) > 1 else 0.0)
    if theta < 0.0:
        theta, phi = -theta, phi + math.pi
        BRANCH_HITS.add("theta<0")
    elif theta > math.pi:
        theta, phi = theta - math.pi, phi + math.pi
        BRANCH_HITS.add("theta>pi")
    while phi < -math.pi:
        phi += 2.0 * math.pi
        BRANCH_HITS.add("phi<-pi")
    while phi > math.pi:
        phi -= 2.0 * math.pi
        BRANCH_HITS.add("phi>pi")
    x[0] = theta
    if len(x) > 1:
        x[1] = phi
    return x


def track_form(case, lag=None, height=None, state=None, t_begin=None):
    """The O(P) form over lag int [P][T], height float32 [P][T] -> dict(x [T][n], K [T][n][n], observed, updated, rounds [T]).
    state: dict(x, K, time, last) to start from (default: the case's initial state at its t_begin)."""
    lag = case["lag"] if lag is None else lag
    height = case["height"] if height is None else height
    prm = case["params"]
    model, n = case["model"], case["n"]
    g = pair_geometry(model, case["mpos"], case["pairs"])
    F, U = np.asarray(prm["F"], np.float64), np.asarray(prm["U"], np.float64)
    sig, c, Ts = prm["sigmaV2"], prm["c"], prm["Ts"]
    tb = case["t_begin"] if t_begin is None else t_begin
    if state is None:
        state = dict(x=np.array(case["x0"], np.float64), K=prm["sigmaK2"] * np.identity(n), time=tb, last=-1)
    x, K, time, last = np.array(state["x"], np.float64), np.array(state["K"], np.float64), state["time"], state["last"]
    P, T = lag.shape
    out = dict(x=np.zeros((T, n)), K=np.zeros((T, n, n)), observed=np.zeros(T, bool), updated=np.zeros(T, bool),
               rounds=np.zeros(T, np.int64), tracked=np.zeros(T, bool))
    for t in range(T):
        if t >= tb:
            out["tracked"][t] = True
            xp = F @ x
            obs = (height[:, t].astype(np.float64) > prm["threshold"]) & (lag[:, t] != NO_PEAK)
            if obs.sum() >= prm["minimum_pairs"]:
                out["observed"][t] = True
                tau, H = model_rows(model, g[obs], xp, c)
                delay = lag[obs, t].astype(np.float64) * Ts
                hx = H @ xp
                s = (delay - (tau - hx)) - hx
                A, b, ss = H.T @ H, H.T @ s, float(s @ s)
                el = (time - last) * prm["time_delta"]
                Kp = F @ K @ F.T + el * el * U
                W = Kp @ np.linalg.inv(sig * np.identity(n) + A @ Kp)
                Wb = W @ b
                d2 = (ss - float(b @ Wb)) / sig
                cdf = gammainc_restated(0.5 * obs.sum(), 0.5 * d2 * d2) if d2 > 0 else 0.0
                if not cdf > prm["gate_prob"]:
                    out["updated"][t] = True
                    if case["type"] == "iekf":
                        eta = xp.copy()
                        for i in range(prm["num_iterations"]):
                            v = b - A @ (xp - eta) if i else b
                            new = xp + W @ v
                            diff = new - eta
                            eta = new
                            out["rounds"][t] = i + 1
                            if float(diff @ diff) < prm["iteration_threshold"]:
                                break
                        xn = eta
                    else:
                        xn = xp + Wb
                    x, K, last = adjust_boundaries(xn), sig * W, time
            time += 1
        out["x"][t], out["K"][t] = x, K
    out["state"] = dict(x=x, K=K, time=time, last=last)
    return out


# ---- this package's classes over stored tables ---------------------------------------------------------------------------------
class TablePairSource:
    """Stands where a TDOAFeature stands: next(frame_no) is [delay, height] of one pair from stored lag / height rows."""

    def __init__(self, lag, height, Ts):
        self.lag, self.height, self.Ts = lag, height, Ts

    def next(self, frame_no):
        if frame_no >= len(self.lag):
            raise StopIteration
        if int(self.lag[frame_no]) == NO_PEAK:
            return [None, 0.0]
        return [float(int(self.lag[frame_no])) * self.Ts, float(self.height[frame_no])]

    def reset(self):
        pass


def table_front_end(mod, case, lag=None, height=None, order=None):
    """The feature vector of the case's model from module `mod` (this package's pytdoa, or the reference's) over the tables;
    order: a permutation of the pairs (the same filter, summed in another order)."""
    lag = case["lag"] if lag is None else lag
    height = case["height"] if height is None else height
    order = range(len(case["pairs"])) if order is None else order
    srcs = []
    for pairx, p in enumerate(order):
        a, b = case["pairs"][p]
        srcs.append(mod.MicrophonePairSource(pairx, int(a), int(b), TablePairSource(lag[p], height[p], case["params"]["Ts"])))
    cls = {"linear": mod.FarfieldLinearArrayTDOAFeatureVector, "circular": mod.FarfieldCircularArrayTDOAFeatureVector,
           "cartesian": mod.TDOAFeatureVector}[case["model"]]
    prm = case["params"]
    with contextlib.redirect_stdout(io.StringIO()):
        return cls(srcs, np.array(case["mpos"], np.float64), prm["minimum_pairs"], prm["threshold"], prm["c"])


def make_tracker(kmod, case, source):
    prm, n = case["params"], case["n"]
    kw = dict(F=np.array(prm["F"], np.float64), U=np.array(prm["U"], np.float64), sigmaV2=prm["sigmaV2"], sigmaK2=prm["sigmaK2"],
              time_delta=prm["time_delta"], initialXk=np.array(case["x0"], np.float64), gate_prob=prm["gate_prob"],
              boundaries=None)
    if case["type"] == "iekf":
        return kmod.IteratedExtendedKalmanFilter(source, num_iterations=prm["num_iterations"],
                                                 iteration_threshold=prm["iteration_threshold"], **kw)
    return kmod.ExtendedKalmanFilter(source, **kw)


def run_host(case, lag=None, height=None, order=None, margins=None):
    """This package's host classes over the tables -> the dict of track_form (K included).  margins: a dict that receives
    cdf [per observed frame] and diffs [(|delta|^2, last round?) per IEKF round]."""
    from distant_speech_recognition_amd import pykalman as kmod
    src = table_front_end(kmod, case, lag, height, order)
    trk = make_tracker(kmod, case, src)
    trk.use_device = False
    return drive(trk, case, margins)


def drive(trk, case, margins=None, count_rounds=False):
    """Run a tracker object (this package's or the reference's) over the case's frames."""
    T, n, tb = case["lag"].shape[1], case["n"], case["t_begin"]
    out = dict(x=np.zeros((T, n)), K=np.zeros((T, n, n)), observed=np.zeros(T, bool), updated=np.zeros(T, bool),
               rounds=np.zeros(T, np.int64), tracked=np.zeros(T, bool))
    calls = [0]
    if count_rounds:                                    # the reference keeps no count: one calc_innovation per round
        orig = trk.calc_innovation

        def counting(yk):
            calls[0] += 1
            return orig(yk)
        trk.calc_innovation = counting
    trk.set_time(tb)
    sink = io.StringIO()
    for t in range(T):
        if t >= tb:
            before, calls[0] = trk.time, 0
            with contextlib.redirect_stdout(sink):
                trk.next(t)
            out["tracked"][t] = True
            out["observed"][t] = trk.is_observed()
            out["updated"][t] = trk.is_observed() and trk.lastUpdateT == before
            if case["type"] == "iekf" and out["updated"][t]:
                out["rounds"][t] = calls[0] if count_rounds else trk.rounds
            if margins is not None and trk.is_observed():
                margins.setdefault("cdf", []).append(trk.gate_cdf)
                if case["type"] == "iekf" and out["updated"][t]:
                    margins.setdefault("diffs", []).extend(trk.round_diffs)
        out["x"][t], out["K"][t] = trk.xk_filter, trk.K_filter
    out["filtered_lines"] = sink.getvalue().count("Filtering innovation")
    return out


def load_cases():
    z = np.load(GOLDEN)
    cases = {}
    for name in json.loads(str(z["names"])):
        meta = json.loads(str(z[name + "_meta"]))
        meta.update(name=name, lag=z[name + "_lag"], height=z[name + "_height"], mpos=z[name + "_mpos"], pairs=z[name + "_pairs"],
                    gold=dict(x=z[name + "_x"], K=z[name + "_K"], observed=z[name + "_observed"], updated=z[name + "_updated"],
                              rounds=z[name + "_rounds"]))
        cases[name] = meta
    return cases
