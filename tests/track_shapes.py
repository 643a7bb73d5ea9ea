"""Shape cases for the tracker beyond its golden fixtures (no test in here; imported by test_track_shapes_cpu.py and
test_gpu_track_shapes.py): many pairs, short LDS tiles, hand-made frames, the gate next to its threshold, many turns of phi.

Nothing is stored: the tables come from the builder of tests/golden/gen_golden_pykalman.py (tables, params, all_pairs, which
import without the reference), the yardsticks are the package's host classes (track_closed_form.run_host) and the O(P) form in
numpy (track_closed_form.track_form).

  * CASES: name -> case, in the layout of track_closed_form.load_cases (without a golden record).
  * tile_of: the frame tile btk_ekf_track picks -- 48 KB of LDS, 48 + 8 tile bytes per pair, at most 32 frames, at most T.
  * yardstick(name): host run, margins, form run, e_form, e_perm -- once per case and process.
  * e_drop_of(name): what one dropped pair in one frame moves x by.
  * gate_launches(): T = 1 cases whose gate value sits at gate_prob + delta on the host, sigmaV2 found by bisection.
  * turn_cases(): T = 1 circular cases whose initial phi lies thousands of turns out.
"""
import functools
import math

import numpy as np

from tests import track_closed_form as cf
from tests.golden.gen_golden_pykalman import all_pairs, params, tables, trajectory

NO_PEAK = cf.NO_PEAK
LDS_BYTES, MAX_TILE, MAX_PAIRS = 48 * 1024, 32, 877
X0 = {"linear": [0.9], "circular": [1.1, 2.6], "cartesian": [1.5, 0.5, 900.0]}
N_OF = {"linear": 1, "circular": 2, "cartesian": 3}
# T = 70: outliers and unobserved frames in every tile of every regime (32 | 32 | 6, 31 | 31 | 8, 26 | 26 | 18, tiles of 8)
OUTLIERS, UNOBSERVED = (5, 17, 18, 40, 41, 58, 65), (3, 24, 25, 26, 27, 28, 45, 63, 64)


def tile_of(P, T):
    return min(MAX_TILE, (LDS_BYTES - 48 * P) // (8 * P), T)


# ---- arrays -------------------------------------------------------------------------------------------------------------------
def line(M):
    return [[40.0 * i, 0.0, 0.0] for i in range(M)]


def ring(M, radius=120.0):
    """a ring with uneven heights"""
    ang = 2 * np.pi * np.arange(M) / M
    return np.stack([radius * np.cos(ang), radius * np.sin(ang), 10.0 * (np.arange(M) % 4)], axis=1).tolist()


def ring_with_apex(M, radius=200.0):
    ang = 2 * np.pi * np.arange(M - 1) / (M - 1)
    flat = np.stack([radius * np.cos(ang), radius * np.sin(ang), np.zeros(M - 1)], axis=1).tolist()
    return flat + [[0.0, 0.0, 150.0]]


ARRAY_OF = {"linear": line, "circular": ring, "cartesian": ring_with_apex}


def exact_pairs(P):
    """(M, pairs): all pairs a < b of the largest array with at most P of them, then reversed ones, then repeated ones"""
    M = 2
    while (M + 1) * M // 2 <= P:
        M += 1
    base = all_pairs(M)
    extra = [(b, a) for a, b in base[::3]] + base
    assert len(base) + len(extra) >= P
    return M, base + extra[:P - len(base)]


def make_case(name, model, type, P, prm, T=70, seed=1, t_begin=0, x0=None, outliers=OUTLIERS, unobserved=UNOBSERVED):
    M, pairs = exact_pairs(P)
    mpos = ARRAY_OF[model](M)
    lag, height = tables(model, mpos, pairs, T, seed, [t for t in outliers if t < T], [t for t in unobserved if t < T])
    return dict(name=name, model=model, type=type, n=N_OF[model], x0=list(X0[model] if x0 is None else x0), t_begin=t_begin,
                params=prm, lag=lag, height=height, mpos=np.array(mpos, np.float64), pairs=np.array(pairs, np.int32))


# ---- hand-made frames ------------------------------------------------------------------------------------------------------------
HAND_FRAMES = dict(second_round_only=10, exactly_minimum=12, one_short=36, no_peak_decides=50)
LOW, HIGH = np.float32(0.03), np.float32(0.5)


def hand_frames(case):
    """Overwrite four frames of a P >= 128 case (lags stay the true ones):
      second_round_only: only pairs 64 .. 127 above the threshold;
      exactly_minimum:   minimum_pairs pairs above it, spread over the lane rounds;
      one_short:         minimum_pairs - 1, spread over all lane rounds;
      no_peak_decides:   minimum_pairs above it, of which pair 70 has no peak -- height alone would pass the frame."""
    P, mp = len(case["pairs"]), case["params"]["minimum_pairs"]
    assert P >= 130 and mp <= P - 8
    lag, height = case["lag"], case["height"]

    def spread(count):
        """`count` pair indices, two of them in the last round, the rest alternating between the first two"""
        tail = [P - 1, P - 2]
        body = [(i // 2) + 64 * (i % 2) for i in range(count - 2)]
        assert len(set(body + tail)) == count and max(body) < 128
        return body + tail

    t = HAND_FRAMES["second_round_only"]
    height[:, t] = LOW
    height[64:128, t] = HIGH
    t = HAND_FRAMES["exactly_minimum"]
    height[:, t] = LOW
    height[spread(mp), t] = HIGH
    t = HAND_FRAMES["one_short"]
    height[:, t] = LOW
    height[spread(mp - 1), t] = HIGH
    t = HAND_FRAMES["no_peak_decides"]
    idx = spread(mp)
    assert 70 in idx
    height[:, t] = LOW
    height[idx, t] = HIGH
    lag[70, t] = NO_PEAK
    return case


# ---- the cases -------------------------------------------------------------------------------------------------------------------
SV = 2e-8                                          # the fixtures' gate-deciding sigmaV2; cases with many pairs need more
F3 = [[1.0, 0.01, 1e-6], [-0.02, 0.995, -1e-6], [1e-3, -2e-3, 1.0]]
U3 = [[10.0, 2.0, 1.0], [2.0, 6.0, -1.0], [1.0, -1.0, 8.0]]


def build_cases():
    cases = {}

    def add(name, *a, **k):
        cases[name] = make_case(name, *a, **k)
        return cases[name]

    # P                                   tile
    add("linear_P64", "linear", "ekf", 64, params(1, 1e2, SV))                                            # 32: one lane round
    add("circular_P65", "circular", "iekf", 65, params(2, 1e2, SV_OF["circular_P65"]))                    # 32: one lane more
    add("cartesian_P161", "cartesian", "ekf", 161, params(3, 1e2, SV_OF["cartesian_P161"]))               # 32: the last full tile
    add("linear_P162", "linear", "iekf", 162, params(1, 1e2, SV_OF["linear_P162"], minimum_pairs=100))    # 31: the first short one
    add("circular_P190", "circular", "iekf", 190, params(2, 1e2, SV_OF["circular_P190"]))                 # 26 + 26 + 18
    add("cartesian_P435", "cartesian", "iekf", 435, params(3, 1e6, SV_OF["cartesian_P435"]))              # 8: eight full, one ragged
    add("linear_P861", "linear", "ekf", 861, params(1, 1e2, SV_OF["linear_P861"]))                        # 1
    add("circular_P877", "circular", "ekf", 877, params(2, 1e2, SV_OF["circular_P877"], minimum_pairs=400))  # 1: the largest
    # block lengths on a tile-32 case with a second lane round: one tile, one frame more, two tiles, three and a frame
    for T in (32, 33, 64, 97):
        add("linear_P70_T%d" % T, "linear", "iekf", 70, params(1, 1e2, SV_OF["linear_P70"]), T=T, seed=2,
            outliers=OUTLIERS + (80, 90), unobserved=UNOBSERVED + (85, 86))
    # a non-identity F and a non-diagonal U at n = 3
    add("cartesian_P78_FU", "cartesian", "iekf", 78,
        params(3, 1e2, SV_OF["cartesian_P78_FU"], F=F3, U=U3, num_iterations=4, iteration_threshold=1e-6))
    # hand-made frames, minimum_pairs within the first lane round and beyond it
    hand_frames(add("linear_P130_hand40", "linear", "ekf", 130, params(1, 1e2, SV_OF["linear_P130_hand40"], minimum_pairs=40)))
    hand_frames(add("linear_P130_hand66", "linear", "iekf", 130, params(1, 1e2, SV_OF["linear_P130_hand66"], minimum_pairs=66)))
    return cases


# sigmaV2 per case: chosen so that at least ten frames update, the outliers are gated and no decision sits near its threshold
# (test_track_shapes_cpu.py asserts all three); the lags are rounded to whole samples, so the residual of P pairs grows like P
SV_OF = {
    "circular_P65": 4e-7, "cartesian_P161": SV, "linear_P162": 4e-7, "circular_P190": 2e-6, "cartesian_P435": 1e-7,
    "linear_P861": 4e-7, "circular_P877": 2e-6, "linear_P70": 4e-7, "cartesian_P78_FU": SV, "linear_P130_hand40": 4e-7,
    "linear_P130_hand66": 4e-7,
}
TILE_OF = {"linear_P64": 32, "circular_P65": 32, "cartesian_P161": 32, "linear_P162": 31, "circular_P190": 26, "cartesian_P435": 8,
           "linear_P861": 1, "circular_P877": 1, "linear_P70_T32": 32, "linear_P70_T33": 32, "linear_P70_T64": 32,
           "linear_P70_T97": 32, "cartesian_P78_FU": 32, "linear_P130_hand40": 32, "linear_P130_hand66": 32}

CASES = build_cases()
NAMES = list(CASES)


def stream_cases():
    """three streams of the P = 435 configuration: their own tables, first frames 0, 7 and 40 (the last beyond a first piece of
    5 or 33 frames), each starting at the source's position in its first frame"""
    base = CASES["cartesian_P435"]
    out = []
    for i, tb in enumerate((0, 7, 40)):
        x0 = trajectory("cartesian", 70, None)[tb].tolist()
        out.append(make_case("stream%d_P435" % i, "cartesian", "iekf", 435, base["params"], seed=20 + i, t_begin=tb, x0=x0,
                             outliers=(9 + i, 44, 58), unobserved=(12 + 2 * i, 47, 48, 49, 66)))
    return out


# ---- yardsticks ------------------------------------------------------------------------------------------------------------------
def permuted(case, order):
    c = dict(case)
    c["pairs"], c["lag"], c["height"] = case["pairs"][order], case["lag"][order], case["height"][order]
    return c


def same_flags(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("tracked", "observed", "updated", "rounds"))


def yardstick_of(case):
    """dict(host, margins, form, e_form (x, K), e_perm (x, K)): e_form the form against the host classes, e_perm the largest
    deviation of the form from itself over four random permutations of the pairs (what the order of the sums alone moves)"""
    margins = {}
    host = cf.run_host(case, margins=margins)
    form = cf.track_form(case)
    e_form = (float(np.abs(form["x"] - host["x"]).max()), float(np.abs(form["K"] - host["K"]).max()))
    rng = np.random.default_rng(7)
    ex = eK = 0.0
    perm_flags = True
    for _ in range(4):
        f = cf.track_form(permuted(case, rng.permutation(len(case["pairs"]))))
        perm_flags = perm_flags and same_flags(f, form)
        ex, eK = max(ex, float(np.abs(f["x"] - form["x"]).max())), max(eK, float(np.abs(f["K"] - form["K"]).max()))
    return dict(host=host, margins=margins, form=form, e_form=e_form, e_perm=(ex, eK), perm_flags=perm_flags)


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """yardstick_of a case of CASES, once per process"""
    return yardstick_of(CASES[name])


def form_bounds(name):
    return form_bounds_of(yardstick(name))


def form_bounds_of(y):
    """(x, K) bounds of the kernel against the form: 64 times the form's own spread under permutation of the pairs, floored at
    1e-13 of the largest entry (the factor and the floor of test_gpu_track.py)"""
    return (max(64 * y["e_perm"][0], 1e-13 * max(1.0, float(np.abs(y["form"]["x"]).max()))),
            max(64 * y["e_perm"][1], 1e-13 * float(np.abs(y["form"]["K"]).max())))


def e_drop_of(name):
    """the smallest change of x (largest over frames and entries) when one observed pair's height is zeroed in one updated frame:
    pairs 0, 63, 64 and P - 1, each in the middle one of the updated frames in which it is observed"""
    case, form = CASES[name], yardstick(name)["form"]
    P = len(case["pairs"])
    thr = case["params"]["threshold"]
    out = []
    for p in sorted({0, 63, 64, P - 1} & set(range(P))):
        seen = (case["height"][p].astype(np.float64) > thr) & (case["lag"][p] != NO_PEAK) & form["updated"]
        ts = np.flatnonzero(seen)
        assert len(ts), (name, p)
        h = case["height"].copy()
        h[p, ts[len(ts) // 2]] = 0.0
        out.append(float(np.abs(cf.track_form(case, height=h)["x"] - form["x"]).max()))
    return min(out)


# ---- the gate next to its threshold --------------------------------------------------------------------------------------------
GATE_NOBS, GATE_PROBS = (2, 3, 66, 861), (0.05, 0.5, 0.95)
GATE_DELTAS = (1e-3, -1e-3, 1e-5, -1e-5, 1e-7, -1e-7)
GATE_SIGMAK2 = 1e-2


def gate_case(nobs, sigmaV2, gate_prob):
    """T = 1, linear model, `nobs` observed pairs of a line; lags of the source at x0, each moved by -1 .. +1 samples"""
    M = {2: 3, 3: 3, 66: 12, 861: 42}[nobs]
    pairs = all_pairs(M)[:nobs]
    mpos = line(M)
    lag, height = tables("linear", mpos, pairs, 1, 3)
    rng = np.random.default_rng(100 + nobs)
    lag = (lag + rng.integers(-1, 2, size=lag.shape)).astype(np.int32)
    if not np.any(lag - tables("linear", mpos, pairs, 1, 3)[0]):
        lag[0, 0] += 1
    return dict(name="gate_n%d_g%g" % (nobs, gate_prob), model="linear", type="ekf", n=1, x0=[0.9], t_begin=0,
                params=params(1, GATE_SIGMAK2, sigmaV2, gate_prob=gate_prob, minimum_pairs=2), lag=lag, height=height,
                mpos=np.array(mpos, np.float64), pairs=np.array(pairs, np.int32))


def gate_sums(case):
    """A, b, s^T s and K_predict of the single frame (n = 1): none depends on sigmaV2"""
    prm = case["params"]
    g = cf.pair_geometry("linear", case["mpos"], case["pairs"])
    xp = np.array(case["x0"], np.float64)
    tau, H = cf.model_rows("linear", g, xp, prm["c"])
    hx = H @ xp
    s = (case["lag"][:, 0].astype(np.float64) * prm["Ts"] - (tau - hx)) - hx
    el = prm["time_delta"]                                            # time 0, last update -1
    return float(H[:, 0] @ H[:, 0]), float(H[:, 0] @ s), float(s @ s), prm["sigmaK2"] + el * el * prm["U"][0][0]


def gate_ax(sums, nobs, sigmaV2):
    """(a, x) of P(a, x) as the kernel forms them"""
    A, b, ss, Kp = sums
    d2 = (ss - b * (Kp / (sigmaV2 + A * Kp)) * b) / sigmaV2
    return 0.5 * nobs, 0.5 * d2 * d2


def host_gate(case):
    m = {}
    h = cf.run_host(case, margins=m)
    return float(m["cdf"][0]), bool(h["updated"][0])


@functools.lru_cache(maxsize=None)
def gate_launches():
    """72 launches: dict(case, nobs, gate_prob, delta, sigmaV2, a, x, cdf (the host's), updated (the host's decision)).
    sigmaV2 by bisection on the closed form of the frame (scipy's gammainc of gate_ax; the squared distance s^T S^-1 s falls
    monotonically as sigmaV2 grows, since S = sigmaV2 I + H K_predict H^T grows with it), then corrected by what the host
    classes' own gate_cdf differs from it by, until the host's value is within 2 % of delta of its target."""
    from scipy import special
    out = []
    for nobs in GATE_NOBS:
        sums = gate_sums(gate_case(nobs, 1.0, 0.5))

        def cdf_of(log_sv):
            return float(special.gammainc(*gate_ax(sums, nobs, math.exp(log_sv))))

        def solve(target):
            lo, hi = math.log(1e-16), math.log(1e2)                   # cdf falls from 1 to 0 as sigmaV2 grows
            assert cdf_of(lo) > target > cdf_of(hi)
            for _ in range(200):
                mid = 0.5 * (lo + hi)
                if cdf_of(mid) > target:
                    lo = mid
                else:
                    hi = mid
            return 0.5 * (lo + hi)

        for gp in GATE_PROBS:
            for delta in GATE_DELTAS:
                want, shift = gp + delta, 0.0
                for _ in range(6):
                    sv = math.exp(solve(want - shift))
                    case = gate_case(nobs, sv, gp)
                    cdf, updated = host_gate(case)
                    if abs(cdf - want) <= 0.02 * abs(delta):
                        break
                    shift += cdf - want
                a, x = gate_ax(sums, nobs, sv)
                out.append(dict(case=case, nobs=nobs, gate_prob=gp, delta=delta, sigmaV2=sv, a=a, x=x, cdf=cdf, updated=updated))
    return out


# ---- thousands of turns ----------------------------------------------------------------------------------------------------------
TURN_SWITCH = 4096                                 # turns the kernel makes one by one, as the reference makes all of them
TURN_PHI = {"plus_1e5": 1.0e5, "minus_1e5": -1.0e5, "plus_4000_turns": 4000 * 2 * math.pi + 0.7,
            "minus_4000_turns": -4000 * 2 * math.pi - 0.7}


def turn_cases():
    """circular model, T = 1, phi_0 thousands of turns out; the tables are those of a source at (theta_0, phi_0 mod 2 pi), and
    sigmaK2 is small enough for the update to move the state by far less than a turn"""
    M, pairs = exact_pairs(28)
    mpos = ring(M)
    g = cf.pair_geometry("circular", mpos, pairs)
    out = {}
    for name, phi0 in TURN_PHI.items():
        true = np.array([1.1, math.fmod(phi0, 2 * math.pi)])
        prm = params(2, 1e-4, 4e-4)
        lag = np.rint(cf.model_rows("circular", g, true, prm["c"])[0] / prm["Ts"]).astype(np.int32)[:, None]
        height = np.full((len(pairs), 1), 0.5, np.float32)
        out[name] = dict(name="turns_" + name, model="circular", type="ekf", n=2, x0=[1.1, phi0], t_begin=0, params=prm, lag=lag,
                         height=height, mpos=np.array(mpos, np.float64), pairs=np.array(pairs, np.int32))
    return out
