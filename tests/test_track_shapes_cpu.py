"""CPU: the conditions the shape cases of tests/track_shapes.py must meet before test_gpu_track_shapes.py may rely on them --
the tile each case gets, frames of every kind, branch decisions away from their thresholds, the O(P) form's flags equal to the
host classes', and teeth: one dropped pair in one frame moves x by at least a hundred times the bound the kernel is held to
against the form.  Per case the test prints the tile, the frame counts, the margins, e_form, e_perm and e_drop.

Figures of this file on the development machine (e_form: form against host; e_perm: form against itself over four permutations
of the pairs; e_drop: one pair dropped in one frame; bound: max(64 e_perm, 1e-13 max(1, max |x|))):
  e_form   x <= 2.2e-9 rad (linear P = 861; 1.3e-10 at P = 64, <= 2.3e-11 elsewhere), K <= 9.6e-8 (Cartesian P = 435, of 1e6)
  e_perm   x <= 3.9e-15 rad, 1.1e-12 mm (Cartesian P = 435); K <= 2.3e-10 (of 1e6), <= 2.2e-14 at sigmaK2 = 1e2
  e_drop   >= 3.5e-8 mm (Cartesian P = 435), >= 6.6e-7 elsewhere; e_drop / bound >= 387 (Cartesian P = 435), >= 7e3 elsewhere
  margins  gate >= 0.017, IEKF threshold >= 2.3e-3 relative
  gate set every target met by the host's gate_cdf to 1e-14; restated against scipy <= 1.3e-13 (at a = 430.5)
The tile reaches one frame at P = 769 (768 pairs still get two: 49152 - 48 * 768 = 2 * 8 * 768).
"""
import numpy as np
import pytest

from tests import track_closed_form as cf
from tests import track_shapes as ts

CASES, NAMES = ts.CASES, ts.NAMES


def test_the_cases_cover_what_they_are_meant_to():
    c = CASES
    shape = {n: c[n]["lag"].shape for n in NAMES}
    assert all(c[n]["lag"].shape == c[n]["height"].shape == (len(c[n]["pairs"]), shape[n][1]) for n in NAMES)
    # the tile the launch picks, from the kernel's documented rule
    for n in NAMES:
        P, T = shape[n]
        assert ts.tile_of(P, T) == ts.TILE_OF[n], n
    assert ts.tile_of(161, 70) == 32 and ts.tile_of(162, 70) == 31 and ts.tile_of(768, 70) == 2 and ts.tile_of(769, 70) == 1
    assert ts.tile_of(ts.MAX_PAIRS, 70) == 1 and ts.tile_of(ts.MAX_PAIRS + 1, 70) == 0
    assert ts.MAX_PAIRS * (48 + 8) <= ts.LDS_BYTES < (ts.MAX_PAIRS + 1) * (48 + 8)
    by_P = {P: (ts.TILE_OF[n], c[n]["model"], c[n]["type"]) for n, (P, T) in shape.items() if T == 70}
    assert {P: v[0] for P, v in by_P.items()}.items() >= {64: 32, 65: 32, 161: 32, 162: 31, 190: 26, 435: 8, 861: 1, 877: 1}.items()
    assert by_P[190][1:] == ("circular", "iekf") and by_P[435][1:] == ("cartesian", "iekf") and by_P[861][1:] == ("linear", "ekf")
    assert c["cartesian_P435"]["params"]["sigmaK2"] == 1e6 and max(c[n]["params"]["sigmaK2"] for n in NAMES) == 1e6
    # block lengths on one tile-32 case with a second lane round
    assert {T for n, (P, T) in shape.items() if n.startswith("linear_P70_T")} == {32, 33, 64, 97} and ts.tile_of(70, 97) == 32
    # a non-identity F and a non-diagonal U at n = 3 with a second lane round
    fu = c["cartesian_P78_FU"]
    F, U = np.array(fu["params"]["F"]), np.array(fu["params"]["U"])
    assert fu["n"] == 3 and shape["cartesian_P78_FU"][0] > 64 and np.all((F - np.identity(3))[~np.identity(3, bool)] != 0) and np.all(U != 0)
    assert np.array_equal(U, U.T) and np.linalg.eigvalsh(U).min() > 0
    assert any(c[n]["params"]["minimum_pairs"] > 64 for n in NAMES)
    # reversed and repeated pairs, every model beyond one lane round
    assert any((c[n]["pairs"][:, 0] > c[n]["pairs"][:, 1]).any() for n in NAMES)
    assert {c[n]["model"] for n in NAMES if shape[n][0] > 128} == {"linear", "circular", "cartesian"}
    # outliers and unobserved frames: in every tile of the tiles of 26 .. 32 frames, in the ragged last one of the tiles of 8
    for tile in (32, 31, 26):
        tiles = set(range(-(-70 // tile)))
        assert {t // tile for t in ts.OUTLIERS} == tiles and {t // tile for t in ts.UNOBSERVED} == tiles
    assert {t // 8 for t in ts.OUTLIERS} & {t // 8 for t in ts.UNOBSERVED} >= {0, 70 // 8}


@pytest.mark.parametrize("name", ["linear_P130_hand40", "linear_P130_hand66"])
def test_hand_made_frames(name):
    case = CASES[name]
    prm, P = case["params"], len(case["pairs"])
    mp = prm["minimum_pairs"]
    high = case["height"].astype(np.float64) > prm["threshold"]
    seen = high & (case["lag"] != cf.NO_PEAK)
    host = ts.yardstick(name)["host"]
    t = ts.HAND_FRAMES["second_round_only"]
    assert not seen[:64, t].any() and seen[64:128, t].all() and not seen[128:, t].any()
    assert host["observed"][t] == (64 >= mp)
    t = ts.HAND_FRAMES["exactly_minimum"]
    assert seen[:, t].sum() == mp and seen[:64, t].any() and seen[64:128, t].any() and seen[128:, t].any() and host["observed"][t]
    t = ts.HAND_FRAMES["one_short"]
    assert seen[:, t].sum() == mp - 1 and seen[:64, t].any() and seen[64:128, t].any() and seen[128:, t].any()
    assert not host["observed"][t]
    t = ts.HAND_FRAMES["no_peak_decides"]
    gone = np.flatnonzero(high[:, t] & ~seen[:, t])
    assert high[:, t].sum() == mp and seen[:, t].sum() == mp - 1 and len(gone) == 1 and gone[0] >= 64 and not host["observed"][t]
    # where such a frame is observed it is also used: the gate lets it pass
    assert host["updated"][ts.HAND_FRAMES["exactly_minimum"]]
    if mp <= 64:
        assert host["updated"][ts.HAND_FRAMES["second_round_only"]]


@pytest.mark.parametrize("name", NAMES)
def test_case_conditions(name):
    """frames of every kind, margins, flags of the form, and teeth"""
    case, y = CASES[name], ts.yardstick(name)
    host, form, m, prm = y["host"], y["form"], y["margins"], case["params"]
    P, T = case["lag"].shape
    updated, gated, unobserved = int(host["updated"].sum()), int((host["observed"] & ~host["updated"]).sum()), int((~host["observed"]).sum())
    cdf = np.array(m["cdf"])
    gate_margin = float(np.abs(cdf - prm["gate_prob"]).min())
    d = np.array(m.get("diffs", []))
    it_margin = float((np.abs(d - prm["iteration_threshold"]) / prm["iteration_threshold"]).min()) if len(d) else float("inf")
    e_drop = ts.e_drop_of(name)
    bx, bK = ts.form_bounds(name)
    print("%-20s P %3d T %2d tile %2d | updated %2d gated %2d unobserved %2d | gate margin %.3g IEKF margin %.3g | e_form x %.3g K %.3g"
          " | e_perm x %.3g K %.3g | e_drop %.3g | bound x %.3g K %.3g, e_drop / bound %.3g" % (
              name, P, T, ts.TILE_OF[name], updated, gated, unobserved, gate_margin, it_margin, y["e_form"][0], y["e_form"][1],
              y["e_perm"][0], y["e_perm"][1], e_drop, bx, bK, e_drop / bx))
    assert updated >= 10 and gated >= 2 and unobserved >= 2
    assert len(cdf) == host["observed"].sum() and gate_margin > 1e-6 and it_margin > 1e-6
    if case["type"] == "iekf":
        assert len(d) >= updated
    thr = np.float32(prm["threshold"])
    h = case["height"]
    assert not ((h >= np.nextafter(thr, np.float32(-1))) & (h <= np.nextafter(thr, np.float32(2)))).any()
    assert ts.same_flags(form, host) and y["perm_flags"]
    # the form is the host's filter: what separates them is the conditioning of the host's P x P inverse (test_track_cpu.py)
    assert y["e_form"][0] <= 1e-6 and y["e_form"][1] <= 1e-6 * max(1.0, prm["sigmaK2"])
    # teeth: one pair less in one frame is at least a hundred times what the kernel may differ from the form by
    assert e_drop >= 100 * bx


def test_stream_cases():
    streams = ts.stream_cases()
    assert [s["t_begin"] for s in streams] == [0, 7, 40] and all(s["lag"].shape == (435, 70) for s in streams)
    assert all(s["params"] == streams[0]["params"] and np.array_equal(s["pairs"], streams[0]["pairs"]) for s in streams)
    assert not np.array_equal(streams[0]["height"], streams[1]["height"])
    for s in streams:
        f = cf.track_form(s)
        tb = s["t_begin"]
        assert not f["tracked"][:tb].any() and f["updated"][tb:].sum() >= 10 and (f["observed"] & ~f["updated"]).sum() >= 2


def test_gate_launches_sit_where_they_are_meant_to():
    """every target is met by the host classes' own gate value, both expansions of the incomplete gamma function are taken, and
    the restated function agrees with scipy's at every (a, x) of the set"""
    from scipy import special
    launches = ts.gate_launches()
    assert len(launches) == 72
    assert {(g["nobs"], g["gate_prob"], g["delta"]) for g in launches} == \
        {(n, p, d) for n in ts.GATE_NOBS for p in ts.GATE_PROBS for d in ts.GATE_DELTAS}
    branches = set()
    for g in launches:
        case = g["case"]
        assert case["lag"].shape == (g["nobs"], 1) and case["params"]["sigmaV2"] == g["sigmaV2"]
        miss = g["cdf"] - g["gate_prob"] - g["delta"]
        restated = cf.gammainc_restated(g["a"], g["x"])
        scipys = float(special.gammainc(g["a"], g["x"]))
        series = g["x"] < g["a"] + 1.0
        branches.add((g["nobs"], series))
        print("nobs %3d gate_prob %.2f delta %+.0e: sigmaV2 %.6e a %.1f x %.6f %s host cdf - gate_prob %+.6e (miss %+.1e) "
              "restated - scipy %+.1e updated %d" % (g["nobs"], g["gate_prob"], g["delta"], g["sigmaV2"], g["a"], g["x"],
                                                     "series  " if series else "fraction", g["cdf"] - g["gate_prob"], miss,
                                                     restated - scipys, g["updated"]))
        assert abs(miss) <= 0.1 * abs(g["delta"])
        assert g["updated"] == (not g["cdf"] > g["gate_prob"]) and g["updated"] == (g["delta"] < 0)
        assert abs(restated - scipys) <= 1e-12
        # the closed form of the frame that steered sigmaV2 is the host's value to far below the smallest delta
        assert abs(scipys - g["cdf"]) <= 1e-8
    assert {s for _, s in branches} == {True, False}
    assert all((n, True) in branches and (n, False) in branches for n in ts.GATE_NOBS)
    # the residual is not zero, and not the state's to absorb: s^T s exceeds what lies along H
    for nobs in ts.GATE_NOBS:
        A, b, ss, Kp = ts.gate_sums(ts.gate_case(nobs, 1.0, 0.5))
        assert ss > 0 and ss - b * b / A > 0.1 * ss / nobs


def test_turn_cases():
    """the initial phi is where it is meant to be relative to the kernel's 4096 single turns, and the update is small"""
    import math
    for name, case in ts.turn_cases().items():
        turns = abs(case["x0"][1]) / (2 * math.pi)
        assert (turns > 15000) if "1e5" in name else (3900 < turns < ts.TURN_SWITCH - 90)
        margins = {}
        host = cf.run_host(case, margins=margins)
        form = cf.track_form(case)
        assert host["updated"][0] and ts.same_flags(form, host)
        phi = host["x"][0, 1]
        want = math.remainder(case["x0"][1], 2 * math.pi)
        print("%-18s %.1f turns: phi %.9f, phi_0 mod 2 pi %.9f, theta %.9f, cdf %.3g" % (name, turns, phi, want, host["x"][0, 0],
                                                                                      margins["cdf"][0]))
        assert -math.pi <= phi <= math.pi and abs(phi - want) < 1e-2 and abs(host["x"][0, 0] - 1.1) < 1e-2
        assert abs(margins["cdf"][0] - case["params"]["gate_prob"]) > 1e-6
