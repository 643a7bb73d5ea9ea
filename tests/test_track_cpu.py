"""CPU: btk20.pykalman's host classes, the O(P) form of track_kernels.hip and its incomplete gamma function against the golden
vectors of the reference's own lib/pykalman.py (tests/golden/gen_golden_pykalman.py), and the margins of the fixtures' branch
decisions.

Figures of this file on the development machine (e_form: O(P) form against the golden, x and K_filter; e_sens: the host classes
against themselves with the pair order reversed -- the same filter, summed in another order):
  sigmaK2 1e2  cases: e_form  <= 1.2e-11 rad (x; 7.6e-8 for the 70-pair case, conditioned 1e5 times worse), <= 1.2e-9 (K)
  sigmaK2 1e6  cases: e_form  <= 4.0e-13 rad, 6.3e-15 mm (x), <= 1.5e-8 (K, of entries up to 1e6)
  sigmaK2 1e10 cases: e_form  3.1e-4 rad linear, 1.5e-4 rad circular, 1.8e-10 mm Cartesian;
                      e_sens  9.6e-4 rad linear, 1.2e-4 rad circular, 2.0e-10 mm Cartesian.
"""
import numpy as np
import pytest

from tests import track_closed_form as cf

CASES = cf.load_cases()
NAMES = sorted(CASES)


@pytest.fixture(scope="module")
def host_runs():
    out = {}
    for name in NAMES:
        margins = {}
        out[name] = (cf.run_host(CASES[name], margins=margins), margins)
    return out


def test_the_cases_cover_what_they_are_meant_to():
    c = CASES
    assert {c[n]["n"] for n in NAMES} == {1, 2, 3}
    assert {len(c[n]["pairs"]) for n in NAMES} >= {1, 6, 15, 70}
    assert {c[n]["lag"].shape[1] for n in NAMES} >= {1, 37}
    assert {c[n]["type"] for n in NAMES} == {"ekf", "iekf"}
    assert {c[n]["params"]["sigmaK2"] for n in NAMES} == {1e2, 1e6, 1e10}
    assert {c[n]["model"] for n in NAMES if c[n]["params"]["sigmaK2"] == 1e10 and c[n]["params"]["sigmaV2"] == 4e-4} == \
        {"linear", "circular", "cartesian"}
    assert any(c[n]["params"]["gate_prob"] == 0.0 for n in NAMES)
    assert sorted(c["stream%d" % i]["t_begin"] for i in range(3)) == [0, 3, 7]
    assert not c["linear_P1_never"]["gold"]["observed"].any()
    fu = c["circular_iekf_FU"]["params"]
    assert not np.array_equal(fu["F"], np.identity(2)) and fu["U"][0][1] != 0
    rounds, gated, gaps = set(), 0, set()
    for n in NAMES:
        g = c[n]["gold"]
        if c[n]["type"] == "iekf":
            rounds |= {(int(r), c[n]["params"]["num_iterations"]) for r in g["rounds"][g["updated"]]}
        gated += int((g["observed"] & ~g["updated"]).sum())
        run = 0
        for t in range(c[n]["t_begin"], len(g["observed"])):
            run = 0 if g["observed"][t] else run + 1
            if run:
                gaps.add(run)
    assert any(r == 1 for r, _ in rounds) and any(r == 2 for r, _ in rounds) and any(r == k and k >= 3 for r, k in rounds)
    assert gated > 0 and {1, 5} <= gaps


@pytest.mark.parametrize("name", NAMES)
def test_host_classes_equal_the_reference(name, host_runs):
    """the same numpy calls in the same order: equality"""
    got, gold = host_runs[name][0], CASES[name]["gold"]
    for k in ("observed", "updated", "rounds", "x", "K"):
        assert np.array_equal(got[k], gold[k]), k
    assert got["filtered_lines"] == int((gold["observed"] & ~gold["updated"]).sum())


@pytest.mark.parametrize("name", NAMES)
def test_fixture_margins(name, host_runs):
    """branch decisions are conditions, not tolerances: no frame of any case may sit near one"""
    case, (run, m) = CASES[name], host_runs[name]
    prm = case["params"]
    cdf = np.array(m.get("cdf", []))
    assert len(cdf) == run["observed"].sum()
    if len(cdf):
        print("%s: min |cdf - gate_prob| = %.3g" % (name, np.abs(cdf - prm["gate_prob"]).min()))
        assert np.abs(cdf - prm["gate_prob"]).min() > 1e-6
    d = np.array(m.get("diffs", []))
    if len(d):
        rel = np.abs(d - prm["iteration_threshold"]) / prm["iteration_threshold"]
        print("%s: min rel | |delta|^2 - iteration_threshold | = %.3g" % (name, rel.min()))
        assert rel.min() > 1e-6
    thr = np.float32(prm["threshold"])
    h = case["height"]
    assert not ((h >= np.nextafter(thr, np.float32(-1))) & (h <= np.nextafter(thr, np.float32(2)))).any()
    assert abs(float(thr) - prm["threshold"]) < 1e-8 and not np.any(h.astype(np.float64) == prm["threshold"])


def test_every_branch_of_adjust_boundaries_is_reached():
    cf.BRANCH_HITS.clear()
    for name in NAMES:
        cf.track_form(CASES[name])
    assert cf.BRANCH_HITS == {"theta<0", "theta>pi", "phi<-pi", "phi>pi"}


def e_form_of(case):
    """(max |x - golden x|, max |K - golden K|) of the O(P) form; its flags must be the golden's"""
    f, g = cf.track_form(case), case["gold"]
    for k in ("observed", "updated", "rounds"):
        assert np.array_equal(f[k], g[k]), (case["name"], k)
    return float(np.abs(f["x"] - g["x"]).max()), float(np.abs(f["K"] - g["K"]).max())


def e_sens_of(case):
    """the reference's own sensitivity: the host classes with the pair order reversed against the golden"""
    rev = cf.run_host(case, order=list(range(len(case["pairs"])))[::-1])
    for k in ("observed", "updated", "rounds"):
        assert np.array_equal(rev[k], case["gold"][k]), (case["name"], k)
    return float(np.abs(rev["x"] - case["gold"]["x"]).max())


@pytest.mark.parametrize("name", NAMES)
def test_form_against_the_reference(name):
    """The O(P) form is algebraically the reference's filter; what separates them is rounding, amplified by the conditioning
    of the reference's S^-1 and (I - G H) K_predict, which grows like sigmaK2 |H|^2 / sigmaV2.  Bounds: 1e-10 at sigmaK2 = 1e2
    and 1e6 with the fixtures' sigmaV2 (conditioning <= 1e4: 1e4 * 2^-52 * a few hundred operations; the 70-pair case is
    conditioned 1e5 and gets 1e-6), and at 1e10 (conditioning 1e7 .. 1e8, the reference's own noise) a small multiple of the
    reference's sensitivity to the order of its own sums."""
    case = CASES[name]
    ex, eK = e_form_of(case)
    print("%s: e_form x %.3g K %.3g" % (name, ex, eK))
    if case["params"]["sigmaK2"] == 1e10:
        es = e_sens_of(case)
        print("%s: e_sens %.3g" % (name, es))
        assert ex <= 4 * es
    else:
        tol = 1e-6 if len(case["pairs"]) == 70 else 1e-10
        assert ex <= tol
        assert eK <= tol * max(1.0, case["params"]["sigmaK2"])          # K_filter starts at sigmaK2 I


def test_incomplete_gamma_restated_against_scipy():
    """series below a + 1, continued fraction from there on; the prefactor exp(-x + a ln x - lgamma(a)) carries the error: its
    exponent is a difference of terms up to |t| = max(x, a ln x, lgamma a), so the relative error is about |t| 2^-52 (a few ulp
    of each term) -- bound 16 |t| 2^-53 + 1e-15, on P where the series runs and on Q = 1 - P where the fraction runs"""
    import math
    from scipy import special
    for a in (0.5, 1.0, 1.5, 3.0, 7.5, 35.0, 1008.0):
        for f in (1e-6, 1e-3, 0.1, 0.5, 0.9, 0.999, 1.0, 1.0 + 0.5 / a, 1.0 + 1.0 / a, 1.0 + 2.0 / a, 1.1, 1.5, 2.0, 5.0, 30.0):
            x = a * f
            got, t = cf.gammainc_restated(a, x), max(x, abs(a * math.log(x)), abs(math.lgamma(a)))
            rel = 16 * t * 2.0 ** -53 + 1e-15
            if x < a + 1.0:
                want = special.gammainc(a, x)
                assert abs(got - want) <= rel * want + 1e-300, (a, x, got, want)
            else:
                want = special.gammaincc(a, x)
                assert abs((1.0 - got) - want) <= rel * want + 2.0 ** -52, (a, x, got, want)
    assert cf.gammainc_restated(3.0, 0.0) == 0.0 and cf.gammainc_restated(3.0, -1.0) == 0.0
    assert cf.gammainc_restated(3.0, float("inf")) == 1.0 and cf.gammainc_restated(3.0, 1e6) == 1.0


def test_kalman_filter_with_a_fixed_H():
    """the conventional filter (host path only): a scalar random walk observed directly converges on the observations"""
    import contextlib
    import io
    from distant_speech_recognition_amd.pykalman import KalmanFilter

    class Source:
        def next(self, frame_no):
            return None if frame_no == 2 else np.array([1.0, 1.0])

    kf = KalmanFilter(Source(), F=np.identity(1), U=np.identity(1), sigmaV2=1e-2, sigmaK2=1e2, time_delta=0.1,
                      H=np.array([[1.0], [1.0]]))
    kf.gate_prob = 1.0                                  # the chi cdf never exceeds one: no gate
    kf.set_time(0)
    seen = []
    with contextlib.redirect_stdout(io.StringIO()):
        for xk in kf:
            seen.append((float(xk[0]), kf.is_observed()))
            if len(seen) == 4:
                break
    assert [o for _, o in seen] == [True, True, False, True]
    assert abs(seen[0][0] - 1.0) < 1e-4 and seen[2][0] == seen[1][0] and kf.time == 4 and kf.lastUpdateT == 3
    assert kf.K_filter[0, 0] < 1e-2 and kf.within_room([0.5]) and kf.adjust_boundaries(np.array([-0.5]))[0] == 0.5


@pytest.mark.parametrize("name", ["linear_P70", "circular_ekf_k2", "cartesian_ekf_k2"])
def test_feature_vectors_hand_the_kernel_their_geometry(name):
    """what the device path of the classes gives engine.ekf_track per pair is what the tests give it"""
    from distant_speech_recognition_amd import pytdoa
    case = CASES[name]
    model, geom = cf.table_front_end(pytdoa, case)._track_model()
    assert model == case["model"] and geom.dtype == np.float64
    assert np.array_equal(geom, cf.pair_geometry(case["model"], case["mpos"], case["pairs"]))
