"""CPU: the float64 closed forms of the adaptive cancellers (tests/canceller_closed_form.py) against the oracle's restatements
of the reference (orc.NLMS, orc.RLSPy) on every fixture tests/test_gpu_canceller_closed_form.py uses, and the proof that
those fixtures reach the branches they are meant to with room to spare.

Figures of this file on the development machine.  e_frame: max over frames of max_k |Y[t] - ref[t]| / max_k |ref[t]|, the norm
the GPU test uses; e_peak: max |Y - ref| / max |ref| over the run.
  NLMS, all fixtures:              e_frame <= 2.6e-14, e_peak <= 1.4e-15
  RLS constraint_option 0:         e_frame <= 4.8e-11, e_peak <= 7.7e-12
  RLS constraint_option 1:         e_frame <= 8.5e-9,  e_peak <= 4.2e-9   (alpha2 = 1e-9 at N = 8; 1.8e-11 with init_diagonal_load = 1e8)
  RLS constraint_option 2:         e_frame <= 4.9e-15, e_peak <= 8.8e-16
  RLS constraint_option 3:         e_frame <= 7.6e-13, e_peak <= 3.0e-13
  NLMS with u, sigma2 and the products in float32 against float64: e_frame <= 3.6e-6 (a quarter of the GPU bound is 5e-5)
With the default init_diagonal_load = 1e6 the constraint_option 1 and 3 fixtures at N >= 24 gave e_frame between 3e-2 and 0.8: the
recursion is chaotic there (tests/canceller_closed_form.py, RLS_WELL), which is why they run at 1e8.
Branch hits (stream 0) and smallest margins |log(lhs / rhs)| of the discontinuous decisions are printed by the tests.
"""
import collections
import ctypes as C

import numpy as np
import pytest

from tests import canceller_closed_form as cf

# 100 x the largest figure measured for the family (see the docstring)
NLMS_BOUND = 2.6e-12
RLS_BOUND = {0: 4.8e-9, 1: 8.5e-7, 2: 4.9e-13, 3: 7.6e-11}
NLMS_IDS = ["N%d_Nc%d" % c for c in cf.NLMS_CASES]


@pytest.fixture(scope="module")
def blocking(orc):
    cache = {}

    def get(N, Nc, M):
        if (N, Nc, M) not in cache:
            vs = cf.manifold(N, M)[1]
            cache[N, Nc, M] = np.stack([orc.blocking_matrix(vs[k], Nc) for k in range(M // 2 + 1)])
        return cache[N, Nc, M]
    return get


@pytest.fixture(scope="module")
def rls_runs(orc, blocking):
    """name -> per stream (closed-form run, oracle output [T][K], oracle object)"""
    cache = {}

    def get(name):
        if name not in cache:
            N, Nc, M, S, _, kw, _ = cf.rls_case(name)
            delays, vs, Xe = cf.rls_input(name)
            B = blocking(N, Nc, M)
            runs = []
            for s in range(S):
                X = cf.full_frames(Xe[s], M)
                o = orc.RLSPy(M, N, Nc, **kw)
                o.calc_beamformer_weights(cf.SAMPLERATE, delays)
                ref = o.run(X)[:, :M // 2 + 1]
                runs.append((cf.rls_py_form(X, vs, B, kw), ref, o))
            cache[name] = runs
        return cache[name]
    return get


@pytest.fixture(scope="module")
def nlms_runs(orc, blocking):
    cache = {}

    def get(N, Nc):
        if (N, Nc) not in cache:
            M, S, kw = cf.nlms_case(N, Nc)
            delays, vs, Xe = cf.nlms_input(N, Nc)
            B = blocking(N, Nc, M)
            runs = []
            for s in range(S):
                X = cf.full_frames(Xe[s], M)
                o = orc.NLMS(M, N, Nc=Nc, **kw)
                o.calc_beamformer_weights(cf.SAMPLERATE, delays)
                ref = o.run(X)[:, :M // 2 + 1]
                runs.append((cf.nlms_form(X, vs, B, kw), ref, o, X))
            cache[N, Nc] = runs
        return cache[N, Nc]
    return get


def _errors(Y, ref):
    e_frame, zeros = cf.per_frame_error(Y, ref)
    return e_frame, float(np.max(np.abs(Y - ref)) / np.max(np.abs(ref))), zeros


# ------------------------------------------------------------------------------------------------ closed form == oracle
@pytest.mark.parametrize("name", cf.RLS_NAMES)
def test_rls_form_equals_the_oracle(orc, blocking, rls_runs, name):
    N, Nc, M, S, _, kw, _ = cf.rls_case(name)
    B = blocking(N, Nc, M)
    bound = RLS_BOUND[kw["constraint_option"]]
    for s, (run, ref, o) in enumerate(rls_runs(name)):
        e_frame, e_peak, zeros = _errors(run["Y"], ref)
        print("rls %s stream %d: e_frame %.3g e_peak %.3g" % (name, s, e_frame, e_peak))
        assert e_frame <= bound and zeros
        for k in range(M // 2 + 1):
            Pz, waH = B[k].T @ run["P"][k] @ np.conj(B[k]), run["w"][k] @ np.conj(B[k])     # P = conj(B) Pz B^T, w = wa^H B^T
            assert np.max(np.abs(waH - o.waH[k])) <= max(bound, 1e-9) * np.max(np.abs(o.waH))
            assert np.max(np.abs(Pz - o.Pz[k])) <= max(bound, 1e-9) * 10 * np.max(np.abs(o.Pz[k]))
        assert run["isamp"] == o.scal[1] and run["ttl_updates"] == o.scal[2]
        assert abs(run["E_avg"] - o.scal[0]) <= 1e-14 * o.scal[0]


@pytest.mark.parametrize("N,Nc", cf.NLMS_CASES, ids=NLMS_IDS)
def test_nlms_form_equals_the_oracle(orc, blocking, nlms_runs, N, Nc):
    M, S, kw = cf.nlms_case(N, Nc)
    K = M // 2 + 1
    B = blocking(N, Nc, M)
    for s, (run, ref, o, _) in enumerate(nlms_runs(N, Nc)):
        e_frame, e_peak, zeros = _errors(run["Y"], ref)
        print("nlms N=%d Nc=%d stream %d: e_frame %.3g e_peak %.3g" % (N, Nc, s, e_frame, e_peak))
        assert e_frame <= NLMS_BOUND and zeros
        wa = np.stack([run["u"][k] @ np.conj(B[k]) for k in range(K)])          # wa^H = u conj(B)
        assert np.max(np.abs(wa - o.wa())) <= NLMS_BOUND * np.max(np.abs(o.wa()))
        L = orc.lib()
        se = np.frombuffer((C.c_double * K).from_address(L.orc_nlms_subband_energy(o._h)), np.float64)
        assert np.max(np.abs(run["sigma2"] - se) / se) <= 1e-13
        assert abs(run["E_avg"] - L.orc_nlms_energy(o._h)) <= 1e-14 * run["E_avg"]


def test_first_lane_fixture(orc, blocking):
    """the hand-set energies put frames 40, 64 and 104 between E_prev / sil_thresh and E_t / sil_thresh, margins kept"""
    N, M = cf.LANE0_N, cf.LANE0_M
    delays, vs, Xe = cf.lane0_input()
    B = blocking(N, 1, M)
    X = cf.full_frames(Xe[0], M)
    for form, kw, bound, mk in ((cf.rls_py_form, cf.LANE0_RLS, RLS_BOUND[0], lambda: orc.RLSPy(M, N, 1, **cf.LANE0_RLS)),
                                (cf.nlms_form, cf.LANE0_NLMS, NLMS_BOUND, lambda: orc.NLMS(M, N, **cf.LANE0_NLMS))):
        run = form(X, vs, B, kw)
        o = mk()
        o.calc_beamformer_weights(cf.SAMPLERATE, delays)
        e_frame, _, _ = _errors(run["Y"], o.run(X)[:, :M // 2 + 1])
        print("first lane %s: e_frame %.3g" % (form.__name__, e_frame))
        assert e_frame <= bound
        assert np.flatnonzero(~run["adapt"]).tolist() == list(cf.LANE0_QUIET)
        assert run["margins"]["gate"] >= 0.1
        # with the chunk's own first value in place of the carried average every one of them would adapt
        E = kw.get("init_diagonal_load", 1.0e6)
        for t in range(cf.LANE0_T):
            e = abs(np.vdot(X[t, 0], X[t, 0])) / M
            E_t = kw["beta"] * E + (1.0 - kw["beta"]) * e
            if t in cf.LANE0_QUIET:
                assert E_t / kw["sil_thresh"] * 1.1 < e < E / kw["sil_thresh"] / 1.1
            E = E_t


# ------------------------------------------------------------------------------------------------ the fixtures reach their branches
def _hold_runs(adapt):
    """[first, last] of every run of held frames"""
    held = np.flatnonzero(~adapt)
    if not len(held):
        return []
    cuts = np.flatnonzero(np.diff(held) > 1)
    return list(zip(held[np.r_[0, cuts + 1]], held[np.r_[cuts, len(held) - 1]]))


def _check_gating(run, Xe0, profile):
    """stream 0 of a gated fixture.  The short profile has eleven quiet frames among its 48, so there the count demanded is
    that every one of them is held, not twenty."""
    adapt, h = run["adapt"], run["hits"]
    quiet = int((cf.frame_gains(profile) < 1).sum())
    assert h["adapt"] >= 20 and h["hold"] >= (20 if profile == "long" else quiet)
    assert not adapt[cf.frame_gains(profile) < 1].any()
    runs = _hold_runs(adapt)
    covered = 64 if profile == "long" else 16
    assert runs[0][0] == 0 and any(a <= covered <= b for a, b in runs)
    assert (~np.any(Xe0 != 0, axis=(0, 1))).sum() >= 1


@pytest.mark.parametrize("name", cf.RLS_NAMES)
def test_rls_fixture_branches_and_margins(rls_runs, name):
    N, Nc, M, S, profile, kw, named = cf.rls_case(name)
    _, _, Xe = cf.rls_input(name)
    runs = rls_runs(name)
    _check_gating(runs[0][0], Xe[0], profile)
    if S > 1:
        assert not np.array_equal(runs[0][0]["adapt"], runs[1][0]["adapt"])    # the streams' ctrl rows differ
    for s, (run, _, _) in enumerate(runs):
        h, m = run["hits"], run["margins"]
        print("rls %s stream %d: %s margins gate %.3g alpha2 %.3g norm %.3g" % (name, s, dict(h), m["gate"], m["alpha2"], m["norm"]))
        # conditions, not tolerances: a fixture that misses one gets another seed or other parameters
        assert m["gate"] >= 0.1 and m["alpha2"] >= 1e-4 and m["norm"] >= 1e-4
    for b in named:
        assert runs[0][0]["hits"][b] >= 5, b


def test_rls_fixtures_cover_every_branch(rls_runs):
    total = sum((rls_runs(n)[0][0]["hits"] for n in cf.RLS_NAMES), collections.Counter())
    assert total["quad_argpos"] and total["quad_argneg"] and total["reset"] and total["hold"] and total["adapt"]
    named = {b for n in cf.RLS_NAMES for b in cf.rls_case(n)[6]}
    assert named == {"quad_argpos", "quad_argneg", "reset"}
    assert {cf.rls_case(n)[5]["constraint_option"] for n in cf.RLS_NAMES} == {0, 1, 2, 3}


@pytest.mark.parametrize("N,Nc", cf.NLMS_CASES, ids=NLMS_IDS)
def test_nlms_fixture_branches_and_margins(nlms_runs, N, Nc):
    _, _, Xe = cf.nlms_input(N, Nc)
    runs = nlms_runs(N, Nc)
    _check_gating(runs[0][0], Xe[0], "long")
    h = runs[0][0]["hits"]
    assert h["floor"] >= 20 and h["halve"] >= 1
    if len(runs) > 1:
        assert not np.array_equal(runs[0][0]["adapt"], runs[1][0]["adapt"])
    for s, (run, _, _, _) in enumerate(runs):
        print("nlms N=%d Nc=%d stream %d: %s gate margin %.3g" % (N, Nc, s, dict(run["hits"]), run["margins"]["gate"]))
        # the kernel's gate compares a float32 energy with a float64 average: 0.1 is six orders above that difference
        assert run["margins"]["gate"] >= 0.1


def test_nlms_fixtures_reach_the_clamp(nlms_runs):
    assert sum(nlms_runs(N, Nc)[0][0]["hits"]["clamp"] > 20 for N, Nc in cf.NLMS_CASES) >= 3


# ------------------------------------------------------------------------------------------------ is the float32 bound feasible
@pytest.mark.parametrize("N,Nc", cf.NLMS_CASES, ids=NLMS_IDS)
def test_nlms_float32_state_stays_within_a_quarter_of_the_gpu_bound(blocking, nlms_runs, N, Nc):
    """the recursion with u, sigma2 and the per-frame products in float32, as the kernel holds them, against float64 in the
    GPU test's norm: an input on which rounding alone takes a quarter of the 2e-4 bound could not tell a wrong kernel from a
    right one, and would be replaced"""
    M, _, kw = cf.nlms_case(N, Nc)
    vs = cf.manifold(N, M)[1]
    B = blocking(N, Nc, M)
    for s, (run, _, _, X) in enumerate(nlms_runs(N, Nc)):
        r32 = cf.nlms_form(X, vs, B, kw, dtype=np.float32)
        e_frame, _ = cf.per_frame_error(r32["Y"], run["Y"])
        print("nlms N=%d Nc=%d stream %d: float32 state against float64 e_frame %.3g" % (N, Nc, s, e_frame))
        assert e_frame <= 5e-5
        assert np.array_equal(r32["adapt"], run["adapt"])
