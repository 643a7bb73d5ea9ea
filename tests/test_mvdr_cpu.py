"""CPU: what lets tests/mvdr_closed_form.py serve as truth and its float32 evaluation as a yardstick, for every case list of
tests/test_gpu_mvdr_closed_form.py.

  * two float64 routes (LU solve; LAPACK Cholesky + triangular solves) agree to 2^-40 of a bin's largest weight
  * cond(R) <= 1e4 for every matrix of every case: a float64 error of cond 2^-53 stays far below FLOOR = 2^-22
  * fails_at(N, j): a float32 Cholesky -- either order -- sees pivot j <= 0 and every earlier pivot > 1e-3 of its diagonal entry
  * |Lambda_cf| >= 1e-3 d^H d / lambda_max: no case divides by a cancelling Lambda
  * the two float32 summation orders (plain right-looking, blocked left-looking) stay within [1/8, 8] of each other per case
"""
import numpy as np
import pytest

from tests import mvdr_closed_form as mcf

FORMS = ("lds", "reg", "panel", "default")


def _all_cases():
    seen = []
    for form in FORMS:
        for c in mcf.case_list(form):
            if c not in seen:
                seen.append(c)
    return seen


CASES = _all_cases()


def test_case_lists_hold_what_the_forms_need():
    assert mcf.panel_max() == 1052 and mcf.panel_lds_bytes(1053) > mcf.LDS_CAP
    assert 2064 + 8 * (137 * 137 + 137) <= mcf.LDS_CAP < 2064 + 8 * (138 * 138 + 138)        # the LDS kernel's largest matrix
    assert max(mcf.SIZES["lds"]) == 137 and max(mcf.SIZES["reg"]) == 271 and mcf.EVERY_SIZE == tuple(range(137, 272))
    for form, sizes in mcf.FAIL_N.items():
        for N in sizes:
            assert sorted(set(mcf.fail_columns(N))) == sorted(mcf.fail_columns(N)) and 0 <= min(mcf.fail_columns(N)) and max(mcf.fail_columns(N)) == N - 1


def test_inputs_are_exactly_hermitian_complex64():
    for kind, N, K in CASES:
        R, d = mcf.case_inputs(kind, N, K)
        assert R.dtype == np.complex64 and d.dtype == np.complex64 and R.shape == (K, N, N) and d.shape == (K, N)
        assert np.array_equal(R, np.conj(R.transpose(0, 2, 1))), (kind, N)
        assert not np.any(R[:, np.arange(N), np.arange(N)].imag)
        if kind == "diffuse":
            assert not np.any(R.imag)
        assert np.allclose(np.abs(d) * N, 1.0, rtol=1e-6)


def test_float64_routes_agree_and_every_case_is_well_conditioned():
    worst_route, worst_cond, worst_lam = 0.0, 0.0, np.inf
    for kind, N, K in CASES:
        R, d = mcf.case_inputs(kind, N, K)
        w, lam, _, _ = mcf.case_forms(kind, N, K)
        w2, lam2 = mcf.design_cf_chol(R, d)
        ev = np.linalg.eigvalsh(R.astype(np.complex128))
        assert np.all(ev[:, 0] > 0)
        cond = ev[:, -1] / ev[:, 0]
        route = np.max(np.abs(w - w2), axis=-1) / np.max(np.abs(w), axis=-1)
        lam_route = np.abs(lam - lam2) / np.abs(lam)
        dd = np.sum(np.abs(d.astype(np.complex128)) ** 2, axis=-1)
        lam_norm = np.abs(lam) / (dd / ev[:, -1])
        print("MVDRCPU %-8s N %4d  cond %9.3e  routes %.2e (Lambda %.2e)  |Lambda| / (d^H d / lmax) %.3g" %
              (kind, N, cond.max(), route.max(), lam_route.max(), lam_norm.min()))
        assert np.all(cond <= 1e4), (kind, N, cond)
        assert np.all(route <= 2.0 ** -40) and np.all(lam_route <= 2.0 ** -40), (kind, N, route, lam_route)
        assert np.all(lam_norm >= 1e-3), (kind, N, lam_norm)
        assert np.all(np.abs(lam.imag) <= 2.0 ** -40 * np.abs(lam))            # d^H z and z^H d are the same number
        worst_route, worst_cond, worst_lam = max(worst_route, route.max()), max(worst_cond, cond.max()), min(worst_lam, lam_norm.min())
    print("MVDRCPU worst: cond %.3e  routes %.2e  Lambda norm %.3g over %d cases" % (worst_cond, worst_route, worst_lam, len(CASES)))


def test_two_float32_orders_stay_within_a_factor_of_eight():
    lo, hi = np.inf, 0.0
    for kind, N, K in CASES:
        w, lam, wp, lp = mcf.case_forms(kind, N, K)
        _, _, wb, lb = mcf.case_forms(kind, N, K, "blocked")
        ep = np.max(np.abs(wp - w)) / np.max(np.abs(w))
        eb = np.max(np.abs(wb - w)) / np.max(np.abs(w))
        print("MVDRCPU orders %-8s N %4d  plain %.3e  blocked %.3e  ratio %.3f" % (kind, N, ep, eb, eb / ep if ep > 0 else (1.0 if eb == 0 else np.inf)))
        if max(ep, eb) <= mcf.FLOOR / mcf.FACTOR:
            continue                                                          # both under the floor of the rule: the rule never compares them
        assert 1.0 / 8.0 <= eb / ep <= 8.0, (kind, N, ep, eb)
        lo, hi = min(lo, eb / ep), max(hi, eb / ep)
    print("MVDRCPU orders: blocked / plain between %.3f and %.3f" % (lo, hi))


def test_identity_cases_have_the_known_answer():
    for kind, N, K in CASES:
        if kind == "identity":
            R, d = mcf.case_inputs(kind, N, K)
            w, lam, _, _ = mcf.case_forms(kind, N, K)
            assert np.max(np.abs(w - mcf.identity_answer(d))) <= 2.0 ** -40 / N           # whatever c is
            assert np.max(np.abs(w - d.astype(np.complex128))) <= 2.0 ** -21 / N           # N d^H d = 1 up to d's own rounding


@pytest.mark.parametrize("form", ["lds", "reg", "panel"])
def test_fails_at_fails_where_it_is_planted(form):
    for N in mcf.FAIL_N[form]:
        R, clean, d, flags = mcf.fail_inputs(N)
        cols = mcf.fail_columns(N)
        assert flags.sum() == len(cols) + 1 and flags[0] == 0 and flags[-1] == 0 and not np.any(flags[:-1] & flags[1:])
        for order in ("plain", "blocked"):
            _, piv = mcf.chol_f32(R, order)
            dg = R[:, np.arange(N), np.arange(N)].real
            for i, j in enumerate(cols):
                k = 2 * i + 1
                assert piv[k, j] < -0.02, (N, j, piv[k, j])                   # -0.5 of a Schur complement >= the 0.05 loading
                assert np.all(piv[k, :j] > 1e-3 * dg[k, :j]), (N, j, order)
            good = flags == 0
            assert np.all(piv[good] > 1e-3 * dg[good])
            assert np.isnan(piv[-2, N // 2]) and np.all(piv[-2, :N // 2] > 0)
        ev = np.linalg.eigvalsh(clean.astype(np.complex128))
        assert np.all(ev[:, -1] / ev[:, 0] <= 1e4)


def test_mode_inputs_are_well_conditioned_and_hermitian():
    for form, N in mcf.MODE_N.items():
        R, d = mcf.mode_inputs(N)
        assert R.shape == (3, 5, N, N) and d.shape == (3, 5, N) and np.array_equal(R, np.conj(R.transpose(0, 1, 3, 2)))
        ev = np.linalg.eigvalsh(R.astype(np.complex128))
        print("MVDRCPU modes %s N %d cond %.3e" % (form, N, (ev[..., -1] / ev[..., 0]).max()))
        assert np.all(ev[..., 0] > 0) and np.all(ev[..., -1] / ev[..., 0] <= 1e4)


def test_element_wise_forms():
    p = mcf.ula(5)
    p[3] = p[1]                                                               # two coincident microphones
    g = mcf.diffuse_cf(p, 8, 16000.0)
    assert g.shape == (5, 5, 5) and np.all(g[0] == 1.0) and np.all(g[:, 1, 3] == 1.0) and np.all(g[:, np.arange(5), np.arange(5)] == 1.0)
    x = 2.0 * 16000.0 * 3 * 40.0 / (8 * mcf.SSPEED)
    assert abs(g[3, 0, 2] - np.sin(np.pi * x) / (np.pi * x)) < 1e-15
    R = mcf.load_cf(g, 0.01)
    assert np.all(R[:, 0, 0] == 1.0 + float(np.float32(0.01))) and np.array_equal(R[:, 0, 1], g[:, 0, 1])
    Q = mcf.divide_nondiag_cf(g, 0.25)
    assert np.all(Q[:, 2, 2] == 1.0) and np.allclose(Q[:, 0, 2], g[:, 0, 2] / 1.25, rtol=1e-16)
    w = mcf.dc_rows(np.zeros((6, 2)), kper=3)
    assert np.all(w[[0, 3]] == 1.0) and not np.any(w[[1, 2, 4, 5]])
    assert not np.any(mcf.dc_rows(np.zeros((3, 2)), first_bin=2)) and np.all(mcf.dc_rows(np.zeros((3, 2)))[0] == 1.0)
