"""The closed forms of tests/sos_closed_form.py against the oracle and the reference's golden outputs, the mutants against the
acceptance rules, and the conditions the design fixtures of tests/test_gpu_sos_closed_form.py rely on.  No GPU."""
import os

import numpy as np
import pytest

from tests import sos_closed_form as scf

F64 = 1e-12          # "float64 rounding" for sums of a few hundred terms and solves at condition <= 1e4


@pytest.fixture(scope="module")
def sosgolden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "pybeamformer_sos_golden.npz"))


@pytest.fixture(scope="module")
def mutant_fixture():
    """One covariance fixture for all the mutants: both weights, odd T, more than one tile row."""
    inp = scf.cov_input(2, 3, 17, 33, seed=1)
    tf, fw, R0 = scf.variant(inp, "both")
    Rcf = scf.cov_form(inp["X"], tf, fw, R0)
    R32 = scf.cov_form(inp["X"], tf, fw, R0, dtype=np.float32)
    return inp, Rcf, R32


# --------------------------------------------------------------------------------------------------- forms vs the oracle
@pytest.mark.parametrize("N,T", [(1, 5), (4, 33), (17, 31)])
@pytest.mark.parametrize("name", scf.WEIGHT_VARIANTS)
def test_cov_form_matches_oracle(orc, N, T, name):
    inp = scf.cov_input(2, 3, N, T)
    tf, fw, _ = scf.variant(inp, name)
    Rcf = scf.cov_form(inp["X"], tf, fw)
    for s in range(2):
        frames = scf.to_frames(inp["X"][s])
        if tf is None:
            ref = orc.cov_accumulate(frames, frame_weights=None if fw is None else fw[s])
        else:
            w = tf[s].astype(np.float64) * (1.0 if fw is None else fw[s].astype(np.float64)[None, :])
            ref = orc.cov_accumulate(frames, masks=np.ascontiguousarray(w.T))
        e = scf.e_elem(Rcf[s], ref)
        assert np.max(e) <= F64, (s, np.max(e))


def test_gated_off_frames_never_touched(orc):
    """NaN and Inf snapshots in frames of weight 0 leave the closed form, the yardstick and the oracle's gate untouched."""
    inp = scf.cov_input(1, 3, 5, 33)
    for how in ("gate", "mask", "both"):
        Xp, Xz, tf, fw = scf.poison(inp["X"], inp["tf"], inp["fw"], how)
        assert not np.all(np.isfinite(Xp.view(np.float32)))
        tfa, fwa = (None if how == "gate" else tf), (None if how == "mask" else fw)
        for dt in (np.float64, np.float32):
            a, b = scf.cov_form(Xp, tfa, fwa, dtype=dt), scf.cov_form(Xz, tfa, fwa, dtype=dt)
            assert np.array_equal(a, b) and np.all(np.isfinite(a.real))
    Xp, Xz, tf, fw = scf.poison(inp["X"], inp["tf"], inp["fw"], "gate")
    ref = orc.cov_accumulate(scf.to_frames(Xp[0]), frame_weights=fw[0])
    assert np.max(scf.e_elem(scf.cov_form(Xp, None, fw)[0], ref)) <= F64


def test_finalize_and_designs_match_oracle(orc):
    rng = np.random.default_rng(5)
    for N in (1, 4, 17):
        Rt, Rn = scf.design_input(N, bin0_real=False, seed=3)
        K = Rt.shape[0]
        ct, cn = rng.integers(3, 90, K).astype(np.float64), rng.integers(3, 90, K).astype(np.float64)
        for gamma in (0.0, 1e-2):
            ft, fn = orc.sos_finalize(Rt, Rn, ct, cn, gamma)
            assert np.max(np.abs(scf.finalize_form(Rt[None], ct[None])[0] - ft)) <= F64 * np.max(np.abs(ft))
            assert np.max(np.abs(scf.finalize_form(Rn[None], cn[None], gamma)[0] - fn)) <= F64 * np.max(np.abs(fn))
            ft, fn = orc.sos_finalize(Rt, Rn, ct, cn, gamma, gev=True)
            mine = scf.trace_normalize_form(scf.finalize_form(Rn[None], cn[None], gamma)[0])
            assert np.max(np.abs(mine - fn)) <= F64 * np.max(np.abs(fn))
        # per-stream counts are the per-bin ones with every bin alike
        a = scf.finalize_form(Rn[None], np.array([7.0]), 1e-2)
        b = scf.finalize_form(Rn[None], np.full((1, K), 7.0), 1e-2)
        assert np.array_equal(a, b)
        for ref_micx, offset in ((0, 0.0), (N // 2, 0.1), (N - 1, 1.0)):
            ref = orc.blind_mvdr_weights(Rt, Rn, ref_micx=ref_micx, offset=offset)
            W = scf.bmvdr_form(Rt, Rn, ref_micx, offset)
            assert np.max(scf.weight_errors(W, ref)) <= 1e-11
        ref = orc.gev_weights(Rt, Rn)
        for route in ("scipy", "cholesky"):
            W = scf.gev_form(Rt, Rn, route)
            c = scf.global_factor(W, ref)
            assert np.max(scf.weight_errors(W, ref, c)) <= scf.MAX_SPREAD
        assert np.array_equal(scf.gev_form(Rt, Rn), ref)                      # the same calls in the same order: no factor at all
        # the kernel's bin-0 convention is one more global factor, and makes the largest component of bin 0 real positive
        Wk = scf.gev_form(Rt, Rn, bin0="largest_real")
        assert np.max(scf.weight_errors(Wk, ref, scf.global_factor(Wk, ref))) <= 1e-13
        j = np.argmax(np.abs(Wk[0]))
        assert Wk[0, j].real > 0 and abs(Wk[0, j].imag) <= 1e-15 * Wk[0, j].real
        assert np.max(np.abs(scf.rn_norm(Wk, Rn) - 1.0)) <= 1e-12


def test_forms_match_reference_golden(orc, proto256, kinect_pcm, sosgolden):
    """The reference's own numpy / scipy run on four Kinect channels, stage by stage."""
    G = sosgolden
    T, M, K = int(G["meta_T"][0]), 256, 129
    h, _ = proto256
    Xo = np.stack([orc.analysis(h, M, 4, 1, 2, kinect_pcm[c][: (T + 8) * 128])[:T] for c in range(4)], axis=1)   # [T][N][M]
    Xe = np.ascontiguousarray(np.transpose(Xo[:, :, :K], (2, 1, 0)))[None]                                         # [1][K][N][T]
    en = np.array([[orc.frame_energy(Xo[t, 0]) for t in range(T)]])
    fw, cnt = scf.gate_form(en, 10.0)
    assert 0 < cnt[0] <= T
    for tag in ("t", "j"):
        tf = np.ascontiguousarray(G["mask_" + tag].T)[None]
        R = scf.cov_form(Xe, tf, fw)
        assert np.max(scf.e_elem(R[0], G["bm_cov_%s_raw" % tag])) <= F64
        c = scf.mask_count_form(tf, fw)
        assert np.array_equal(c[0], G["bm_cnt_" + tag])
        fin = scf.finalize_form(G["bm_cov_%s_raw" % tag][None], c, 0.0 if tag == "t" else 1e-6)
        assert np.max(scf.e_elem(fin[0], G["bm_cov_" + tag])) <= F64
    W = scf.bmvdr_form(G["bm_cov_t"], G["bm_cov_j"], ref_micx=1, offset=0.0)
    cond = max(np.linalg.cond(G["bm_cov_j"][k]) for k in range(K))
    assert np.max(scf.weight_errors(W, G["bm_wqH"])) <= 1e-15 * cond * 10
    # GEV: the noise matrices of the golden are trace normalised, and the weights agree up to the one global factor
    assert np.max(scf.e_elem(scf.trace_normalize_form(G["gev_cov_j"]), G["gev_cov_j"])) <= F64
    e = scf.measured_gap(G["gev_cov_t"], G["gev_cov_j"])
    Wg = scf.gev_form(G["gev_cov_t"], G["gev_cov_j"])
    err = scf.weight_errors(Wg, G["gev_wqH"], scf.global_factor(Wg, G["gev_wqH"]))
    condg = np.array([np.linalg.cond(G["gev_cov_j"][k]) for k in range(K)])
    print("golden GEV: worst error %.1e, smallest gap %.1e, worst cond %.1e" % (err.max(), e.min(), condg.max()))
    assert np.all(err <= 1e-15 * condg / e * 10)


# --------------------------------------------------------------------------------------------------- the yardstick
def test_yardstick_is_float32_and_exact_fixture_is_exact():
    inp = scf.cov_input(2, 3, 17, 33)
    tf, fw, R0 = scf.variant(inp, "both")
    Rcf, R32 = scf.cov_form(inp["X"], tf, fw, R0), scf.cov_form(inp["X"], tf, fw, R0, dtype=np.float32)
    assert Rcf.dtype == np.complex128 and R32.dtype == np.complex64
    y = np.max(scf.e_elem(R32, Rcf))
    assert 2.0 ** -26 < y < 2e-6, y                                          # a float32 sum of 33 terms, not more and not exact
    assert np.ptp(20 * np.log10(inp["gain"])) == pytest.approx(60.0)
    assert 0.2 < np.mean(inp["tf"] == 0) < 0.4 and inp["tf"].max() <= 1.0 and set(np.unique(inp["fw"])) == {0.0, 1.0}
    assert not np.any(inp["X"][:, 0].imag) and np.any(inp["X"][:, 1].imag)
    assert np.array_equal(inp["R0"], np.conj(np.swapaxes(inp["R0"], -1, -2))) and np.any(inp["R0"])
    ex = scf.exact_input(2, 3, 17, 257)
    for name in scf.WEIGHT_VARIANTS:
        tf, fw, _ = scf.variant(ex, name)
        a, b = scf.cov_form(ex["X"], tf, fw), scf.cov_form(ex["X"], tf, fw, dtype=np.float32)
        assert np.array_equal(a, b.astype(np.complex128))
        assert np.array_equal(b, np.conj(np.swapaxes(b, -1, -2))) and not np.any(np.diagonal(b, axis1=-2, axis2=-1).imag)
        assert np.max(np.abs(a.real)) < 2 ** 24 and np.max(np.abs(a.imag)) < 2 ** 24
    assert set(np.unique(ex["tf"])) == {0.0, 1.0, 2.0} and np.max(np.abs(ex["X"].real)) <= 64
    # counters: floor() matters on both sides of 1
    tf = np.array([[[0.0, 0.4, 0.999, 1.0, 1.5, 2.0, 2.7, -0.5]]], np.float32)
    assert scf.mask_count_form(tf)[0, 0] == 0 + 0 + 0 + 1 + 1 + 2 + 2 + 0
    assert scf.mask_count_form(tf, np.array([[1, 1, 1, 0, 1, 1, 0, 1]], np.float32), count0=np.array([[3.0]]))[0, 0] == 3 + 1 + 2


# --------------------------------------------------------------------------------------------------- the mutants
def test_new_rule_rejects_every_mutant_and_old_rule_does_not(mutant_fixture):
    inp, Rcf, R32 = mutant_fixture
    tf, fw, R0 = scf.variant(inp, "both")
    ok, fig = scf.accept_matrix(Rcf.astype(np.complex64), R32, Rcf)
    assert ok, fig                                                          # the closed form itself, rounded, passes
    old_accepts, rejected = [], []
    for m in scf.COV_MUTANTS:
        Rm = scf.cov_form(inp["X"], tf, fw, R0, mutant=m).astype(np.complex64)
        ok, fig = scf.accept_matrix(Rm, R32, Rcf)
        if not ok:
            rejected.append(m)
        if scf.old_rule(Rm, Rcf):
            old_accepts.append(m)
        print("%-30s element-wise %.2e (yardstick %.2e) -> %s; old per-bin Frobenius rule -> %s"
              % (m, fig["e"], fig["y"], "accepted" if ok else "rejected", "accepted" if m in old_accepts else "rejected"))
    Rt, Rn = scf.design_input(17, bin0_real=False)
    Wcf = scf.bmvdr_form(Rt, Rn, 3, 0.1)
    assert scf.accept_weights(Wcf.astype(np.complex64), Wcf)[0]
    for m in scf.BMVDR_MUTANTS:
        ok, e = scf.accept_weights(scf.bmvdr_form(Rt, Rn, 3, 0.1, mutant=m).astype(np.complex64), Wcf)
        print("%-30s weight error %.2e -> %s" % (m, e, "accepted" if ok else "rejected"))
        if not ok:
            rejected.append(m)
    Gcf = scf.gev_form(Rt, Rn)
    assert scf.accept_weights(scf.gev_form(Rt, Rn, "cholesky", bin0="largest_real").astype(np.complex64), Gcf, up_to_factor=True)[0]
    for m in scf.GEV_MUTANTS:
        ok, e = scf.accept_weights(scf.gev_form(Rt, Rn, mutant=m).astype(np.complex64), Gcf, up_to_factor=True)
        print("%-30s weight error %.2e -> %s" % (m, e, "accepted" if ok else "rejected"))
        if not ok:
            rejected.append(m)
    print("mutants the old per-bin Frobenius %.0e rule accepts: %s" % (scf.OLD_FROBENIUS, ", ".join(old_accepts) or "none"))
    assert sorted(rejected) == sorted(scf.MUTANTS)
    assert "weak_channel_row_off" in old_accepts                            # the gap being closed


def test_zero_closed_form_must_be_exactly_zero():
    Rcf = np.zeros((2, 3, 3), np.complex128)
    Rcf[1] = np.eye(3)
    R = Rcf.astype(np.complex64)
    assert scf.accept_matrix(R, R, Rcf)[0]
    R[0, 1, 2] = 1e-30
    assert not scf.accept_matrix(R, Rcf.astype(np.complex64), Rcf)[0]
    R[0, 1, 2] = np.nan
    assert not scf.accept_matrix(R, Rcf.astype(np.complex64), Rcf)[0]


# --------------------------------------------------------------------------------------------------- the design fixtures
@pytest.mark.parametrize("N,gap,bin0_real", scf.design_cases())
def test_design_fixture_conditions(N, gap, bin0_real):
    Rt, Rn = scf.design_input(N, gap=gap, bin0_real=bin0_real)
    assert not np.any(Rt[0].imag) == bin0_real or N == 1
    assert np.array_equal(Rn, np.conj(np.swapaxes(Rn, -1, -2))) and np.array_equal(Rt, np.conj(np.swapaxes(Rt, -1, -2)))
    cond = max(np.linalg.cond(Rn[k].astype(np.complex128)) for k in range(Rn.shape[0]))
    assert cond <= scf.MAX_COND, cond
    if N > 1:
        g = scf.measured_gap(Rt, Rn)
        assert np.all(g <= 2 * gap) and np.all(g >= gap / 2), g
    a, b = scf.gev_form(Rt, Rn, "scipy"), scf.gev_form(Rt, Rn, "cholesky")
    spread = scf.weight_errors(b, a, scf.global_factor(b, a))
    print("N %d gap %.0e: cond %.1f, spread of the two float64 routes %.1e" % (N, gap, cond, spread.max()))
    assert np.all(spread <= scf.MAX_SPREAD), spread
    Z = scf.bmvdr_form(Rt, Rn, N // 2, 0.1)
    assert np.all(np.isfinite(Z.view(np.float64)))


def test_known_answer_and_degenerate_fixtures():
    for N in (4, 17, 66):
        for jstar in (0, N - 1):
            Rt, Rn = scf.known_answer_input(N, jstar)
            W = scf.gev_form(Rt, Rn, bin0="largest_real")
            want = np.zeros(N)
            want[jstar] = 1.0
            assert np.max(np.abs(np.abs(W) - want[None])) == 0.0
            top = np.sort(np.diagonal(Rt, axis1=-2, axis2=-1).real, axis=-1)[:, -2:]
            assert np.all(top[:, 1] == 1.0) and np.all(top[:, 0] == np.float32(1 - 2.0 ** -23))
    Rt, Rn = scf.design_input(17, degenerate=True, bin0_real=False)
    for k in range(Rt.shape[0]):
        e, _ = scf.gev_pairs(Rt[k], Rn[k])
        assert (e[-1] - e[-2]) / e[-1] <= 1e-6 and (e[-2] - e[-3]) / e[-1] >= 0.4
