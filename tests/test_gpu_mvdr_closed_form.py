"""GPU: the fixed MVDR design (csrc/mvdr_kernels.hip) and its three Cholesky solvers against the float64 closed forms of
tests/mvdr_closed_form.py under closed_forms.accept (FACTOR 4 x the error of a plain float32 evaluation of the same inputs, never
less than FLOOR = 2^-22); tests/test_mvdr_cpu.py proves the conditions that let those forms serve as truth.

The library reads its switches once per process, so every solver form runs in a child process of its own (mvdr_closed_form.ENV):

    lds      the LDS-resident kernel for every N <= 137        reg      the register-resident solver (chol_reg.h) for every N <= 271
    panel    the blocked solver (chol_blocked.h) for every N   default  the shipped dispatch

The parent builds inputs and closed forms on the CPU; one child per form runs every case of the form and writes an .npz; the parent
judges.  A child that does not end with status 0 is the last one started in the session.

Per form: the weights and Lambda of three matrix kinds (dense complex Wishart, the product's loaded diffuse model, scaled identity) at
the sizes where the form can go wrong (mvdr_closed_form.SIZES; the panel solver up to the largest size its LDS panel allows, derived
from cholb::lds_bytes), bin 0 all ones in the weights and solved in Lambda, the distortionless known answer; slices (first_bin > 0) and
stacked streams bit-equal to the plain call; a pivot failure planted at a chosen column (first, inside a panel, on a panel / tile-row
boundary, last) and a NaN diagonal entry, through btk_mvdr_weights_flags directly so that no pseudo-inverse re-solve hides the raw
result; the refusals (first size above the panel cap, missing scratch) leaving every output as it was.  The element-wise kernels
(diffuse model, diagonal loading, divide_nondiagonal) run in the parent.

Measured on one MI355X (largest over the cases of a form and kind; ratio = the worst single case's accept ratio, bound 4):

    error = max |Y - Y_cf| / max |Y_cf| of a case     kernel     float32    worst ratio of one case
    weights  lds      wishart                       1.39e-06   1.38e-06   1.24 (N = 100)
             lds      diffuse                       3.36e-05   3.36e-05   1.45 (N = 2)
             lds      identity                      2.12e-07   2.23e-07   1.36 (N = 137)
             reg      wishart                       3.95e-06   3.34e-06   1.72 (N = 127)
             reg      wishart, every N 137 .. 271   5.02e-06   3.60e-06   2.33 (N = 268)
             reg      diffuse                       5.30e-05   4.99e-05   1.48 (N = 32)
             reg      identity                      2.01e-07   2.46e-07   1.54 (N = 31)
             panel    wishart                       9.00e-06   6.26e-06   1.44 (N = 1052)
             panel    diffuse                       1.22e-04   5.27e-04   1.14 (N = 64)
             panel    identity                      2.70e-07   2.76e-07   1.49 (N = 33)
             default  wishart                       3.92e-06   2.90e-06   1.39 (N = 271)
             default  diffuse                       5.30e-05   5.39e-05   1.24 (N = 64)
             default  identity                      1.94e-07   2.23e-07   1.38 (N = 137)
    Lambda   lds      wishart                       2.28e-07   2.60e-07   2.06 (N = 137)
             lds      diffuse                       8.45e-06   8.45e-06   1.00 (N = 2)
             lds      identity                      1.36e-07   2.07e-07   1.00 (N = 2)
             reg      wishart                       7.42e-07   3.93e-07   3.02 (N = 137)
             reg      diffuse                       1.38e-05   8.45e-06   2.84 (N = 256)
             reg      identity                      1.09e-07   2.07e-07   1.77 (N = 270)
             panel    wishart                       6.11e-07   6.72e-07   1.51 (N = 15)
             panel    diffuse                       4.74e-06   2.57e-05   1.78 (N = 33)
             panel    identity                      1.24e-07   2.07e-07   2.02 (N = 33)
             default  wishart                       7.42e-07   5.73e-07   3.02 (N = 137)
             default  diffuse                       8.39e-06   1.69e-05   1.26 (N = 271)
             default  identity                      7.82e-08   2.07e-07   0.54 (N = 272)

Every form passes with the plain right-looking yardstick alone: no kernel fix was needed and the second, blocked
float32 order (tests/test_mvdr_cpu.py: 0.22 to 1.17 times the plain one's error) was not called upon.  The diffuse model is bit-equal to
float32(closed form) at every shape tested, divide_nondiagonal within 0.504 x 2^-23.  A deliberate mutation -- the low eight mantissa
bits of one operand of the trailing update cleared in each of the three solvers -- raises the ratios to 14 .. 185 and fails 15 of these
tests (errors up to 5.3e-5 on the register-resident solver, 1.1e-3 on the blocked one and only on diffuse matrices it had never been
given), while every pre-existing MVDR test of test_gpu_postfilter_cov_mvdr.py still passes for those two solvers; the LDS kernel's
mutation also fails the pre-existing oracle run of that kernel at N = 64.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mvdr_closed_form as mcf
from tests.closed_forms import FACTOR, FLOOR, accept, cfratio_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ("lds", "reg", "panel", "default")

CHILD = r'''
import sys
import numpy as np, torch
sys.path.insert(0, %r)
from distant_speech_recognition_amd import engine as eng, _lib
from tests import mvdr_closed_form as m
form, path = sys.argv[1], sys.argv[2]
dev = torch.device("cuda:0")
L = _lib.lib()
out = {}
dv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
host = lambda t: t.cpu().numpy()

for kind, N, K in m.case_list(form):
    R, d = m.case_inputs(kind, N, K)
    Rt, dt = dv(R), dv(d)
    W, nid = eng.mvdr_weights(Rt, dt, svd_rule="exact")
    st = eng.CoherencePostFilterState(1, K, N, dev)
    nl = st.set_lambda(Rt, dt, 1.0e-8, svd_rule="exact")
    key = "%%s_%%d_%%d" %% (kind, N, K)
    out["W_" + key], out["L_" + key] = host(W), host(st.lam)
    out["n_" + key] = np.array([nid, nl, L.btk_mvdr_scratch_bytes(K, N)], np.int64)

if form in m.MODE_N:
    N = m.MODE_N[form]
    R, d = m.mode_inputs(N)
    S, K = d.shape[:2]
    Rt, dt = dv(R), dv(d)
    Ws, ns = eng.mvdr_weights(Rt, dt, svd_rule="exact")
    out["mode_stacked"], out["mode_n"] = host(Ws), np.array([ns])
    for s in range(S):
        out["mode_plain%%d" %% s] = host(eng.mvdr_weights(Rt[s].contiguous(), dt[s].contiguous(), svd_rule="exact")[0])
    out["mode_slice2"] = host(eng.mvdr_weights(Rt[0, 2:].contiguous(), dt[0, 2:].contiguous(), first_bin=2, svd_rule="exact")[0])
    out["mode_slice3_all"] = host(eng.mvdr_weights(Rt[0].contiguous(), dt[0].contiguous(), first_bin=3, svd_rule="exact")[0])
    swap = [1, 0, 2, 3, 4]
    out["mode_swapped"] = host(eng.mvdr_weights(Rt[0][swap].contiguous(), dt[0][swap].contiguous(), svd_rule="exact")[0])


def raw(Rt, dt, first_bin, scratch=True, fill=7.0, count0=0):
    """btk_mvdr_weights_flags itself: (code, W, flags, counter) with W / flags / counter pre-filled"""
    K, N = dt.shape
    W = torch.full((K, N), fill + 1j * fill, dtype=torch.complex64, device=dev)
    fl = torch.full((K,), -3, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), count0, dtype=torch.int32, device=dev)
    sb = L.btk_mvdr_scratch_bytes(K, N)
    buf = torch.empty((max(sb, 16),), dtype=torch.uint8, device=dev)
    code = L.btk_mvdr_weights_flags(Rt.data_ptr(), dt.data_ptr(), W.data_ptr(), K, N, first_bin, 1.0e-8, buf.data_ptr() if scratch else None,
                                    cnt.data_ptr(), fl.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return code, host(W), host(fl), int(cnt.item()), sb

for N in m.FAIL_N.get(form, ()):
    R, clean, d, flags = m.fail_inputs(N)
    for tag, mat in (("planted", R), ("clean", clean)):
        code, W, fl, cnt, sb = raw(dv(mat), dv(d), 1)
        out["fail_%%s_%%d_W" %% (tag, N)], out["fail_%%s_%%d_flags" %% (tag, N)] = W, fl
        out["fail_%%s_%%d_n" %% (tag, N)] = np.array([code, cnt])

def refusal(tag, N, K, scratch):
    Rt = torch.eye(N, dtype=torch.complex64, device=dev).repeat(K, 1, 1).contiguous()
    code, W, fl, cnt, sb = raw(Rt, dv(m.unit_d(K, N, 1)), 0, scratch=scratch, count0=5)
    out["refuse_" + tag] = np.array([code, int(np.all(W == 7.0 + 7.0j)), int(np.all(fl == -3)), cnt, sb, N], np.int64)

if form == "panel":
    refusal("above_cap", m.panel_max() + 1, 1, True)
    refusal("no_scratch", 40, 2, False)
if form == "default":
    refusal("no_scratch", 272, 1, False)
    out["scratch_271"] = np.array([L.btk_mvdr_scratch_bytes(4, 271)], np.int64)
np.savez(path, **out)
'''


@pytest.fixture(scope="module")
def forms(dev, tmp_path_factory):
    """forms(name) -> the .npz of that form's child, started once; after a child that did not end with status 0 no further child starts."""
    state = {"stop": None, "res": {}}
    tmp = tmp_path_factory.mktemp("mvdr_forms")

    def get(form):
        if form in state["res"]:
            return state["res"][form]
        if state["stop"] is not None:
            pytest.fail("no child for form %r: %s" % (form, state["stop"]))
        env = dict(os.environ)
        for name in ("BTK_MVDR_REG_MIN", "BTK_WPE_SOLVE_PANEL", "BTK_WPE_SOLVE_REG", "BTK_MVDR_SVD_RULE"):
            env.pop(name, None)
        env.update(mcf.ENV[form])
        path = str(tmp / (form + ".npz"))
        try:
            r = subprocess.run([sys.executable, "-c", CHILD % ROOT, form, path], env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
        except subprocess.TimeoutExpired:
            state["stop"] = "the child of form %r ran into its 300 s limit" % form
            pytest.fail(state["stop"])
        if r.returncode != 0:
            state["stop"] = "the child of form %r ended with status %d" % (form, r.returncode)
            pytest.fail(state["stop"] + "\n" + r.stderr[-2000:])
        state["res"][form] = dict(np.load(path))
        return state["res"][form]

    return get


def _yardstick(kind, N, K, what):
    """(closed form, plain float32 yardstick) of the weights' solved rows ("W") or of Lambda ("L", one column per bin)"""
    w, lam, w32, l32 = mcf.case_forms(kind, N, K)
    return (w[1:], w32[1:]) if what == "W" else (lam[:, None], l32[:, None])


def _judge_cases(form, cases, res, what):
    """accept() over the cases; prints every figure, returns the failures"""
    bad, worst = [], None
    for kind, N, K in cases:
        key = "%s_%d_%d" % (kind, N, K)
        cf, y32 = _yardstick(kind, N, K, what)
        got = res["W_" + key][1:] if what == "W" else res["L_" + key][:, None]
        ok, fig = accept(got, y32, cf)
        label = "mvdr %s %-7s %-8s N %4d K %d" % (what, form, kind, N, K)
        print(cfratio_line(label, fig))
        if not ok:
            bad.append((label, fig))
        if worst is None or fig["ratio"] > worst[1]["ratio"]:
            worst = (label, fig)
    if worst is not None:
        print(cfratio_line("WORST " + worst[0], worst[1]))
    return bad


@pytest.mark.parametrize("kind", mcf.KINDS)
@pytest.mark.parametrize("form", FORMS)
def test_weights_against_the_closed_form(forms, form, kind):
    res = forms(form)
    cases = [c for c in mcf.case_list(form) if c[0] == kind and not (form == "reg" and c[2] == 2)]        # (those: test_register_solver_every_size)
    assert cases
    for knd, N, K in cases:
        key = "%s_%d_%d" % (knd, N, K)
        W = res["W_" + key]
        assert W.dtype == np.complex64 and np.all(W[0] == 1.0), key                   # bin 0: exactly all ones
        assert res["n_" + key][0] == 0, key                                          # nident
    bad = _judge_cases(form, cases, res, "W")
    assert not bad, bad
    # the distortionless known answer w^H d = 1 / N: the kernel's miss against the yardstick's own, same FACTOR; never asked to be
    # better than FLOOR of the answer
    for knd, N, K in cases:
        key = "%s_%d_%d" % (knd, N, K)
        _, d = mcf.case_inputs(knd, N, K)
        _, w32 = _yardstick(knd, N, K, "W")
        miss, miss32 = mcf.distortionless_miss(res["W_" + key][1:], d[1:]).max(), mcf.distortionless_miss(w32, d[1:]).max()
        print("MVDRDL %-7s %-8s N %4d  |w^H d - 1/N| N = %.3e (f32 %.3e)" % (form, knd, N, miss * N, miss32 * N))
        assert miss <= max(FACTOR * miss32, FLOOR / N), (key, miss, miss32)


@pytest.mark.parametrize("kind", mcf.KINDS)
@pytest.mark.parametrize("form", FORMS)
def test_lambda_against_the_closed_form(forms, form, kind):
    """set_lambda(svd_rule="exact") for all bins: bin 0 is solved like every other"""
    res = forms(form)
    cases = [c for c in mcf.case_list(form) if c[0] == kind and not (form == "reg" and c[2] == 2)]
    for knd, N, K in cases:
        key = "%s_%d_%d" % (knd, N, K)
        assert res["L_" + key].shape == (K,) and res["n_" + key][1] == 0, key
    bad = _judge_cases(form, cases, res, "L")
    assert not bad, bad


def test_register_solver_every_size(forms):
    """every N the shipped dispatch gives the register-resident solver beyond the LDS kernel's reach (137 .. 271: every padding count of the
    last tile row), one system each"""
    res = forms("reg")
    cases = [c for c in mcf.case_list("reg") if c[2] == 2]
    assert [c[1] for c in cases] == list(mcf.EVERY_SIZE)
    for knd, N, K in cases:
        key = "%s_%d_%d" % (knd, N, K)
        assert np.all(res["W_" + key][0] == 1.0) and res["n_" + key][0] == 0 and res["n_" + key][2] == 0, key
    bad = _judge_cases("reg", cases, res, "W")
    assert not bad, bad


@pytest.mark.parametrize("form", ["lds", "reg", "panel"])
def test_slices_and_stacked_streams_are_the_same_arithmetic(forms, form):
    res = forms(form)
    N = mcf.MODE_N[form]
    plain = [res["mode_plain%d" % s] for s in range(3)]
    assert res["mode_n"][0] == 0
    for s in range(3):
        assert np.all(plain[s][0] == 1.0) and np.all(np.isfinite(plain[s].view(np.float32)))
        assert np.array_equal(res["mode_stacked"][s].view(np.uint32), plain[s].view(np.uint32)), (N, s)     # every stream's bin 0 all ones
    assert np.array_equal(res["mode_slice2"].view(np.uint32), plain[0][2:].view(np.uint32))
    # a slice that starts above bin 0 solves its local row 0: bit for bit what a plain call gives that matrix in row 1
    sl = res["mode_slice3_all"]
    assert np.array_equal(sl[1:].view(np.uint32), plain[0][1:].view(np.uint32))
    assert np.array_equal(sl[0].view(np.uint32), res["mode_swapped"][1].view(np.uint32)) and not np.all(sl[0] == 1.0)
    R, d = mcf.mode_inputs(N)
    w, _ = mcf.design_cf(R[0], d[0])
    assert np.max(np.abs(sl - w)) <= 1e-3 * np.max(np.abs(w))                   # (and it is the solution, coarsely: accept judges the sizes above)


@pytest.mark.parametrize("form", ["lds", "reg", "panel"])
def test_pivot_failure_at_a_chosen_column(forms, form):
    """fails_at(N, j) for j on the first column, inside a panel, on a panel / tile-row boundary, at the last pivot, and a NaN diagonal
    entry, each between two solvable bins: flags exactly as planted, the counter their sum, the flagged bins the identity answer, the
    neighbours bit for bit what a launch without the planted bins gives"""
    res = forms(form)
    for N in mcf.FAIL_N[form]:
        R, clean, d, flags = mcf.fail_inputs(N)
        code, cnt = res["fail_planted_%d_n" % N]
        W, fl = res["fail_planted_%d_W" % N], res["fail_planted_%d_flags" % N]
        Wc, flc = res["fail_clean_%d_W" % N], res["fail_clean_%d_flags" % N]
        assert code == 0 and res["fail_clean_%d_n" % N][0] == 0
        assert np.array_equal(fl, flags), (N, fl)
        assert cnt == flags.sum()
        assert not np.any(flc) and res["fail_clean_%d_n" % N][1] == 0
        assert np.all(np.isfinite(W.view(np.float32))), N                           # the NaN stays in its own bin's matrix
        ident = mcf.identity_answer(d)
        for k in np.nonzero(flags)[0]:
            assert np.max(np.abs(W[k] - ident[k])) <= FLOOR * np.max(np.abs(ident[k])), (N, k)
        good = flags == 0
        assert np.array_equal(W[good].view(np.uint32), Wc[good].view(np.uint32)), N
        w, _ = mcf.design_cf(clean, d)
        assert np.max(np.abs(Wc - w)) <= 1e-3 * np.max(np.abs(w))                   # the neighbours are solved (first_bin = 1: no all-ones row)


def test_panel_solver_refuses_the_first_size_above_its_cap_and_a_missing_scratch(forms):
    from distant_speech_recognition_amd import _lib
    res = forms("panel")
    code, w_kept, f_kept, cnt, sb, N = res["refuse_above_cap"]
    assert N == mcf.panel_max() + 1 == 1053 and mcf.panel_lds_bytes(N) > mcf.LDS_CAP >= mcf.panel_lds_bytes(N - 1)
    assert code == _lib.BTK_ERR_DIMENSION and w_kept and f_kept and cnt == 5
    code, w_kept, f_kept, cnt, sb, N = res["refuse_no_scratch"]
    assert sb == 8 * 2 * N * N > 0
    assert code == _lib.BTK_ERR_PARAMETER and w_kept and f_kept and cnt == 5


def test_shipped_dispatch_runs_the_form_it_claims(forms):
    """N = 63 on the LDS kernel, 64 / 137 / 271 on the register-resident solver, 272 on the blocked one: bit for bit the forced form's result,
    scratch asked for from 272 on, and a missing scratch refused there"""
    from distant_speech_recognition_amd import _lib
    res = forms("default")
    for N, form in mcf.DEFAULT_RUNS.items():
        other = forms(form)
        for kind in mcf.KINDS:
            key = "%s_%d_%d" % (kind, N, mcf.K_CASE)
            for what in ("W_", "L_"):
                assert np.array_equal(res[what + key].view(np.uint32), other[what + key].view(np.uint32)), (N, form, kind, what)
            assert (res["n_" + key][2] > 0) == (form == "panel"), key
    assert res["scratch_271"][0] == 0
    code, w_kept, f_kept, cnt, sb, N = res["refuse_no_scratch"]
    assert N == 272 and sb == 8 * N * N
    assert code == _lib.BTK_ERR_PARAMETER and w_kept and f_kept and cnt == 5


# --------------------------------------------------------------------------- the element-wise kernels (no switch: in this process)
def _geometry(N, seed):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-400.0, 400.0, (N, 3)).astype(np.float32)                        # mm
    if N >= 3:
        p[2] = p[0]                                                                  # two coincident microphones
    return p


@pytest.mark.parametrize("c", [mcf.SSPEED, 340000.0])
@pytest.mark.parametrize("M", [8, 64])
@pytest.mark.parametrize("N", [1, 3, 17, 64])
def test_diffuse_model_within_one_ulp(dev, N, M, c):
    """the kernel rounds a double once: every element within one float32 ulp of float32(closed form) (one ulp: ties between sinpi and
    numpy's sine), the diagonal and coincident microphones exactly 1, the imaginary part exactly 0"""
    from distant_speech_recognition_amd import engine as eng
    p = _geometry(N, 10 * N + M)
    G = eng.mvdr_diffuse_model(p, M, 16000.0, sspeed=c, device=dev).cpu().numpy()
    ref = mcf.diffuse_cf(p, M, 16000.0, c).astype(np.float32)
    assert G.shape == (M // 2 + 1, N, N) and G.dtype == np.complex64
    assert not np.any(G.imag)
    assert np.all(G.real[:, np.arange(N), np.arange(N)] == 1.0) and np.all(G.real[0] == 1.0)
    if N >= 3:
        assert np.all(G.real[:, 0, 2] == 1.0) and np.all(G.real[:, 2, 0] == 1.0)
    ulps = np.abs(G.real.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)
    print("MVDRELEM diffuse N %d M %d c %.0f: %.2f ulp, %d of %d elements differ" % (N, M, c, ulps.max(), np.count_nonzero(ulps), ulps.size))
    assert np.all(np.abs(G.real.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64))
    if N >= 17:
        assert np.min(ref) < -0.1 and np.count_nonzero(np.abs(ref) < 0.05) > N       # the geometry reaches well past the first zero of the sinc


def test_diagonal_loading_is_one_float32_addition(dev):
    """N = 65: the 64-thread stride wraps.  Diagonal real parts bit-equal to float32(R_ii) + float32(w), everything else untouched"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    N, K, w = 65, 3, 0.01
    rng = np.random.default_rng(65)
    R = (rng.normal(size=(K, N, N)) + 1j * rng.normal(size=(K, N, N))).astype(np.complex64)
    out = eng.mvdr_diagonal_loading(torch.from_numpy(R.copy()).to(dev), w).cpu().numpy()
    want = R.copy()
    want.real[:, np.arange(N), np.arange(N)] = R.real[:, np.arange(N), np.arange(N)] + np.float32(w)
    assert np.array_equal(out.view(np.uint32), want.view(np.uint32))
    assert np.max(np.abs(want - mcf.load_cf(R, w))) <= 2.0 ** -24 * (np.max(np.abs(R.real)) + w)       # ... which is the float64 form, rounded once


def test_divide_nondiagonal_within_two_roundings(dev):
    """N = 17: the 256-thread loop covers N N > 256.  Off-diagonal parts within 2^-23 relative of R / (1 + mu) (the float32 reciprocal,
    then the product), the diagonal untouched bit for bit"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    N, K, mu = 17, 2, 0.01
    rng = np.random.default_rng(17)
    R = (rng.normal(size=(K, N, N)) + 1j * rng.normal(size=(K, N, N))).astype(np.complex64)
    out = eng.mvdr_divide_nondiagonal(torch.from_numpy(R.copy()).to(dev), mu).cpu().numpy()
    ref = mcf.divide_nondiag_cf(R, mu)
    dg = np.eye(N, dtype=bool)
    assert out[:, dg].tobytes() == R[:, dg].tobytes()
    for part in ("real", "imag"):
        got, want = getattr(out, part).astype(np.float64)[:, ~dg], getattr(ref, part)[:, ~dg]
        print("MVDRELEM divide %s: %.3f x 2^-23" % (part, np.max(np.abs(got - want) / np.abs(want)) * 2.0 ** 23))
        assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want))
        assert np.any(got != getattr(R, part)[:, ~dg])
