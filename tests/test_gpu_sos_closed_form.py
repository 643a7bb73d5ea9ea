"""The batch second-order-statistics kernels (csrc/cov_kernels.hip, csrc/sos_kernels.hip) against the float64 closed forms of
tests/sos_closed_form.py, at the shapes where each kernel form takes another path.

Covariances are judged element by element, e_ij = |R - Rcf|_ij / sqrt(Rcf_ii Rcf_jj), against the float32 yardstick of the same
sums: max e <= max(FACTOR * max e(yardstick), FLOOR).  The designs compute in float64 and round to complex64, so their bound is
FLOOR (four float32 ulps) of the bin's largest weight; tests/test_sos_cpu.py checks what that relies on (cond(Rn), the
eigenvalue gaps, the 2^-26 spread of two float64 routes).  Every test prints the kernel's figure next to the yardstick's.

Measured on an MI355X (largest figure over the cases of a test; yardstick = numpy float32, frame by frame):
    covariance, largest e over every shape and weight variant          kernel      yardstick   worst kernel / yardstick of one case
      cov_small_kernel (N 1..16, 177 cases)                            1.73e-07    9.08e-07    1.00
      cov_mfma_kernel  (N 17..129, 105 cases)                          9.28e-07    6.14e-07    1.69
      cov_valu_kernel  (N 17..129, 105 cases)                          9.28e-07    6.14e-07    1.73
      cov_mfma_kernel forced at N 1, 5, 8, 16                          4.94e-07    3.96e-07    1.34
      cov_finalize (36 cases)                                          1.75e-07    2.41e-07    1.24
      cov_trace_normalize (12 cases)                                   5.91e-08    2.02e-07    1.00
    exact fixture: all four kernel forms bit equal; row-padded runs bit equal to the contiguous ones; counters and gate exact;
    non-finite snapshots behind weight 0: no non-finite value in R in any kernel form (before the tiled kernels selected zero
    ahead of the multiply, the MFMA and VALU forms returned NaN there and cov_small_kernel did not)
    designs, largest per-bin weight error, bound FLOOR = 2.38e-07
      blind MVDR, N 1..66, 3 reference channels x 3 offsets            5.76e-08
      GEV up to one factor, N 1..66, gaps 0.5 .. 1e-6                  5.35e-08    (5.35e-08 with the bin-0 convention and no factor)
      GEV |w^H Rn w - 1| and Rayleigh quotient                         9.6e-08     (bounds 4.8e-07 .. 5.1e-05)
      GEV next to a failed or an all-zero bin                          4.24e-08
    known answers e_0 and e_(N-1) exact at N 4, 17, 66; an all-zero target bin gives finite weights with w^H Rn w = 1 and
    failed == 0 (NaN weights before gev_vectors_kernel replaced a target without positive trace by I / N)
"""
import functools

import numpy as np
import pytest

from tests import sos_closed_form as scf
from tests.closed_forms import FLOOR

pytestmark = pytest.mark.gpu

S, K = 2, 3
SMALL_CASES = [(N, 67) for N in range(1, 17)] + [(N, T) for N in (4, 9, 13, 16) for T in (1, 63, 64, 65, 255, 256, 257)]
TILED_CASES = sorted(set([(N, 33) for N in (17, 31, 32, 33, 63, 64, 65, 127, 128, 129)]
                         + [(N, T) for N in (33, 65) for T in (1, 2, 31, 32, 33, 63, 64, 65, 97)]))
KERNEL_FORMS = {"small": True, "mfma": True, "valu": False, "mfma_forced": 2}        # name -> use_mfma


@functools.lru_cache(maxsize=None)
def _case(N, T):
    """The inputs of a shape and, per weight variant, (closed form, yardstick): computed once, never modified."""
    inp = scf.cov_input(S, K, N, T)
    forms = {}
    for name in scf.WEIGHT_VARIANTS:
        tf, fw, R0 = scf.variant(inp, name)
        forms[name] = (scf.cov_form(inp["X"], tf, fw, R0), scf.cov_form(inp["X"], tf, fw, R0, dtype=np.float32))
    return inp, forms


def _to(dev, a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _accumulate(dev, X, tf, fw, R0, use_mfma):
    from distant_speech_recognition_amd import engine as eng
    R = eng.cov_accumulate(_to(dev, X), R=_to(dev, R0), tf_weights=_to(dev, tf), frame_weights=_to(dev, fw), use_mfma=use_mfma)
    return R.cpu().numpy()


def _check_variants(dev, N, T, form):
    inp, forms = _case(N, T)
    for name in scf.WEIGHT_VARIANTS:
        tf, fw, R0 = scf.variant(inp, name)
        R = _accumulate(dev, inp["X"], tf, fw, R0, KERNEL_FORMS[form])
        Rcf, R32 = forms[name]
        ok, fig = scf.accept_matrix(R, R32, Rcf)
        print("cov %-11s N %3d T %3d %-4s: kernel %.2e, yardstick %.2e" % (form, N, T, name, fig["e"], fig["y"]))
        assert ok, (form, N, T, name, fig)


# --------------------------------------------------------------------------------------------------- covariance accumulation
@pytest.mark.parametrize("N,T", SMALL_CASES)
def test_cov_small_kernel(dev, N, T):
    """Every cov_small_kernel<N> instance, and one N per pair-group split at frame counts around the 64-lane and 4-wave strides."""
    _check_variants(dev, N, T, "small")


@pytest.mark.parametrize("form", ["mfma", "valu"])
@pytest.mark.parametrize("N,T", TILED_CASES)
def test_cov_tiled_kernels(dev, N, T, form):
    """The 32-row quadrants and 64-row tiles, the 32-frame LDS tile and its two-frame loads."""
    _check_variants(dev, N, T, form)


@pytest.mark.parametrize("N", [1, 5, 16])
def test_cov_mfma_forced_for_small_arrays(dev, N):
    _check_variants(dev, N, 67, "mfma_forced")


@pytest.mark.parametrize("N,form", [(8, "small"), (8, "mfma_forced"), (65, "mfma"), (65, "valu")])
def test_cov_row_padded_snapshots_bit_equal(dev, N, form):
    """Snapshots and weights as [..., :T] views of buffers with padded rows, the padding NaN: bit for bit the contiguous result."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    T, pad = 67, 5
    inp, forms = _case(N, T)
    tf, fw, R0 = scf.variant(inp, "both")
    want = _accumulate(dev, inp["X"], tf, fw, R0, KERNEL_FORMS[form])
    Xp = torch.full((S, K, N, T + pad), float("nan"), dtype=torch.complex64, device=dev)[..., :T]
    Xp.copy_(_to(dev, inp["X"]))
    tfp, fwp = eng.rows_like(Xp, (S, K, T), torch.float32), eng.rows_like(Xp, (S, T), torch.float32)
    assert Xp.stride(-2) == tfp.stride(-2) == fwp.stride(-2) == T + pad
    for view, src in ((tfp, tf), (fwp, fw)):
        view._base.fill_(float("nan"))
        view.copy_(_to(dev, src))
    got = eng.cov_accumulate(Xp, R=_to(dev, R0), tf_weights=tfp, frame_weights=fwp, use_mfma=KERNEL_FORMS[form]).cpu().numpy()
    assert np.array_equal(got.view(np.float32), want.view(np.float32))
    ok, fig = scf.accept_matrix(got, forms["both"][1], forms["both"][0])
    print("cov %-11s N %3d row padded: kernel %.2e, yardstick %.2e" % (form, N, fig["e"], fig["y"]))
    assert ok, fig


@pytest.mark.parametrize("N,form", [(13, "small"), (65, "mfma"), (65, "valu"), (5, "mfma_forced")])
def test_cov_exact_fixture_bit_equal(dev, N, form):
    """Integer snapshots and weights in {0, 1, 2}: every float32 sum is exact, so every kernel form equals the closed form bit
    for bit, with R exactly Hermitian and Im R_ii == 0."""
    ex = scf.exact_input(S, K, N, 257)
    for name in scf.WEIGHT_VARIANTS:
        tf, fw, _ = scf.variant(ex, name)
        Rcf = scf.cov_form(ex["X"], tf, fw)
        R = _accumulate(dev, ex["X"], tf, fw, None, KERNEL_FORMS[form])
        assert np.array_equal(R.astype(np.complex128), Rcf), (form, name, float(np.max(np.abs(R - Rcf))))
        assert np.array_equal(R, np.conj(np.swapaxes(R, -1, -2)))
        assert not np.any(np.diagonal(R, axis1=-2, axis2=-1).imag)
    print("cov %-11s N %3d exact fixture: bit equal" % (form, N))


@pytest.mark.parametrize("how", ["gate", "mask", "both"])
@pytest.mark.parametrize("N,form", [(5, "small"), (13, "small"), (33, "mfma"), (33, "valu"), (5, "mfma_forced")])
def test_cov_gated_off_frames_are_never_touched(dev, N, form, how):
    """NaN / Inf snapshots in frames of weight 0 (through the gate, a mask zero, or both): R equals the run with those frames
    zeroed, bit for bit, as in the reference, which never touches a gated-off frame (pybeamformer.py:1080, :1137-1147)."""
    inp, _ = _case(N, 67)
    Xp, Xz, tf, fw = scf.poison(inp["X"], inp["tf"], inp["fw"], how)
    tf, fw = (None if how == "gate" else tf), (None if how == "mask" else fw)
    got = _accumulate(dev, Xp, tf, fw, None, KERNEL_FORMS[form])
    want = _accumulate(dev, Xz, tf, fw, None, KERNEL_FORMS[form])
    bad = int(np.sum(~np.isfinite(got.view(np.float32))))
    print("cov %-11s N %3d non-finite snapshots behind %-4s: %d non-finite values in R" % (form, N, how, bad))
    assert bad == 0 and np.array_equal(got.view(np.float32), want.view(np.float32))
    ok, fig = scf.accept_matrix(got, scf.cov_form(Xp, tf, fw, dtype=np.float32), scf.cov_form(Xp, tf, fw))
    assert ok, fig


# --------------------------------------------------------------------------------------------------- counters, gate, finalize
@pytest.mark.parametrize("T", [1, 257])
def test_mask_count_and_frame_gate(dev, T):
    """floor() on both sides of 1, negative and zero masks, the strict threshold, and counters carried over two calls: all
    sums are small integers, so the kernels equal the forms exactly."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    rng = np.random.default_rng(T)
    tf1 = (rng.random((S, K, T)) * 3.0 - 0.5).astype(np.float32)
    tf1[..., ::5] = np.array([1.0, 0.0, 2.0, 0.999, 1.5], np.float32)[np.arange(len(tf1[0, 0, ::5])) % 5]
    tf2 = (rng.random((S, K, T)) * (rng.random((S, K, T)) > 0.3)).astype(np.float32)
    fw = (rng.random((S, T)) > 0.3).astype(np.float32)
    c = eng.cov_mask_count(_to(dev, tf1), _to(dev, fw))
    assert np.array_equal(c.cpu().numpy(), scf.mask_count_form(tf1, fw).astype(np.float32))
    c = eng.cov_mask_count(_to(dev, tf2), None, count=c)
    c = eng.cov_mask_count(_to(dev, 2 * tf1), _to(dev, fw), count=c)
    want = scf.mask_count_form(2 * tf1, fw, scf.mask_count_form(tf2, None, scf.mask_count_form(tf1, fw)))
    assert np.array_equal(c.cpu().numpy(), want.astype(np.float32)) and (T == 1 or want.min() > 0)
    thr = 10.0
    en = (rng.random((S, T)) * 20.0).astype(np.float32)
    en[:, ::3] = np.float32(thr)                                      # energy == threshold is gated off
    if T > 1:
        en[:, 1] = np.nextafter(np.float32(thr), np.float32(np.inf))
    label = (rng.random((S, T)) > 0.4).astype(np.float32)
    for lab in (None, label):
        w, cnt = eng.cov_frame_gate(_to(dev, en), _to(dev, lab), thr)
        w2, cnt2 = eng.cov_frame_gate(_to(dev, en[:, ::-1].copy()), _to(dev, None if lab is None else lab[:, ::-1].copy()), thr, count=cnt)
        wf, cf = scf.gate_form(en, thr, lab)
        assert np.array_equal(w.cpu().numpy(), wf.astype(np.float32)) and np.array_equal(w2.cpu().numpy(), wf[:, ::-1].astype(np.float32))
        assert np.array_equal(cnt2.cpu().numpy(), (2 * cf).astype(np.float32))
    print("mask count and frame gate T %3d: exact" % T)


@pytest.mark.parametrize("N", [1, 4, 65])
@pytest.mark.parametrize("T", [1, 257])
def test_finalize_and_trace_normalize(dev, N, T):
    """cov_finalize with gamma = 0 and > 0, per-stream and per-bin counts (the latter accumulated over two calls from masks
    above and below 1), and cov_trace_normalize with a complex trace, element-wise against the forms."""
    from distant_speech_recognition_amd import engine as eng
    inp, forms = _case(N, T)
    R = forms["both"][0].astype(np.complex64)                          # Hermitian with Im R_ii == 0, like an accumulated sum
    fw = inp["fw"]
    ones = np.ones((S, K), np.float32)
    c_bin = eng.cov_mask_count(_to(dev, inp["tf"] * np.float32(2.5)), _to(dev, fw), count=_to(dev, ones))
    c_bin = eng.cov_mask_count(_to(dev, inp["tf"]), None, count=c_bin)
    want_bin = scf.mask_count_form(inp["tf"], None, scf.mask_count_form(inp["tf"] * np.float32(2.5), fw, ones))
    assert np.array_equal(c_bin.cpu().numpy(), want_bin.astype(np.float32)) and want_bin.min() >= 1
    c_str = _to(dev, fw.sum(axis=1).astype(np.float32))
    assert fw.sum(axis=1).min() >= 1
    for gamma in (0.0, 1e-6, 1e-2):
        for tag, cd, ch in (("per bin", c_bin, want_bin), ("per stream", c_str, fw.sum(axis=1))):
            got = eng.cov_finalize(_to(dev, R), cd, gamma=gamma).cpu().numpy()
            ok, fig = scf.accept_matrix(got, scf.finalize_form(R, ch, gamma, dtype=np.float32), scf.finalize_form(R, ch, gamma))
            print("finalize N %3d T %3d gamma %.0e %-10s: kernel %.2e, yardstick %.2e" % (N, T, gamma, tag, fig["e"], fig["y"]))
            assert ok, fig
    Rc = R.copy()
    idx = np.arange(0, N, 2)
    Rc[..., idx, idx] += (0.05j * Rc[..., idx, idx].real).astype(np.complex64)          # Im tr R != 0: the trace is complex (:1328)
    for tag, A in (("hermitian", R), ("complex trace", Rc)):
        got = eng.cov_trace_normalize(_to(dev, A)).cpu().numpy()
        ok, fig = scf.accept_matrix(got, scf.trace_normalize_form(A, dtype=np.float32), scf.trace_normalize_form(A))
        print("trace normalize N %3d T %3d %-13s: kernel %.2e, yardstick %.2e" % (N, T, tag, fig["e"], fig["y"]))
        assert ok, fig


# --------------------------------------------------------------------------------------------------- blind MVDR
@functools.lru_cache(maxsize=None)
def _design(N, gap, bin0_real):
    return scf.design_input(N, gap=gap, bin0_real=bin0_real)


@pytest.mark.parametrize("bin0_real", [True, False])
@pytest.mark.parametrize("N", scf.DESIGN_N)
def test_bmvdr_weights(dev, N, bin0_real):
    """Float64 kernel, complex64 result: every bin within FLOOR of its largest weight, on both sides of the dispatch switches."""
    from distant_speech_recognition_amd import engine as eng
    Rt, Rn = _design(N, 0.5, bin0_real)
    Rtd, Rnd = _to(dev, Rt), _to(dev, Rn)
    worst = 0.0
    for ref_micx in sorted({0, N // 2, N - 1}):
        for offset in (0.0, 0.1, 1.0):
            W, failed = eng.bmvdr_weights(Rtd, Rnd, ref_micx=ref_micx, offset=offset)
            ok, e = scf.accept_weights(W.cpu().numpy(), scf.bmvdr_form(Rt, Rn, ref_micx, offset))
            worst = max(worst, e)
            assert failed == 0 and ok, (N, ref_micx, offset, e)
    print("bmvdr N %2d bin 0 %-7s: largest weight error %.2e (bound %.2e)" % (N, "real" if bin0_real else "complex", worst, FLOOR))
    # a noise bin that is not positive definite: counted, zero weights there, the other bins untouched
    Rbad = Rn.copy()
    Rbad[2] = -Rbad[2]
    W, failed = eng.bmvdr_weights(Rtd, _to(dev, Rbad), ref_micx=N // 2, offset=0.1)
    W = W.cpu().numpy()
    good = [0, 1, 3, 4]
    assert failed == 1 and not np.any(W[2])
    ok, e = scf.accept_weights(W[good], scf.bmvdr_form(Rt[good], Rn[good], N // 2, 0.1))
    assert ok, e


# --------------------------------------------------------------------------------------------------- GEV
def _norm_bound(N, Rn):
    """|w^H Rn w - 1| and the relative error of w^H Rt w for weights within FLOOR max|w| <= FLOOR sqrt(N) |w|_2 of exact ones:
    2 |dw| |Rn| |w| <= 2 sqrt(N) FLOOR cond(Rn) w^H Rn w, per bin."""
    return np.array([2.0 * np.sqrt(N) * FLOOR * np.linalg.cond(Rn[k].astype(np.complex128)) for k in range(Rn.shape[0])])


def _gev_groups(W, Rt, Rn, groups):
    """Largest per-bin error of each run of bins against the closed form of that run alone, up to the run's own factor."""
    worst = 0.0
    for g in groups:
        Wcf = scf.gev_form(Rt[g], Rn[g])
        ok, e = scf.accept_weights(W[g], Wcf, up_to_factor=True)
        worst = max(worst, e)
        assert ok, (g, e)
    return worst


@pytest.mark.parametrize("N,gap,bin0_real", scf.design_cases())
def test_gev_weights(dev, N, gap, bin0_real):
    """All bins against the closed form up to ONE factor, the bin-0 convention, the Rn norm and the Rayleigh quotient."""
    from distant_speech_recognition_amd import engine as eng
    Rt, Rn = _design(N, gap, bin0_real)
    W, failed = eng.gev_weights(_to(dev, Rt), _to(dev, Rn))
    W = W.cpu().numpy()
    assert failed == 0
    Wcf = scf.gev_form(Rt, Rn)
    ok, e = scf.accept_weights(W, Wcf, up_to_factor=True)
    # the kernel's own convention for bin 0 fixes the factor as well: the closed form that states it needs none
    e0 = float(np.max(scf.weight_errors(W, scf.gev_form(Rt, Rn, bin0="largest_real"))))
    j = int(np.argmax(np.abs(W[0])))
    bound = _norm_bound(N, Rn)
    lam = np.array([scf.gev_pairs(Rt[k], Rn[k])[0][-1] for k in range(Rt.shape[0])])
    en, er = np.abs(scf.rn_norm(W, Rn) - 1.0), np.abs(scf.rayleigh(W, Rt) - lam) / lam
    print("gev N %2d gap %.0e bin 0 %-7s: weight error %.2e up to one factor, %.2e with the bin-0 convention (bound %.2e); "
          "|w^H Rn w - 1| %.1e, Rayleigh %.1e (bound %.1e)" % (N, gap, "real" if bin0_real else "complex", e, e0, FLOOR, en.max(), er.max(), bound.max()))
    assert ok, e
    assert e0 <= FLOOR
    assert W[0, j].real > 0 and abs(W[0, j].imag) <= FLOOR * W[0, j].real
    assert np.all(en <= bound) and np.all(er <= bound)


@pytest.mark.parametrize("N", [4, 17, 66])
def test_gev_known_answer_and_degenerate(dev, N):
    from distant_speech_recognition_amd import engine as eng
    for jstar in (0, N - 1):
        Rt, Rn = scf.known_answer_input(N, jstar)
        W, failed = eng.gev_weights(_to(dev, Rt), _to(dev, Rn))
        want = np.zeros((Rt.shape[0], N), np.complex64)
        want[:, jstar] = 1.0
        assert failed == 0 and np.array_equal(W.cpu().numpy(), want), (N, jstar)
    # two equal top eigenvalues (split only by the complex64 rounding of Rt): any vector of their plane is principal
    Rt, Rn = scf.design_input(N, degenerate=True, bin0_real=False)
    W, failed = eng.gev_weights(_to(dev, Rt), _to(dev, Rn))
    W = W.cpu().numpy()
    ev = [scf.gev_pairs(Rt[k], Rn[k])[0] for k in range(Rt.shape[0])]
    lam = np.array([e[-1] for e in ev])
    split = np.array([(e[-1] - e[-2]) / e[-1] for e in ev])
    bound = _norm_bound(N, Rn)
    en, er = np.abs(scf.rn_norm(W, Rn) - 1.0), np.abs(scf.rayleigh(W, Rt) - lam) / lam
    print("gev N %2d known answers exact; degenerate: |w^H Rn w - 1| %.1e, Rayleigh %.1e (split %.1e, bound %.1e)" % (N, en.max(), er.max(), split.max(), bound.max()))
    assert failed == 0 and np.all(en <= bound) and np.all(er <= split + bound)


@pytest.mark.parametrize("N", [4, 17, 66])
def test_gev_failed_bin_and_zero_target(dev, N):
    """A noise bin that is not positive definite: zeros there, failed == 1, and the runs of bins before and after it match the
    closed form up to their own factor.  A target bin that is all zero: finite weights with w^H Rn w = 1 and not counted as
    failed, like scipy.linalg.eigh, which returns an Rn-normalised vector there."""
    from distant_speech_recognition_amd import engine as eng
    Rt, Rn = _design(N, 0.5, False)
    Rbad = Rn.copy()
    Rbad[2] = -Rbad[2]
    W, failed = eng.gev_weights(_to(dev, Rt), _to(dev, Rbad))
    W = W.cpu().numpy()
    assert failed == 1 and not np.any(W[2])
    e1 = _gev_groups(W, Rt, Rn, ([0, 1], [3, 4]))
    bound = _norm_bound(N, Rn)
    for zero in ([2], [0], [0, 1, 2, 3, 4]):
        Rz = Rt.copy()
        Rz[zero] = 0
        W, failed = eng.gev_weights(_to(dev, Rz), _to(dev, Rn))
        W = W.cpu().numpy()
        finite = bool(np.all(np.isfinite(W.view(np.float32))))
        print("gev N %2d target zero in bins %s: finite %s, failed %d" % (N, zero, finite, failed))
        assert finite and failed == 0
        assert np.all(np.abs(scf.rn_norm(W, Rn) - 1.0) <= bound)
        live = [k for k in range(5) if k not in zero]
        # every vector is principal in a zero bin, so the chain restarts behind it: runs of live bins, each up to its own factor
        runs = [r for r in ([k for k in live if k < zero[0]], [k for k in live if k > zero[-1]]) if r]
        e1 = max(e1, _gev_groups(W, Rz, Rn, runs)) if runs else e1
    print("gev N %2d failed / zero bins: largest weight error of the other bins %.2e (bound %.2e)" % (N, e1, FLOOR))
