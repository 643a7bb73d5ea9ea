"""GPU: subband acoustic echo cancellation (csrc/aec_kernels.hip, engine.aec_process) against the float64 closed form of
tests/aec_closed_form.py on the same complex64 inputs.

Tolerances are the project's stated ones for recurrences (as in tests/test_gpu_rls.py): E within 1e-4 max|E_ref|,
R within 1e-4 relative, K within 1e-3 relative, sigma2_v and the DTD scalars within 1e-5 relative, and the set of skipped
(frame, bin) updates identical.  The inputs are conditioned: the closed form's smallest gate margin is >= 1e-8 and float64 and
longdouble take identical decisions (asserted here for the case at hand, and for every case by tests/test_aec_cpu.py)."""
import numpy as np
import pytest

from tests import aec_closed_form as cf

pytestmark = pytest.mark.gpu

TOL_E, TOL_R, TOL_K, TOL_S = 1e-4, 1e-4, 1e-3, 1e-5


def _rel(a, b):
    d = np.max(np.abs(b))
    return float(np.max(np.abs(a - b)) / d) if d > 0 else float(np.max(np.abs(a)))


def _state(eng, dev, case, S=None):
    name, kind, S0, M, P, T, ts, fn0, kw = case
    return eng.AECState(kind, S0 if S is None else S, M, P, device=dev, **kw)


def _padded(torch, dev, x, ts):
    """complex64 [S][K][T] host array -> [..., :T] view of a device buffer with row stride ts"""
    S, K, T = x.shape
    buf = torch.zeros((S, K, ts), dtype=torch.complex64, device=dev)
    buf[..., :T] = torch.from_numpy(x).to(dev)
    return buf[..., :T]


def _run_gpu(eng, torch, dev, case, V, A, splits=None, S=None):
    name, kind, S0, M, P, T, ts, fn0, kw = case
    st = _state(eng, dev, case, S=V.shape[0])
    Vd, Ad = _padded(torch, dev, V, ts), _padded(torch, dev, A, ts)
    E = torch.zeros((V.shape[0], V.shape[1], ts), dtype=torch.complex64, device=dev)[..., :T]
    fl = torch.zeros((V.shape[0], V.shape[1], ts), dtype=torch.uint8, device=dev)[..., :T]
    t0 = 0
    for n in (splits or [T]):
        f0 = fn0 if (fn0 is None or fn0 < 0) else fn0 + t0
        eng.aec_process(Vd[..., t0:t0 + n], Ad[..., t0:t0 + n], st, out=E[..., t0:t0 + n], frame_no0=f0, adapted=fl[..., t0:t0 + n])
        t0 += n
    torch.cuda.synchronize()
    return E.cpu().numpy(), fl.cpu().numpy(), st


def _state_arrays(st):
    return dict(R=st.R.cpu().numpy(), K=st.K.cpu().numpy(), sig=st.sigma2_v.cpu().numpy(), hist=st.history.cpu().numpy(),
                dtd=st.dtd.cpu().numpy())


@pytest.mark.parametrize("case", cf.CASES, ids=[c[0] for c in cf.CASES])
def test_aec_matches_closed_form(dev, case):
    import torch
    from distant_speech_recognition_amd import engine as eng
    name, kind, S, M, P, T, ts, fn0, kw = case
    V, A = cf.case_inputs(case)
    ref = cf.case_reference(case)
    E, fl, st = _run_gpu(eng, torch, dev, case, V, A)
    g = _state_arrays(st)
    if kind == 3 and M == 32:
        # both state placements of the double-talk kernel are covered: K in LDS up to P = 24 at M = 32, in the exported state above
        assert st.dtd_state_in_lds() == (P <= 24)
    for s in range(S):
        Er, flr, mg, sr = ref[s]
        assert mg.smallest() >= 1e-8, (name, s, mg.smallest())
        errs = dict(E=float(np.max(np.abs(E[s] - Er)) / np.max(np.abs(Er))), R=_rel(g["R"][s], sr["R"]),
                    K=_rel(g["K"][s], sr["K"]) if kind else 0.0, sig=_rel(g["sig"][s], sr["sig"]) if kind else 0.0,
                    hist=_rel(g["hist"][s], sr["hist"]) if kind >= 2 else 0.0,
                    dtd=float(np.max(np.abs(g["dtd"][s][:3] - sr["dtd"]) / np.maximum(np.abs(sr["dtd"]), 1e-300))) if kind == 3 else 0.0)
        print("aec %s stream %d: margin %.3g, skipped %d of %d, errors %s" % (name, s, mg.smallest(), flr.size - int(flr.sum()), flr.size,
                                                                               {k: "%.2g" % v for k, v in errs.items()}))
        assert np.array_equal(fl[s], flr), (name, s, int(np.sum(fl[s] != flr)))
        assert errs["E"] <= TOL_E and errs["R"] <= TOL_R and errs["K"] <= TOL_K and errs["sig"] <= TOL_S and errs["dtd"] <= TOL_S, errs
        assert errs["hist"] == 0.0
        assert g["dtd"][s][3] == T


@pytest.mark.parametrize("name", ["kalman", "bk_p5", "bk_p36", "dtd_p5", "dtd_p25", "dtd_p5_neg"])
def test_aec_continuation_is_bit_identical(dev, name):
    """one block, or the same frames as 64 + the rest: E and every piece of state bit for bit"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    case = [c for c in cf.CASES if c[0] == name][0]
    V, A = cf.case_inputs(case)
    T = case[5]
    E1, f1, s1 = _run_gpu(eng, torch, dev, case, V, A)
    E2, f2, s2 = _run_gpu(eng, torch, dev, case, V, A, splits=[64, T - 64])
    assert np.array_equal(E1.view(np.float32), E2.view(np.float32)) and np.array_equal(f1, f2)
    a, b = _state_arrays(s1), _state_arrays(s2)
    for k in a:
        assert np.array_equal(a[k].view(np.float64), b[k].view(np.float64)), k
    # three uneven pieces, one shorter than the filter
    E3, f3, s3 = _run_gpu(eng, torch, dev, case, V, A, splits=[3, 70, T - 73])
    assert np.array_equal(E1.view(np.float32), E3.view(np.float32))
    c = _state_arrays(s3)
    for k in a:
        assert np.array_equal(a[k].view(np.float64), c[k].view(np.float64)), k


@pytest.mark.parametrize("name", ["kalman", "bk_p2", "dtd_p2", "dtd_p5_neg"])
def test_aec_streams_are_independent(dev, name):
    """stream 1 of the S = 3 run equals its own S = 1 run bit for bit (kind 3: no shared-scalar leakage between streams)"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    case = [c for c in cf.CASES if c[0] == name][0]
    assert case[2] == 3
    V, A = cf.case_inputs(case)
    E3, f3, s3 = _run_gpu(eng, torch, dev, case, V, A)
    E1, f1, s1 = _run_gpu(eng, torch, dev, case, V[1:2], A[1:2])
    assert np.array_equal(E3[1].view(np.float32), E1[0].view(np.float32)) and np.array_equal(f3[1], f1[0])
    a, b = _state_arrays(s3), _state_arrays(s1)
    for k in a:
        assert np.array_equal(a[k][1].view(np.float64), b[k][0].view(np.float64)), k


def test_aec_reset_semantics(dev):
    """reset(): kinds 0 and 1 zero the filter only (kind 1 keeps sigma2_v and K); kinds 2 and 3 keep everything (aec.h:41,78,111-114)"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    for name in ("nlms", "kalman", "bk_p5", "dtd_p5"):
        case = [c for c in cf.CASES if c[0] == name][0]
        V, A = cf.case_inputs(case)
        _, _, st = _run_gpu(eng, torch, dev, case, V, A)
        before = _state_arrays(st)
        st.reset()
        after = _state_arrays(st)
        if case[1] < 2:
            assert np.all(after["R"] == 0) and np.any(before["R"] != 0)
        else:
            assert np.array_equal(after["R"], before["R"])
        for k in ("K", "sig", "hist", "dtd"):
            assert np.array_equal(after[k], before[k]), (name, k)


def test_aec_limits_are_clean_errors(dev):
    import torch
    from distant_speech_recognition_amd import engine as eng, _lib
    with pytest.raises(_lib.BtkError, match="sample_num P=65 exceeds this kernel"):
        eng.AECState(2, 1, 64, 65, device=dev)
    with pytest.raises(_lib.BtkError, match="M=4096 exceeds this kernel"):
        eng.AECState(3, 1, 4096, 4, device=dev)
    with pytest.raises(_lib.BtkError, match="one-tap"):
        eng.AECState(0, 1, 64, 2, device=dev)
    st = eng.AECState(2, 1, 64, 64, device=dev)                     # the largest filter the kernel takes
    V = torch.zeros((1, 33, 8), dtype=torch.complex64, device=dev)
    E = eng.aec_process(V, V, st)
    assert E.shape == (1, 33, 8) and float(E.abs().max()) == 0.0
    with pytest.raises(_lib.BtkError):
        eng.aec_process(V[:, :32], V[:, :32], st)
    # the C-ABI itself refuses what the front end refuses
    import ctypes
    p = np.zeros(8)
    rc = _lib.lib().btk_aec_process(2, p.ctypes.data_as(ctypes.c_void_p), st.R.data_ptr(), st.R.data_ptr(), st.R.data_ptr(), None, 1, 64, 65,
                                    8, 8, 0, st.R.data_ptr(), st.K.data_ptr(), st.sigma2_v.data_ptr(), st.history.data_ptr(),
                                    st.dtd.data_ptr(), None)
    assert rc == _lib.BTK_ERR_DIMENSION and b"sample_num" in _lib.lib().btk_last_error()
