"""GPU: every launch form of the two adaptive sidelobe cancellers (csrc/nlms_kernels.hip, csrc/rls_kernels.hip) on gated
input against the float64 closed forms of tests/canceller_closed_form.py, frame by frame.

The norm is per frame, max_k |Y[t] - ref[t]| <= tol max_k |ref[t]| with the project's stated figures: 1e-4 for
the RLS recursion, 2e-4 for NLMS; a frame whose input is exactly zero must come out exactly zero.  The fixtures, and the
proof that they reach the hold path, the energy floor, both roots of the quadratic constraint and the norm reset with room
to spare, are in tests/canceller_closed_form.py and tests/test_canceller_cpu.py.  Every form is reached by its shape alone.

Measured on one MI355X (each test prints its own): largest per-frame error 5.9e-8 for RLS in every form and both modes (the
complex64 rounding of the output), 3.6e-6 for NLMS on even and on odd blocks; |P - P^H| <= 1.2e-14 |P| (register kernel, 0 in the
Hermitian forms), |P n| <= 4.2e-16 |P|.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import canceller_closed_form as cf

pytestmark = pytest.mark.gpu

RLS_TOL, NLMS_TOL = 1e-4, 2e-4


@functools.lru_cache(maxsize=None)
def _blocking(orc, N, Nc, M):
    _, vs = cf.manifold(N, M)
    return np.stack([orc.blocking_matrix(vs[k], Nc) for k in range(M // 2 + 1)])


@functools.lru_cache(maxsize=None)
def _rls_reference(orc, name):
    """the closed form of every stream of an RLS fixture, computed once"""
    N, Nc, M, S, _, kw, _ = cf.rls_case(name)
    _, vs, Xe = cf.rls_input(name)
    B = _blocking(orc, N, Nc, M)
    return vs, Xe, B, [cf.rls_py_form(cf.full_frames(Xe[s], M), vs, B, kw) for s in range(S)]


@functools.lru_cache(maxsize=None)
def _nlms_reference(orc, N, Nc):
    """... and of an NLMS fixture: both block splits compare with the same run"""
    M, S, kw = cf.nlms_case(N, Nc)
    _, vs, Xe = cf.nlms_input(N, Nc)
    B = _blocking(orc, N, Nc, M)
    return vs, Xe, B, [cf.nlms_form(cf.full_frames(Xe[s], M), vs, B, kw) for s in range(S)]


def _blocks(fn, Xd, lengths):
    import torch
    out, a = [], 0
    for n in lengths:
        out.append(fn(Xd[..., a:a + n].contiguous()))
        a += n
    assert a == Xd.shape[-1]
    return torch.cat(out, dim=-1).cpu().numpy()


def _check_frames(tag, Y, ref, Xe_s, tol):
    """Y, ref [T][K]; Xe_s [K][N][T]"""
    worst, _ = cf.per_frame_error(Y, ref)
    zero_in = ~np.any(Xe_s != 0, axis=(0, 1))
    print("%s: largest per-frame error %.3g (bound %.0e), %d all-zero frames" % (tag, worst, tol, int(zero_in.sum())))
    assert np.all(Y[zero_in] == 0), "a frame of zeros must come out as zeros"
    peak = np.max(np.abs(ref), axis=1)
    err = np.max(np.abs(Y - ref), axis=1)
    assert np.all(err <= tol * peak), (worst, int(np.argmax(err - tol * peak)))
    return worst


def _check_rls_state(tag, eng, st, s, ref, B):
    """exported state of stream s against the closed form's, in the reference's basis as tests/test_gpu_rls.py does, the
    stream scalars, and the invariants of P"""
    Pd, wd = st.P[s].cpu().numpy(), st.w[s].cpu().numpy()
    K = Pd.shape[0]
    wa_scale = max(np.max(np.abs(ref["w"])), 1e-30)
    for k in range(K):
        Pz, waH = eng.rls_state_to_reference(1, Pd[k], wd[k], B[k])
        Pz_ref, waH_ref = eng.rls_state_to_reference(1, ref["P"][k], ref["w"][k], B[k])
        assert np.max(np.abs(waH - waH_ref)) <= 1e-4 * wa_scale
        assert np.max(np.abs(Pz - Pz_ref)) <= 1e-3 * np.max(np.abs(Pz_ref))
    ss = st.stream_state[s].cpu().numpy()
    assert ss[2] == ref["isamp"] and ss[3] == ref["ttl_updates"]
    assert abs(ss[0] - ref["E_avg"]) <= 1e-5 * ref["E_avg"]
    _check_P_invariants(tag, st, s)


def _check_P_invariants(tag, st, s):
    Pd = st.P[s].cpu().numpy()
    v = (st.v[s] if st.per_stream else st.v).cpu().numpy()
    v = v / np.linalg.norm(v, axis=1, keepdims=True)
    dirs = [np.conj(v) if st.mode == 0 else v]               # mode 0 blocks conj(wq); state.cx holds the directions as blocked
    if st.cx is not None:
        cx = st.cx.cpu().numpy()
        dirs += [cx[:, j] for j in range(cx.shape[1])]
    herm = leak = 0.0
    for k in range(Pd.shape[0]):
        scale = np.max(np.abs(Pd[k]))
        herm = max(herm, np.max(np.abs(Pd[k] - Pd[k].conj().T)) / scale)
        for d in dirs:
            leak = max(leak, np.max(np.abs(Pd[k] @ d[k])) / scale)
    print("%s: |P - P^H| / |P| = %.3g, |P n| / |P| = %.3g" % (tag, herm, leak))
    assert herm <= 1e-12
    # rounding of about 2^-53 N, grown by at most mu^-16 within a tile before the next re-projection: 1e-13 at N = 256
    assert leak <= 1e-10


# ------------------------------------------------------------------------------------------------ RLS, mode 1, gated
@pytest.mark.parametrize("name", cf.RLS_NAMES)
def test_rls_gated_against_closed_form(orc, dev, name):
    import torch
    from distant_speech_recognition_amd import engine as eng
    N, Nc, M, S, profile, kw, _ = cf.rls_case(name)
    vs, Xe, B, refs = _rls_reference(orc, name)
    T = Xe.shape[-1]
    T1 = 53 if profile == "long" else 21                                   # not a multiple of 16: the tile phase changes
    st = eng.RLSState(1, S, M, N, torch.from_numpy(vs).to(dev), Nc=Nc, **kw)
    Y = _blocks(lambda x: eng.rls_process(x, st), torch.from_numpy(Xe).to(dev), (T1, T - T1))
    for s in range(S):
        tag = "rls %s stream %d" % (name, s)
        _check_frames(tag, Y[s].T, refs[s]["Y"], Xe[s], RLS_TOL)
        _check_rls_state(tag, eng, st, s, refs[s], B)


def test_rls_control_scan_first_lane(orc, dev):
    """frames whose gate differs between the average carried into a 64-frame scan chunk and the chunk's own first value"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    N, M = cf.LANE0_N, cf.LANE0_M
    _, vs, Xe = cf.lane0_input()
    B = _blocking(orc, N, 1, M)
    ref = cf.rls_py_form(cf.full_frames(Xe[0], M), vs, B, cf.LANE0_RLS)
    assert not ref["adapt"][list(cf.LANE0_QUIET)].any() and ref["hits"]["hold"] == len(cf.LANE0_QUIET)
    for lengths in (cf.LANE0_SPLIT, (cf.LANE0_T,)):
        st = eng.RLSState(1, 1, M, N, torch.from_numpy(vs).to(dev), **cf.LANE0_RLS)
        Y = _blocks(lambda x: eng.rls_process(x, st), torch.from_numpy(Xe).to(dev), lengths)
        _check_frames("rls first lane %s" % (lengths,), Y[0].T, ref["Y"], Xe[0], RLS_TOL)
        _check_rls_state("rls first lane", eng, st, 0, ref, B)


# ------------------------------------------------------------------------------------------------ NLMS, gated
def _nlms_run(dev, vs, Xe, N, Nc, M, kw, lengths):
    import torch
    from distant_speech_recognition_amd import engine as eng
    st = eng.NLMSState(Xe.shape[0], M, N, dev, Nc=Nc, **kw)
    st.set_constraints(vs)
    vd = torch.from_numpy(vs.astype(np.complex64)).to(dev)
    return _blocks(lambda x: eng.nlms_process(vd, x, st), torch.from_numpy(Xe).to(dev), lengths), st


def _check_nlms_state(eng, st, s, ref, B):
    u = st.u[s].cpu().numpy().astype(np.complex128)
    wa_ref = np.stack([eng.nlms_u_to_wa(ref["u"][k], B[k]) for k in range(u.shape[0])])
    wa = np.stack([eng.nlms_u_to_wa(u[k], B[k]) for k in range(u.shape[0])])
    assert np.max(np.abs(wa - wa_ref)) <= 2e-4 * np.max(np.abs(wa_ref))
    assert np.max(np.abs(st.sigma2[s].cpu().numpy() - ref["sigma2"]) / ref["sigma2"]) <= 1e-4
    ss = st.stream_state[s].cpu().numpy()
    assert ss[2] == ref["isamp"] and ss[3] == ref["ttl_updates"] and ss[1] == ref["gamma"]
    assert abs(ss[0] - ref["E_avg"]) <= 1e-5 * ref["E_avg"]


@pytest.mark.parametrize("split", ["even", "odd"])
@pytest.mark.parametrize("N,Nc", cf.NLMS_CASES)
def test_nlms_gated_against_closed_form(orc, dev, N, Nc, split):
    """even block lengths take the nlms_bin2 forms, odd ones the nlms_bin_kernel fallbacks; neither split is a multiple of
    64, so the control kernel's aligned chunks start part-way into the second block"""
    from distant_speech_recognition_amd import engine as eng, _lib
    M, S, kw = cf.nlms_case(N, Nc)
    vs, Xe, B, refs = _nlms_reference(orc, N, Nc)
    if Nc > 1 and split == "odd":
        # the documented limit of btk_nlms_process_nc: Nc > 1 has no scalar form, and must not return frames
        with pytest.raises(_lib.BtkError):
            _nlms_run(dev, vs, Xe, N, Nc, M, kw, cf.NLMS_SPLITS[split])
        return
    Y, st = _nlms_run(dev, vs, Xe, N, Nc, M, kw, cf.NLMS_SPLITS[split])
    for s in range(S):
        _check_frames("nlms N=%d Nc=%d %s stream %d" % (N, Nc, split, s), Y[s].T, refs[s]["Y"], Xe[s], NLMS_TOL)
        _check_nlms_state(eng, st, s, refs[s], B)


def test_nlms_control_scan_first_lane(orc, dev):
    from distant_speech_recognition_amd import engine as eng
    N, M = cf.LANE0_N, cf.LANE0_M
    _, vs, Xe = cf.lane0_input()
    B = _blocking(orc, N, 1, M)
    ref = cf.nlms_form(cf.full_frames(Xe[0], M), vs, B, cf.LANE0_NLMS)
    assert not ref["adapt"][list(cf.LANE0_QUIET)].any() and ref["hits"]["hold"] == len(cf.LANE0_QUIET)
    for lengths in (cf.LANE0_SPLIT, (cf.LANE0_T,)):
        Y, st = _nlms_run(dev, vs, Xe, N, 1, M, cf.LANE0_NLMS, lengths)
        _check_frames("nlms first lane %s" % (lengths,), Y[0].T, ref["Y"], Xe[0], NLMS_TOL)
        _check_nlms_state(eng, st, 0, ref, B)


# ------------------------------------------------------------------------------------------------ a block of holds only
HOLD_LOUD, HOLD_ZERO, HOLD_SLOWDOWN = 25, 20, 30         # a halving (frame 30) falls inside the zero frames 25..44


@pytest.mark.parametrize("N,M", [(8, 16), (40, 16), (100, 8)])
def test_nlms_block_of_zero_frames_changes_nothing(dev, N, M):
    import torch
    from distant_speech_recognition_amd import engine as eng
    _, vs = cf.manifold(N, M)
    kw = dict(cf.NLMS_COMMON, slowdown_after=HOLD_SLOWDOWN)
    Xe = cf.gated_frames(np.random.default_rng(N), 2, 150, N, M, "long_ones")[..., :HOLD_LOUD]
    st = eng.NLMSState(2, M, N, dev, **kw)
    vd = torch.from_numpy(vs.astype(np.complex64)).to(dev)
    eng.nlms_process(vd, torch.from_numpy(np.ascontiguousarray(Xe)).to(dev), st)
    u0, sig0, ss0 = st.u.clone(), st.sigma2.clone(), st.stream_state.cpu().numpy().copy()
    assert u0.abs().max() > 0 and np.all(ss0[:, 3] > 0)
    Y = eng.nlms_process(vd, torch.zeros((2, M // 2 + 1, N, HOLD_ZERO), dtype=torch.complex64, device=dev), st)
    ss = st.stream_state.cpu().numpy()
    assert torch.equal(st.u.view(torch.float32), u0.view(torch.float32)) and torch.equal(st.sigma2, sig0)
    assert torch.count_nonzero(torch.view_as_real(Y)) == 0
    assert np.array_equal(ss[:, 3], ss0[:, 3]) and np.array_equal(ss[:, 2], ss0[:, 2] + HOLD_ZERO)
    assert np.array_equal(ss[:, 1], ss0[:, 1] / 2)
    beta = float(np.float32(0.97))                           # btk_nlms_process_nc takes its parameters as float32
    assert np.all(np.abs(ss[:, 0] - ss0[:, 0] * beta ** HOLD_ZERO) <= 1e-12 * ss0[:, 0])


@pytest.mark.parametrize("N,Nc,M", [(8, 1, 16), (40, 2, 8), (100, 1, 8), (129, 1, 8)])
def test_rls_block_of_zero_frames_changes_nothing(dev, N, Nc, M):
    import torch
    from distant_speech_recognition_amd import engine as eng
    _, vs = cf.manifold(N, M)
    kw = dict(cf.RLS_COMMON, constraint_option=0)
    Xe = cf.gated_frames(np.random.default_rng(N), 2, 150, N, M, "long_ones")[..., :HOLD_LOUD]
    st = eng.RLSState(1, 2, M, N, torch.from_numpy(vs).to(dev), Nc=Nc, **kw)
    eng.rls_process(torch.from_numpy(np.ascontiguousarray(Xe)).to(dev), st)
    P0, w0, ss0 = st.P.cpu().numpy().copy(), st.w.clone(), st.stream_state.cpu().numpy().copy()
    assert w0.abs().max() > 0 and np.all(ss0[:, 3] > 0)
    Y = eng.rls_process(torch.zeros((2, M // 2 + 1, N, HOLD_ZERO), dtype=torch.complex64, device=dev), st)
    ss = st.stream_state.cpu().numpy()
    assert torch.equal(st.w.view(torch.float64), w0.view(torch.float64))
    assert torch.count_nonzero(torch.view_as_real(Y)) == 0
    assert np.array_equal(ss[:, 3], ss0[:, 3]) and np.array_equal(ss[:, 2], ss0[:, 2] + HOLD_ZERO)
    assert np.all(np.abs(ss[:, 0] - ss0[:, 0] * 0.97 ** HOLD_ZERO) <= 1e-12 * ss0[:, 0])
    # a tile without an adapting frame skips the re-projection too: P keeps its bits
    assert np.array_equal(st.P.cpu().numpy(), P0)


# ------------------------------------------------------------------------------------------------ RLS, mode 0
def _cc_oracle(orc, M, N, delays, opts, Nc):
    o = orc.RLSCc(M, N, delays, cf.SAMPLERATE, mu=opts["mu"], sigma2=opts["sigma2"], Nc=Nc)
    o.init_precision_matrix(0.01)
    if "qc" in opts:
        o.set_quadratic_constraint(*opts["qc"])
    return o


def _cc_state(eng, dev, o, S, M, N, Nc, opts, v=None):
    import torch
    K = M // 2 + 1
    kw = dict(mu=o.mu, diagonal_weight=o.diag_w)
    if "qc" in opts:
        kw.update(alpha=float(np.float32(opts["qc"][0])), qctype=opts["qc"][1])
    v = np.ascontiguousarray(o.wq[:K]) if v is None else v
    st = eng.RLSState(0, S, M, N, torch.from_numpy(v).to(dev), Nc=Nc, **kw)
    st.init_precision_matrix(float(np.float32(1) / np.float32(0.01)))
    return st


def _unit_frames(seed, S, T, N, M):
    """unit-scale snapshots as in tests/test_gpu_rls.py: int16-scale data cancels ten digits of the reference's own Pz_0 = 100 I"""
    return np.ascontiguousarray(cf.gated_frames(np.random.default_rng(seed), S, 150, N, M, "long_ones", scale=0.5)[..., :T])


# diagonal_weight: the reference's update wa <- (I - sigma2 Pz) wa + ... multiplies wa by 1 - sigma2 Pz_0 mu^-t along every direction
# the snapshots have not visited, and N - 1 of these exceed the frames of a test: 1e-4 keeps that factor inside the unit
# circle over 40 frames (1e-4 * 100 * 0.9^-40 = 0.7), 0.01 as in tests/test_gpu_rls.py at N = 8 would not (68)
def test_rls_cc_packed_128_threads_against_oracle(orc, dev):
    """mode 0 on the packed kernel at 128 threads, two blocked directions, diagonal weight on"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    N, Nc, M, T = 40, 2, 8, 30
    K = M // 2 + 1
    opts = dict(mu=0.9, sigma2=1e-4)
    delays = cf.manifold(N, M, 0.6)[0]
    Xe = _unit_frames(N * 77 + M, 2, T, N, M)
    st = _cc_state(eng, dev, _cc_oracle(orc, M, N, delays, opts, Nc), 2, M, N, Nc, opts)
    Y = _blocks(lambda x: eng.rls_process(x, st), torch.from_numpy(Xe).to(dev), (T // 3 + 1, T - T // 3 - 1))
    for s in range(2):
        o = _cc_oracle(orc, M, N, delays, opts, Nc)
        ref = o.run(cf.full_frames(Xe[s], M))[:, :K]
        tag = "rls mode 0 N=%d Nc=%d stream %d" % (N, Nc, s)
        _check_frames(tag, Y[s].T, ref, Xe[s], RLS_TOL)
        _check_cc_state(eng, st, s, o, K)
        _check_P_invariants(tag, st, s)


def _check_cc_state(eng, st, s, o, K):
    Pd, wd = st.P[s].cpu().numpy(), st.w[s].cpu().numpy()
    for k in range(1, K):
        Pz, wa = eng.rls_state_to_reference(0, Pd[k], wd[k], o.B[k])
        assert np.max(np.abs(wa - o.wa[k])) <= 1e-4 * np.max(np.abs(o.wa[:K]))
        assert np.max(np.abs(Pz - o.Pz[k])) <= 1e-3 * np.max(np.abs(o.Pz[k]))


def test_rls_cc_threshold_limitation_on_8_frame_tiles(orc, dev):
    """mode 0, N = 128 (8-frame tiles), qc = (0.05, THRESHOLD_LIMITATION): wa is rescaled to |wa| = alpha whenever |wa|^2 >= alpha.
    Weights learnt from this input stay near |wq|^2 = 1 / N and never get there, so the recursion starts from weights carried
    in: |wa|^2 = 0.2 in half of the bins (above the threshold: rescaled on the first frame) and 0.001 in the others (below it for
    the whole run).  After one frame the former sit at alpha and the latter below it, and both go on as the oracle's do."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    N, M, T = 128, 8, 30
    K = M // 2 + 1
    opts = dict(mu=0.9, sigma2=0.0, qc=(0.05, 2))
    alpha = float(np.float32(0.05))
    delays = cf.manifold(N, M, 0.6)[0]
    Xe = _unit_frames(N * 77 + M, 2, T, N, M)
    os_ = [_cc_oracle(orc, M, N, delays, opts, 1) for _ in range(2)]
    st = _cc_state(eng, dev, os_[0], 2, M, N, 1, opts)
    rng = np.random.default_rng(128)
    w0 = np.zeros((2, K, N), np.complex128)
    high = np.zeros((2, K), bool)
    for s in range(2):
        for k in range(1, K):
            high[s, k] = (k + s) % 2 == 0
            wa0 = rng.normal(size=N - 1) + 1j * rng.normal(size=N - 1)
            wa0 *= np.sqrt((0.2 if high[s, k] else 0.001) / np.sum(np.abs(wa0) ** 2))
            os_[s].wa[k] = wa0
            os_[s].wl[k] = w0[s, k] = os_[s].B[k] @ wa0                  # wl = B wa
    st.w.copy_(torch.from_numpy(w0))
    Xd = torch.from_numpy(Xe).to(dev)
    Y1 = eng.rls_process(Xd[..., :1].contiguous(), st)
    wd = st.w.cpu().numpy()
    for s in range(2):
        n2 = np.array([np.sum(np.abs(eng.rls_state_to_reference(0, np.eye(N), wd[s, k], os_[s].B[k])[1]) ** 2) for k in range(1, K)])
        print("mode 0 stream %d |wa|^2 after one frame %s, alpha^2 = %.6g" % (s, n2, alpha * alpha))
        assert np.all(np.abs(n2[high[s, 1:]] - alpha * alpha) <= 1e-12) and high[s, 1:].any()
        low = n2[~high[s, 1:]]
        assert np.all(low < alpha) and np.all(np.abs(low - alpha * alpha) > 1e-3 * alpha * alpha) and len(low)
    Y = torch.cat([Y1, eng.rls_process(Xd[..., 1:].contiguous(), st)], dim=-1).cpu().numpy()
    for s in range(2):
        ref = os_[s].run(cf.full_frames(Xe[s], M))[:, :K]
        tag = "rls mode 0 N=128 threshold limitation stream %d" % s
        _check_frames(tag, Y[s].T, ref, Xe[s], RLS_TOL)
        _check_cc_state(eng, st, s, os_[s], K)
        _check_P_invariants(tag, st, s)
        assert np.all(np.sum(np.abs(os_[s].wa[1:K]) ** 2, axis=1) < alpha)       # no bin is above the threshold at the end


def test_rls_cc_update_off_keeps_the_state(orc, dev):
    """update = False on the packed kernel: the output is the fixed GSC of the weights carried in, and P and w are not touched"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    N, M, T = 100, 8, 40
    K = M // 2 + 1
    opts = dict(mu=0.9, sigma2=0.0)
    delays = cf.manifold(N, M, 0.6)[0]
    Xe = _unit_frames(100, 1, T, N, M)
    o = _cc_oracle(orc, M, N, delays, opts, 1)
    st = _cc_state(eng, dev, o, 1, M, N, 1, opts)
    Xd = torch.from_numpy(Xe).to(dev)
    eng.rls_process(Xd[..., :19].contiguous(), st)
    P0, w0 = st.P.clone(), st.w.clone()
    assert w0[0, 1:].abs().max() > 0
    st.p["update"] = False
    Y = eng.rls_process(Xd[..., 19:].contiguous(), st).cpu().numpy()[0]
    assert torch.equal(st.P.view(torch.float64), P0.view(torch.float64)) and torch.equal(st.w.view(torch.float64), w0.view(torch.float64))
    x = Xe[0][..., 19:].astype(np.complex128)
    wl = w0.cpu().numpy()[0]
    wl[0] = 0                                                           # beamformer.cc:1540-1558: bin 0 has no sidelobe canceller
    ref = np.einsum("kn,knt->kt", np.conj(o.wq[:K]), x) - np.einsum("kn,knt->kt", np.conj(wl), x)
    _check_frames("rls mode 0 update off", Y.T, ref.T, Xe[0][..., 19:], 2e-6)


@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("N,M,T", [(8, 16, 60), (100, 8, 40)])
def test_rls_per_stream_quiescent_vectors(orc, dev, mode, N, M, T):
    """v given as [S][K][N] from two look directions: each stream must agree with its own oracle run"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    K = M // 2 + 1
    angles = (-1.306379, 0.6)
    opts = dict(mu=0.9, sigma2=0.01 if N == 8 else 1e-4)     # (see test_rls_cc_packed_128_threads_against_oracle)
    kw = dict(cf.RLS_COMMON, constraint_option=2, max_wa_l2norm=1e-3)
    Xe = _unit_frames(N + mode, 2, T, N, M) if mode == 0 else \
        np.ascontiguousarray(cf.gated_frames(np.random.default_rng(N), 2, 150, N, M, "long_ones")[..., :T])
    dl = [cf.manifold(N, M, a)[0] for a in angles]
    if mode == 0:
        os_ = [_cc_oracle(orc, M, N, d, opts, 1) for d in dl]
        st = _cc_state(eng, dev, os_[0], 2, M, N, 1, opts, v=np.stack([np.ascontiguousarray(o.wq[:K]) for o in os_]))
    else:
        os_ = [orc.RLSPy(M, N, 1, **kw) for _ in dl]
        for o, d in zip(os_, dl):
            o.calc_beamformer_weights(cf.SAMPLERATE, d)
        st = eng.RLSState(1, 2, M, N, torch.from_numpy(np.stack([cf.manifold(N, M, a)[1] for a in angles])).to(dev), **kw)
    assert st.per_stream == 1
    Y = _blocks(lambda x: eng.rls_process(x, st), torch.from_numpy(Xe).to(dev), (T // 2 + 3, T - T // 2 - 3))
    for s in range(2):
        ref = os_[s].run(cf.full_frames(Xe[s], M))[:, :K]
        _check_frames("rls mode %d per-stream v N=%d stream %d" % (mode, N, s), Y[s].T, ref, Xe[s], RLS_TOL)
        _check_P_invariants("rls mode %d per-stream v N=%d stream %d" % (mode, N, s), st, s)


# ------------------------------------------------------------------------------------------------ the C interface
@pytest.mark.parametrize("name", ["reg8", "packed256_t16_a"])
def test_rls_row_stride_longer_than_the_block(orc, dev, name):
    """btk_rls_process_nc with T_stride = T + 3: the same bits as the contiguous run, and the padding is not written"""
    import torch
    from distant_speech_recognition_amd import engine as eng, _lib
    N, Nc, M, S, _, kw, _ = cf.rls_case(name)
    vs, Xe, _, _ = _rls_reference(orc, name)
    K, T, pad = M // 2 + 1, Xe.shape[-1], 3
    vd = torch.from_numpy(vs).to(dev)
    st0 = eng.RLSState(1, S, M, N, vd, Nc=Nc, **kw)
    Y0 = eng.rls_process(torch.from_numpy(Xe).to(dev), st0)
    st = eng.RLSState(1, S, M, N, vd, Nc=Nc, **kw)
    Xp = torch.zeros((S, K, N, T + pad), dtype=torch.complex64, device=dev)
    Xp[..., :T] = torch.from_numpy(Xe).to(dev)
    Xp[..., T:] = 1e30                                                   # whatever lies behind a row must not be read as a frame
    sentinel = complex(-7.0, 3.0)
    Yp = torch.full((S, K, T + pad), sentinel, dtype=torch.complex64, device=dev)
    params = st.params_array()
    ws = st.workspace(T)
    vp = lambda t: C.c_void_p(t.data_ptr())
    _lib.check(_lib.lib().btk_rls_process_nc(1, params.ctypes.data_as(C.c_void_p), vp(st.v), st.per_stream, None, 1, vp(Xp), vp(Yp),
                                             S, M, N, T + pad, T, vp(st.P), vp(st.w), vp(st.stream_state), vp(ws),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert torch.equal(Yp[..., :T].contiguous().view(torch.float32), Y0.view(torch.float32))
    assert torch.all(Yp[..., T:] == sentinel)
    assert torch.equal(st.P.view(torch.float64), st0.P.view(torch.float64)) and torch.equal(st.w.view(torch.float64), st0.w.view(torch.float64))
    assert torch.equal(st.stream_state, st0.stream_state)


def test_rls_process_checks_its_tensors(dev):
    import torch
    from distant_speech_recognition_amd import engine as eng, _lib
    N, M, T = 8, 16, 8
    K = M // 2 + 1
    st = eng.RLSState(1, 1, M, N, torch.from_numpy(cf.manifold(N, M)[1]).to(dev))
    X = torch.zeros((1, K, N, T), dtype=torch.complex64, device=dev)
    with pytest.raises(_lib.BtkError):
        eng.rls_process(X.to(torch.complex128), st)
    with pytest.raises(_lib.BtkError):
        eng.rls_process(X[0], st)
    with pytest.raises(_lib.BtkError):
        eng.rls_process(X, st, out=torch.zeros((1, K, T + 1), dtype=torch.complex64, device=dev))
    with pytest.raises(_lib.BtkError):
        eng.rls_process(X, st, out=torch.zeros((1, K, T), dtype=torch.complex128, device=dev))
    assert eng.rls_process(X, st, out=torch.zeros((1, K, T), dtype=torch.complex64, device=dev)).shape == (1, K, T)
