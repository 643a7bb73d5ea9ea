"""GPU: steered response power (srp_power / srp_select / SRPState) against the float64 closed form of
tests/srp_closed_form.py on the same float32 snapshots.

Bounds (derived, not tuned):
  rp      |rp_gpu - rp_f64| <= (2N + 8 + nb) 2^-24 e[u][t],  e = sum_k c_k (sum_n |sv| |x|)^2 / nb: the worst-case rounding of a
          float32 dot product of N terms, squared, summed over nb bins, with a table rounded to float32.
  energy  4 (N + nb) 2^-24 relative (all terms non-negative).
Indices are compared on a grid of 0..pi only: the delays depend on cos(theta), so the default grid -pi/2..pi/2 holds every
direction twice and its N-best is a list of mathematical ties."""
import numpy as np
import pytest
import torch

from tests import srp_closed_form as cf

pytestmark = pytest.mark.gpu

FS = 16000.0
EPS = 2.0 ** -24
DEG = 0.0174533


def positions(N, pitch_mm=20.0):
    return np.arange(N) * pitch_mm / 343740.0


def make_case(N, M, T, width, src_idx, snr_db, seed, S=1):
    """(positions, thetas, sv float64, X complex64 [S][K][N][T] numpy): plane waves from grid directions + noise."""
    pos = positions(N)
    th = cf.grid(0.0, np.pi, width)
    rng = np.random.default_rng(seed)
    Xs = []
    for s in range(S):
        idx = [(i + 3 * s) % len(th) for i in src_idx]
        X, _ = cf.plane_wave_snapshots(rng, M, FS, pos, [th[i] for i in idx], T, snr_db=snr_db, amp=100.0 * (s + 1))
        Xs.append(X.astype(np.complex64))
    return pos, th, np.stack(Xs)


def gpu_power(eng, dev, X, M, N, pos, th, fmin=1, fmax=None, padded=False):
    tbl = eng.srp_table(M, N, FS, pos, th, fmin, M // 2 if fmax is None else fmax)
    if padded:
        buf = torch.zeros(X.shape[:-1] + (X.shape[-1] + 48,), dtype=torch.complex64, device=dev)
        Xd = buf[..., :X.shape[-1]]
        Xd.copy_(torch.from_numpy(X))
        assert not Xd.is_contiguous()
    else:
        Xd = torch.from_numpy(X).to(dev)
    rp, en = eng.srp_power(Xd, eng.SRPTable(tbl, dev), M, fmin, fmax)
    return tbl, rp, en


def check_power(X, M, N, tbl, rp, en, fmin=1, fmax=None, tag=""):
    """rp and energy of every stream within the bounds; returns the largest ratio error / bound seen."""
    fmax = M // 2 if fmax is None else fmax
    nb = fmax - fmin + 1
    worst = 0.0
    rp, en = rp.cpu().numpy(), en.cpu().numpy()
    refs = []
    for s in range(X.shape[0]):
        r64, e = cf.response_power(X[s], tbl, M, fmin, fmax)
        bound = (2 * N + 8 + nb) * EPS * e
        ratio = float(np.max(np.abs(rp[s] - r64) / bound))
        en64 = cf.energy(X[s], M, fmin, fmax)
        erel = float(np.max(np.abs(en[s] - en64) / en64))
        print("srp %s s=%d: max |rp err| / bound = %.4f, energy rel err %.3g (bound %.3g)" % (tag, s, ratio, erel, 4 * (N + nb) * EPS))
        assert ratio <= 1.0, (tag, s, ratio)
        assert erel <= 4 * (N + nb) * EPS, (tag, s, erel)
        worst = max(worst, ratio)
        refs.append((r64, bound))
    return worst, refs


#            N    M     T     width  sources   SNR  nBest
SHAPES = [(8, 512, 512, 0.1, (10,), 10.0, 3),
          (64, 512, 256, 0.1, (10,), -10.0, 3),
          (64, 512, 128, DEG, (60,), 0.0, 3),
          (16, 256, 512, 0.05, (15, 42), 0.0, 3),
          (4, 64, 2048, 0.1, (10,), 0.0, 4),
          (256, 2048, 96, 0.1, (10,), 5.0, 2)]


@pytest.mark.parametrize("N,M,T,width,src,snr,nbest", SHAPES)
def test_response_power_and_selection(dev, N, M, T, width, src, snr, nbest):
    from distant_speech_recognition_amd import engine as eng
    pos, th, X = make_case(N, M, T, width, src, snr, seed=N * 1000 + T)
    tbl, rp, en = gpu_power(eng, dev, X, M, N, pos, th)
    assert np.max(np.abs(tbl - cf.table(M, FS, pos, th))) <= 1e-15
    tag = "N=%d M=%d T=%d U=%d" % (N, M, T, len(th))
    _, refs = check_power(X, M, N, tbl, rp, en, tag=tag)
    r64, bound = refs[0]
    # selection, exact: the kernel's N-best on its own float32 powers == the reference's insertion loop on those numbers
    rp_h = rp.cpu().numpy()[0]
    for nb_ in (1, 3, 16):
        nb_rp, nb_idx, gate, acc = eng.srp_select(rp, en, nb_)
        nb_rp, nb_idx = nb_rp.cpu().numpy()[0], nb_idx.cpu().numpy()[0]
        assert bool(gate.all())
        for t in range(T):
            v, i = cf.nbest_insert(rp_h[:, t], nb_)
            assert np.array_equal(nb_rp[t], v.astype(np.float32)) and np.array_equal(nb_idx[t], i), (tag, nb_, t)
        a64 = rp_h.astype(np.float64).sum(axis=1)
        assert np.max(np.abs(acc.cpu().numpy()[0] - a64) / a64) <= 1e-12
    # selection against float64: equal indices wherever the top nBest + 1 float64 powers are further apart than twice the bound
    nb_rp, nb_idx, _, _ = eng.srp_select(rp, en, nbest)
    nb_idx = nb_idx.cpu().numpy()[0]
    left_out = 0
    for t in range(T):
        order = np.argsort(-r64[:, t], kind="stable")[:nbest + 1]
        vals, bnds = r64[order, t], bound[order, t]
        clear = all(abs(vals[a] - vals[b]) > 2.0 * max(bnds[a], bnds[b]) for a in range(len(order)) for b in range(a + 1, len(order)))
        if not clear:
            left_out += 1
            continue
        _, i64 = cf.nbest_insert(r64[:, t], nbest)
        assert np.array_equal(nb_idx[t], i64), (tag, t)
    print("srp %s: %d of %d frames left out of the float64 index comparison" % (tag, left_out, T))
    assert left_out <= 0.02 * T, (tag, left_out)


@pytest.mark.parametrize("N,M,T,width,src,snr,nbest", SHAPES)
def test_finds_the_source_at_0db(dev, N, M, T, width, src, snr, nbest):
    from distant_speech_recognition_amd import engine as eng
    pos, th, X = make_case(N, M, T, width, src, 0.0, seed=77 + N)
    nsrc = len(src)
    # a condition on the inputs: the float64 closed form itself ranks the source directions first
    sv = cf.table(M, FS, pos, th)
    acc64 = cf.run(X[0], sv, M, nsrc)[5]
    assert set(cf.nbest_insert(acc64, nsrc)[1]) == set(src)
    st = eng.SRPState(1, M, FS, pos, dev, nbest=nsrc, min_theta=0.0, max_theta=np.pi, width_theta=width, min_phi=-0.25)
    st.process(torch.from_numpy(X).to(dev))
    rps, doas = st.final_nbest_hypotheses()
    assert set(np.round(doas[0, :, 0], 9)) == set(np.round(th[list(src)], 9))
    if nsrc == 1:
        assert doas[0, 0, 0] == th[src[0]]
    assert np.all(doas[0, :, 1] == np.float64(np.float32(-0.25)))           # (theta_u, minPhi), beamformer.cc:2971-2972
    assert abs(rps[0, 0] - acc64.max()) <= 1e-5 * acc64.max()


@pytest.mark.parametrize("N,M,T,fmin,fmax,S,padded", [
    (7, 128, 100, 1, None, 1, False),       # odd N
    (8, 128, 1, 1, None, 1, False),         # T = 1
    (8, 128, 33, 1, None, 1, False),        # one frame beyond a strip
    (8, 128, 70, 5, 40, 1, False),          # restricted range
    (8, 128, 70, 9, 9, 1, False),           # fmin == fmax
    (8, 128, 70, 64, 64, 1, False),         # the Nyquist bin alone (c_k = 1)
    (12, 128, 150, 1, None, 3, False),      # three streams, different content
    (8, 512, 512, 1, None, 2, True),        # row-padded X
    (2, 64, 40, 1, None, 1, False),
    (80, 128, 40, 1, None, 1, False),       # more than one channel chunk, not a multiple of it
])
def test_shapes_and_tails(dev, N, M, T, fmin, fmax, S, padded):
    from distant_speech_recognition_amd import engine as eng
    pos, th, X = make_case(N, M, T, 0.1, (10,), 5.0, seed=N + T, S=S)
    tbl, rp, en = gpu_power(eng, dev, X, M, N, pos, th, fmin, fmax, padded=padded)
    assert rp.shape == (S, len(th), T) and en.shape == (S, T)
    check_power(X, M, N, tbl, rp, en, fmin, fmax, tag="N=%d M=%d T=%d f=%s..%s S=%d" % (N, M, T, fmin, fmax, S))


def test_many_directions_run_in_passes(dev):
    """More directions than one pass holds (128): the passes write disjoint rows and agree with the closed form."""
    from distant_speech_recognition_amd import engine as eng
    N, M, T = 16, 128, 50
    pos, th, X = make_case(N, M, T, DEG / 2, (100,), 5.0, seed=5)
    assert len(th) == 360
    tbl, rp, en = gpu_power(eng, dev, X, M, N, pos, th)
    check_power(X, M, N, tbl, rp, en, tag="U=360")


def test_select_crafted_ties_and_reset_values(dev):
    from distant_speech_recognition_amd import engine as eng
    U, T = 40, 6
    rng = np.random.default_rng(0)
    rp = rng.uniform(1.0, 2.0, size=(1, U, T)).astype(np.float32)
    rp[0, [7, 30], 0] = 5.0                              # two equal maxima
    rp[0, [3, 9, 17, 25, 33], 1] = 7.0                   # five equal maxima
    rp[0, :, 2] = 4.25                                   # all equal
    rp[0, :, 3] = -3.0e11                                # all below the reset value: nothing is inserted
    rp[0, :, 4] = -3.0e11
    rp[0, 12, 4] = -1.0e9                                # one above it
    en = np.ones((1, T), np.float32)
    rpd, end = torch.from_numpy(rp).to(dev), torch.from_numpy(en).to(dev)
    for nbest in (1, 3, 16):
        nb_rp, nb_idx, gate, _ = eng.srp_select(rpd, end, nbest)
        nb_rp, nb_idx = nb_rp.cpu().numpy()[0], nb_idx.cpu().numpy()[0]
        for t in range(T):
            v, i = cf.nbest_insert(rp[0, :, t], nbest)
            assert np.array_equal(nb_rp[t], v.astype(np.float32)) and np.array_equal(nb_idx[t], i), (nbest, t)
        assert nb_idx[0, 0] == 7 and nb_idx[1, 0] == 3 and nb_idx[2, 0] == 0
        assert np.all(nb_idx[3] == -1) and np.all(nb_rp[3] == np.float32(-10e10))
        assert nb_idx[4, 0] == 12 and np.all(nb_idx[4, 1:] == -1)
        if nbest >= 3:
            assert list(nb_idx[0, :2]) == [7, 30] and list(nb_idx[1, :3]) == [3, 9, 17] and list(nb_idx[2, :3]) == [0, 1, 2]
    with pytest.raises(eng._lib.BtkError):
        eng.srp_select(rpd, end, 17)
    with pytest.raises(eng._lib.BtkError):
        eng.srp_select(rpd, end, 0)


def test_gate_and_accumulator(dev):
    """Frames with energy < threshold keep the reset N-best and stay out of acc; the threshold is compared on the float32 energy
    the kernel wrote; acc is the float64 sum of the gated float32 powers and two runs give the same bits."""
    from distant_speech_recognition_amd import engine as eng
    N, M, T = 8, 128, 300
    pos, th, X = make_case(N, M, T, 0.1, (10,), 5.0, seed=9, S=2)
    X[:, :, :, 50:120] *= 0.01                           # quiet frames
    tbl, rp, en = gpu_power(eng, dev, X, M, N, pos, th)
    en_h, rp_h = en.cpu().numpy(), rp.cpu().numpy()
    thr = float(en_h[0, 200])                            # a frame exactly at the threshold passes (energy < threshold is false)
    nb_rp, nb_idx, gate, acc = eng.srp_select(rp, en, 3, threshold=thr)
    g = gate.cpu().numpy().astype(bool)
    assert np.array_equal(g, ~(en_h < np.float32(thr))) and g[0, 200] and not g[:, 50:120].any() and g.sum() > 100
    nb_rp, nb_idx = nb_rp.cpu().numpy(), nb_idx.cpu().numpy()
    assert np.all(nb_idx[~g] == -1) and np.all(nb_rp[~g] == np.float32(-10e10)) and np.all(nb_idx[g] >= 0)
    a64 = np.einsum("sut,st->su", rp_h.astype(np.float64), g.astype(np.float64))
    assert np.max(np.abs(acc.cpu().numpy() - a64) / a64) <= 1e-12
    acc2 = eng.srp_select(rp, en, 3, threshold=thr)[3]
    assert torch.equal(acc, acc2)
    acc3 = eng.srp_select(rp, en, 3, threshold=thr, acc=acc2.clone())[3]             # += across blocks
    assert np.max(np.abs(acc3.cpu().numpy() - 2 * a64) / a64) <= 1e-12
    _, rp2, en2 = gpu_power(eng, dev, X, M, N, pos, th)
    assert torch.equal(rp, rp2) and torch.equal(en, en2)


def test_power_through_real_analysis_banks(dev):
    """Snapshots of real analysis banks (row-padded view): agreement with the closed form on the same snapshots, and the
    last-direction beam equals bf_apply with the last table row."""
    from distant_speech_recognition_amd import engine as eng
    from tests.util import design_prototype, synthetic_pcm
    M, m, r, N = 512, 4, 1, 8
    pcm, _ = synthetic_pcm(2, N, 60 * 256, seed=3)
    afb = eng.FilterBank(design_prototype(M, m), M, m, r, 2)
    Xd = afb.analysis(torch.from_numpy(pcm).to(dev), pad_rows=True)
    X = Xd.cpu().numpy()
    pos, th = positions(N), cf.grid(0.0, np.pi, 0.1)
    st = eng.SRPState(2, M, FS, pos, dev, nbest=3, min_theta=0.0, max_theta=np.pi, fbin_min=2, fbin_max=200)
    rp, en, nb_rp, nb_idx, gate = st.process(Xd)
    check_power(X, M, N, st.table_host, rp, en, 2, 200, tag="banks")
    Y = st.last_beam(Xd).cpu().numpy()
    W = cf.table(M, FS, pos, th, 2, 200)[-1]
    ref = np.einsum("kn,sknt->skt", np.conj(W[2:201]), X[:, 2:201].astype(np.complex128))
    assert np.all(Y[:, :2] == 0) and np.all(Y[:, 201:] == 0)
    assert np.max(np.abs(Y[:, 2:201] - ref)) <= 1e-5 * np.max(np.abs(ref))


def test_bad_arguments(dev):
    from distant_speech_recognition_amd import engine as eng
    N, M, T = 8, 128, 16
    pos, th, X = make_case(N, M, T, 0.1, (10,), 5.0, seed=1)
    Xd = torch.from_numpy(X).to(dev)
    tbl = eng.SRPTable(eng.srp_table(M, N, FS, pos, th), dev)
    for fmin, fmax in ((0, 10), (11, 10), (1, 65)):
        with pytest.raises(eng._lib.BtkError) as ei:
            eng.srp_power(Xd, tbl, M, fmin, fmax)
        assert ei.value.code == eng._lib.BTK_ERR_PARAMETER
    with pytest.raises(eng._lib.BtkError) as ei:
        eng.srp_power(Xd[:, :, :1].contiguous(), eng.SRPTable(np.ones((3, 65, 1), complex), dev), M)
    assert ei.value.code == eng._lib.BTK_ERR_DIMENSION
    L = eng._lib.lib()
    assert L.btk_srp_power(None, None, None, None, 1, M, N, T, T, 31, 1, 64, None) == eng._lib.BTK_ERR_PARAMETER
    assert b"null" in L.btk_last_error()


# ------------------------------------------------------------------------------------------------ the node
NM, Nm, Nr, ND, NN = 512, 4, 1, 256, 8
NFMIN, NFMAX, NNBEST = 2, 200, 3


class _Frames:
    """A Python source node of complex frames (stream/pyStream.h protocol)."""

    def __init__(self, frames):
        self.frames, self.i = frames, 0

    def size(self):
        return self.frames.shape[1]

    def __iter__(self):
        self.i = 0
        return self

    def next(self):
        if self.i >= len(self.frames):
            raise StopIteration
        self.i += 1
        return self.frames[self.i - 1]

    __next__ = next

    def reset(self):
        self.i = 0


def _estimator(threshold):
    from distant_speech_recognition_amd.btk20.beamformer import DOAEstimatorSRPDSBLAPtr
    est = DOAEstimatorSRPDSBLAPtr(nBest=NNBEST, samplerate=int(FS), fftlen=NM)
    est.set_array_geometry(positions=positions(NN))
    est.set_search_param(minTheta=0.0, maxTheta=np.pi, minPhi=-0.25, maxPhi=0.25, widthTheta=0.1)
    est.set_frequency_range(fbinMin=NFMIN, fbinMax=NFMAX)
    est.set_energy_threshold(engeryThreshold=threshold)
    return est


def _over_banks(pcm, threshold, block_frames):
    from distant_speech_recognition_amd.btk20 import SampleFeaturePtr, OverSampledDFTAnalysisBankPtr
    from tests.util import design_prototype
    est, keep = _estimator(threshold), []
    for x in pcm:
        sf = SampleFeaturePtr(block_len=ND, shift_len=ND, pad_zeros=True)
        sf.setSamples(np.asarray(x, np.float64), int(FS))
        a = OverSampledDFTAnalysisBankPtr(sf, prototype=design_prototype(NM, Nm), M=NM, m=Nm, r=Nr, delay_compensation_type=2)
        a.set_block_frames(block_frames)
        est.set_channel(a)
        keep.append((sf, a))
    return est, keep


def _over_python_sources(X, threshold, block_frames):
    from distant_speech_recognition_amd.btk20 import PyVectorComplexFeatureStreamPtr
    est, keep = _estimator(threshold), []
    K, N, T = X.shape
    for n in range(N):
        fr = np.zeros((T, NM), np.complex128)
        fr[:, :K] = X[:, n, :].T
        fr[:, K:] = np.conj(fr[:, 1:K - 1][:, ::-1])
        src = PyVectorComplexFeatureStreamPtr(_Frames(fr))
        est.set_channel(src)
        keep.append(src)
    est.set_block_frames(block_frames)
    return est, keep


def _drain(est, want_snapshots=False):
    out = {"rps": [], "doas": [], "energy": [], "rpm": [], "vec": []}
    X = None
    for v in est:
        if want_snapshots and X is None:
            X = est.device_snapshots().clone()
        out["vec"].append(np.array(v)); out["rps"].append(np.array(est.nbest_rps())); out["doas"].append(np.array(est.nbest_doas()))
        out["energy"].append(est.energy()); out["rpm"].append(np.array(est.response_power_matrix())[:, 0])
    out = {k: np.array(v) for k, v in out.items()}
    out["acc"] = np.array(est.accumulated_rps())
    est.final_nbest_hypotheses()
    out["final_rps"], out["final_doas"] = np.array(est.nbest_rps()), np.array(est.nbest_doas())
    return out, X


def test_node_equals_block_api_at_every_block_size(dev):
    from distant_speech_recognition_amd import engine as eng
    from tests.util import synthetic_pcm
    pcm, _ = synthetic_pcm(1, NN, 300 * ND, seed=11)
    pcm = pcm[0]
    pcm[:, 100 * ND:160 * ND] *= 0.05                          # a quiet stretch for the energy gate
    est, keep = _over_banks(pcm, 0.0, 0)
    first, Xd = _drain(est, want_snapshots=True)
    T = Xd.shape[-1]
    assert len(first["energy"]) == T == 300 + 7 - 3 and Xd.shape == (1, NM // 2 + 1, NN, T)
    with pytest.raises(StopIteration):
        est.next()
    thr = float(np.sort(first["energy"])[T // 4])
    # the block API on the same snapshots
    st = eng.SRPState(1, NM, FS, positions(NN), dev, nbest=NNBEST, min_theta=0.0, max_theta=np.pi, min_phi=-0.25,
                      fbin_min=NFMIN, fbin_max=NFMAX, energy_threshold=thr)
    rp, en, nb_rp, nb_idx, gate = (a.cpu().numpy()[0] for a in st.process(Xd))
    Y = st.last_beam(Xd).cpu().numpy()[0]
    frps, fdoas = st.final_nbest_hypotheses()
    assert 0 < gate.sum() < T and np.array_equal(first["energy"].astype(np.float32), en)
    runs = {}
    for name, bfr in (("whole", 0), ("64", 64), ("200", 200)):
        est, keep = _over_banks(pcm, thr, bfr)
        runs[name] = (_drain(est)[0], est)
    est, keep = _over_python_sources(Xd.cpu().numpy()[0], thr, 50)
    runs["python sources"] = (_drain(est)[0], est)
    prev_rpm, prev_vec = np.zeros(len(st.thetas)), np.zeros(NM, complex)
    w = runs["whole"][0]
    for t in range(T):
        assert np.float32(w["energy"][t]) == en[t]
        if gate[t]:
            assert np.array_equal(w["rps"][t], nb_rp[t].astype(np.float64)), t
            assert np.array_equal(w["doas"][t][:, 0], st.thetas[nb_idx[t]]) and np.all(w["doas"][t][:, 1] == 0.0), t
            assert np.array_equal(w["rpm"][t], rp[:, t].astype(np.float64)), t
            vec = np.zeros(NM, complex)
            vec[NFMIN:NFMAX + 1] = Y[NFMIN:NFMAX + 1, t]
            vec[NM - NFMAX:NM - NFMIN + 1] = np.conj(Y[NFMIN:NFMAX + 1, t])[::-1]
            assert np.array_equal(w["vec"][t], vec), t
            prev_rpm, prev_vec = w["rpm"][t], w["vec"][t]
        else:
            assert np.all(w["rps"][t] == -10e10) and np.all(w["doas"][t] == -np.pi), t
            assert np.array_equal(w["rpm"][t], prev_rpm) and np.array_equal(w["vec"][t], prev_vec), t
    assert np.array_equal(w["acc"], st.acc.cpu().numpy()[0])
    assert np.array_equal(w["final_rps"], frps[0]) and np.array_equal(w["final_doas"], fdoas[0])
    assert np.all(w["final_doas"][:, 1] == np.float64(np.float32(-0.25)))
    for name in ("64", "200", "python sources"):
        o = runs[name][0]
        for key in w:
            assert np.array_equal(o[key], w[key]), (name, key)
    # reset() keeps the accumulated powers, init_accs() clears them (on the Python sources: they replay after reset())
    est = runs["python sources"][1]
    est.reset()
    assert np.array_equal(np.array(est.accumulated_rps()), w["acc"])
    second, _ = _drain(est)
    st.process(Xd)
    assert np.array_equal(second["acc"], st.acc.cpu().numpy()[0]) and np.all(second["acc"] > w["acc"])
    assert np.array_equal(second["rps"], w["rps"])
    est.init_accs()
    assert np.all(np.array(est.accumulated_rps()) == 0.0) and np.all(np.array(est.nbest_rps()) == -10e10)
    # init_accs() in the middle of a block: the frames that follow still count, the ones before do not
    est.reset()
    for i, _ in enumerate(est):
        if i == 99:
            est.init_accs()
    want = np.zeros(len(st.thetas))
    for t in range(100, T):
        if gate[t]:
            want += rp[:, t].astype(np.float64)
    assert np.array_equal(np.array(est.accumulated_rps()), want)
    # a new frequency range rebuilds the table and keeps the accumulated powers (the grid is the same); a new search range clears them
    est.reset()
    est.set_frequency_range(fbinMin=3, fbinMax=100)
    est.next()
    kept = np.array(est.accumulated_rps())
    assert kept.shape == want.shape and np.all(kept >= want) and np.all(want > 0)
    est.set_search_param(minTheta=0.0, maxTheta=np.pi, widthTheta=0.2)
    assert len(est.accumulated_rps()) == 0
    est.reset()
    est.next()
    assert len(est.accumulated_rps()) == 16 and len(est.search_thetas()) == 16 and est.response_power_matrix().shape == (16, 1)


# ------------------------------------------------------------------------------------------------ the tool
def test_tool_writes_a_configuration_online_beamforming_accepts(orc, dev, tmp_path):
    import json
    import os
    import subprocess
    import sys
    import wave
    from tests.util import design_prototype
    from tools.online_beamforming import check_position_data_format, SSPEED
    from distant_speech_recognition_amd.pybeamformer import calc_delays
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    N, fs, L, M, m, r = 8, 16000, 32000, 512, 4, 1
    mic_x = np.arange(N) * 40.0
    th = cf.grid(0.0, np.pi, 0.1)
    true_idx = (7, 22)
    rng = np.random.default_rng(2026)
    # fractional delays by a phase ramp on the whole signal's FFT
    f = np.fft.rfftfreq(L, 1.0 / fs)
    pcm = rng.normal(0.0, 3000.0, size=(N, L))
    for seg, u in enumerate(true_idx):
        s = np.zeros(L)
        s[seg * fs:(seg + 1) * fs] = rng.normal(0.0, 3000.0, fs)
        d = cf.delays(mic_x / SSPEED, th[u])
        for n in range(N):
            pcm[n] += np.fft.irfft(np.fft.rfft(s) * np.exp(-2j * np.pi * f * d[n]), L)
    pcm = np.clip(np.rint(pcm), -32767, 32767).astype(np.int16)
    wavs = []
    for n in range(N):
        p = str(tmp_path / ("c%d.wav" % n))
        w = wave.open(p, "wb")
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(fs)
        w.writeframes(pcm[n].tobytes())
        w.close()
        wavs.append(p)
    h = design_prototype(M, m)
    np.savez(str(tmp_path / "proto.npz"), h=h, g=design_prototype(M, m, "g"))
    conf = {"array_type": "linear", "microphone_positions": [[float(x), 0.0, 0.0] for x in mic_x],
            "target": {"positions": [[0.0, [0.0, None, None]]]}, "beamformer": {"type": "delay_and_sum"}}
    json.dump(conf, open(str(tmp_path / "in.json"), "w"))
    # the float64 closed form on the oracle's analysis of the same samples, segment by segment as the tool cuts them
    X = np.stack([orc.analysis(h, M, m, r, 2, pcm[n].astype(np.float32))[:, :M // 2 + 1].T for n in range(N)], axis=1)
    T = X.shape[-1]
    rp, _ = cf.response_power(X, cf.table(M, fs, mic_x / SSPEED, th), M)
    ends = [t for t in range(T) if (t + 1) * (M // 2) / fs >= 1.0][0], [t for t in range(T) if (t + 1) * (M // 2) / fs >= 2.0][0]
    picks = [int(np.argmax(rp[:, :ends[0] + 1].sum(axis=1))), int(np.argmax(rp[:, ends[0] + 1:ends[1] + 1].sum(axis=1)))]
    assert all(abs(p - u) <= 1 for p, u in zip(picks, true_idx)), picks       # a condition on the test's inputs
    res = subprocess.run([sys.executable, os.path.join(root, "tools", "estimate_doa.py"), "-q", "-a", str(tmp_path / "proto.npz"),
                          "-M", str(M), "-m", str(m), "-r", str(r), "-c", str(tmp_path / "in.json"), "-o", str(tmp_path / "out.json"),
                          "--segment-sec", "1.0", "-i"] + wavs, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    out = json.load(open(str(tmp_path / "out.json")))
    check_position_data_format(out)                                            # online_beamforming.py's loader accepts it
    pos = out["target"]["positions"]
    assert out["microphone_positions"] == conf["microphone_positions"] and out["beamformer"] == conf["beamformer"]
    assert len(pos) == 3 and pos[0][0] == 1.0 and pos[1][0] == 2.0 and pos[0][1][1:] == [None, None]
    for (t_end, (az, _, _)), p, u in zip(pos[:2], picks, true_idx):
        assert az == float(np.pi - np.float64(np.float32(th[p]))), (t_end, az, p)
        assert abs((np.pi - az) - th[u]) <= 0.1 + 1e-6
        d_tool = calc_delays("linear", out["microphone_positions"], [az, None, None], sspeed=SSPEED)
        d_row = cf.delays(mic_x / SSPEED, th[p])
        assert np.max(np.abs((d_tool - d_row) - (d_tool - d_row)[0])) <= 1e-12
