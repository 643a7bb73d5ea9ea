"""GPU: the WPE kernels of csrc/wpe_kernels.hip stage by stage and on the branches the end-to-end tests never reach.
  (a) prediction alone (btk_wpe_apply with taps drawn at random, not estimated) against the float64 closed form of
      tests/wpe_closed_form.py under a derived float32 bound, on both prediction kernels and every path between them
  (b) the same with band limiting: taps of the bins outside the band are NaN and must never be read
  (c) band-limited estimate + apply against the oracle, one case per normal-equation family, both solvers, the btk20 node
  (d) strip kernels <2> / <4>, several streams through the lag-product and block kernels, against the oracle
  (e) the loading rule and the normal equations under heavy loading, where the taps show the accuracy of R and r themselves
Inputs go through complex64 before the float64 references see them.  M = 16 (K = 9 bins) unless a case says otherwise."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import wpe_closed_form as cf
from tests.test_gpu_btk20_api import FS as API_FS, M as API_M, _build, _oracle_X, wavs  # noqa: F401  (wavs is a fixture)
from tests.test_wpe_cpu import (E_CASES, FS, e_input, e_reference, e_tolerance, oracle_output, oracle_taps, rounded_input)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M16, K16 = 16, 9
U32 = 2.0 ** -24                                                           # unit roundoff of float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _gpu_apply(dev, X, G, M, lower, upper, bw=0.0):
    import torch
    from distant_speech_recognition_amd import engine as eng
    out = eng.wpe_apply(torch.from_numpy(X).to(dev), torch.from_numpy(G).to(dev), M, lower_num=lower, upper_num=upper, band_width=bw,
                        samplerate=FS)
    return out.cpu().numpy()


def _gpu_estimate_apply(dev, X, M, lower, upper, iters=2, load_db=-18.0, bias=1e-4, bw=0.0):
    import torch
    from distant_speech_recognition_amd import engine as eng
    Xd = torch.from_numpy(X).to(dev)
    G = eng.wpe_estimate(Xd, M, lower_num=lower, upper_num=upper, iterations_num=iters, load_db=load_db, band_width=bw,
                         diagonal_bias=bias, samplerate=FS)
    out = eng.wpe_apply(Xd, G, M, lower_num=lower, upper_num=upper, band_width=bw, samplerate=FS)
    return G.cpu().numpy(), out.cpu().numpy()


# ------------------------------------------------------------------------------------------------ (a), (b): prediction alone
# (C, lower, upper): launch_wpe_predict takes the matrix cores for 4 <= C <= 16 when conj(G) and the channel spans fit 64 KB of LDS
A_ROWS = [(1, 0, 3),        # vector kernel
          (3, 1, 5),        # vector kernel
          (4, 0, 7),        # matrix cores
          (5, 2, 6),        # matrix cores, C % 4 != 0
          (8, 1, 33),       # matrix cores, L = 33 is no multiple of 4: the lane's (channel, lag) carry loop runs
          (8, 0, 0),        # matrix cores, L = 1
          (12, 3, 5),       # matrix cores, lower = L: no tap applies at apply time
          (16, 0, 13),      # matrix cores, the largest L at 16 channels: 8 (16 * 228 + 16 * 269) = 63 616 bytes of LDS
          (16, 0, 14),      # 8 (16 * 260 + 16 * 270) = 67 840 bytes: silent fallback to the vector kernel
          (16, 0, 15),      # vector kernel by the same rule
          (17, 0, 3),       # vector kernel, C > 16
          (8, 5, 6)]        # matrix cores, lower > L
T_SET = (1, 17, 256, 257, 300)       # one frame, a 16-column tile edge, both sides of the 256-frame workgroup
B_ROWS = [(3, 1, 5), (4, 0, 7), (8, 1, 33)]


def _prediction_case(C, lower, upper, T, nan_bins=()):
    """S = 2 streams with different signals and different taps; sum |g||x| is of the order of |y|"""
    S, L = 2, upper - lower + 1
    P = C * L
    rng = np.random.default_rng(1000 * C + 37 * lower + upper + 100003 * T)
    X = ((rng.normal(size=(S, K16, C, T)) + 1j * rng.normal(size=(S, K16, C, T))) * 300).astype(np.complex64)
    G = ((rng.normal(size=(S, C, K16, P)) + 1j * rng.normal(size=(S, C, K16, P))) / P).astype(np.complex64)
    for k in nan_bins:
        G[:, :, k] = np.nan + 1j * np.nan
    return X, G


def _check_prediction(dev, C, lower, upper, bw):
    L = upper - lower + 1
    P = C * L
    lo, up = cf.band(M16, bw, FS)
    inactive = [k for k in range(K16) if not cf.active(k, lo, up)]
    act = [k for k in range(K16) if cf.active(k, lo, up)]
    for T in T_SET:
        X, G = _prediction_case(C, lower, upper, T, nan_bins=inactive)
        ref, mag = cf.predict(X.astype(np.complex128), G.astype(np.complex128), lower, upper, lo, up, apply=True)
        assert np.max(np.abs(ref)) > 0.1 * np.max(np.abs(X))
        got = _gpu_apply(dev, X, G, M16, lower, upper, bw)
        assert got.shape == X.shape and got.dtype == np.complex64
        assert np.all(np.isfinite(got.view(np.float32)))
        # every component is a float32 sum of at most 2P + 1 terms: gamma_(2P+1) * sum |terms| per component, sqrt(2) of it for the
        # modulus, and |gr xr| + |gi xi| <= |g||x|
        err = np.abs(got.astype(np.complex128) - ref)
        bound = 2 * (2 * P + 2) * U32 * mag
        worst = float(np.max(err[:, act] / bound[:, act]))
        print("WPE prediction C=%d lags %d..%d T=%d band %g: largest error / bound = %.3g" % (C, lower, upper, T, bw, worst))
        assert np.all(err <= bound), (T, worst)
        assert np.array_equal(_bits(got[..., :lower]), _bits(X[..., :lower])), T            # rows t < lower pass through
        if inactive:
            assert np.array_equal(_bits(got[:, inactive]), _bits(X[:, inactive])), T        # so do the bins outside the band
        if lower >= L:                                                                      # no tap applies: the input, bit for bit
            assert np.array_equal(_bits(got), _bits(X)), T
        elif T > lower + 1:                                     # otherwise the taps did something (P terms of 1 / P at random phases)
            assert np.max(np.abs(ref[:, act] - X[:, act])) > 0.25 / np.sqrt(P) * np.max(np.abs(X)), T


@pytest.mark.parametrize("C,lower,upper", A_ROWS)
def test_prediction_alone(dev, C, lower, upper):
    _check_prediction(dev, C, lower, upper, 0.0)


@pytest.mark.parametrize("C,lower,upper", B_ROWS)
def test_prediction_band_limited_never_reads_taps_outside_the_band(dev, C, lower, upper):
    """band_width 3000 Hz at M = 16: lo = 3, bins 4..8 are outside the band and their taps are NaN"""
    _check_prediction(dev, C, lower, upper, 3000.0)


# ------------------------------------------------------------------------------------------------ (c), (d): against the oracle
_ORACLE = {}


def _oracle_case(orc, C, lower, upper, M, bw, T, S=1):
    """-> (X [S][K][C][T] complex64, Gref [S][C][K][P], ref [S][K][C][T]); 2 iterations, load_db -18, bias 1e-4; computed once"""
    key = (C, lower, upper, M, bw, T, S)
    if key not in _ORACLE:
        X = rounded_input(52000 + 100 * C + 10 * lower + upper + M, S, C, M, T)
        Gs, outs = [], []
        for s in range(S):
            Gk, Gfull = oracle_taps(orc, X[s], M, lower, upper, 2, -18.0, bw, 1e-4)
            Gs.append(Gk)
            outs.append(oracle_output(orc, X[s], Gfull, M, lower, upper, bw))
        val = (X, np.stack(Gs), np.stack(outs))
        for a in val:
            a.flags.writeable = False
        _ORACLE[key] = val
    return _ORACLE[key]


def _check_against_oracle(what, X, Gg, got, Gref, ref, M, bw, guard=1e-2):
    """the bounds of tests/test_gpu_wpe.py for these sizes, per stream; outside the band: zero taps and the input bit for bit"""
    lo, up = cf.band(M, bw, FS)
    K = M // 2 + 1
    inactive = [k for k in range(K) if not cf.active(k, lo, up)]
    assert Gg.shape == Gref.shape and got.shape == ref.shape == X.shape
    for s in range(X.shape[0]):
        gscale = np.max(np.abs(Gref[s]))
        gerr, oerr = np.max(np.abs(Gg[s] - Gref[s])) / gscale, np.max(np.abs(got[s] - ref[s])) / np.max(np.abs(ref[s]))
        print("WPE %s stream %d: largest tap %.3g, tap error %.3g of it, output error %.3g of the largest sample" % (what, s, gscale, gerr, oerr))
        assert gscale > guard
        assert gerr <= 2e-3
        assert oerr <= 1e-3
        assert np.all(Gg[s][:, inactive] == 0)
        assert np.array_equal(_bits(got[s][inactive]), _bits(X[s][inactive]))
    if X.shape[0] > 1:
        assert np.max(np.abs(Gref[0] - Gref[1])) > 1e-2 * np.max(np.abs(Gref))


# (C, lower, upper, M, band_width): one per normal-equation family
C_CASES = [(8, 1, 10, 16, 3000.0),      # float16 lag products, panel solver by default
           (4, 0, 15, 16, 3000.0),      # float32 lag products
           (5, 1, 9, 16, 3000.0),       # herk32<1> plus strip, P = 45
           (2, 0, 5, 16, 3000.0),       # herk32<2>, vector prediction
           (8, 0, 13, 16, 3000.0),      # P = 112: the register solver by default.  (Bin 0 is real-valued: in the second iteration one
                                        # frame of one channel sits at the 1e-3 floor, weight 1e6.  With one float16 scale per bin for
                                        # the weights of all channels this case was 1.6e-2 off in the taps; per-channel scales: 2.7e-4.)
           (8, 1, 10, 64, 2000.0)]      # lo = 8 of K = 33 bins
C_T = 300


@pytest.mark.parametrize("C,lower,upper,M,bw", C_CASES)
def test_band_limited_estimate_and_apply(orc, dev, C, lower, upper, M, bw):
    X, Gref, ref = _oracle_case(orc, C, lower, upper, M, bw, C_T)
    Gg, got = _gpu_estimate_apply(dev, X, M, lower, upper, bw=bw)
    _check_against_oracle("band %g C=%d lags %d..%d M=%d" % (bw, C, lower, upper, M), X, Gg, got, Gref, ref, M, bw)


@pytest.mark.parametrize("C,lower,upper", [(8, 1, 10), (5, 1, 9)])
def test_band_width_at_nyquist_is_the_full_band(dev, C, lower, upper):
    from distant_speech_recognition_amd import _lib
    X = rounded_input(77, 1, C, M16, C_T)
    G0, Y0 = _gpu_estimate_apply(dev, X, M16, lower, upper, bw=0.0)
    G1, Y1 = _gpu_estimate_apply(dev, X, M16, lower, upper, bw=8000.0)
    assert np.max(np.abs(G0)) > 1e-2
    assert np.array_equal(_bits(G0), _bits(G1)) and np.array_equal(_bits(Y0), _bits(Y1))
    with pytest.raises(_lib.BtkError):
        _gpu_estimate_apply(dev, X, M16, lower, upper, bw=8001.0)
    with pytest.raises(_lib.BtkError):
        _gpu_apply(dev, X, G0, M16, lower, upper, bw=8001.0)


def test_band_limited_btk20_node_flow(orc, dev, proto256, kinect_pcm, wavs):  # noqa: F811
    """the flow of test_gpu_btk20_api.py::test_wpe_chain_flow with band_width = 3000 Hz (M = 256: lo = 48): the host node's own
    band rule, its zero-initialised filters outside the band, estimate and apply, against the oracle"""
    from distant_speech_recognition_amd.btk20 import (MultiChannelWPEDereverberationPtr, MultiChannelWPEDereverberationFeaturePtr,
                                                      OverSampledDFTSynthesisBankPtr)
    h, g = proto256
    M, m, r = API_M, 4, 1
    sample_feats, afbs = _build(wavs[:2], h)
    pre = MultiChannelWPEDereverberationPtr(subbands_num=M, channels_num=2, lower_num=0, upper_num=7, iterations_num=2,
                                            load_db=-18.0, band_width=3000.0, diagonal_bias=1e-4, samplerate=API_FS)
    for a in afbs:
        pre.set_input(a)
    assert pre.estimate_filter() == 317
    for c, p in enumerate(wavs[:2]):
        sample_feats[c].read(p, API_FS)
    sfbs = [OverSampledDFTSynthesisBankPtr(MultiChannelWPEDereverberationFeaturePtr(pre, channel_no=c), prototype=g, M=M, m=m, r=r,
                                           delay_compensation_type=2) for c in range(2)]
    bufs = [[], []]
    while True:
        try:
            for c in range(2):
                bufs[c].append(np.array(sfbs[c].next()))
        except StopIteration:
            break
    outs = [np.concatenate(b) for b in bufs]
    X = _oracle_X(orc, h, kinect_pcm)[:, :2]
    G = orc.wpe_estimate(X, 0, 7, 2, -18.0, 3000.0, 1e-4, API_FS)
    assert np.all(G[:, 49:208] == 0) and np.max(np.abs(G[:, :49])) > 1e-2
    Yd = orc.wpe_apply(X, G, 0, 7, 3000.0, API_FS)
    for c in range(2):
        ref = orc.synthesis(g, M, m, r, 2, Yd[:, c])
        assert outs[c].shape == ref.shape
        assert np.max(np.abs(outs[c] - ref)) < 1e-3 * np.max(np.abs(ref)) + 0.5
    # The recording has little energy above 3 kHz, so the PCM bound alone would pass a node that ignored the band: the node's
    # subband frames next to its own input (a fresh analysis of the same samples) -- outside the band the input, value for value.
    Yfull = orc.wpe_apply(X, orc.wpe_estimate(X, 0, 7, 2, -18.0, 0.0, 1e-4, API_FS), 0, 7, 0.0, API_FS)
    _, afbs2 = _build(wavs[:2], h)
    for c, p in enumerate(wavs[:2]):
        sample_feats[c].read(p, API_FS)
    pre.reset()
    chans = [MultiChannelWPEDereverberationFeaturePtr(pre, channel_no=c) for c in range(2)]
    frames = [[], []]
    while True:
        try:
            for c in range(2):
                frames[c].append(np.array(chans[c].next()))
        except StopIteration:
            break
    for c in range(2):
        got = np.array(frames[c])[:, :M // 2 + 1]
        Xin = np.array([np.array(f) for f in afbs2[c]])[:, :M // 2 + 1]
        assert got.shape == Xin.shape == (317, M // 2 + 1)
        assert np.array_equal(got[:, 49:], Xin[:, 49:])
        # (full-band filters would move these bins by 2.5e-3 / 3.9e-2 of their largest sample: far from value for value)
        assert np.max(np.abs(Yfull[:, c, 49:129] - Yd[:, c, 49:129])) > 1e-3 * np.max(np.abs(Yd[:, c, 49:129]))
        assert np.max(np.abs(got - Yd[:, c, :M // 2 + 1])) <= 1e-3 * np.max(np.abs(Yd[:, c]))


SOLVER_CASES = [c for c in C_CASES if c[0] == 8]
CHILD = r'''
import sys, numpy as np, torch
sys.path.insert(0, %r)
from distant_speech_recognition_amd import engine as eng
dev = torch.device("cuda:0")
inp = np.load(sys.argv[1])
out = {}
for i, (C, lo, up, M, bw) in enumerate(%r):
    X = torch.from_numpy(inp["X%%d" %% i]).to(dev)
    G = eng.wpe_estimate(X, M, lower_num=lo, upper_num=up, iterations_num=2, load_db=-18.0, band_width=bw, diagonal_bias=1e-4)
    Y = eng.wpe_apply(X, G, M, lower_num=lo, upper_num=up, band_width=bw)
    out["G%%d" %% i] = G.cpu().numpy(); out["Y%%d" %% i] = Y.cpu().numpy()
np.savez(sys.argv[2], **out)
'''


def test_band_limited_with_each_solver_forced(orc, dev, tmp_path):
    """the C = 8 cases of (c) with the panel solver forced, then with the register solver forced (the library reads the switches once
    per process: one child each, one after the other; a child that does not end cleanly fails the test before the next starts)"""
    refs = [_oracle_case(orc, C, lower, upper, M, bw, C_T) for (C, lower, upper, M, bw) in SOLVER_CASES]
    inp = str(tmp_path / "in.npz")
    np.savez(inp, **{"X%d" % i: ref[0] for i, ref in enumerate(refs)})
    for switch in ("BTK_WPE_SOLVE_PANEL", "BTK_WPE_SOLVE_REG"):
        env = dict(os.environ)
        env[switch] = "1"
        path = str(tmp_path / (switch + ".npz"))
        r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, SOLVER_CASES), inp, path], env=env, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 0, (switch, r.returncode, r.stderr[-2000:])
        res = np.load(path)
        for i, (C, lower, upper, M, bw) in enumerate(SOLVER_CASES):
            X, Gref, ref = refs[i]
            _check_against_oracle("%s band %g C=%d lags %d..%d M=%d" % (switch, bw, C, lower, upper, M), X, res["G%d" % i], res["Y%d" % i],
                                  Gref, ref, M, bw)


# (C, lower, upper, S)
D_CASES = [(6, 0, 6, 1),        # P = 42: herk32<2> plus the 16-row strip <2>
           (16, 1, 3, 1),       # P = 48: strip <4>
           (12, 0, 3, 1),       # P = 48: strip <4>
           (3, 0, 14, 1),       # P = 45: strip <1>
           (8, 1, 10, 3),       # K S = 27 bins: a ragged group of eight in the float16 lag-product launch
           (4, 0, 15, 2),       # float32 lag products, several streams
           (5, 1, 6, 2)]        # block HERK, several streams
D_T = 200


@pytest.mark.parametrize("C,lower,upper,S", D_CASES)
def test_branches_never_run_against_the_oracle(orc, dev, C, lower, upper, S):
    X, Gref, ref = _oracle_case(orc, C, lower, upper, M16, 0.0, D_T, S)
    Gg, got = _gpu_estimate_apply(dev, X, M16, lower, upper)
    _check_against_oracle("C=%d lags %d..%d S=%d" % (C, lower, upper, S), X, Gg, got, Gref, ref, M16, 0.0)


# ------------------------------------------------------------------------------------------------ (e): heavy loading
# Tolerance per case: 4 x the largest tap difference between the closed form in float32 and in float64 arithmetic (relative to the
# largest tap; tests/test_wpe_cpu.py measures and lists them), floor 1e-6 -- 1e-6 for the 0 dB and +10 dB cases, 2.3e-6 for two
# iterations at 0 dB, 2.0e-5 .. 2.8e-5 at -18 dB / bias 10, 1.8e-3 .. 1.0e-2 at -40 dB / bias 1e-2.
# Observed on an MI355X: 3.7e-7 .. 8.4e-7 at 0 / +10 dB, 1.2e-6 for two iterations, 9.5e-6 .. 1.4e-5 at -18 dB, 8.1e-4 .. 2.9e-3 at -40 dB.
@pytest.mark.parametrize("case", E_CASES, ids=lambda c: "C%d-%d_%d-%gdB-%g-it%d" % (c[0], c[1], c[2], c[4], c[5], c[6]))
def test_loading_rule_and_normal_equations(dev, case):
    C, lower, upper, T, load_db, bias, iters = case
    Gref, gscale, ratio, cond = e_reference(case)
    tol = e_tolerance(case)
    assert gscale > 1e-3
    if load_db >= 0:
        assert cond < 50                                                   # a condition on the inputs, computed on the CPU
    Gg, _ = _gpu_estimate_apply(dev, e_input(C, lower, upper, T), M16, lower, upper, iters=iters, load_db=load_db, bias=bias)
    err = float(np.max(np.abs(Gg - Gref))) / gscale
    print("WPE heavy loading %s: cond %.3g, float32/float64 of the closed form %.3g, tolerance %.3g, GPU tap error %.3g"
          % (case, cond, ratio, tol, err))
    assert err <= tol
