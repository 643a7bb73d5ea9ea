"""GPU parity of svd_rule = "linpack_full": the reference's float32 SVD pseudo-inverse itself (beamformer/beamformer.cc:232-289,
matrix/linpack_c.cc:9516 with job = 11) on the device.  btk_csvdc_full and btk_pinv_linpack bit for bit against the reference's
compiled csvdc (oracle/_ref; the serial g++ build of the same bodies stands in where it is absent) and the numpy restatement of the
assembly; the designs that use the rule against the float64 weight formula on that inverse."""
import os

import numpy as np
import pytest

from tests import linpack_full_host as lf
from tests import linpack_host as lh
from tests.test_linpack_full import dead_channel_matrices
from tests.util import la_delays, ula_positions

pytestmark = pytest.mark.gpu
GOLDEN_C5 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "c5_csvdc_info.npz")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _ref_full(orc, A):
    """(s, e, U, V, info) of the reference's csvdc, job = 11"""
    return lf.ref_csvdc_full(orc, A) if orc.ref_lib() is not None else lf.csvdc_full(A)


def _expected_bin(orc, Rk, d, threshold=1.0e-8):
    """(w complex128 [N], Lambda, ok, info): the float64 weight step (beamformer.cc:2386-2396) on the numpy-restated inverse
    (:262-280) of the reference's U, V, s -- the identity where pseudoinverse() returns false"""
    s, e, U, V, info = _ref_full(orc, Rk)
    inv, ok = lf.pinv_restated(s, U, V, info, threshold)
    w, lam = lf.mvdr_from_inverse(inv, ok, d)
    return w, lam, ok, info


def _same_full(got, want, i=None):
    s, e, U, V, info = got
    sr, er, ur, vr, ir = want
    assert int(info) == ir, (i, int(info), ir)
    assert np.array_equal(_bits(s), _bits(sr)) and np.array_equal(_bits(e), _bits(er)), i
    assert np.array_equal(_bits(U), _bits(ur)) and np.array_equal(_bits(V), _bits(vr)), i


def test_csvdc_full_bit_exact_all_test_matrices(orc, dev):
    """s, e, INFO, U and V of every test matrix -- tall, wide, rank deficient, zero columns -- equal the reference's to the last bit"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    by_shape = {}
    for A in lh.test_matrices():
        by_shape.setdefault(A.shape, []).append(A)
    for shape, group in by_shape.items():
        out = [x.cpu().numpy() for x in eng.csvdc_full(torch.from_numpy(np.stack(group)).to(dev))]
        for i, A in enumerate(group):
            _same_full([x[i] for x in out], _ref_full(orc, A), (shape, i))


def test_csvdc_full_large_batch_and_extreme_scales_same_bits(orc, dev):
    """A batch far beyond what is resident at once (K = 1100 of 40 x 40): the same bits as the same matrices in small batches and
    as the reference on a sample; matrices scaled by 2^-70 / 2^+70 / with tiny entries (the plain IEEE path of the wavefront's
    srotg) as well."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    rng = np.random.default_rng(5)
    K, N = 1100, 40
    A = (rng.standard_normal((K, N, N + 6)) + 1j * rng.standard_normal((K, N, N + 6)))
    R = (A @ np.conj(np.transpose(A, (0, 2, 1))) / (N + 6)).astype(np.complex64)
    R[7, :, 3] = 0; R[7, 3, :] = 0
    R[11] = np.diag(np.arange(1, N + 1)).astype(np.complex64)
    Rd = torch.from_numpy(R).to(dev)
    big = [x.cpu().numpy() for x in eng.csvdc_full(Rd)]
    for lo in range(0, K, 400):
        part = [x.cpu().numpy() for x in eng.csvdc_full(Rd[lo:lo + 400].contiguous())]
        for a, b in zip(big, part):
            assert np.array_equal(_bits(a[lo:lo + 400]), _bits(b)), lo
    for i in (0, 7, 11, 555, 1099):
        _same_full([x[i] for x in big], _ref_full(orc, R[i]), i)
    X = []
    for i, sc in enumerate((2.0 ** -70, 2.0 ** 70, 2.0 ** -100, 2.0 ** 40)):
        X.append((R[20 + i].astype(np.complex128) * sc).astype(np.complex64))
    Z = R[30].copy(); Z[:, 5] *= np.float32(2.0 ** -80); Z[5, :] *= np.float32(2.0 ** -80); X.append(Z)
    X = np.stack(X)
    out = [x.cpu().numpy() for x in eng.csvdc_full(torch.from_numpy(X).to(dev))]
    for i in range(len(X)):
        _same_full([x[i] for x in out], _ref_full(orc, X[i]), i)


def test_pinv_linpack_bit_exact(orc, dev):
    """engine.pinv_linpack against the numpy restatement of beamformer.cc:262-280 on the reference's U, V, s: every value equal,
    `ok` and INFO equal; every M >= N test matrix.  M < N is rejected."""
    import torch
    from distant_speech_recognition_amd import _lib, engine as eng
    by_shape = {}
    for A in lh.test_matrices():
        by_shape.setdefault(A.shape, []).append(A)
    for shape, group in by_shape.items():
        Ad = torch.from_numpy(np.stack(group)).to(dev)
        if shape[0] < shape[1]:
            with pytest.raises(_lib.BtkError):
                eng.pinv_linpack(Ad)
            continue
        inv, ok, info = [x.cpu().numpy() for x in eng.pinv_linpack(Ad)]
        for i, A in enumerate(group):
            s, e, U, V, ir = _ref_full(orc, A)
            want, wok = lf.pinv_restated(s, U, V, ir)
            assert int(info[i]) == ir and bool(ok[i]) == wok, (shape, i)
            assert np.all(inv[i] == want), (shape, i, float(np.max(np.abs(inv[i] - want))))


@pytest.mark.parametrize("N", [8, 64])
def test_dead_channel_in_the_middle_gets_the_reference_weights(orc, dev, N):
    """The stated deviation of the default rule is gone when "linpack_full" is selected: the bin with the dead channel in the
    middle gets the reference's weights (its inverse of sigma ~ 5e-8), only the one at the end takes the identity.  The default
    rule still returns the identity for both."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    from tests.test_gpu_postfilter_cov_mvdr import _oracle_mvdr_bin
    R, d = dead_channel_matrices(N)
    Rd, dd = torch.from_numpy(R).to(dev), torch.from_numpy(d).to(dev)
    W, nident = eng.mvdr_weights(Rd, dd, svd_rule="linpack_full")
    W = W.cpu().numpy()
    assert nident == 1 and eng.mvdr_weights.last_counts == (0, 1, 0)
    assert np.allclose(W[0], 1.0)
    if orc.ref_lib() is not None:
        w_ref = _oracle_mvdr_bin(orc, R[1].astype(np.complex128), d[1].astype(np.complex128))
    else:
        w_ref = _expected_bin(orc, R[1], d[1])[0]
    rel = np.linalg.norm(W[1] - w_ref) / np.linalg.norm(w_ref)
    print("\nN = %d, dead channel in the middle: || W - w_ref || / || w_ref || = %.3g" % (N, rel))
    assert rel <= 1e-6
    ident = d[2] / (N * np.vdot(d[2], d[2]))
    assert np.linalg.norm(W[2] - ident) <= 1e-6 * np.linalg.norm(ident)
    Wd, nd = eng.mvdr_weights(Rd, dd)                                   # the default rule: unchanged
    Wd = Wd.cpu().numpy()
    assert eng.svd_rule_default() == "linpack" and nd == 2
    for k in (1, 2):
        assert np.allclose(Wd[k], d[k] / (N * np.vdot(d[k], d[k])), atol=1e-6)


@pytest.mark.parametrize("N,M", [(4, 256), (8, 64), (64, 64), (100, 64), (140, 64)])
def test_diffuse_designs_match_the_restated_reference(orc, dev, N, M):
    """The designs of test_mvdr_weights_match_oracle: every bin, converging or identity, within 1e-6 of the float64 weight
    formula on the restated inverse of the reference's U, V, s (W is complex64; everything before the last rounding is the same
    float32 values and float64 sums).  Against the oracle (pairwise sums) only the existing 3e-3 holds; the distance is printed."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    from tests.test_gpu_postfilter_cov_mvdr import _oracle_mvdr_bin
    K = M // 2 + 1
    mpos = ula_positions(N, 20.0)
    mpos[:, 2] = 2.0
    wq = orc.calc_mainlobe(M, N, 16000, la_delays(mpos, -1.306379))[:K].astype(np.complex64)
    Rd = eng.mvdr_diffuse_model(mpos, M, 16000, device=dev)
    eng.mvdr_diagonal_loading(Rd, 0.01)
    W, nident = eng.mvdr_weights(Rd, torch.from_numpy(wq).to(dev), svd_rule="linpack_full")
    W, R = W.cpu().numpy(), Rd.cpu().numpy()
    assert np.allclose(W[0], 1.0)
    nbad, worst, dist = 0, 0.0, 0.0
    for k in range(1, K):
        w, lam, ok, info = _expected_bin(orc, R[k], wq[k])
        nbad += not ok
        rel = np.linalg.norm(W[k] - w) / np.linalg.norm(w)
        worst = max(worst, rel)
        assert rel <= 1e-6, (k, info, rel)
        if orc.ref_lib() is not None:
            ref = _oracle_mvdr_bin(orc, R[k].astype(np.complex128), wq[k].astype(np.complex128))
            dk = np.linalg.norm(W[k] - ref) / np.linalg.norm(ref)
            dist = max(dist, dk)
            assert dk <= (3e-3 if ok else 1e-6), (k, info, dk)
    assert nident == nbad and eng.mvdr_weights.last_counts[2] == 0
    print("\nN = %d: worst distance to the restated reference %.3g, to the oracle %.3g; %d identity bins" % (N, worst, dist, nbad))


def test_c5_weights_are_the_reference_weights(orc, dev):
    """BASELINE C5 (256 microphones, 1025 bins): 505 bins take the identity; the sampled bins of
    test_c5_weights_follow_the_reference_rule within 1e-6 of the restated reference, within the existing 2e-2 of the oracle."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    z = np.load(GOLDEN_C5)
    N, M = 256, 2048
    K = M // 2 + 1
    mpos = ula_positions(N, 20.0)
    wq = orc.calc_mainlobe(M, N, 16000, la_delays(mpos, 0.8))[:K].astype(np.complex64)
    R = orc.diagonal_loading(orc.diffuse_noise_model(mpos, M, 16000), M, 0.01).astype(np.complex64)
    W, nident = eng.mvdr_weights(torch.from_numpy(R).to(dev), torch.from_numpy(wq).to(dev), svd_rule="linpack_full")
    assert nident == 505 and eng.mvdr_weights.last_counts == (505, 0, 0)
    W = W.cpu().numpy()
    assert np.allclose(W[0], 1.0)
    bins = sorted(set(list(range(1, K, 37)) + [108, 109, 110, 160, 161, 641, 769, 770, 1024]))
    worst, dist, nid = 0.0, [], 0
    for k in bins:
        w, lam, ok, info = _expected_bin(orc, R[k], wq[k])
        assert info == int(z["info"][0, k])
        nid += not ok
        rel = np.linalg.norm(W[k] - w) / np.linalg.norm(w)
        worst = max(worst, rel)
        assert rel <= 1e-6, (k, info, rel)
        if orc.ref_lib() is not None and ok:
            inv, ok2 = orc.pseudoinverse(R[k].astype(np.complex128), 1.0e-8)
            ref = lf.mvdr_from_inverse(inv, ok2, wq[k])[0]
            dk = np.linalg.norm(W[k] - ref) / np.linalg.norm(ref)
            dist.append(dk)
            assert ok2 and dk <= 2e-2, (k, dk)
    assert nid >= 8
    print("\nC5 sampled bins: worst distance to the restated reference %.3g; to the oracle on converging bins: median %.3g, max %.3g"
          % (worst, float(np.median(dist)) if dist else 0.0, float(np.max(dist)) if dist else 0.0))


def test_stacked_streams_and_bin_ranges(orc, dev):
    """Stacked streams [S][K][N][N] equal the single-stream result; a first_bin > 0 slice equals the rows of the full call"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    rng = np.random.default_rng(3)
    N, K = 24, 9
    R = np.zeros((K, N, N), np.complex64)
    for k in range(K):
        B = rng.normal(size=(N, N + 4)) + 1j * rng.normal(size=(N, N + 4))
        R[k] = (B @ B.conj().T / N + 0.01 * np.eye(N)).astype(np.complex64)
    u = rng.normal(size=(N, 2)) + 1j * rng.normal(size=(N, 2))
    R[2] = (u @ u.conj().T).astype(np.complex64)                          # rank 2: under the threshold -> identity
    wq = np.exp(1j * rng.uniform(0, 6.28, size=(K, N))).astype(np.complex64)
    Rd, wd = torch.from_numpy(R).to(dev), torch.from_numpy(wq).to(dev)
    W, nid = eng.mvdr_weights(Rd, wd, 1e-4, svd_rule="linpack_full")
    assert nid == 1 and eng.mvdr_weights.last_counts == (0, 1, 0)
    W2, nid2 = eng.mvdr_weights(torch.stack([Rd, Rd]), torch.stack([wd, wd]), 1e-4, svd_rule="linpack_full")
    assert nid2 == 2 and torch.equal(W2[0], W) and torch.equal(W2[1], W)
    assert torch.all(W2[:, 0] == 1.0)
    Ws, nids = eng.mvdr_weights(Rd[2:6].contiguous(), wd[2:6].contiguous(), 1e-4, first_bin=2, svd_rule="linpack_full")
    assert nids == 1 and torch.equal(Ws, W[2:6])
    w, lam, ok, info = _expected_bin(orc, R[4], wq[4], 1e-4)
    assert np.linalg.norm(W[4].cpu().numpy() - w) <= 1e-6 * np.linalg.norm(w)


class _ZeroSource:
    def __init__(self, M):
        self._M = M

    def size(self):
        return self._M

    def __iter__(self):
        return self

    def next(self):
        raise StopIteration

    __next__ = next

    def reset(self):
        pass


def test_cpp_node_and_lefkimmiatis_lambda_take_the_new_rule(orc, dev):
    """SubbandMVDR (C++ node, pybind) with set_svd_rule("linpack_full") designs what engine.mvdr_weights designs from the same
    device-built model; an unknown rule still raises.  The Lefkimmiatis Lambda is d^H A+ d from the restated inverse on converging
    bins, d^H d on the others."""
    import torch
    from distant_speech_recognition_amd import btk20, engine as eng
    N, M = 140, 64
    K = M // 2 + 1
    mpos = ula_positions(N, 20.0)
    mpos[:, 2] = 2.0
    delays = la_delays(mpos, -1.306379)
    bf = btk20.SubbandMVDRPtr(fftlen=M, half_band_shift=False)
    src = btk20.PyVectorComplexFeatureStreamPtr(_ZeroSource(M))
    for c in range(N):
        bf.set_channel(src)
    bf.calc_array_manifold_vectors(16000.0, delays)
    bf.set_diffuse_noise_model(mpos, 16000.0, 343740.0)
    bf.set_all_diagonal_loading(0.01)
    bf.set_svd_rule("linpack_full")
    assert bf.svd_rule() == "linpack_full"
    bf.calc_mvdr_weights(16000.0, 1.0e-8, True)
    wq = orc.calc_mainlobe(M, N, 16000, delays)[:K].astype(np.complex64)
    Rd = eng.mvdr_diffuse_model(mpos, M, 16000, device=dev)
    eng.mvdr_diagonal_loading(Rd, 0.01)
    d = torch.from_numpy(wq).to(dev)
    W, nident = eng.mvdr_weights(Rd, d, svd_rule="linpack_full")
    W, R = W.cpu().numpy(), Rd.cpu().numpy()
    assert bf.identity_fallbacks() == nident and bf.csvdc_not_converged() == eng.mvdr_weights.last_counts[0]
    # the same device-built model, the same look direction, the same entry point: the same weights, and both the reference's
    for k in (1, 5, 16, 17, 32):
        w = _expected_bin(orc, R[k], wq[k])[0]
        wn = np.asarray(bf.mvdr_weights(k))
        assert np.array_equal(wn.astype(np.complex64), W[k]), k
        assert np.linalg.norm(wn - w) <= 1e-6 * np.linalg.norm(w), k
    with pytest.raises(Exception):
        bf.set_svd_rule("lapack")
    pf = eng.CoherencePostFilterState(1, K, N, dev, lefkimmiatis=True)
    nid = pf.set_lambda(Rd, d, svd_rule="linpack_full")
    lam = pf.lam.cpu().numpy()
    nbad = 0
    for k in range(K):                                                    # bin 0 is decomposed as well (postfilter.cc:971)
        w, lk, ok, info = _expected_bin(orc, R[k], wq[k])
        nbad += not ok
        want = lk if ok else np.vdot(wq[k].astype(np.complex128), wq[k].astype(np.complex128))
        assert abs(lam[k] - want) <= 1e-6 * abs(want), (k, ok)
    assert nid == nbad
