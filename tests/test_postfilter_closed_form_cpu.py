"""CPU: the oracle's Zelinski, McCowan and Lefkimmiatis post-filters pinned to the float64 closed forms of
tests/postfilter_closed_form.py (a statement of the reference's equations, pair by pair), known answers that need neither, and a
check that the acceptance rule of test_gpu_postfilter_closed_form.py rejects the faults it is there to catch.

Bound: 1e-12 relative.  Both sides are float64 evaluations of the same sums in another order; the pair weights 1 / (1 - R_ij) reach
1 / (1 - 0.99) = 100 and the terms they weight cancel to 1 / 100 of their size, which leaves about 1e4 * 2^-53 = 1e-12.
"""
import numpy as np
import pytest

from tests import closed_forms as cf
from tests import postfilter_closed_form as pf

TYPES = (0, 1, 2, 8, 10)
T_CPU = 12


def _full(Xe, M):
    """[K][..][T] -> [T][..][M] with the mirror bins, as the oracle takes snapshots and beamformer outputs."""
    K = Xe.shape[0]
    a = np.moveaxis(np.asarray(Xe, np.complex128), (0, -1), (-1, 0))
    full = np.zeros(a.shape[:-1] + (M,), np.complex128)
    full[..., :K] = a
    full[..., K:] = np.conj(full[..., M // 2 - 1:0:-1])
    return full


def _inputs(N, M, thr, real, seed=0):
    K = M // 2 + 1
    R, twins = pf.coherence(K, N, thr, seed=seed, real=real)
    d = pf.alignment(1, K, N, seed=seed)
    X = pf.snapshots(d, T_CPU, twins, seed=seed)[0]
    w = cf.unit_weights(1, K, N, seed=seed)[0]
    return R, d[0], X, pf.beamform(w, X)


def _oracle_lambda(orc, R, d, min_sv=1.0e-8):
    """d^H pinv(R_k) d with the identity where pseudoinverse() returns false (postfilter.cc:967-994)."""
    lam = np.zeros(R.shape[0], np.complex128)
    for k in range(R.shape[0]):
        inv, ok = orc.pseudoinverse(R[k].astype(np.complex128), min_sv)
        inv = inv if ok else np.eye(R.shape[1])
        lam[k] = np.vdot(np.conj(inv.T) @ d[k].astype(np.complex128), d[k].astype(np.complex128))
    return lam


def _close(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    scale = max(1.0, float(np.nanmax(np.abs(want))))
    err = float(np.nanmax(np.abs(got - want))) / scale
    assert err <= 1e-12, (what, err)
    return err


@pytest.mark.parametrize("M", [8, 16])
@pytest.mark.parametrize("N", [2, 5, 17, 33])
def test_oracle_zelinski_equals_closed_form(orc, N, M):
    K = M // 2 + 1
    _, d, X, y = _inputs(N, M, 0.99, False)
    Xo, yo, do = _full(X, M), _full(y, M), _full(d[..., None], M)[0].T
    worst = 0.0
    for type_ in TYPES:
        for alpha in (0.0, 0.7):
            for minf in (0, 3, T_CPU + 5):
                ref, Wref = orc.zelinski_frames(Xo, yo, do, alpha, type_, minf)
                W, out, _ = pf.zelinski(X, d, y, alpha, type_, minf)
                what = (type_, alpha, minf)
                worst = max(worst, _close(Wref[:, :K].real.T, W, what), _close(ref[:, :K].T, out, what))
                assert np.array_equal(out != y, (pf.applied(T_CPU, minf) & (type_ != 0))[None, :] & (W != 1.0)), what
    print("zelinski N=%d M=%d worst %.2e" % (N, M, worst))


@pytest.mark.parametrize("M", [8, 16])
@pytest.mark.parametrize("N", [2, 5, 17, 33])
def test_oracle_mccowan_equals_closed_form(orc, N, M):
    K = M // 2 + 1
    worst = 0.0
    for thr in (0.99, 0.5):
        for real in (False, True):
            R, d, X, y = _inputs(N, M, thr, real)
            Xo, yo, do = _full(X, M), _full(y, M), _full(d[..., None], M)[0].T
            for type_ in TYPES:
                for alpha in (0.0, 0.7):
                    for minf in (0, 3, T_CPU + 5):
                        ref, Wref = orc.mccowan_frames(Xo, yo, do, R, alpha=alpha, type_=type_, min_frames=minf, threshold=thr)
                        W, out, _ = pf.mccowan(X, d, y, R, alpha, type_, minf, thr)
                        what = (thr, real, type_, alpha, minf)
                        worst = max(worst, _close(Wref[:, :K].real.T, W, what), _close(ref[:, :K].T, out, what))
                        # the gain is applied by the frame count alone, type 0 and 8 included
                        assert np.array_equal(out != y, pf.applied(T_CPU, minf)[None, :] & (W != 1.0)), what
    print("mccowan N=%d M=%d worst %.2e" % (N, M, worst))


@pytest.mark.parametrize("M", [8, 16])
@pytest.mark.parametrize("N", [2, 5, 17, 33])
def test_oracle_lefkimmiatis_equals_closed_form(orc, N, M):
    K = M // 2 + 1
    worst = 0.0
    for thr in (0.99, 0.5):
        for real in (False, True):
            R, d, X, y = _inputs(N, M, thr, real)
            Xo, yo, do = _full(X, M), _full(y, M), _full(d[..., None], M)[0].T
            lam = _oracle_lambda(orc, R, d)
            # every value of every parameter and every pair of (type, alpha); the oracle inverts R anew in each call
            for i, (type_, alpha) in enumerate((t, a) for t in TYPES for a in (0.0, 0.7)):
                minf, x1 = (0, 3, T_CPU + 5)[i % 3], (0, 3, K)[(i // 3 + i) % 3]
                ref, Wref = orc.lefkimmiatis_frames(Xo, yo, do, R, fbin_x1=x1, alpha=alpha, type_=type_, min_frames=minf, threshold=thr)
                W, out, _ = pf.lefkimmiatis(X, d, y, R, lam, x1, alpha, type_, minf, thr)
                what = (thr, real, type_, alpha, minf, x1)
                worst = max(worst, _close(Wref[:, :K].real.T, W, what), _close(ref[:, :K].T, out, what))
    print("lefkimmiatis N=%d M=%d worst %.2e" % (N, M, worst))


def test_stream_in_blocks_equals_the_stream_whole_and_resets_restart_the_history():
    N, K, S, T = 5, 5, 2, 40
    R, twins = pf.coherence(K, N, 0.99)
    d = pf.alignment(S, K, N)
    X = pf.snapshots(d, T, twins)
    y = pf.beamform(cf.unit_weights(S, K, N), X)
    lam = np.linspace(2.0, 4.0, K) * (1.0 + 0.3j)
    for f, extra in ((pf.zelinski, ()), (pf.mccowan, (R,)), (pf.lefkimmiatis, (R, lam, 3))):
        W, out, st = f(X, d, y, *extra, 0.7, 1, 3, resets=(17,))
        parts, state = [], None
        for a, b in ((0, 1), (1, 2), (2, 17), (17, 40)):
            w, o, state = f(X[..., a:b], d, y[..., a:b], *extra, 0.7, 1, 3, frame_base=a, state=state, resets=(17,))
            parts.append((w, o))
        # (numpy's strided and contiguous loops round a complex product differently: a few ulps, not bit equality)
        assert np.max(np.abs(np.concatenate([p[0] for p in parts], -1) - W)) <= 1e-14
        assert np.max(np.abs(np.concatenate([p[1] for p in parts], -1) - out)) <= 1e-14 * np.max(np.abs(out))
        assert all(np.max(np.abs(state[k] - st[k])) <= 1e-14 * np.max(np.abs(st[k])) for k in st)
        # a reset at frame 17 = a new filter fed from frame 17 on whose counter starts at 17
        w2, _, _ = f(X[..., 17:], d, y[..., 17:], *extra, 0.7, 1, 3, frame_base=17)
        assert np.max(np.abs(w2 - W[..., 17:])) <= 1e-14
        assert np.max(np.abs(f(X, d, y, *extra, 0.7, 1, 3)[0][..., 17:] - W[..., 17:])) > 1e-3


def test_float32_forms_keep_their_types_and_stay_close():
    N, K, S, T = 8, 5, 2, 40
    R, twins = pf.coherence(K, N, 0.5)
    d = pf.alignment(S, K, N)
    X = pf.snapshots(d, T, twins)
    w = cf.unit_weights(S, K, N)
    y, y32 = pf.beamform(w, X), pf.beamform(w, X, np.float32)
    assert y32.dtype == np.complex64 and 1e-9 < cf.e_max(y32, y) < 2e-6
    lam = np.full(K, 3.0 + 1.0j)
    for f, extra in ((pf.zelinski, ()), (pf.mccowan, (R,)), (pf.lefkimmiatis, (R, lam, 3))):
        W, out, _ = f(X, d, y, *extra, 0.7, 2, 0)
        W32, out32, st32 = f(X, d, y32, *extra, 0.7, 2, 0, dtype=np.float32)
        assert W32.dtype == np.float32 and out32.dtype == np.complex64 and st32["phi"].dtype == np.complex64
        assert 1e-9 < cf.e_max(W32, W) < 5e-6 and 1e-9 < cf.e_max(out32, out) < 5e-6


# ---- known answers ------------------------------------------------------------------------------------------------
def _zelinski_both(orc, X, d, y, alpha, type_):
    """closed form and oracle gains [K][T] of one stream; M = 2 (K - 1)."""
    K = X.shape[0]
    M = 2 * (K - 1)
    W = pf.zelinski(X, d, y, alpha, type_, 0)[0]
    Wo = orc.zelinski_frames(_full(X, M), _full(y, M), _full(d[..., None], M)[0].T, alpha, type_, 0)[1]
    return W, Wo[:, :K].real.T


@pytest.mark.parametrize("N", [2, 3, 5, 9])
def test_one_coherent_source_gives_gain_one(orc, N):
    """N identical aligned channels: every phi_ij equals every phi_ii, W = (N (N - 1) / 2) / N * 2 / (N - 1) = 1.  Integer-valued
    samples and alignment entries from {1, -1, j, -j}: every sum is exact, and so is 2 / (N - 1) for these N."""
    K, T = 5, 9
    rng = np.random.default_rng(N)
    s = rng.integers(-2000, 2000, (K, 1, T)) + 1j * rng.integers(-2000, 2000, (K, 1, T))
    s[s == 0] = 1.0
    d = (1j ** rng.integers(0, 4, (K, N))).astype(np.complex128)
    X = d[..., None] * s
    y = X[:, 0]
    for alpha in (0.0, 0.5):
        for type_ in (1, 2):
            for W in _zelinski_both(orc, X, d, y, alpha, type_):
                assert np.all(W == 1.0), (alpha, type_)


def test_independent_channels_drive_the_gain_to_the_floor(orc):
    """Mutually independent channels: the cross densities average out, the auto densities do not; the gain falls as the
    averaging gets longer, about sqrt(2 / (N (N - 1))) / sqrt((1 + a) / (1 - a)) for |.| and less for Re."""
    K, N = 3, 8
    rng = np.random.default_rng(3)
    d = np.ones((K, N), np.complex128)
    med = []
    for alpha, T in ((0.0, 50), (0.9, 200), (0.99, 1500)):
        X = rng.normal(size=(K, N, T)) + 1j * rng.normal(size=(K, N, T))
        W = pf.zelinski(X, d, X[:, 0], alpha, 2, 0)[0]
        med.append(float(np.median(W[:, T // 2:])))
    assert med[0] > 3 * med[1] > 9 * med[2] and med[2] < 0.02
    X = rng.normal(size=(K, N, 400)) + 1j * rng.normal(size=(K, N, 400))
    W, Wo = _zelinski_both(orc, X, d, X[:, 0], 0.99, 1)
    assert np.mean(W[:, 200:] == pf.SPECTRAL_FLOOR) > 0.3 and np.array_equal(W == pf.SPECTRAL_FLOOR, Wo == pf.SPECTRAL_FLOOR)


@pytest.mark.parametrize("type_", [1, 2])
def test_mccowan_with_zero_coherence_is_zelinski(orc, type_):
    N, K, T = 6, 5, 30
    d = pf.alignment(1, K, N)
    X = pf.snapshots(d, T)[0]
    y = pf.beamform(cf.unit_weights(1, K, N)[0], X)
    R = np.broadcast_to(np.eye(N, dtype=np.complex128), (K, N, N)).copy()
    # min_frames = -1: Zelinski takes |.| in a frame with frame_no_ < min_frames, the first one for min_frames = 0
    Wz, oz, _ = pf.zelinski(X, d[0], y, 0.7, type_, -1)
    Wm, om, _ = pf.mccowan(X, d[0], y, R, 0.7, type_, -1)
    assert np.max(np.abs(Wz - Wm)) <= 1e-14 and np.max(np.abs(oz - om)) <= 1e-14 * np.max(np.abs(oz))
    M = 2 * (K - 1)
    Wo = orc.mccowan_frames(_full(X, M), _full(y, M), _full(d[0][..., None], M)[0].T, R, alpha=0.7, type_=type_, min_frames=-1)[1]
    assert np.max(np.abs(Wo[:, :K].real.T - Wz)) <= 1e-14


# ---- conditions on the inputs the GPU tests use ---------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 7, 16, 33])
@pytest.mark.parametrize("thr", [0.99, 0.5])
def test_inputs_reach_every_clip_branch_and_leave_the_gains_off_the_clamps(N, thr):
    K, S, T = 5, 2, 80
    R, twins = pf.coherence(K, N, thr)                        # asserts the four clip branches itself
    Rr, _ = pf.coherence(K, N, thr, real=True)
    assert not np.any(Rr.imag)
    d = pf.alignment(S, K, N)
    X = pf.snapshots(d, T, twins)
    y = pf.beamform(cf.unit_weights(S, K, N), X)
    lam = np.full(K, 2.0 + 1.0j)
    Wz = pf.zelinski(X, d, y, 0.7, 2, 0)[0]
    assert 0.55 < np.mean(Wz) < 0.95 and pf.clamp_share(Wz) < 0.25
    for W in (pf.mccowan(X, d, y, R, 0.7, 2, 0, thr)[0], pf.lefkimmiatis(X, d, y, R, lam, 3, 0.7, 2, 0, thr)[0]):
        assert pf.clamp_share(W) <= 0.5 and 0.3 < np.mean(W) < 0.97


# ---- the acceptance rule has teeth ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teeth():
    N, K, S, T = 8, 5, 2, 80
    R, twins = pf.coherence(K, N, 0.99)
    d = pf.alignment(S, K, N)
    X = pf.snapshots(d, T, twins)
    w = cf.unit_weights(S, K, N)
    return dict(N=N, K=K, T=T, R=R, d=d, X=X, y=pf.beamform(w, X), y32=pf.beamform(w, X, np.float32),
                lam=np.linspace(2.0, 3.0, K) * (1.0 + 0.5j))


def _rows(a):
    return a.reshape(-1, a.shape[-1])


def _rejects(f, t, extra, kw, mutant_kw, pick, type_=2, minf=3):
    """accept() passes the float32 yardstick itself and rejects the float32 evaluation of a mutant; pick 0 = gains, 1 = output."""
    want = f(t["X"], t["d"], t["y"], *extra, 0.7, type_, minf, **kw)[pick]
    y32 = f(t["X"], t["d"], t["y32"], *extra, 0.7, type_, minf, dtype=np.float32, **kw)[pick]
    args = dict(kw, **mutant_kw)
    minf2 = args.pop("min_frames", minf)
    bad = f(t["X"], t["d"], t["y32"], *extra, 0.7, type_, minf2, dtype=np.float32, **args)[pick]
    assert pf.clamp_share(f(t["X"], t["d"], t["y"], *extra, 0.7, type_, minf, **kw)[0]) <= 0.5
    ok, fig = cf.accept(_rows(y32), _rows(y32), _rows(want))
    assert ok and fig["ratio"] <= 1.0
    ok, fig = cf.accept(_rows(bad), _rows(y32), _rows(want))
    print(mutant_kw, fig)
    assert not ok and fig["ratio"] > 10 * cf.FACTOR


def test_rule_rejects_memory_from_the_second_frame(teeth):
    _rejects(pf.zelinski, teeth, (), {}, dict(mutant="memory_from_second_frame"), 0)
    _rejects(pf.mccowan, teeth, (teeth["R"],), {}, dict(mutant="memory_from_second_frame"), 0)


def test_rule_rejects_a_dropped_pair(teeth):
    assert teeth["N"] == 8
    _rejects(pf.zelinski, teeth, (), {}, dict(mutant="drop_pair"), 0)
    _rejects(pf.mccowan, teeth, (teeth["R"],), {}, dict(mutant="drop_pair"), 0)


def test_rule_rejects_a_clean_psd_clip_without_the_imaginary_part_test(teeth):
    _rejects(pf.mccowan, teeth, (teeth["R"],), {}, dict(mutant="clean_clip_ignores_imag"), 0)


def test_rule_rejects_a_noise_psd_clip_that_keeps_the_imaginary_part(teeth):
    _rejects(pf.lefkimmiatis, teeth, (teeth["R"], teeth["lam"], teeth["K"]), {}, dict(mutant="noise_clip_keeps_imag"), 0)
    _rejects(pf.lefkimmiatis, teeth, (teeth["R"], teeth["lam"], 3), {}, dict(mutant="noise_clip_keeps_imag"), 0)


def test_rule_rejects_min_frames_off_by_one(teeth):
    _rejects(pf.zelinski, teeth, (), {}, dict(min_frames=4), 1)
    _rejects(pf.mccowan, teeth, (teeth["R"],), {}, dict(min_frames=2), 1)
    _rejects(pf.zelinski, teeth, (), {}, dict(min_frames=4), 0, type_=1)      # |.| below min_frames, Re from there on


def test_rule_rejects_a_lost_scan_carry(teeth):
    for f, extra in ((pf.zelinski, ()), (pf.mccowan, (teeth["R"],)), (pf.lefkimmiatis, (teeth["R"], teeth["lam"], 3))):
        _rejects(f, teeth, extra, {}, dict(resets=(64,)), 0)


def test_rule_rejects_mccowan_without_gain_for_type_8(teeth):
    _rejects(pf.mccowan, teeth, (teeth["R"],), {}, dict(mutant="no_gain_for_type0"), 1, type_=8)
