"""CPU: the oracle's analysis and synthesis banks pinned to the numpy.fft closed forms of tests/closed_forms.py,
known answers that go through neither restatement, and a check that the acceptance rule of test_gpu_fused_closed_form.py
rejects the faults it is there to catch -- also at the one-channel [K][T] shape of test_gpu_analysis_closed_form.py and the
[blocks][D] shape of test_gpu_synthesis_closed_form.py, where it must accept a second correct float32 evaluation as well.

Bounds (derived, not tuned):
  analysis   1e-13 max|X|: two float64 FFT algorithms differ by a few eps log2 M (measured <= 1.7e-15 over the sweep below).
  synthesis  R 2^-23 max|out|: the oracle returns float32 after a float32 running sum of R terms (measured <= 0.47 of the bound).
"""
import numpy as np
import pytest

from tests import closed_forms as cf
from tests.util import design_prototype

GEOMS = [(M, m) for M in (64, 128, 256, 512, 1024, 2048) for m in (2, 3, 4)]


def _lengths(M, m, r):
    D = M >> r
    return (0, 1, D - 1, D, D + 1, (3 * m * M // 2 + 37) if M <= 512 else (m * M + D + 3))


def _protos(M, m):
    return (("dense", cf.dense_prototype(M, m)), ("shipped", design_prototype(M, m)))


@pytest.mark.parametrize("M,m", GEOMS)
def test_delay_rule_and_frame_count(orc, M, m):
    for r in (0, 1, 2):
        for dct in (0, 1, 2):
            for syn in (False, True):
                assert cf.fb_delays(m, r, syn, dct) == orc.fb_delays(m, r, syn, dct)
            for L in _lengths(M, m, r):
                assert cf.num_frames(L, M, m, r, dct) == orc.analysis_num_frames(L, M, m, r, dct)


@pytest.mark.parametrize("M,m", GEOMS)
def test_oracle_analysis_equals_closed_form(orc, M, m):
    for r in (0, 1, 2):
        for dct in (0, 1, 2):
            for name, h in _protos(M, m):
                for L in _lengths(M, m, r):
                    x = cf.int_pcm(1, 1, L, seed=L + r)[0, 0]
                    a = orc.analysis(h, M, m, r, dct, x)
                    b = cf.analysis_cf(h, M, m, r, dct, x)
                    assert a.shape == b.shape == (cf.num_frames(L, M, m, r, dct), M), (r, dct, name, L)
                    if b.size:
                        assert np.max(np.abs(a - b)) <= 1e-13 * np.max(np.abs(b)), (r, dct, name, L)


@pytest.mark.parametrize("M,m", GEOMS)
def test_oracle_synthesis_equals_closed_form(orc, M, m):
    rng = np.random.default_rng(M + m)
    for r in (0, 1, 2):
        for dct in (0, 1, 2):
            pd, _ = cf.fb_delays(m, r, True, dct)
            for name, g in (("dense", cf.dense_prototype(M, m, seed=1)), ("shipped", design_prototype(M, m, "g"))):
                for T in (1, pd, pd + 1, pd + 2, pd + 19):
                    Y = rng.normal(size=(T, M)) + 1j * rng.normal(size=(T, M))
                    a = orc.synthesis(g, M, m, r, dct, Y)
                    b = cf.synthesis_cf(g, M, m, r, dct, Y)
                    assert a.shape == b.shape == (max(T - pd, 0) * (M >> r),), (r, dct, name, T)
                    if b.size:
                        assert np.max(np.abs(a - b)) <= (1 << r) * 2.0 ** -23 * np.max(np.abs(b)), (r, dct, name, T)


def test_float32_forms_keep_their_types_and_stay_close():
    M, m, r, dct, N = 512, 4, 1, 2, 3
    h = cf.dense_prototype(M, m)
    pcm = cf.int_pcm(1, N, cf.num_samples(20, M, m, r, dct) + 5, seed=1)[0]
    W = cf.unit_weights(1, M // 2 + 1, N)[0]
    Y32, Y = cf.plain_f32(h, M, m, r, dct, pcm, W), cf.fused_cf(h, M, m, r, dct, pcm, W)
    assert Y32.dtype == np.complex64 and Y.dtype == np.complex128 and Y32.shape == Y.shape
    assert 1e-8 < cf.e_max(Y32, Y) < 2e-6                    # float32 arithmetic, not float64 and not broken
    X = np.stack([cf.analysis_cf(h, M, m, r, dct, pcm[n]) for n in range(N)], axis=1)                  # [T][N][M]
    assert np.max(np.abs(cf.beamform_cf(W, X) - Y)) <= 1e-14 * np.max(np.abs(Y))
    Yf = cf.hermitian(Y, M)
    g = cf.dense_prototype(M, m, seed=1)
    o32, o = cf.synthesis_f32(g, M, m, r, dct, Yf), cf.synthesis_cf(g, M, m, r, dct, Yf)
    assert o32.dtype == np.float32 and o32.shape == o.shape and 1e-8 < cf.e_max(o32, o) < 2e-6


# ---- known answers that use neither restatement ---------------------------------------------------------------------
def _impls(orc):
    return (("oracle", orc.analysis), ("closed form", cf.analysis_cf))


@pytest.mark.parametrize("M,m,r,dct", [(512, 4, 1, 2), (256, 4, 2, 0), (64, 2, 0, 1), (128, 3, 1, 2)])
def test_complex_exponential_lands_in_plus_kappa(orc, M, m, r, dct):
    """x = exp(j 2 pi kappa n / M) through an all-ones prototype: X_t[kappa] = m M exp(j 2 pi kappa n_t / M), every other bin 0 --
    in particular bin M - kappa (the FFT's direction).  The banks take real samples: cos and sin go in separately."""
    D, kappa = M >> r, 5
    _, la = cf.fb_delays(m, r, False, dct)
    L = 3 * m * M
    n = np.arange(L)
    h = np.ones(m * M)
    for name, f in _impls(orc):
        X = f(h, M, m, r, dct, np.cos(2 * np.pi * kappa * n / M).astype(np.float32)) \
            + 1j * f(h, M, m, r, dct, np.sin(2 * np.pi * kappa * n / M).astype(np.float32))
        ts = [t for t in range(X.shape[0]) if m * M - 1 <= (t + la + 1) * D - 1 < L]      # window inside the recording
        assert len(ts) >= 2 * m
        for t in ts:
            nt = (t + la + 1) * D - 1
            want = np.zeros(M, np.complex128)
            want[kappa] = m * M * np.exp(2j * np.pi * ((kappa * nt) % M) / M)
            assert np.max(np.abs(X[t] - want)) <= 1e-5 * m * M, (name, t)                # float32 samples of cos / sin


@pytest.mark.parametrize("M,m,r,dct", [(512, 4, 1, 2), (256, 4, 0, 2), (64, 2, 2, 0)])
def test_constant_input_gives_c_times_sum_of_taps(orc, M, m, r, dct):
    D, c = M >> r, 1234.0
    _, la = cf.fb_delays(m, r, False, dct)
    L = 3 * m * M
    for pname, h in _protos(M, m):
        for name, f in _impls(orc):
            X = f(h, M, m, r, dct, np.full(L, c, np.float32))
            ts = [t for t in range(X.shape[0]) if m * M - 1 <= (t + la + 1) * D - 1 < L]
            assert ts
            for t in ts:
                assert abs(X[t, 0] - c * np.sum(h)) <= 1e-12 * c * np.sum(np.abs(h)), (name, pname, t)   # no 1/M


@pytest.mark.parametrize("M,m,r,dct", [(512, 4, 1, 2), (512, 4, 2, 0), (256, 4, 1, 2), (64, 2, 0, 1), (128, 3, 2, 2)])
def test_unit_impulse_reads_the_prototype_back(orc, M, m, r, dct):
    """x = delta(n - n0): frame t sees tap l = n_t - n0 alone, X_t[q] = h[l] exp(j 2 pi q l / M) (n_t, tap order, frame count)."""
    D = M >> r
    pd, la = cf.fb_delays(m, r, False, dct)
    h = cf.dense_prototype(M, m)
    L = 2 * m * M + 17
    q = np.arange(M)
    for n0 in (0, 1, D - 1, m * M + 3, L - 1):
        x = np.zeros(L, np.float32)
        x[n0] = 1.0
        for name, f in _impls(orc):
            X = f(h, M, m, r, dct, x)
            assert X.shape[0] == -(-L // D) - la + pd
            seen = 0
            for t in range(X.shape[0]):
                l = (t + la + 1) * D - 1 - n0
                want = h[l] * np.exp(2j * np.pi * ((q * l) % M) / M) if 0 <= l < m * M else np.zeros(M)
                seen += 0 <= l < m * M
                assert np.max(np.abs(X[t] - want)) <= 1e-12, (name, n0, t)
            assert seen >= 1


# ---- the acceptance rule has teeth ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def teeth():
    M, m, r, dct, N, T = 512, 4, 1, 2, 64, 48
    pcm = cf.int_pcm(1, N, cf.num_samples(T, M, m, r, dct), seed=5)[0]
    W = cf.unit_weights(1, M // 2 + 1, N, seed=1)[0]
    out = {}
    for name, h in _protos(M, m):
        Ycf = cf.fused_cf(h, M, m, r, dct, pcm, W)
        assert Ycf.shape == (M // 2 + 1, T)
        out[name] = (h, Ycf, cf.plain_f32(h, M, m, r, dct, pcm, W))
    return (M, m, r, dct, pcm, W), out


@pytest.mark.parametrize("proto,tap", [("dense", 0), ("dense", 1), ("dense", 2047), ("shipped", 1), ("shipped", 2047)])
def test_rule_rejects_a_dropped_tap(teeth, proto, tap):
    (M, m, r, dct, pcm, W), d = teeth
    h, Ycf, Y32 = d[proto]
    ok, fig = cf.accept(Y32, Y32, Ycf)
    assert ok and fig["ratio"] <= 1.0                         # the yardstick passes its own rule
    h2 = h.copy()
    assert h2[tap] != 0.0
    h2[tap] = 0.0
    ok, fig = cf.accept(cf.fused_cf(h2, M, m, r, dct, pcm, W), Y32, Ycf)
    print(proto, tap, fig)
    assert not ok and fig["e_max"] > 10 * cf.FACTOR * fig["y_max"]


@pytest.mark.parametrize("proto", ["dense", "shipped"])
def test_rule_rejects_wrong_channel_bin_and_frame(teeth, proto):
    (M, m, r, dct, pcm, W), d = teeth
    h, Ycf, Y32 = d[proto]
    W2 = W.copy()
    W2[100, [3, 4]] = W2[100, [4, 3]]                          # two channels' weights swapped in one bin
    ok, fig = cf.accept(cf.fused_cf(h, M, m, r, dct, pcm, W2), Y32, Ycf)
    assert not ok and fig["bad_rows"] == [100]
    Y2 = Ycf.copy()
    Y2[256] = np.conj(Y2[256])                                 # bin 256 conjugated
    ok, fig = cf.accept(Y2, Y32, Ycf)
    assert not ok and fig["bad_rows"] == [256]
    Y3 = Ycf.copy()
    Y3[:, 16:32] = Ycf[:, 17:33]                               # frame t replaced by t + 1 in one tile
    assert not cf.accept(Y3, Y32, Ycf)[0]
    Y4 = Ycf.astype(np.complex64).astype(np.complex128)
    Y4[7, 3] += 40 * cf.FLOOR * np.max(np.abs(Ycf))           # one bad value in a quiet place
    assert not cf.accept(Y4, Y32, Ycf)[0]


# ---- ... and at the shapes of test_gpu_analysis_closed_form.py / test_gpu_synthesis_closed_form.py: one channel, [K][T] ---------
REJECT = 10 * cf.FACTOR                                       # loose floor under every seeded fault's ratio; the smallest measured is 176 (shipped tap 1, M = 2048)
ANA_TEETH = [(512, 4, 1), (256, 4, 2), (2048, 4, 1), (64, 2, 1)]
SYN_TEETH = [(512, 4, 0), (512, 4, 2), (128, 3, 1)]


def _analysis_f32_again(h, M, m, r, dct, x):
    """A second correct float32 evaluation: taps summed in reverse order, float64 FFT rounded to complex64."""
    _, la = cf.fb_delays(m, r, False, dct)
    w = (cf._windows(x, cf.num_frames(len(x), M, m, r, dct), M, m, r, la, np.float32) * np.asarray(h, np.float32)[None, :]).reshape(-1, m, M)
    p = w[:, m - 1]
    for k in range(m - 2, -1, -1):
        p = p + w[:, k]
    assert p.dtype == np.float32
    return (np.fft.ifft(p.astype(np.float64), axis=1) * M).astype(np.complex64)


@pytest.fixture(scope="module", params=ANA_TEETH, ids=lambda g: "M%d-m%d-r%d" % g)
def ana_teeth(request):
    M, m, r = request.param
    dct, T, K = 2, 40, M // 2 + 1
    pcm = cf.int_pcm(1, 2, cf.num_samples(T, M, m, r, dct), seed=8)[0]
    out = {}
    for name, h in _protos(M, m):
        out[name] = (h, [cf.analysis_cf(h, M, m, r, dct, x)[:, :K].T for x in pcm],
                     [np.ascontiguousarray(cf.analysis_f32(h, M, m, r, dct, x)[:, :K].T) for x in pcm])
        assert out[name][1][0].shape == (K, T)
    return (M, m, r, dct, K, pcm), out


@pytest.mark.parametrize("proto", ["dense", "shipped"])
def test_analysis_rule_rejects_a_dropped_tap(ana_teeth, proto):
    (M, m, r, dct, K, pcm), d = ana_teeth
    h, Xcf, X32 = d[proto]
    ok, fig = cf.accept(X32[0], X32[0], Xcf[0])
    assert ok and fig["ratio"] <= 1.0
    for tap in ((0, 1, m * M - 1) if proto == "dense" else (1,)):
        h2 = h.copy()
        assert h2[tap] != 0.0
        h2[tap] = 0.0
        ok, fig = cf.accept(cf.analysis_cf(h2, M, m, r, dct, pcm[0])[:, :K].T, X32[0], Xcf[0])
        print("TEETH analysis M=%d m=%d r=%d %s tap %d dropped: ratio %.1f" % (M, m, r, proto, tap, fig["ratio"]))
        assert not ok and fig["ratio"] > REJECT


@pytest.mark.parametrize("proto", ["dense", "shipped"])
def test_analysis_rule_rejects_late_frame_swapped_channels_and_shifted_shard(ana_teeth, proto):
    (M, m, r, dct, K, pcm), d = ana_teeth
    h, Xcf, X32 = d[proto]
    late = Xcf[0].copy()
    late[:, 5] = cf.analysis_cf(h, M, m, r, dct, np.append(pcm[0][1:], 0.0))[5, :K]                  # frame 5 taken one sample late
    swapped = Xcf[1]                                                                              # the other channel's snapshots
    k0, k1 = K // 3, K // 3 + 7
    for what, Y, Y32, Ycf in (("frame late", late, X32[0], Xcf[0]), ("channels swapped", swapped, X32[0], Xcf[0]),
                              ("shard one row off", Xcf[0][k0 + 1:k1 + 1], X32[0][k0:k1], Xcf[0][k0:k1])):
        ok, fig = cf.accept(Y, Y32, Ycf)
        print("TEETH analysis M=%d m=%d r=%d %s %s: ratio %.3g" % (M, m, r, proto, what, fig["ratio"]))
        assert not ok and fig["ratio"] > REJECT
    ok, fig = cf.accept(X32[0][k0:k1], X32[0][k0:k1], Xcf[0][k0:k1])                                 # the shard itself passes
    assert ok and fig["ratio"] <= 1.0


@pytest.mark.parametrize("proto", ["dense", "shipped"])
def test_analysis_rule_accepts_a_second_float32_evaluation(ana_teeth, proto):
    (M, m, r, dct, K, pcm), d = ana_teeth
    h, Xcf, X32 = d[proto]
    for n in range(2):
        ok, fig = cf.accept(np.ascontiguousarray(_analysis_f32_again(h, M, m, r, dct, pcm[n])[:, :K].T), X32[n], Xcf[n])
        print("TEETH analysis M=%d m=%d r=%d %s second float32 evaluation: ratio %.2f" % (M, m, r, proto, fig["ratio"]))
        assert ok and fig["ratio"] < 2.0


def _synthesis_f32_again(g, M, m, r, dct, Y):
    """A second correct float32 evaluation: float64 FFT rounded to float32, taps summed in reverse order."""
    R, D = 1 << r, M >> r
    pd, _ = cf.fb_delays(m, r, True, dct)
    T = Y.shape[0]
    v = np.fft.fft(np.asarray(Y, np.complex128), axis=1).real.astype(np.float32)
    vp = np.concatenate([np.zeros((m * R, M), np.float32), v])
    gi = np.asarray(g, np.float32).reshape(m, M)[:, ::-1]
    s = np.zeros((T, M), np.float32)
    for k in range(m - 1, -1, -1):
        s += gi[k][None, :] * vp[m * R - R * k: m * R - R * k + T]
    s[:pd] = 0.0
    sp = np.concatenate([np.zeros((R, M), np.float32), s])
    out = np.zeros((T - pd, D), np.float32)
    for j in range(R - 1, -1, -1):
        out += sp[R + pd - (R - 1 - j): R + pd - (R - 1 - j) + T - pd, j * D:(j + 1) * D]
    assert out.dtype == np.float32
    return out[:, ::-1]


@pytest.mark.parametrize("proto", ["dense", "shipped"])
@pytest.mark.parametrize("M,m,r", SYN_TEETH)
def test_synthesis_rule_at_r0_r2_and_three_taps(M, m, r, proto):
    """Judged as the GPU tests judge it: [blocks][D]."""
    dct, T, D = 2, 40, M >> r
    g = cf.dense_prototype(M, m, seed=1) if proto == "dense" else design_prototype(M, m, "g")
    rng = np.random.default_rng(M + r)
    Yh = ((rng.normal(size=(M // 2 + 1, T)) + 1j * rng.normal(size=(M // 2 + 1, T))) * 1000.0).astype(np.complex64)
    Y = cf.hermitian(Yh, M)
    B = T - cf.fb_delays(m, r, True, dct)[0]
    ocf, o32 = cf.synthesis_cf(g, M, m, r, dct, Y).reshape(B, D), cf.synthesis_f32(g, M, m, r, dct, Y).reshape(B, D)
    ok, fig = cf.accept(_synthesis_f32_again(g, M, m, r, dct, Y), o32, ocf)
    print("TEETH synthesis M=%d m=%d r=%d %s second float32 evaluation: ratio %.2f" % (M, m, r, proto, fig["ratio"]))
    assert ok and fig["ratio"] < 2.0
    faults = []
    for tap in ((0, 1, m * M - 1) if proto == "dense" else (1,)):
        g2 = g.copy()
        assert g2[tap] != 0.0
        g2[tap] = 0.0
        faults.append(("tap %d dropped" % tap, cf.synthesis_cf(g2, M, m, r, dct, Y).reshape(B, D)))
    Y2 = Y.copy()
    Y2[20] = Y[21]                                              # one frame's spectrum taken from its neighbour
    faults.append(("frame from the neighbour", cf.synthesis_cf(g, M, m, r, dct, Y2).reshape(B, D)))
    moved = ocf.copy()
    moved[10] = ocf[11]                                         # one output block taken from its neighbour
    faults.append(("block from the neighbour", moved))
    for what, out in faults:
        ok, fig = cf.accept(out, o32, ocf)
        print("TEETH synthesis M=%d m=%d r=%d %s %s: ratio %.3g" % (M, m, r, proto, what, fig["ratio"]))
        assert not ok and fig["ratio"] > REJECT


def test_rule_floor_and_zero_cases():
    Ycf = np.zeros((3, 5), np.complex128)
    assert cf.accept(np.zeros((3, 5), np.complex64), np.zeros((3, 5), np.complex64), Ycf)[0]
    bad = np.zeros((3, 5), np.complex64)
    bad[1, 2] = 1e-30
    assert not cf.accept(bad, np.zeros((3, 5), np.complex64), Ycf)[0]       # closed form identically zero: exactly zero
    Ycf = np.arange(1, 16, dtype=np.float64).reshape(3, 5) * 1000 + 0j
    exact = Ycf.astype(np.complex64)                                          # float32 produces these exactly: yardstick 0
    assert cf.accept(exact, exact, Ycf)[0]
    off = exact.copy()
    off[0, 0] += np.float32(15000 * 3 * cf.FLOOR)
    assert not cf.accept(off, exact, Ycf)[0]
    off[0, 0] = exact[0, 0] + np.float32(15000 * 0.5 * cf.FLOOR)
    assert cf.accept(off, exact, Ycf)[0]                                      # within the floor of 2^-22 max|Y_cf|
