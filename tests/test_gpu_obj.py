"""GPU: the objective measures (csrc/obj_kernels.hip through engine.snr / segmental_snr / is_distance) against the closed forms
of tests/obj_closed_form.py.

SNR.  Samples are integer-valued at int16 scale, so every float64 order gives the same sum of x: the means, the signed maxima and
the scales of option 2 are compared with ==; a2 of options 4 and 8 within one float32 unit in the last place.  sum and err are
compared with math.fsum over the same float32 values (the kernel's own mu and a): every term is a square of a float32, exact in
float64 and not negative, so the relative error is at most the number of roundings on the longest chain of additions times
2^-53.  The chain (csrc/obj_kernels.hip): 64 additions in a thread, 6 in the wavefront butterfly, 3 over the wavefronts, then
ceil(chunks / 64) + 6 over a pair's chunks of 16384 samples; fsum adds one rounding: DEPTH(n) = 80 + ceil(ceil(n / 16384) / 64).
A segment row: ceil(L / 64) additions in a lane, 6 in the butterfly, one for fsum.
Largest measured error on an MI355X: 2.22 units of 2^-53 against DEPTH = 81 or 82 (the errors of a sum do not line up); segment
rows: 2.01 units.

Itakura-Saito distance.  (a) against the closed form on the complex64 frames of STFTBank.analysis, per term
4 2^-52 max(ratio, |log ratio|, 1) for the three roundings and the device log's one unit, summed over the frame: it fails if the
fused kernel's spectra are not stft_kernel's bits.  (b) against a float64 transform of the windowed samples, on white noise at
int16 scale and its copy plus independent noise 10 dB down: the largest relative error of Eis_t measured on an MI355X over the
shapes below was 6.56e-05 (IS_F64_MEASURED, at M = 512, r = 1; float32 spectra), the bound is four times that."""
import ctypes as C

import numpy as np
import pytest

from tests import obj_closed_form as cf

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
NS = [1, 63, 64, 65, 255, 256, 257, 4095, 4097, 2 ** 20 + 3]
IS_F64_MEASURED = 6.56e-05
IS_F64_BOUND = 4.0 * IS_F64_MEASURED
BANKS = [(8, 1), (8, 3), (64, 2), (512, 1), (2048, 0), (2048, 1)]
worst = {"sum": 0.0, "seg": 0.0, "is_a": 0.0, "is_b": 0.0}


def depth(n):
    return 80 + -(-(-(-n // 16384)) // 64)


@pytest.fixture(scope="module")
def eng(dev):
    from distant_speech_recognition_amd import engine
    return engine


@pytest.fixture(scope="module")
def torch_():
    import torch
    return torch


def _signals(rng, n1, n2):
    """Integer-valued clean signal and a noisier copy (int16 scale), lengths n1 and n2."""
    n = max(n1, n2)
    x1 = rng.integers(-8000, 8000, n).astype(np.float32)
    x2 = (x1 + rng.integers(-900, 900, n)).astype(np.float32)
    return x1[:n1].copy(), x2[:n2].copy()


def _rows(torch, dev, xs, stride):
    """The signals as rows of a NaN-filled buffer [S][stride]."""
    buf = np.full((len(xs), stride), np.nan, np.float32)
    for s, x in enumerate(xs):
        buf[s, :len(x)] = x
    return torch.from_numpy(buf).to(dev)


def _run_snr(eng, torch, dev, pairs, option, stride_extra=(5, 9), segment=None):
    n1 = [len(a) for a, _ in pairs]
    n2 = [len(b) for _, b in pairs]
    x1 = _rows(torch, dev, [a for a, _ in pairs], max(n1) + stride_extra[0])
    x2 = _rows(torch, dev, [b for _, b in pairs], max(n2) + stride_extra[1])
    return eng.snr(x1, x2, n1, n2, option, segment=segment)


def _check_pair(x1, x2, option, st, db):
    mu1, mu2, a1, a2 = cf.snr_scales(x1, x2, option)
    assert st[0] == mu1 and st[1] == mu2
    assert st[2] == a1
    if option & 2 or not option & 12 or not np.isfinite(a2):
        assert st[3] == a2 or (np.isnan(st[3]) and np.isnan(a2))
    else:
        assert abs(st[3] - float(a2)) <= float(np.spacing(np.float32(abs(a2))))
    s, e = cf.snr_sums(x1, x2, st[0], st[1], st[2], st[3])
    d = depth(max(len(x1), len(x2)))
    for got, want in ((st[4], s), (st[5], e)):
        if np.isfinite(want):
            assert abs(got - want) <= d * U * want
            if want > 0:
                worst["sum"] = max(worst["sum"], abs(got - want) / (U * want))
    want_db = cf.snr_db(s, e)
    if np.isfinite(want_db) and want_db != cf.FLT_MAX:
        assert abs(float(db) - float(want_db)) <= float(np.spacing(np.float32(abs(want_db)))) + 4.343 * 2.0 ** -23
    else:
        assert db == want_db or (np.isnan(db) and np.isnan(want_db))


@pytest.mark.parametrize("rel", ["lt", "eq", "gt"])
@pytest.mark.parametrize("n", NS)
def test_snr_lengths(eng, torch_, dev, n, rel):
    n1, n2 = {"lt": (n, n + 37), "eq": (n, n), "gt": (n + 37, n)}[rel]
    x1, x2 = _signals(np.random.default_rng(n * 3 + len(rel)), n1, n2)
    options = [0, 1, 2, 3, 4, 5, 6, 12, 15] + ([8, 9] if n1 >= n2 else [])
    if n > 5000:
        options = [5, 9 if n1 >= n2 else 3]
    for option in options:
        db, st = _run_snr(eng, torch_, dev, [(x1, x2)], option)
        _check_pair(x1, x2, option, st[0], db[0])
    print("largest sum error in units of 2^-53 so far: %.2f (depth %d)" % (worst["sum"], depth(max(n1, n2))))


@pytest.mark.parametrize("n1,n2", [(20000, 50000), (50000, 20000), (16384, 16385), (32768, 16384)])
def test_snr_tail_over_chunks(eng, torch_, dev, n1, n2):
    x1, x2 = _signals(np.random.default_rng(n1 + n2), n1, n2)
    for option in (0, 5, 3):
        db, st = _run_snr(eng, torch_, dev, [(x1, x2)], option)
        _check_pair(x1, x2, option, st[0], db[0])


@pytest.mark.parametrize("option", [5, 2, 9, 0])
@pytest.mark.parametrize("S", [1, 3, 70])
def test_snr_batches(eng, torch_, dev, S, option):
    rng = np.random.default_rng(S * 16 + option)
    lens = [63, 64, 65, 255, 256, 257, 4095, 4097, 1, 20000]
    pairs = []
    for s in range(S):
        n = lens[s % len(lens)]
        n1, n2 = [(n, n + 37), (n, n), (n + 37, n)][(s // len(lens) + s) % 3]
        if option & 8 and n1 < n2:
            n1, n2 = n2, n1
        pairs.append(_signals(rng, n1, n2))
    db, st = _run_snr(eng, torch_, dev, pairs, option)
    for s, (x1, x2) in enumerate(pairs):
        _check_pair(x1, x2, option, st[s], db[s])


def test_snr_identical_inputs_give_flt_max(eng, torch_, dev):
    x1, _ = _signals(np.random.default_rng(1), 777, 777)
    db, st = _run_snr(eng, torch_, dev, [(x1, x1.copy())], 1)
    assert st[0, 5] == 0.0 and db[0] == np.finfo(np.float32).max


def test_snr_signed_maximum(eng, torch_, dev):
    # the scale of option 2 is the signed maximum: a signal whose peak is negative is scaled by its smallest magnitude
    x1 = np.array([-5.0, -20000.0, -7.0, -3.0], np.float32)
    x2 = np.array([-6.0, -3000.0, -2.0, -9.0, -4.0], np.float32)
    db, st = _run_snr(eng, torch_, dev, [(x1, x2)], 2)
    assert st[0, 2] == np.float32(1) / np.float32(-3) and st[0, 3] == np.float32(1) / np.float32(-2)
    _check_pair(x1, x2, 2, st[0], db[0])
    # below the initial value -10000 the initial value stays
    db, st = _run_snr(eng, torch_, dev, [(np.full(9, -20000.0, np.float32), x2)], 2)
    assert st[0, 2] == np.float32(1) / np.float32(-10000)


def test_snr_option8_short_first_signal_is_refused(eng, torch_, dev):
    from distant_speech_recognition_amd import _lib
    x1 = _rows(torch_, dev, [np.ones(10, np.float32)], 16)
    x2 = _rows(torch_, dev, [np.ones(12, np.float32)], 16)
    stats = torch_.full((1, 6), -7.0, dtype=torch_.float64, device=dev)
    seg = torch_.full((1, 4, 2), -7.0, dtype=torch_.float64, device=dev)
    ws = torch_.zeros(64, dtype=torch_.float64, device=dev)
    n1, n2 = np.array([10], np.int64), np.array([12], np.int64)

    def call(option, a=n1, b=n2):
        return _lib.lib().btk_obj_snr(x1.data_ptr(), 16, x2.data_ptr(), 16, 1, a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p),
                                      option, stats.data_ptr(), 3, seg.data_ptr(), 4, ws.data_ptr(), None)
    for option in (8, 9):
        assert call(option) == _lib.BTK_ERR_DIMENSION
    assert call(16) == _lib.BTK_ERR_PARAMETER
    assert call(0, np.array([17], np.int64)) == _lib.BTK_ERR_DIMENSION
    assert call(0, np.array([0], np.int64)) == _lib.BTK_ERR_DIMENSION
    torch_.cuda.synchronize()
    assert bool((stats == -7.0).all()) and bool((seg == -7.0).all())
    with pytest.raises(_lib.BtkError) as e:
        eng.snr(x1, x2, 10, 12, 8)
    assert e.value.code == _lib.BTK_ERR_DIMENSION
    assert call(10) == _lib.BTK_OK           # 2 goes before 8: nothing is read past the first signal
    assert call(8, n2, n1) == _lib.BTK_OK


@pytest.mark.parametrize("L", [1, 64, 100])
def test_snr_segment_rows(eng, torch_, dev, L):
    rng = np.random.default_rng(L)
    pairs = [_signals(rng, 257, 300), _signals(rng, 63, 70), _signals(rng, 1000, 640), _signals(rng, 4097, 4097)]
    # clamps and the two zero rules in the last pair: err_b = 0, sum_b = 0, a very noisy and a nearly clean segment
    x1, x2 = pairs[3]
    x2[0:200] = x1[0:200]
    x1[200:400] = 0
    x2[400:600] = x1[400:600] * 40
    x1[600:800] = 30000
    x2[600:800] = 30001
    for option in (0, 5):
        db, st, seg = _run_snr(eng, torch_, dev, pairs, option, segment=L)
        seg = seg.cpu().numpy()
        for s, (a, b) in enumerate(pairs):
            want = cf.segment_rows(a, b, st[s, 0], st[s, 1], st[s, 2], st[s, 3], L)
            B = len(want)
            assert B == min(len(a), len(b)) // L and np.isnan(seg[s, B:]).all()
            bound = (-(-L // 64) + 7) * U * want
            assert (np.abs(seg[s, :B] - want) <= bound).all()
            nz = want > 0
            if nz.any():
                worst["seg"] = max(worst["seg"], float((np.abs(seg[s, :B] - want)[nz] / (U * want[nz])).max()))
            if L > 1 and option == 0 and s == 3:
                assert (want[:, 1] == 0).any() and (want[:, 0] == 0).any()
        got, _ = eng.segmental_snr(_rows(torch_, dev, [a for a, _ in pairs], 4200), _rows(torch_, dev, [b for _, b in pairs], 4200),
                                   L, [len(a) for a, _ in pairs], [len(b) for _, b in pairs], option)
        for s in range(len(pairs)):
            B = min(len(pairs[s][0]), len(pairs[s][1])) // L
            want = cf.segmental_snr(seg[s, :B])
            assert (np.isnan(got[s]) and np.isnan(want)) or abs(got[s] - want) <= 1e-12 * max(1.0, abs(want))
        if L > 63:
            assert np.isnan(got[1])                       # B = 0
            rows = cf.segment_rows(*pairs[3], 0, 0, 1, 1, L) if option == 0 else None
            if rows is not None:
                vals = [cf.segmental_snr(r[None]) for r in rows]
                assert 35.0 in vals and -10.0 in vals
    print("largest segment error in units of 2^-53: %.2f" % worst["seg"])


@pytest.mark.parametrize("option", [0, 5, 3, 9])
def test_snr_invariance(eng, torch_, dev, option):
    rng = np.random.default_rng(option)
    x1, x2 = _signals(rng, 40001, 33333)
    alone = _run_snr(eng, torch_, dev, [(x1, x2)], option)
    others = [_signals(rng, int(rng.integers(1, 60000)), 100) for _ in range(9)]
    others[5] = (x1, x2)
    batch = _run_snr(eng, torch_, dev, others, option)
    assert np.array_equal(alone[1][0], batch[1][5]) and alone[0][0] == batch[0][5]
    with_seg = _run_snr(eng, torch_, dev, [(x1, x2)], option, segment=100)
    assert np.array_equal(alone[1], with_seg[1])
    seg_batch = _run_snr(eng, torch_, dev, others, option, segment=100)
    assert np.array_equal(batch[1], seg_batch[1])
    assert np.array_equal(with_seg[2][0].cpu().numpy(), seg_batch[2][5, :333].cpu().numpy())
    # rows 16-byte aligned (vector loads) and rows at odd offsets (scalar loads): the same additions in the same order
    for extra in ((3, 7), (0, 0), (40003 * 3 + 1, 2)):
        n1s, n2s = [40001] * 3, [33333] * 3
        a = _rows(torch_, dev, [x1] * 3, 40004 + extra[0])
        b = _rows(torch_, dev, [x2] * 3, 33336 + extra[1])
        db, st = eng.snr(a, b, n1s, n2s, option)
        for s in range(3):
            assert np.array_equal(st[s], alone[1][0]) and db[s] == alone[0][0], (extra, s)


# ------------------------------------------------------------------ Itakura-Saito distance
def _tile(eng, bank):
    from distant_speech_recognition_amd import _lib
    return _lib.lib().btk_obj_is_tile_frames(bank._h)


def _len_for_frames(F, D):
    """A length that gives F frames and is no multiple of D (where D > 1)."""
    if F == 1:
        return 0
    return (F - 2) * D + 1 if D > 1 else F - 1


def _is_pairs(rng, M, r, TT):
    """Pairs whose frame counts are 1, 2, TT - 1, TT, TT + 1, and two whose lengths differ by more than a tile (either way);
    signal 1 white noise at int16 scale, signal 2 its copy plus independent noise 10 dB down.  The last two pairs carry a stretch
    of exact zeros in signal 2 and another in signal 1, each longer than a frame and its shift."""
    D = M >> r
    out = []
    for F in (1, 2, max(TT - 1, 1), TT, TT + 1):
        n = _len_for_frames(F, D)
        out.append((n, n))
    z = M + 2 * D
    na = max(_len_for_frames(2 * TT + 2, D), 2 * z + 3 * D + 1)
    nb = na + (TT + 3) * D + (1 if D > 1 else 0)
    out += [(na, nb), (nb, na)]
    pairs = []
    for n1, n2 in out:
        n = max(n1, n2, 1)
        x1 = np.rint(rng.normal(size=n) * 3000).astype(np.float32)
        x2 = (x1 + np.rint(rng.normal(size=n) * 3000 * 10 ** -0.5)).astype(np.float32)
        pairs.append([x1[:n1].copy(), x2[:n2].copy()])
    for x1, x2 in pairs[-2:]:
        x2[D:D + z] = 0
        x1[2 * D + z:2 * D + 2 * z] = 0
    return pairs


def _run_is(eng, torch, dev, bank, pairs, bframe=0, eframe=-1, extra=(5, 9)):
    n1 = [len(a) for a, _ in pairs]
    n2 = [len(b) for _, b in pairs]
    x1 = _rows(torch, dev, [a for a, _ in pairs], max(n1) + extra[0])
    x2 = _rows(torch, dev, [b for _, b in pairs], max(n2) + extra[1])
    dist, count, eis = eng.is_distance(bank, x1, x2, n1, n2, bframe, eframe, rows=True)
    return dist.cpu().numpy(), count.cpu().numpy(), eis.cpu().numpy()


def _unfused(eng, torch, dev, bank, x):
    """complex64 frames [F][M] of STFTBank.analysis over a NaN-padded row."""
    row = _rows(torch, dev, [x], len(x) + 3)
    X = bank.analysis(row.view(1, 1, -1), nsamples=len(x))
    return X[0, :, 0, :].cpu().numpy().T


@pytest.fixture(scope="module")
def is_cases(eng, torch_, dev):
    """Per bank shape: the bank, the pairs, the fused rows and the unfused frames, computed once."""
    cases = {}
    for M, r in BANKS:
        bank = eng.STFTBank(M, r, 1)
        TT = _tile(eng, bank)
        pairs = _is_pairs(np.random.default_rng(M * 8 + r), M, r, TT)
        dist, count, eis = _run_is(eng, torch_, dev, bank, pairs)
        cases[(M, r)] = (bank, TT, pairs, dist, count, eis)
    return cases


@pytest.mark.parametrize("M,r", BANKS)
def test_is_against_unfused_route(eng, torch_, dev, is_cases, M, r):
    bank, TT, pairs, dist, count, eis = is_cases[(M, r)]
    D = M >> r
    skipped = 0
    for s, (x1, x2) in enumerate(pairs):
        F = min(cf.num_frames(len(x1), D), cf.num_frames(len(x2), D))
        X1, X2 = _unfused(eng, torch_, dev, bank, x1), _unfused(eng, torch_, dev, bank, x2)
        assert len(X1) == cf.num_frames(len(x1), D)
        want, bound = cf.eis_rows(X1, X2)
        assert len(want) == F == count[s] and np.isnan(eis[s, F:]).all()
        assert (np.abs(eis[s, :F] - want) <= bound).all()
        nz = bound > 0
        if nz.any():
            worst["is_a"] = max(worst["is_a"], float((np.abs(eis[s, :F] - want)[nz] / bound[nz]).max()))
        skipped += int((want == 0).sum())
        want_d = cf.is_distance(eis[s, :F])
        assert abs(dist[s] - want_d) <= (-(-F // 256) + 12) * U * abs(want_d)
    assert skipped >= 2                       # frames inside the zero stretches (and the empty signals) have no term
    print("largest error / bound (a): %.3f" % worst["is_a"])


@pytest.mark.parametrize("M,r", BANKS)
def test_is_against_float64_transform(eng, torch_, dev, is_cases, M, r):
    bank, TT, pairs, dist, count, eis = is_cases[(M, r)]
    for s, (x1, x2) in enumerate(pairs[:-2]):          # the pairs without zero stretches: every ratio is moderate
        want, _ = cf.eis_rows(cf.stft64(x1, M, r), cf.stft64(x2, M, r))
        F = len(want)
        # the frame behind the last sample holds few samples; the frames whose value is 0 hold none
        nz = want > 0
        if nz.any():
            rel = np.abs(eis[s, :F][nz] - want[nz]) / want[nz]
            worst["is_b"] = max(worst["is_b"], float(rel.max()))
            print("M=%d r=%d pair %d: largest relative error of Eis_t against float64 spectra %.3e" % (M, r, s, rel.max()))
            assert rel.max() <= IS_F64_BOUND
        assert (eis[s, :F][~nz] == 0).all()
    print("largest so far (b): %.3e" % worst["is_b"])


@pytest.mark.parametrize("bframe,eframe", [(0, -1), (3, 3), (5, 2), (2, 10 ** 6), (0, 0)])
def test_is_frame_ranges(eng, torch_, dev, is_cases, bframe, eframe):
    bank, TT, pairs, dist0, count0, eis0 = is_cases[(64, 2)]
    dist, count, eis = _run_is(eng, torch_, dev, bank, pairs, bframe, eframe)
    assert np.array_equal(eis, eis0, equal_nan=True)
    for s, (x1, x2) in enumerate(pairs):
        F = min(cf.num_frames(len(x1), 16), cf.num_frames(len(x2), 16))
        lo, hi = cf.frame_range(F, bframe, eframe)
        assert count[s] == hi - lo
        want = cf.is_distance(eis0[s, :F], bframe, eframe)
        if hi == lo:
            assert np.isnan(dist[s]) and np.isnan(want)
        else:
            assert abs(dist[s] - want) <= (-(-(hi - lo) // 256) + 12) * U * abs(want)
    if (bframe, eframe) == (5, 2):
        assert np.isnan(dist).all()


@pytest.mark.parametrize("M,r", [(8, 1), (512, 1), (2048, 0)])
def test_is_invariance(eng, torch_, dev, is_cases, M, r):
    bank, TT, pairs, dist, count, eis = is_cases[(M, r)]
    for s in (4, 5, 6):
        d1, c1, e1 = _run_is(eng, torch_, dev, bank, [pairs[s]], extra=(0, 0))
        F = int(c1[0])
        assert d1[0] == dist[s] and c1[0] == count[s] and np.array_equal(e1[0, :F], eis[s, :F])
        d2, c2, e2 = _run_is(eng, torch_, dev, bank, [pairs[0], pairs[s], pairs[3]], extra=(2, 1))
        assert d2[1] == dist[s] and np.array_equal(e2[1, :F], eis[s, :F])


def test_is_arguments(eng, torch_, dev):
    from distant_speech_recognition_amd import _lib
    bank = eng.STFTBank(64, 1, 1)
    x = _rows(torch_, dev, [np.ones(100, np.float32)], 128)
    with pytest.raises(_lib.BtkError) as e:
        eng.is_distance(bank, x, x, 100, 129)
    assert e.value.code == _lib.BTK_ERR_DIMENSION
    with pytest.raises(_lib.BtkError) as e:
        eng.is_distance(bank, x, x, 100, 100, bframe=-1)
    assert e.value.code == _lib.BTK_ERR_DIMENSION
    for M, rr in ((48, 1), (4096, 1), (64, 7)):
        with pytest.raises(_lib.BtkError) as e:
            eng.STFTBank(M, rr, 1)
        assert e.value.code == _lib.BTK_ERR_PARAMETER
    dist = torch_.full((1,), -7.0, dtype=torch_.float64, device=dev)
    n = np.array([100], np.int64)
    p = n.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().btk_obj_is_distance(bank._h, x.data_ptr(), 128, x.data_ptr(), 128, 1, p, p, 0, -1, dist.data_ptr(), dist.data_ptr(),
                                        dist.data_ptr(), 2, None)
    torch_.cuda.synchronize()
    assert rc == _lib.BTK_ERR_DIMENSION and float(dist[0]) == -7.0
    d, c = eng.is_distance(bank, x, x, 100, 100)
    assert float(d[0]) == 0.0 and int(c[0]) == 5
