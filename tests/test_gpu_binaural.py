"""GPU: binaural binary-mask filters and threshold estimators (csrc/binaural_kernels.hip through engine.binaural_mask /
binaural_stats / binaural_threshold) against the float64 closed forms of tests/binaural_closed_form.py on the same complex64
inputs.

Decisions.  The kernels take every decision in float64 from float32 inputs (include/btkhip.h).  With v = 2^-52:
  arg = atan2 in float64: a few ulp of a value <= pi on either side (device library and numpy); d = arg XL - arg XR, |d -+ 2 pi| and
    the minimum are roundings of values <= 3 pi: the wrapped phase difference of the two sides differs by < 32 v pi.  The division
    by 2 pi k / M and the comparison are the same IEEE operations on both sides, so a Kim decision can differ only where
    |pd - thr omega_k| is that small.
  |X| = sqrt(re^2 + im^2): squares of float32 values are exact in float64, one rounding in the sum, one in the root, against
    numpy's hypot (< 1 ulp): relative 3 v each, so an IID decision can differ only where ||X_T| - |X_I| - thr| <= 8 v (|X_T| + |X_I| + |thr|).
MARGIN = 2^-44 = 256 v covers both with room.  A decision inside the margin may go either way: the mask filter's (stream, bin) row
is left out from that frame on, an estimator's (frame, candidate) pair (FD-IID: (bin, candidate) pair) is left out; at most 1 %
of a case may be left out (asserted on the float64 side; with this margin standard-normal inputs leave out nothing).

Mask output, u = 2^-24.  b_t in {fl(1 - alpha), fl(fl(1 - alpha) eta)} are the same float32 constants on both sides; alpha, eta >= 0,
so every quantity of the recursion is >= 0 and relative errors only add up.  The scan of a 64-frame chunk (six steps of
b <- fl(a p' + b), a <- fl(a a')) leaves B_t with relative 6u + 15u = 21u and A_t with 6u (see tests/test_gpu_ss.py);
mu_t = fl32(fma64(A_t, carry, B_t)) adds u, and the carry is the float32 mask of the chunk before:
    |mu^ - mu| <= (22 + 7 n) u mu =: eps mu   after n chunks,     Y = fl(mu^ x) per component: |Y^ - Y| <= (eps + u) |Y|
Bin 0 is a copy: bit for bit.  Blocks cut at multiples of 64 of the stream's frame counter give the SAME BITS, other cuts stay
within the bound with n counted over all launches; a repeated run gives the same bits.

Sums, all float64 and all terms >= 0.  pow: 16 ulp (the OpenCL profile's grant for a float64 pow) + 1 for numpy's.
  Kim: P = sum over nb bins of |mu X|^2 (3 roundings per term, nb - 1 per sum, either side): relative (nb + 3) v;
       R = P^pc: dR = (17 + pc (nb + 3)) v;  products of two R: 2 dR + v;  a sum over T frames in any order: + (T + 8) v
  IID: y = |mu X|^(2 pc), |mu X| relative 4 v: dy = (17 + 8 pc) v;  y^2, y^4: 2 dy + v, 4 dy + 3 v;  sums over nb bins (per frame)
       and T frames: + (nb + T + 8) v.   FD-IID: the same per bin: 4 dy + (T + 11) v.
Second-order terms are covered by a factor 1.01.  The largest error/bound of every case is printed."""
import ctypes as C

import numpy as np
import pytest

from tests import binaural_closed_form as cf

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
V = 2.0 ** -52
MARGIN = 2.0 ** -44
SLACK = 1.01
KINDS = {cf.KIM: "kim", cf.IID: "iid", cf.FDIID: "fdiid"}


def _chunks(splits, frames_done=0):
    n, g = 0, frames_done
    for T in splits:
        n += ((g & 63) + T + 63) // 64
        g += T
    return n


def _inputs(M, S, T, seed):
    rng = np.random.default_rng(seed)
    shape = (S, M // 2 + 1, T)
    XL = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    XR = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(np.complex64)
    return XL, XR


def _padded(torch, dev, x, pad, fill=float("nan")):
    """complex64 host array [..., T] -> [..., :T] view of a device buffer whose rows are T + pad apart, the padding filled"""
    T = x.shape[-1]
    buf = torch.full(x.shape[:-1] + (T + pad,), complex(fill, fill), dtype=torch.complex64, device=dev)
    buf[..., :T] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return buf, buf[..., :T]


def _mask_run(eng, torch, dev, XL, XR, kind, chan, thr, alpha, eta, pad=0, splits=None, frames_done=0, thresholds=None, mu0=None):
    S, K, T = XL.shape
    _, Ld = _padded(torch, dev, XL, pad)
    _, Rd = _padded(torch, dev, XR, pad)
    Ybuf, Yd = _padded(torch, dev, np.zeros((S, K, T), np.complex64), pad)
    st = eng.binaural_mask_state(S, 2 * (K - 1), dev)
    if mu0 is not None:
        st.copy_(torch.from_numpy(mu0.astype(np.float32)))
    t0, g = 0, frames_done
    for n in (splits or [T]):
        eng.binaural_mask(Ld[..., t0:t0 + n], Rd[..., t0:t0 + n], KINDS[kind], chan, thr, alpha, eta, state=st, thresholds=thresholds,
                          frames_done=g, out=Yd[..., t0:t0 + n])
        t0 += n
        g += n
    torch.cuda.synchronize()
    return Yd.cpu().numpy(), st.cpu().numpy(), Ybuf.cpu().numpy()


def _check_mask(Yg, mug, XL, XR, kind, chan, thr, alpha, eta, nchunks, what, thresholds=None, mu0=None):
    S, K, T = XL.shape
    m0 = np.ones((S, K)) if mu0 is None else mu0.astype(np.float64).copy()
    Y, mu = cf.mask_closed_form(XL, XR, kind, chan, thr, alpha, eta, m0, thresholds)
    out = np.logical_or.accumulate(cf.mask_ambiguous(XL, XR, kind, chan, thr, MARGIN, thresholds), axis=2)
    assert out.mean() <= 0.01, "%s: %.3g of the cells lie within the margin" % (what, out.mean())
    eps = (22 + 7 * nchunks) * U
    bound = SLACK * (eps + U) * np.abs(Y)
    err = np.abs(Yg - Y)
    keep = ~out
    assert np.array_equal(Yg[:, 0], XL[:, 0]), what + ": bin 0 is the left input's, bit for bit"
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = float(np.nanmax(np.where(keep & (bound > 0), err / bound, 0.0)))
    assert np.all(err[keep] <= bound[keep]), "%s: error/bound %.3g" % (what, ratio)
    kept_rows = ~out[:, :, -1]
    dmu = np.abs(mug - m0)
    assert np.all(dmu[kept_rows] <= SLACK * eps * np.abs(m0[kept_rows])), what + ": prevMu"
    assert np.all(mug[:, 0] == (1.0 if mu0 is None else mu0[:, 0])), what + ": prevMu of bin 0 is never touched"
    print("%s: largest error/bound %.3f, %d cells left out" % (what, ratio, int(out.sum())))
    return ratio


MASK_CASES = [  # M, S, T, pad, alpha, chan
    (16, 1, 1, 0, 0.0, 0), (16, 3, 63, 5, 0.6, 1), (64, 1, 64, 0, 0.6, 0), (64, 3, 65, 1, 0.0, 1), (64, 3, 130, 3, 0.6, 0),
    (512, 1, 130, 0, 0.6, 1), (512, 3, 65, 7, 0.0, 0), (16, 3, 130, 2, 0.6, 1), (512, 1, 1, 0, 0.6, 0), (64, 1, 63, 0, 0.0, 0),
]


@pytest.mark.parametrize("kind", [cf.KIM, cf.IID], ids=["kim", "iid"])
@pytest.mark.parametrize("case", MASK_CASES, ids=["M%d_S%d_T%d_p%d_a%g_c%d" % c for c in MASK_CASES])
def test_mask_matches_closed_form(dev, kind, case):
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, T, pad, alpha, chan = case
    XL, XR = _inputs(M, S, T, 10 + M + T)
    thr = 0.9 if kind == cf.KIM else 0.3
    Yg, mug, Ybuf = _mask_run(eng, torch, dev, XL, XR, kind, chan, thr, alpha, 0.01, pad=pad)
    _check_mask(Yg, mug, XL, XR, kind, chan, thr, alpha, 0.01, _chunks([T]), "mask %s %s" % (KINDS[kind], case))
    if pad:
        assert np.all(np.isnan(Ybuf[..., T:].real)) and np.all(np.isnan(Ybuf[..., T:].imag)), "the padding of the output is not written"
        assert not np.any(np.isnan(Yg.real)), "the padding of the inputs is not read"


def test_mask_iid_per_bin_thresholds_and_kim_ignores_them(dev):
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, T = 64, 3, 70
    XL, XR = _inputs(M, S, T, 3)
    thrs = np.linspace(-1.0, 1.0, M // 2 + 1).astype(np.float32)
    for chan in (0, 1):
        Yg, mug, _ = _mask_run(eng, torch, dev, XL, XR, cf.IID, chan, 0.0, 0.6, 0.05, thresholds=thrs)
        _check_mask(Yg, mug, XL, XR, cf.IID, chan, 0.0, 0.6, 0.05, _chunks([T]), "iid per-bin thresholds chan %d" % chan, thresholds=thrs)
    a = _mask_run(eng, torch, dev, XL, XR, cf.KIM, 0, 0.7, 0.6, 0.05, thresholds=thrs)
    b = _mask_run(eng, torch, dev, XL, XR, cf.KIM, 0, 0.7, 0.6, 0.05)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_mask_exact_ties_fall_as_in_the_reference(dev):
    import torch
    from distant_speech_recognition_amd import engine as eng
    XL, _ = _inputs(64, 3, 65, 4)
    eta = np.float32(0.25)
    # XL == XR bit for bit: ITD is exactly 0 <= 0 -> chan 0 keeps the target (mu = 1), chan 1 floors it
    Yg, mug, _ = _mask_run(eng, torch, dev, XL, XL, cf.KIM, 0, 0.0, 0.0, eta)
    assert np.array_equal(Yg, XL) and np.all(mug == 1.0)
    Yg, mug, _ = _mask_run(eng, torch, dev, XL, XL, cf.KIM, 1, 0.0, 0.0, eta)
    floored = (XL.real * eta + 1j * (XL.imag * eta)).astype(np.complex64)
    floored[:, 0] = XL[:, 0]
    assert np.array_equal(Yg, floored) and np.all(mug[:, 1:] == eta)
    # |X_T| <= |X_I| + 0 holds with equality -> eta
    for chan in (0, 1):
        Yg, mug, _ = _mask_run(eng, torch, dev, XL, XL, cf.IID, chan, 0.0, 0.0, eta)
        assert np.array_equal(Yg, floored) and np.all(mug[:, 1:] == eta)


@pytest.mark.parametrize("kind", [cf.KIM, cf.IID], ids=["kim", "iid"])
def test_mask_cuts(dev, kind):
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, T, alpha, eta = 64, 3, 200, 0.6, 0.01
    XL, XR = _inputs(M, S, T, 5)
    thr = 0.9 if kind == cf.KIM else 0.3
    one = _mask_run(eng, torch, dev, XL, XR, kind, 1, thr, alpha, eta, pad=3)
    again = _mask_run(eng, torch, dev, XL, XR, kind, 1, thr, alpha, eta, pad=3)
    assert np.array_equal(one[0], again[0]) and np.array_equal(one[1], again[1]), "a repeated run gives the same bits"
    for splits in ([64, 64, 72], [128, 72], [64, 128, 8]):
        cut = _mask_run(eng, torch, dev, XL, XR, kind, 1, thr, alpha, eta, pad=3, splits=splits)
        assert np.array_equal(one[0], cut[0]) and np.array_equal(one[1], cut[1]), "cuts %s at multiples of 64: same bits" % splits
    # a stream that stands at frame 37: cuts at 64 and 128 of ITS counter
    mu0 = (0.3 + 0.7 * np.random.default_rng(6).random((S, M // 2 + 1))).astype(np.float32)
    one = _mask_run(eng, torch, dev, XL, XR, kind, 0, thr, alpha, eta, frames_done=37, mu0=mu0)
    cut = _mask_run(eng, torch, dev, XL, XR, kind, 0, thr, alpha, eta, frames_done=37, mu0=mu0, splits=[27, 64, 109])
    assert np.array_equal(one[0], cut[0]) and np.array_equal(one[1], cut[1])
    _check_mask(one[0], one[1], XL, XR, kind, 0, thr, alpha, eta, _chunks([T], 37), "from frame 37", mu0=mu0)
    # cuts elsewhere: within the bound, chunks counted over all launches; prevMu carried across the calls
    splits = [37, 64, 99]
    cut = _mask_run(eng, torch, dev, XL, XR, kind, 0, thr, alpha, eta, splits=splits)
    _check_mask(cut[0], cut[1], XL, XR, kind, 0, thr, alpha, eta, _chunks(splits), "cuts %s" % splits)


# ---------------------------------------------------------------------------------------------------------------- estimators
def _stats_run(eng, torch, dev, XL, XR, kind, cands, eta, pc, k0, k1, pad=0, splits=None, per_frame=True):
    T = XL.shape[-1]
    _, Ld = _padded(torch, dev, XL, pad)
    _, Rd = _padded(torch, dev, XR, pad)
    st, pfs, t0 = None, [], 0
    for n in (splits or [T]):
        r = eng.binaural_stats(Ld[..., t0:t0 + n], Rd[..., t0:t0 + n], KINDS[kind], cands, eta, pc, k0, k1, state=st,
                               per_frame=per_frame and kind != cf.FDIID)
        if per_frame and kind != cf.FDIID:
            st, pf = r
            pfs.append(pf.cpu().numpy())
        else:
            st = r
        t0 += n
    torch.cuda.synchronize()
    return st, (np.concatenate(pfs, axis=1) if pfs else None)


def _stats_bounds(kind, nb, T, pc):
    """relative bounds (per-frame terms, sums)"""
    pc = cf.f32(pc)
    if kind == cf.KIM:
        dR = (17 + pc * (nb + 3)) * V
        return SLACK * dR, SLACK * (2 * dR + V + (T + 8) * V)
    dy = (17 + 8 * pc) * V
    if kind == cf.IID:
        return SLACK * (4 * dy + 3 * V + (nb + 8) * V), SLACK * (4 * dy + 3 * V + (nb + T + 8) * V)
    return None, SLACK * (4 * dy + (T + 11) * V)


def _check_stats(st, pfg, XL, XR, kind, cands, eta, pc, k0, k1, what, allow_ambiguous=True):
    walk, n_cand = cands
    S, K, T = XL.shape
    nb = k1 - k0
    sums, pf = cf.stats_closed_form(XL, XR, kind, walk, n_cand, eta, pc, k0, k1)
    amb = cf.stats_ambiguous(XL, XR, kind, walk, MARGIN, k0, k1)
    assert amb.mean() <= (0.01 if allow_ambiguous else 0.0), "%s: %.3g of the pairs lie within the margin" % (what, amb.mean())
    bpf, bsum = _stats_bounds(kind, nb, T, pc)
    g = st.sums.cpu().numpy()
    assert np.array_equal(st.count.cpu().numpy(), np.full(S, T)), what + ": frame count"
    nw = len(walk)
    ratios = []
    if kind == cf.FDIID:
        keep = ~amb
        err, bound = np.abs(g - sums)[:, :, :nw], bsum * np.abs(sums)[:, :, :nw]
        assert np.all(err[keep] <= bound[keep]), what
        assert np.all(g[:, 0] == 0) and np.all(g[:, :, nw:] == 0), what + ": bin 0 and the slots beyond the walk stay 0"
        with np.errstate(divide="ignore", invalid="ignore"):
            ratios.append(float(np.nanmax(np.where(keep[..., None] & (bound > 0), err / bound, 0.0))))
    else:
        keep = ~amb                                                       # [S][T][nw]
        err, bound = np.abs(pfg - pf)[:, :, :nw], bpf * np.abs(pf)[:, :, :nw]
        assert np.all(err[keep] <= bound[keep]), what + ": per-frame terms"
        with np.errstate(divide="ignore", invalid="ignore"):
            ratios.append(float(np.nanmax(np.where(keep[..., None] & (bound > 0), err / bound, 0.0))))
        assert np.all(pfg[:, :, nw:] == 0) and np.all(g[:, nw:] == 0), what + ": slots beyond the walk stay 0"
        # the sums are the sums of the launch's own per-frame terms (ambiguous pairs included, whichever way they fell) ...
        if kind == cf.KIM:
            RT, RI = pfg[..., 0], pfg[..., 1]
            own = np.stack([(RT * RI).sum(1), RT.sum(1), RI.sum(1), (RT * RT).sum(1), (RI * RI).sum(1)], axis=-1)
        else:
            own = pfg.sum(axis=1)
        assert np.all(np.abs(g - own) <= SLACK * (T + 10) * V * np.abs(own)), what + ": sums against the per-frame terms"
        # ... and, where no pair of a candidate was left out, the closed form's
        clean = ~amb.any(axis=1)                                           # [S][nw]
        err, bound = np.abs(g - sums)[:, :nw], bsum * np.abs(sums)[:, :nw]
        assert np.all(err[clean] <= bound[clean]), what + ": sums"
        with np.errstate(divide="ignore", invalid="ignore"):
            ratios.append(float(np.nanmax(np.where(clean[..., None] & (bound > 0), err / bound, 0.0))))
    print("%s: largest error/bound %.3f, %d pairs left out" % (what, max(ratios), int(amb.sum())))
    return sums


KIM_DEFAULT = (float(np.float32(-0.2 * 16000 / 340)), float(np.float32(0.2 * 16000 / 340)), 0.02)
STATS_CASES = [  # kind, M, S, T, pad, (min, max, width), walk, slots, k0, k1 (None: M/2 + 1)
    (cf.KIM, 16, 1, 1, 0, (0.5, 0.5, 0.1), 1, 1, 1, None),
    (cf.KIM, 64, 3, 63, 5, (0.0, 1.0, 0.0625), 17, 17, 1, None),
    (cf.KIM, 64, 1, 64, 0, (-2.0, 2.0, 0.0625), 65, 65, 0, None),
    (cf.KIM, 512, 1, 130, 3, KIM_DEFAULT, 942, 942, 1, 200),
    (cf.KIM, 16, 3, 65, 1, (0.0, 2.0, 0.1), 20, 21, 0, 7),
    (cf.IID, 16, 1, 1, 0, (0.5, 0.5, 0.1), 1, 1, 1, None),
    (cf.IID, 64, 3, 65, 2, (-1.0, 1.0, 0.125), 17, 17, 1, None),
    (cf.IID, 64, 1, 63, 0, (-2.0, 2.0, 0.0625), 65, 65, 0, 20),
    (cf.IID, 512, 1, 130, 0, KIM_DEFAULT, 942, 942, 1, None),
    (cf.IID, 16, 3, 64, 1, (0.0, 2.0, 0.1), 20, 21, 0, None),
    (cf.FDIID, 16, 1, 1, 0, (0.5, 0.5, 0.1), 1, 1, 1, None),
    (cf.FDIID, 64, 3, 65, 2, (-1.0, 1.0, 0.125), 17, 17, 1, None),
    (cf.FDIID, 64, 1, 130, 0, (-2.0, 2.0, 0.0625), 65, 65, 1, None),
    (cf.FDIID, 512, 1, 63, 1, (-1e5, 1e5, 1e3), 201, 201, 1, None),
    (cf.FDIID, 16, 3, 64, 0, KIM_DEFAULT, 942, 942, 1, None),
    (cf.FDIID, 16, 1, 300, 0, (0.0, 2.0, 0.1), 20, 21, 1, None),
]


@pytest.mark.parametrize("case", STATS_CASES, ids=["%s_M%d_S%d_T%d_p%d_c%d_k%d_%s" % (KINDS[c[0]], c[1], c[2], c[3], c[4], c[6], c[8], c[9])
                                                    for c in STATS_CASES])
def test_stats_match_closed_form(dev, case):
    import torch
    from distant_speech_recognition_amd import engine as eng
    kind, M, S, T, pad, rng_, n_walk, n_slots, k0, k1 = case
    k1 = M // 2 + 1 if k1 is None else k1
    XL, XR = _inputs(M, S, T, 20 + M + T)
    cands = eng.binaural_candidates(*rng_)
    assert (len(cands[0]), cands[1]) == (n_walk, n_slots)
    pc = 1 / 15.0 if kind != cf.IID else 0.5
    st, pfg = _stats_run(eng, torch, dev, XL, XR, kind, cands, 0.01, pc, k0, k1, pad=pad)
    sums = _check_stats(st, pfg, XL, XR, kind, cands, 0.01, pc, k0, k1, "stats %s" % (case,))
    # a repeated run gives the same bits
    st2, pf2 = _stats_run(eng, torch, dev, XL, XR, kind, cands, 0.01, pc, k0, k1, pad=pad)
    assert np.array_equal(st.sums.cpu().numpy(), st2.sums.cpu().numpy())
    assert pfg is None or np.array_equal(pfg, pf2)
    if T >= 63:
        # the threshold the closed form picks from its sums is the one picked from the device's, cost function included
        for s in range(S):
            got = eng.binaural_threshold(KINDS[kind], st, cands, stream=s)
            ref = cf.threshold_closed_form(kind, sums[s], T, *cands)
            _, bsum = _stats_bounds(kind, k1 - k0, T, pc)
            # (a cost is a mean m <= scale less, for the IID kinds, 3 (2 m)^2: its error is within 26 bsum max(scale, scale^2))
            scale = np.abs(sums[s]).max() / T
            assert np.all(np.abs(got[1] - ref[1]) <= 64 * bsum * max(scale, scale * scale, 1.0)), "cost function"
            assert got[0] == ref[0], "threshold of stream %d: %r, closed form %r" % (s, got[0], ref[0])
            if kind == cf.FDIID:
                assert np.array_equal(got[2], ref[2]), "per-bin thresholds"


def _midway_inputs(kind, M, S, T, walk, width, seed):
    """Inputs whose decision variables sit midway between two candidates (or beyond the last) in every cell"""
    rng = np.random.default_rng(seed)
    K = M // 2 + 1
    j = rng.integers(0, len(walk), size=(S, K, T))
    target = walk.astype(np.float64)[j] + width / 2
    phi = rng.uniform(-np.pi, np.pi, size=(S, K, T))
    if kind == cf.KIM:
        w = cf.omega(K)[None, :, None]
        pd = np.minimum(target * w, np.pi * (1 - 1 / 64))
        sign = rng.choice([-1.0, 1.0], size=(S, K, T))
        XL = rng.uniform(0.5, 2.0, size=(S, K, T)) * np.exp(1j * (phi + sign * pd))
        XR = rng.uniform(0.5, 2.0, size=(S, K, T)) * np.exp(1j * phi)
    else:
        XL = (3.0 + target / 2) * np.exp(1j * phi)
        XR = (3.0 - target / 2) * np.exp(1j * rng.uniform(-np.pi, np.pi, size=(S, K, T)))
    return XL.astype(np.complex64), XR.astype(np.complex64)


@pytest.mark.parametrize("kind", [cf.KIM, cf.IID, cf.FDIID], ids=["kim", "iid", "fdiid"])
def test_accumulated_sums_without_any_ambiguous_decision(dev, kind):
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, T = 64, 3, 130
    rng_ = (0.0, 1.0, 0.0625) if kind == cf.KIM else (-1.0, 1.0, 0.125)
    cands = eng.binaural_candidates(*rng_)
    assert len(cands[0]) == 17
    XL, XR = _midway_inputs(kind, M, S, T, cands[0], rng_[2], 7)
    K = M // 2 + 1
    # first: no decision is anywhere near a candidate (a margin 2^20 times the derived one)
    assert not cf.stats_ambiguous(XL, XR, kind, cands[0], 2.0 ** -24, 1, K).any()
    pc = 1 / 15.0 if kind != cf.IID else 0.5
    st, pfg = _stats_run(eng, torch, dev, XL, XR, kind, cands, 0.01, pc, 1, K, pad=1)
    _check_stats(st, pfg, XL, XR, kind, cands, 0.01, pc, 1, K, "midway %s" % KINDS[kind], allow_ambiguous=False)
    # the state carried across calls: within the bound of one call, and of the closed form
    st2, pf2 = _stats_run(eng, torch, dev, XL, XR, kind, cands, 0.01, pc, 1, K, pad=1, splits=[50, 1, 79])
    _check_stats(st2, pf2, XL, XR, kind, cands, 0.01, pc, 1, K, "midway %s in three calls" % KINDS[kind], allow_ambiguous=False)
    a, b = st.sums.cpu().numpy(), st2.sums.cpu().numpy()
    assert np.all(np.abs(a - b) <= SLACK * (T + 10) * V * np.abs(a))
    if pfg is not None:
        assert np.array_equal(pfg, pf2), "the per-frame terms do not depend on the cut"
    st2.clear()
    assert not st2.sums.any() and not st2.count.any()


def test_dimension_limits(dev):
    import torch
    from distant_speech_recognition_amd import _lib, engine as eng
    L = _lib.lib()

    def expect(fn):
        with pytest.raises(_lib.BtkError) as e:
            fn()
        assert e.value.code == _lib.BTK_ERR_DIMENSION, e.value

    XL, XR = _inputs(16, 1, 8, 1)
    Ld, Rd = torch.from_numpy(XL).to(dev), torch.from_numpy(XR).to(dev)
    big = torch.zeros((1, 1026, 2), dtype=torch.complex64, device=dev)
    mu = eng.binaural_mask_state(1, 16, dev)
    expect(lambda: eng.binaural_mask(big, big, "kim", 0, 0.0, 0.0, 0.01))
    expect(lambda: eng.binaural_mask(Ld, Rd[:, :8], "kim", 0, 0.0, 0.0, 0.01))
    expect(lambda: eng.binaural_mask(Ld, Rd, "iid", 2, 0.0, 0.0, 0.01, state=mu))
    expect(lambda: eng.binaural_mask(Ld, Rd, "iid", 0, 0.0, 0.0, 0.01, state=mu, thresholds=np.zeros(5, np.float32)))
    expect(lambda: eng.binaural_mask(Ld, Rd, "iid", 0, 0.0, 0.0, 0.01, state=torch.ones((1, 8), device=dev)))
    out = torch.zeros_like(Ld)
    for M, S, ts, T in [(2050, 1, 8, 8), (15, 1, 8, 8), (16, 0, 8, 8), (16, 70000, 8, 8), (16, 1, 4, 8), (16, 1, 8, -1)]:
        rc = L.btk_binaural_mask(Ld.data_ptr(), Rd.data_ptr(), out.data_ptr(), S, M, ts, T, 0, 0, 0.0, None, 0.0, 0.01, 0, mu.data_ptr(), None)
        assert rc == _lib.BTK_ERR_DIMENSION, (M, S, ts, T, rc)
    torch.cuda.synchronize()
    assert torch.all(mu == 1) and not out.any(), "a refused call touches neither state nor output"
    cands = eng.binaural_candidates(0.0, 1.0, 0.25)
    st = eng.BinauralStatsState("kim", 1, 16, cands[1], dev)
    expect(lambda: eng.binaural_stats(Ld, Rd, "kim", cands, 0.01, 0.2, 0, 10, state=st))
    expect(lambda: eng.binaural_stats(Ld, Rd, "kim", cands, 0.01, 0.2, 5, 4, state=st))
    expect(lambda: eng.binaural_stats(Ld, Rd, "iid", cands, 0.01, 0.2, 1, 9, state=st))
    expect(lambda: eng.binaural_stats(Ld, Rd, "kim", (cands[0], 3), 0.01, 0.2, 1, 9))
    expect(lambda: eng.BinauralStatsState("kim", 1, 16, L.btk_binaural_max_candidates() + 1, dev))
    expect(lambda: eng.BinauralStatsState("fdiid", 1, 4096, 4, dev))
    expect(lambda: eng.binaural_candidates(-1e6, 1e6, 1.0))
    dc = torch.from_numpy(cands[0]).to(dev)
    scratch = torch.zeros(1 << 16, dtype=torch.float64, device=dev)
    for M, ncand, nwalk, k0, k1 in [(2050, 5, 5, 1, 9), (16, 5, 5, 1, 10), (16, 5, 5, -1, 9), (16, 5, 6, 1, 9), (16, 5000, 5, 1, 9), (16, 0, 0, 1, 9)]:
        rc = L.btk_binaural_stats(Ld.data_ptr(), Rd.data_ptr(), 1, M, 8, 8, 0, dc.data_ptr(), nwalk, ncand, 0.01, 0.2, k0, k1,
                                  st.sums.data_ptr(), st.count.data_ptr(), None, scratch.data_ptr(), scratch.numel() * 8, None)
        assert rc == _lib.BTK_ERR_DIMENSION, (M, ncand, nwalk, k0, k1, rc)
    torch.cuda.synchronize()
    assert not st.sums.any() and not st.count.any(), "a refused call leaves the state untouched"
    thr, cost = C.c_double(0), np.zeros(5)
    rc = L.btk_binaural_threshold(0, 2050, 5, 5, cands[0].ctypes.data, st.sums.cpu().numpy().ctypes.data, 1, 3.0, C.byref(thr), cost.ctypes.data, None)
    assert rc == _lib.BTK_ERR_DIMENSION
