"""GPU: spectral subtraction, Wiener filter and spectral high-pass (csrc/ss_kernels.hip through engine.spectral_subtract /
wiener_filter / spec_highpass) against the float64 closed forms of tests/ss_closed_form.py on the same complex64 inputs.

The bound is derived per element from the arithmetic the kernels use (include/btkhip.h: |X|^2, the scan inside a 64-frame chunk
and the subtraction in float32; carry, state and averaging sum in float64), with u = 2^-24 and the precision the OpenCL numerical
profile grants a float32 sqrt (3 ulp = 6u) and division (2.5 ulp = 5u) when they are not correctly rounded:

  p^ = fl(xr xr + fl(xi xi)):  both summands >= 0, two roundings                                  |p^ - p| <= 2u p
  b^ = fl(fl(1 - alpha) p^):                                                                       relative 4u  (first sample: 2u)
  the scan: six steps of  b <- fl(a p' + b),  a <- fl(a a'),  everything >= 0, so relative errors only add up.  A summand of B_t
    passes at most 6 such roundings, and each of the at most 6 merges multiplies it by a partial product of alphas that was
    formed by 0, 1, .. 5 multiplications:  6u + 15u.  B_t: relative 25u;  A_t: 6u.
  est_t = fma(A_t, carry, B_t) in float64, so after n chunks   |est^ - est| <= (25 + 6 n) u est =: eps est,  + u for (float)est^
  an averaging channel's estimate is acc (1/count) in float64 (<= (T + 8) 2^-52 relative) and is rounded to float32 once: u
  S2^ = fl(p^ - ft est^):   D2 := |S2^ - S2| <= 2u p + ft est (eps + u) + u |p - ft est|
  flooring is 1-Lipschitz;  |sqrt a - sqrt b| <= |a - b|/(sqrt a + sqrt b) with a, b >= floor:      D2/(sqrt S2f + sqrt floor)
    (floor = 0:  min(sqrt D2, D2/sqrt S2f)),  + 6u sqrt S2f for sqrtf                              =: Dr
  |X|^ = sqrtf(p^): 7u;  g = r^/|X|^: 5u;  g x: u     ->  |term^ - term| <= Dr + 13u sqrt S2f     (X = 0: the term is (r^, 0): Dr)
  a frame that is not subtracted contributes X itself: no error
  Y^ = fl(1/C) x (sequential float32 sum of C terms):    |Y^ - Y| <= (1/C) (sum_c err_c + (C + 1) u sum_c |term_c|)
Second-order terms are covered by a factor 1.01.  No case may pass on a bound that permits anything: the largest bound of a case
is held to RATIO = 5 % of the mean magnitude (1/C) sum_c |term_c| it guards (the floor = 0 case, where sqrt D2 ~ 1e-2 against
terms ~ 1, needs that much; with a floor >= 1e-3 the largest bound stays below 2 %).

Wiener filter (all of PSDs, PSDn, beta >= 0): both PSDs carry eps as above; H = ps/(fl(beta pn + ps)): (eps + u) + (eps + 2u) + 5u;
Y = H S: u  ->  |Y^ - Y| <= (2 eps + 9u) |Y|, held to 1e-4 |Y|.  Bin 0 and the high-pass are copies: bit for bit.

State: est and the PSDs within eps (relative), acc within 2 (T + 8) 2^-53 (products and sum are float64 on both sides), count and
added exactly.  Blocks cut at multiples of 64 of the stream's frame counter, and the frame-parallel form against the row form,
give the SAME BITS; other cuts (37 + 64 + 99) stay within the bound with n counted over all launches."""
import functools

import numpy as np
import pytest

from tests import ss_closed_form as cf

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
RATIO = 0.05
SLACK = 1.01


def _chunks(splits, frames_done=0):
    """64-frame chunks the launches of a run scan, counted over all of them."""
    n, g = 0, frames_done
    for T in splits:
        n += ((g & 63) + T + 63) // 64
        g += T
    return n


def _eps(nchunks):
    return (25 + 6 * nchunks) * U


def ss_bound(X, flags, ft, floor, alphas, st0, nchunks, T_avg):
    """Per-element bound on |Y_gpu - Y_closed_form|, [S][K][T], and the magnitude it guards."""
    mag, est, P = cf.ss_term_magnitudes(X, flags, ft, floor, alphas, st0)          # [S][K][C][T]
    S, K, C, T = P.shape
    eps = np.array([_eps(nchunks) if a >= 0 else (T_avg + 8) * 2.0 ** -52 for a in alphas])[None, None, :, None] + U
    sub = ((flags & cf.SUBTRACT) != 0)[None, None, None, :]
    d2 = 2 * U * P + ft * np.abs(est) * eps + U * np.abs(P - ft * est)
    if floor > 0:
        dr = d2 / (mag + np.sqrt(floor))
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            dr = np.minimum(np.sqrt(d2), np.where(mag > 0, d2 / mag, np.inf))
    err = np.where(sub, dr + 6 * U * mag + 13 * U * mag, 0.0)
    bound = SLACK * (err.sum(axis=2) + (C + 1) * U * mag.sum(axis=2)) / C
    return bound, mag.sum(axis=2) / C


def _padded(torch, dev, x, pad, fill=float("nan")):
    """complex64 host array [..., T] -> [..., :T] view of a device buffer whose rows are T + pad apart, the padding filled"""
    T = x.shape[-1]
    buf = torch.full(x.shape[:-1] + (T + pad,), complex(fill, fill), dtype=torch.complex64, device=dev)
    buf[..., :T] = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    return buf, buf[..., :T]


def _ss_state(eng, dev, S, C, M, alphas, st0=None):
    st = eng.SpectralSubtractionState(S, C, M, alphas, device=dev)
    if st0 is not None:
        import torch
        st.est.copy_(torch.from_numpy(st0["est"]))
        st.acc.copy_(torch.from_numpy(st0["acc"]))
        st.count.copy_(torch.from_numpy(st0["count"]))
        st.added.copy_(torch.from_numpy(st0["added"]))
        st.frames_done = st0["frames_done"]
    return st


def _ss_run(eng, torch, dev, X, flags, ft, floor, alphas, M, pad=0, splits=None, st0=None, form=None):
    S, K, C, T = X.shape
    st = _ss_state(eng, dev, S, C, M, alphas, st0)
    _, Xd = _padded(torch, dev, X, pad)
    Ybuf, Yd = _padded(torch, dev, np.zeros((S, K, T), np.complex64), pad)
    t0 = 0
    for n in (splits or [T]):
        eng.spectral_subtract(Xd[..., t0:t0 + n], st, ft=ft, floor=floor, flags=flags[t0:t0 + n], out=Yd[..., t0:t0 + n], form=form)
        t0 += n
    torch.cuda.synchronize()
    return Yd.cpu().numpy(), st, Ybuf


def _st_arrays(st):
    return dict(est=st.est.cpu().numpy(), acc=st.acc.cpu().numpy(), count=st.count.cpu().numpy(), added=st.added.cpu().numpy())


def _case_params(case):
    M, S, C, T, pad, alphas, sched, ft, floor = case
    return M, S, C, T, pad, tuple(cf.f32(a) for a in alphas), cf.schedule(sched, T, seed=T), cf.f32(ft), cf.f32(floor)


@functools.lru_cache(maxsize=None)
def _case_reference(i):
    """inputs, closed-form output and final state of CASES[i], computed once"""
    M, S, C, T, pad, alphas, flags, ft, floor = _case_params(cf.CASES[i])
    X = cf.make_input(S, M // 2 + 1, C, T, seed=i)
    st = cf.ss_new_state(S, C, M)
    Y = cf.ss_closed_form(X, flags, ft, floor, alphas, st)
    return X, Y, st


def _check_ss(Y, g, Yr, str_, X, flags, ft, floor, alphas, st0, nchunks, what):
    S, K, C, T = X.shape
    bound, guard = ss_bound(X, flags, ft, floor, alphas, st0, nchunks, T)
    assert bound.max() <= RATIO * guard.mean(), (what, bound.max(), guard.mean())
    err = np.abs(Y - Yr)
    ratio = float(np.max(err / np.maximum(bound, 1e-300)))
    print("%s: max |Y error| %.3g, largest error/bound %.3f, largest bound/mean magnitude %.2g"
          % (what, err.max(), ratio, bound.max() / guard.mean()))
    assert np.all(err <= bound), (what, ratio)
    eps = _eps(nchunks)
    for c, a in enumerate(alphas):
        if a >= 0:
            assert np.all(np.abs(g["est"][:, c] - str_["est"][:, c]) <= SLACK * eps * np.abs(str_["est"][:, c])), (what, c)
        else:
            assert np.array_equal(g["est"][:, c], str_["est"][:, c]), (what, c)      # moves in finish_training only
        assert np.all(np.abs(g["acc"][:, c] - str_["acc"][:, c]) <= 2 * (T + 8) * 2.0 ** -53 * str_["acc"][:, c]), (what, c)
    assert np.array_equal(g["count"], str_["count"]) and np.array_equal(g["added"], str_["added"]), what
    return ratio


@pytest.mark.parametrize("i", range(len(cf.CASES)), ids=["M%d_S%d_C%d_T%d_%s" % (c[0], c[1], c[2], c[3], c[6]) for c in cf.CASES])
def test_ss_matches_closed_form(dev, i):
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, C, T, pad, alphas, flags, ft, floor = _case_params(cf.CASES[i])
    X, Yr, str_ = _case_reference(i)
    Y, st, Ybuf = _ss_run(eng, torch, dev, X, flags, ft, floor, alphas, M, pad=pad)
    _check_ss(Y, _st_arrays(st), Yr, str_, X, flags, ft, floor, alphas, cf.ss_new_state(S, C, M), _chunks([T]), "case %d" % i)
    assert st.frames_done == T
    if pad:
        assert bool(torch.isnan(Ybuf[..., T:].real).all()), "the padding between T and T_stride was written"


def test_ss_cuts_at_multiples_of_64_give_the_same_bits(dev):
    import torch
    from distant_speech_recognition_amd import engine as eng
    i = 5                                                       # M = 32, S = 3, C = 3 (recursive, averaging, recursive), T = 200, vad
    M, S, C, T, pad, alphas, flags, ft, floor = _case_params(cf.CASES[i])
    X = _case_reference(i)[0]
    Y1, st1, _ = _ss_run(eng, torch, dev, X, flags, ft, floor, alphas, M)
    Y2, st2, _ = _ss_run(eng, torch, dev, X, flags, ft, floor, alphas, M, pad=pad, splits=[64, 128, 8])
    assert np.array_equal(Y1.view(np.uint32), Y2.view(np.uint32))
    a, b = _st_arrays(st1), _st_arrays(st2)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k
    # a stream whose counter does not start at a multiple of 64: cuts where the COUNTER is one
    st0 = cf.ss_new_state(S, C, M)
    st0["frames_done"] = 100
    Y3, st3, _ = _ss_run(eng, torch, dev, X, flags, ft, floor, alphas, M, st0=st0)
    Y4, st4, _ = _ss_run(eng, torch, dev, X, flags, ft, floor, alphas, M, st0=st0, splits=[28, 64, 108])
    assert np.array_equal(Y3.view(np.uint32), Y4.view(np.uint32))
    a, b = _st_arrays(st3), _st_arrays(st4)
    for k in a:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), k


@pytest.mark.parametrize("i", [5, 6])
def test_ss_cuts_elsewhere_stay_within_the_bound(dev, i):
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, C, T, pad, alphas, flags, ft, floor = _case_params(cf.CASES[i])
    X, Yr, str_ = _case_reference(i)
    splits = [37, 64, 99]
    Y, st, _ = _ss_run(eng, torch, dev, X, flags, ft, floor, alphas, M, pad=pad, splits=splits)
    _check_ss(Y, _st_arrays(st), Yr, str_, X, flags, ft, floor, alphas, cf.ss_new_state(S, C, M), _chunks(splits), "cuts 37+64+99, case %d" % i)


@pytest.mark.parametrize("M,S,C,T,pad", [(8, 1, 1, 1, 0), (32, 3, 3, 200, 8), (8, 3, 2, 65, 1), (32, 1, 5, 300, 0)])
def test_ss_frame_parallel_form_has_the_bits_of_the_row_form(dev, M, S, C, T, pad):
    """The production case: a fixed noise model, subtraction only.  engine.spectral_subtract then runs the frame-parallel kernel
    (more than one workgroup along T at T = 300); BTK_SS_FORM_ROWS forces the row scan.  Same bits, and both within the bound."""
    import torch
    from distant_speech_recognition_amd import engine as eng, _lib
    K = M // 2 + 1
    X = cf.make_input(S, K, C, T, seed=40 + T)
    rng = np.random.default_rng(T)
    alphas = tuple([0.5, -1.0, 0.75, -1.0, 0.0][:C])
    st0 = cf.ss_new_state(S, C, M)
    st0["est"][:] = rng.random((S, C, K)) * 2.0
    ft, floor = 1.5, cf.f32(1e-2)
    for subtract in (True, False):
        out = []
        for form in (None, _lib.BTK_SS_FORM_ROWS):
            st = _ss_state(eng, dev, S, C, M, alphas, st0)
            _, Xd = _padded(torch, dev, X, pad)
            Ybuf, Yd = _padded(torch, dev, np.zeros((S, K, T), np.complex64), pad)
            eng.spectral_subtract(Xd, st, ft=ft, floor=floor, train=False, subtract=subtract, out=Yd, form=form)
            torch.cuda.synchronize()
            out.append(Yd.cpu().numpy())
            g = _st_arrays(st)
            for k in g:
                assert np.array_equal(g[k], st0[k]), k               # nothing trains: the state keeps its bits
            assert bool(torch.isnan(Ybuf[..., T:].real).all())
        assert np.array_equal(out[0].view(np.uint32), out[1].view(np.uint32))
        flags = np.full(T, cf.SUBTRACT if subtract else 0, np.uint8)
        Yr = cf.ss_closed_form(X, flags, ft, floor, alphas, cf.ss_copy_state(st0))
        bound, guard = ss_bound(X, flags, ft, floor, alphas, st0, 0, T)
        assert bound.max() <= RATIO * guard.mean()
        assert np.all(np.abs(out[0] - Yr) <= bound)


def test_ss_training_flow_finish_and_clear(dev):
    """train (flags) -> finish_training -> subtract, then clear() and a second training: the averaging channel's estimate appears
    with finish_training, count = 0 gives NaN, clear() makes the recursive channel's next training frame a first sample again."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, C, T = 8, 3, 2, 70
    K = M // 2 + 1
    alphas = (-1.0, 0.75)
    ft, floor = 1.0, cf.f32(1e-2)
    X = cf.make_input(S, K, C, 2 * T, seed=77)
    st = eng.SpectralSubtractionState(S, C, M, alphas, device=dev)
    r = cf.ss_new_state(S, C, M)
    st.finish_training()
    cf.ss_finish_training(alphas, r)                                   # count = 0: 0 x inf
    assert bool(torch.isnan(st.est[:, 0]).all()) and np.isnan(r["est"][:, 0]).all() and bool((st.est[:, 1] == 0).all())
    Xd = torch.from_numpy(X).to(dev)
    ftrain, fsub = np.full(T, cf.TRAIN, np.uint8), np.full(T, cf.SUBTRACT, np.uint8)
    # (no flags: one constant mode for the block, the row kernel without a flag stream)
    Y0 = eng.spectral_subtract(Xd[..., :T].contiguous(), st, ft=ft, floor=floor, train=True, subtract=False).cpu().numpy()
    Yr0 = cf.ss_closed_form(X[..., :T], ftrain, ft, floor, alphas, r)
    bound, guard = ss_bound(X[..., :T], ftrain, ft, floor, alphas, cf.ss_new_state(S, C, M), 2, T)      # the mean of X
    assert bound.max() <= RATIO * guard.mean() and np.all(np.abs(Y0 - Yr0) <= bound)
    st.finish_training()
    cf.ss_finish_training(alphas, r)
    g = _st_arrays(st)
    assert np.array_equal(g["count"], r["count"]) and int(g["count"][0, 0]) == T and int(g["count"][0, 1]) == 0
    assert np.all(np.abs(g["est"][:, 0] - r["est"][:, 0]) <= 2 * (T + 8) * 2.0 ** -53 * r["est"][:, 0])
    st_mid = dict(g, frames_done=T)
    Y1 = eng.spectral_subtract(Xd[..., T:].contiguous(), st, ft=ft, floor=floor, train=False, subtract=True).cpu().numpy()
    Yr1 = cf.ss_closed_form(X[..., T:], fsub, ft, floor, alphas, r)
    bound, guard = ss_bound(X[..., T:], fsub, ft, floor, alphas, st_mid, 0, T)
    assert bound.max() <= RATIO * guard.mean() and np.all(np.abs(Y1 - Yr1) <= bound)
    # clear_noise_samples keeps est and added; clear() drops added as well
    st.reset_training()
    g = _st_arrays(st)
    assert not g["acc"].any() and not g["count"].any() and g["added"][:, 1].all() and np.array_equal(g["est"], st_mid["est"])
    st.clear()
    cf.ss_clear(r, True)
    assert not _st_arrays(st)["added"].any()
    both = np.full(3, cf.TRAIN | cf.SUBTRACT, np.uint8)
    eng.spectral_subtract(Xd[..., :3].contiguous(), st, ft=ft, floor=floor, flags=both)
    cf.ss_closed_form(X[..., :3], both, ft, floor, alphas, r)
    g = _st_arrays(st)
    assert np.all(np.abs(g["est"][:, 1] - r["est"][:, 1]) <= SLACK * _eps(2) * r["est"][:, 1])      # restarted from |X_0|^2
    assert np.array_equal(g["count"], r["count"]) and np.array_equal(g["added"], r["added"])


def test_ss_neighbours_and_padding_do_not_leak(dev):
    """NaN in the other streams and between T and T_stride leaves a stream's bits unchanged."""
    import torch
    from distant_speech_recognition_amd import engine as eng
    i = 5
    M, S, C, T, pad, alphas, flags, ft, floor = _case_params(cf.CASES[i])
    X = _case_reference(i)[0]
    Yall, stall, _ = _ss_run(eng, torch, dev, X, flags, ft, floor, alphas, M, pad=pad)
    Xn = np.full_like(X, complex(np.nan, np.nan))
    Xn[1] = X[1]
    Yn, stn, _ = _ss_run(eng, torch, dev, Xn, flags, ft, floor, alphas, M, pad=0)
    assert np.array_equal(Yall[1].view(np.uint32), Yn[1].view(np.uint32))
    a, b = _st_arrays(stall), _st_arrays(stn)
    assert np.array_equal(a["est"][1].view(np.uint64), b["est"][1].view(np.uint64))
    assert np.array_equal(a["acc"][1].view(np.uint64), b["acc"][1].view(np.uint64))
    Y1, st1, _ = _ss_run(eng, torch, dev, X[1:2], flags, ft, floor, alphas, M, pad=3)
    assert np.array_equal(Yall[1].view(np.uint32), Y1[0].view(np.uint32))


# ------------------------------------------------------------------------------------------------------------------ Wiener
# M, S, T, pad, alpha, floor, beta, schedule of the noise update
WIENER_CASES = [
    (8, 1, 1, 3, 0.75, 1e-3, 1.0, "on"),
    (8, 3, 63, 1, 0.0, 1e-3, 1.0, "on"),
    (32, 3, 64, 0, 0.9375, 1e-2, 2.0, "stop_mid"),
    (32, 1, 65, 7, 0.5, 1e-3, 0.5, "never"),
    (8, 3, 130, 2, 0.875, 1e-3, 1.0, "alternate"),
    (32, 3, 200, 8, 0.96875, 1e-2, 1.5, "stop_mid"),
]


def _wiener_flags(name, T):
    f = np.zeros(T, np.uint8)
    if name == "on":
        f[:] = 1
    elif name == "stop_mid":
        f[:(T + 1) // 2] = 1
    elif name == "alternate":
        f[np.random.default_rng(T).random(T) < 0.5] = 1
    return f


def _wiener_inputs(M, S, T, seed):
    K = M // 2 + 1
    Sx = cf.make_input(S, K, 1, T, seed=seed)[:, :, 0]
    Nx = (0.3 * cf.make_input(S, K, 1, T, seed=seed + 1000, zeros=False)[:, :, 0]).astype(np.complex64)
    if T > 4:
        Nx[0, 1, 2] = 0                                         # a noise frame below the floor
        Sx[0, 1, 0] = 0                                         # no target energy in a frame without memory: PSDs = 0
    return Sx, Nx


def _wiener_run(eng, torch, dev, Sx, Nx, flags, alpha, floor, beta, M, pad=0, splits=None, frames_done=0):
    S, K, T = Sx.shape
    st = eng.WienerState(S, M, device=dev)
    st.frames_done = frames_done
    _, Sd = _padded(torch, dev, Sx, pad)
    _, Nd = _padded(torch, dev, Nx, pad)
    Ybuf, Yd = _padded(torch, dev, np.zeros((S, K, T), np.complex64), pad)
    t0 = 0
    for n in (splits or [T]):
        eng.wiener_filter(Sd[..., t0:t0 + n], Nd[..., t0:t0 + n], st, alpha=alpha, floor=floor, beta=beta, flags=flags[t0:t0 + n],
                          out=Yd[..., t0:t0 + n])
        t0 += n
    torch.cuda.synchronize()
    return Yd.cpu().numpy(), st, Ybuf


def _check_wiener(Y, st, Sx, Nx, flags, alpha, floor, beta, M, nchunks, what, frames_done=0):
    r = cf.wiener_new_state(Sx.shape[0], M)
    r["frames_done"] = frames_done
    Yr = cf.wiener_closed_form(Sx, Nx, flags, alpha, floor, beta, r)
    eps = _eps(nchunks)
    rel = SLACK * (2 * eps + 9 * U)
    assert rel <= 1e-4
    nan = np.isnan(Yr.real)
    assert np.array_equal(np.isnan(Y.real), nan), what                # 0/0 stays NaN, nowhere else
    err = np.abs(np.where(nan, 0, Y - Yr))
    bound = rel * np.abs(np.where(nan, 0, Yr))
    ratio = float(np.max(err[:, 1:] / np.maximum(bound[:, 1:], 1e-300)))
    print("%s: Wiener largest error/bound %.3f" % (what, ratio))
    assert np.all(err <= bound), (what, ratio)
    assert np.array_equal(Y[:, 0], Sx[:, 0]), what                    # bin 0 is the target's
    ps, pn = st.psd_s.cpu().numpy(), st.psd_n.cpu().numpy()
    assert not ps[:, 0].any() and not pn[:, 0].any()                  # its state is never touched
    assert np.all(np.abs(ps - r["psd_s"]) <= SLACK * eps * r["psd_s"]) and np.all(np.abs(pn - r["psd_n"]) <= SLACK * eps * r["psd_n"])
    return Yr


@pytest.mark.parametrize("case", WIENER_CASES, ids=["M%d_S%d_T%d_%s" % (c[0], c[1], c[2], c[7]) for c in WIENER_CASES])
def test_wiener_matches_closed_form(dev, case):
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, T, pad, alpha, floor, beta, sched = case
    alpha, floor, beta = cf.f32(alpha), cf.f32(floor), cf.f32(beta)
    Sx, Nx = _wiener_inputs(M, S, T, seed=T)
    flags = _wiener_flags(sched, T)
    Y, st, Ybuf = _wiener_run(eng, torch, dev, Sx, Nx, flags, alpha, floor, beta, M, pad=pad)
    _check_wiener(Y, st, Sx, Nx, flags, alpha, floor, beta, M, _chunks([T]), "wiener %s T=%d" % (sched, T))
    assert st.frames_done == T
    if pad:
        assert bool(torch.isnan(Ybuf[..., T:].real).all())
    if sched == "never":
        # update stopped before any frame: PSDn stays 0 and H = 1 wherever PSDs > 0; the one frame with PSDs = 0 is 0/0 = NaN
        assert not st.psd_n.cpu().numpy().any()
        nan = np.isnan(Y.real)
        assert nan.sum() == 1 and nan[0, 1, 0] and np.array_equal(Y[~nan], Sx[~nan])


def test_wiener_cuts(dev):
    import torch
    from distant_speech_recognition_amd import engine as eng
    M, S, T, pad, alpha, floor, beta, sched = WIENER_CASES[5]
    alpha, floor, beta = cf.f32(alpha), cf.f32(floor), cf.f32(beta)
    Sx, Nx = _wiener_inputs(M, S, T, seed=T)
    flags = _wiener_flags(sched, T)
    Y1, st1, _ = _wiener_run(eng, torch, dev, Sx, Nx, flags, alpha, floor, beta, M)
    Y2, st2, _ = _wiener_run(eng, torch, dev, Sx, Nx, flags, alpha, floor, beta, M, pad=pad, splits=[128, 64, 8])
    assert np.array_equal(Y1.view(np.uint32), Y2.view(np.uint32))
    assert torch.equal(st1.psd_s, st2.psd_s) and torch.equal(st1.psd_n, st2.psd_n)
    splits = [37, 64, 99]
    Y3, st3, _ = _wiener_run(eng, torch, dev, Sx, Nx, flags, alpha, floor, beta, M, splits=splits)
    _check_wiener(Y3, st3, Sx, Nx, flags, alpha, floor, beta, M, _chunks(splits), "wiener cuts 37+64+99")
    # the two frames without memory are the STREAM's first two: a block that starts at frame 1 has one of them
    Y4, st4, _ = _wiener_run(eng, torch, dev, Sx, Nx, flags, alpha, floor, beta, M, splits=[1, 199])
    _check_wiener(Y4, st4, Sx, Nx, flags, alpha, floor, beta, M, _chunks([1, 199]), "wiener cuts 1+199")
    Y5, st5, _ = _wiener_run(eng, torch, dev, Sx, Nx, flags, alpha, floor, beta, M, frames_done=100)
    _check_wiener(Y5, st5, Sx, Nx, flags, alpha, floor, beta, M, _chunks([T], 100), "wiener from frame 100", frames_done=100)


# ------------------------------------------------------------------------------------------------------------------ high-pass
@pytest.mark.parametrize("M,S,T,pad", [(8, 1, 1, 2), (32, 3, 300, 4)])
def test_highpass_bit_for_bit(dev, M, S, T, pad):
    import torch
    from distant_speech_recognition_amd import engine as eng
    K = M // 2 + 1
    X = cf.make_input(S, K, 1, T, seed=T)[:, :, 0]
    for cutoff in (0, 1, 2, M // 2, K):
        _, Xd = _padded(torch, dev, X, pad)
        Ybuf, Yd = _padded(torch, dev, np.zeros((S, K, T), np.complex64), pad)
        eng.spec_highpass(Xd, cutoff, out=Yd)
        ref = cf.highpass_closed_form(X, cutoff).astype(np.complex64)
        assert np.array_equal(Yd.cpu().numpy().view(np.uint32), ref.view(np.uint32)), cutoff
        assert bool(torch.isnan(Ybuf[..., T:].real).all())
        eng.spec_highpass(Xd, cutoff, out=Xd)                         # in place
        assert np.array_equal(Xd.cpu().numpy().view(np.uint32), ref.view(np.uint32)), cutoff
    assert eng.highpass_cutoff_bin(512, 150, 16000) == cf.highpass_cutoff_bin(512, 150, 16000) == 4


# ------------------------------------------------------------------------------------------------------------------ limits
def test_dimension_limits(dev):
    import ctypes
    import torch
    from distant_speech_recognition_amd import engine as eng, _lib
    L = _lib.lib()
    one = torch.zeros(4096, dtype=torch.float64, device=dev)
    p = ctypes.c_void_p(one.data_ptr())
    al = (ctypes.c_double * 80)(*([0.5] * 80))
    assert L.btk_ss_max_channels() == 64

    def ss(S, M, C, ts, T):
        return L.btk_ss_process(p, p, S, M, C, ts, T, None, 2, 1.0, 0.001, al, 0, p, p, p, p, 0, None)
    assert ss(1, 4096, 1, 4, 4) == _lib.BTK_ERR_DIMENSION
    assert ss(1, 9, 1, 4, 4) == _lib.BTK_ERR_DIMENSION
    assert ss(1, 8, 65, 4, 4) == _lib.BTK_ERR_DIMENSION and b"64" in L.btk_last_error()
    assert ss(1, 8, 0, 4, 4) == _lib.BTK_ERR_DIMENSION
    assert ss(0, 8, 1, 4, 4) == _lib.BTK_ERR_DIMENSION
    assert ss(1, 8, 1, 3, 4) == _lib.BTK_ERR_DIMENSION
    assert L.btk_ss_process(p, p, 1, 8, 1, 4, 4, None, 4, 1.0, 0.001, al, 0, p, p, p, p, 0, None) == _lib.BTK_ERR_PARAMETER
    assert L.btk_ss_process(p, None, 1, 8, 1, 4, 4, None, 2, 1.0, 0.001, al, 0, p, p, p, p, 0, None) == _lib.BTK_ERR_PARAMETER
    assert L.btk_wiener_process(p, p, p, 1, 4096, 4, 4, None, 1, 0.5, 0.001, 1.0, 0, p, p, None) == _lib.BTK_ERR_DIMENSION
    assert L.btk_wiener_process(p, None, p, 1, 8, 4, 4, None, 1, 0.5, 0.001, 1.0, 0, p, p, None) == _lib.BTK_ERR_PARAMETER
    assert L.btk_spec_highpass(p, p, 1, 4096, 1, 4, 4, None) == _lib.BTK_ERR_DIMENSION
    assert L.btk_spec_highpass(p, p, 1, 8, 6, 4, 4, None) == _lib.BTK_ERR_DIMENSION
    assert L.btk_ss_finish_training(1, 8, 65, al, p, p, p, None) == _lib.BTK_ERR_DIMENSION
    assert L.btk_ss_clear(1, 8, 1, 2, p, p, p, None) == _lib.BTK_ERR_PARAMETER
    with pytest.raises(_lib.BtkError):
        eng.SpectralSubtractionState(1, 65, 8, device=dev)
    st = eng.SpectralSubtractionState(1, 2, 8, device=dev)
    with pytest.raises(_lib.BtkError):
        eng.spectral_subtract(torch.zeros((1, 5, 3, 4), dtype=torch.complex64, device=dev), st)
    with pytest.raises(_lib.BtkError):
        eng.spectral_subtract(torch.zeros((1, 5, 2, 4), dtype=torch.complex64, device=dev), st, flags=np.zeros(3, np.uint8))
    torch.cuda.synchronize()


def test_noise_file_through_the_state(dev, tmp_path):
    """write_noise_file / read_noise_file of the state: six decimals, and a file shorter than K lines leaves the other bins alone"""
    import torch
    from distant_speech_recognition_amd import engine as eng
    st = eng.SpectralSubtractionState(2, 2, 8, [-1.0, 0.5], device=dev)
    est = torch.rand((2, 2, 5), dtype=torch.float64, device=dev) + 0.25
    st.set_noise_psd(est)
    fn = str(tmp_path / "n.txt")
    assert st.write_noise_file(fn, channel=1, stream=1)
    other = eng.SpectralSubtractionState(2, 2, 8, [-1.0, 0.5], device=dev)
    other.set_noise_psd(torch.full((5,), 9.0, dtype=torch.float64), channel=0)
    assert other.read_noise_file(fn, channel=0) and not other.read_noise_file(str(tmp_path / "missing.txt"))
    got = other.noise_psd().cpu().numpy()
    assert np.max(np.abs(got[:, 0] - est[1, 1].cpu().numpy())) <= 5e-7 and not got[:, 1].any()
    with open(fn, "w") as fp:
        fp.write("1.500000\n2.500000\n")
    assert other.read_noise_file(fn, channel=0, stream=0)
    now = other.noise_psd().cpu().numpy()
    assert list(now[0, 0, :2]) == [1.5, 2.5] and np.array_equal(now[0, 0, 2:], got[0, 0, 2:]) and np.array_equal(now[1], got[1])
