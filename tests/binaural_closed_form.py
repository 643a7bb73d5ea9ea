"""float64 numpy closed forms of the binaural binary-mask filters and threshold estimators (csrc/binaural_kernels.hip,
include/btkhip.h), over whole blocks in the engine's layout -- what tests/test_gpu_binaural.py holds the kernels against and what
tests/test_binaural_cpu.py holds against a frame-by-frame, bin-by-bin restatement of the reference's loops
(postfilter/binauralprocessing.cc).

    candidates          the float32 walk `for(float t=min;t<=max;t+=width)` and nCand_ = (int)((max-min)/width + 1.5)
    itd                 calcITDf over a block                                  XL, XR [S][K][T] -> [S][K][T]
    mask_closed_form    Kim / IID masking1 with the mask recursion in float64  XL, XR [S][K][T] -> Y [S][K][T]
    mask_ambiguous      cells whose decision variable lies within a margin of its threshold
    stats_closed_form   the three accumStats1: the sums and the per-(frame, candidate) terms
    stats_ambiguous     (frame, candidate) pairs with a decision within the margin
    threshold_closed_form  the three calc_threshold

Parameters enter as the reference's float members hold them (f32()); everything else is float64."""
import numpy as np

KIM, IID, FDIID = 0, 1, 2
NV = {KIM: 5, IID: 6, FDIID: 3}
NPF = {KIM: 2, IID: 6}


def f32(v):
    """A parameter as the kernels and the reference hold it: rounded to float32."""
    return float(np.float32(v))


def candidates(lo, hi, width):
    """(walk float32 [nWalk], nCand): the walk in float32 arithmetic, cut at nCand."""
    lo, hi, width = np.float32(lo), np.float32(hi), np.float32(width)
    n_cand = int(np.float64(np.float32(hi - lo) / width) + 1.5)
    walk = []
    t = lo
    while t <= hi and len(walk) < n_cand:
        walk.append(t)
        t = np.float32(t + width)
    return np.array(walk, np.float32), n_cand


def _arg(z):
    """gsl_complex_arg: atan2(im, re), 0 for z = 0 whatever the signs of its zeros"""
    return np.where((z.real == 0) & (z.imag == 0), 0.0, np.arctan2(z.imag, z.real))


def phase_difference(XL, XR):
    """min(|d|, |d - 2 pi|, |d + 2 pi|), d = arg XL - arg XR (calcITDf, :20-34)"""
    d = _arg(np.asarray(XL, np.complex128)) - _arg(np.asarray(XR, np.complex128))
    d1, d2, d3 = np.abs(d), np.abs(d - 2 * np.pi), np.abs(d + 2 * np.pi)
    pd = np.where(d1 < d2, d1, d2)
    return np.where(d3 < pd, d3, pd)


def omega(K):
    """2 pi k / M for k = 0 .. M/2, evaluated as the reference does (:36)"""
    M = 2 * (K - 1)
    return 2 * np.pi * np.arange(K, dtype=np.float64) / M


def itd(XL, XR):
    K = XL.shape[-2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return phase_difference(XL, XR) / omega(K)[:, None]


def _mask_decision(XL, XR, kind, chan, threshold, thresholds):
    """b_t == 1 per cell [S][K][T] (bin 0 meaningless)"""
    XL, XR = np.asarray(XL, np.complex128), np.asarray(XR, np.complex128)
    K = XL.shape[1]
    if kind == KIM:
        le = itd(XL, XR) <= f32(threshold)
        return le if chan == 0 else ~le
    thr = np.full(K, f32(threshold)) if thresholds is None else np.asarray(thresholds, np.float32).astype(np.float64)
    xt, xi = (XL, XR) if chan == 0 else (XR, XL)
    return ~(np.abs(xt) <= np.abs(xi) + thr[None, :, None])


def mask_closed_form(XL, XR, kind, chan, threshold, alpha, eta, mu0, thresholds=None):
    """Returns (Y complex128 [S][K][T], mu [S][K][T]); mu0 float64 [S][K] is updated in place (row 0 stays)."""
    XL, XR = np.asarray(XL, np.complex128), np.asarray(XR, np.complex128)
    S, K, T = XL.shape
    one = _mask_decision(XL, XR, kind, chan, threshold, thresholds)
    a = f32(alpha)
    om = f32(np.float32(1) - np.float32(alpha))                  # ( 1 - alpha_ ), a float expression
    ome = f32(np.float32(om) * np.float32(eta))                  # ( 1 - alpha_ ) * dEta_
    X = XL if chan == 0 else XR
    mu = np.zeros((S, K, T))
    Y = np.zeros((S, K, T), np.complex128)
    prev = mu0.copy()
    for t in range(T):
        prev = a * prev + np.where(one[:, :, t], om, ome)
        mu[:, :, t] = prev
        Y[:, :, t] = X[:, :, t] * prev
    Y[:, 0] = XL[:, 0]
    mu[:, 0] = 1.0
    mu0[:, 1:] = prev[:, 1:]
    return Y, mu


def mask_ambiguous(XL, XR, kind, chan, threshold, margin, thresholds=None):
    """Cells [S][K][T] whose decision could fall either way under a relative perturbation `margin` of the decision variables:
    Kim |pd - thr omega_k| <= margin pi (pd the wrapped phase difference); IID ||X_T| - |X_I| - thr| <= margin (|X_T| + |X_I| + |thr|).
    Bin 0 is never decided."""
    XL, XR = np.asarray(XL, np.complex128), np.asarray(XR, np.complex128)
    K = XL.shape[1]
    if kind == KIM:
        amb = np.abs(phase_difference(XL, XR) - f32(threshold) * omega(K)[:, None]) <= margin * np.pi
    else:
        thr = np.full(K, f32(threshold)) if thresholds is None else np.asarray(thresholds, np.float32).astype(np.float64)
        thr = thr[None, :, None]
        xt, xi = (XL, XR) if chan == 0 else (XR, XL)
        amb = np.abs(np.abs(xt) - np.abs(xi) - thr) <= margin * (np.abs(xt) + np.abs(xi) + np.abs(thr))
    amb[:, 0] = False
    return amb


def _iid_terms(XL, XR, eta, pc):
    """|XL|, |XR| and y = |mu X|^(2 pc) for mu = 1, eta: six arrays shaped like XL"""
    pl, pr = np.abs(XL), np.abs(XR)
    e = 2.0 * pc
    return pl, pr, pl ** e, np.abs(XL * eta) ** e, pr ** e, np.abs(XR * eta) ** e


def stats_closed_form(XL, XR, kind, walk, n_cand, eta, pc, k0=1, k1=None):
    """Returns (sums, per_frame): Kim [S][nCand][5], [S][T][nCand][2]; IID [S][nCand][6], [S][T][nCand][6];
    FD-IID [S][K][nCand][3], None.  Slots beyond the walk stay 0."""
    XL, XR = np.asarray(XL, np.complex128), np.asarray(XR, np.complex128)
    S, K, T = XL.shape
    k1 = K if k1 is None else k1
    eta, pc = f32(eta), f32(pc)
    c = np.asarray(walk, np.float32).astype(np.float64)
    nw = c.size
    if kind == FDIID:
        sums = np.zeros((S, K, n_cand, 3))
        pl, pr, a1, ae, b1, be = _iid_terms(XL, XR, eta, pc)
        for t in range(T):
            sl = (slice(None), slice(None), t, None)
            a = np.where(pl[sl] <= pr[sl] + c, ae[sl], a1[sl])           # [S][K][nw]
            b = np.where(pr[sl] <= pl[sl] + c, be[sl], b1[sl])
            a2, b2 = a * a, b * b
            sums[:, 1:, :nw, 0] += (a2 * a2 + b2 * b2)[:, 1:]
            sums[:, 1:, :nw, 1] += (a + b)[:, 1:]
            sums[:, 1:, :nw, 2] += (a2 + b2)[:, 1:]
        return sums, None
    pf = np.zeros((S, T, n_cand, NPF[kind]))
    if kind == KIM:
        d = itd(XL, XR)[:, k0:k1]
        # gsl_complex_abs2(mul_real(X, mu)): |XL|^2, |eta XL|^2, |XR|^2, |eta XR|^2
        p = [((X.real * m) ** 2 + (X.imag * m) ** 2)[:, k0:k1] for X in (XL, XR) for m in (1.0, eta)]
        for t in range(T):
            le = d[:, :, t, None] <= c                                                 # [S][nb][nw]; NaN, inf: never
            PT = np.where(le, p[0][:, :, t, None], p[1][:, :, t, None]).sum(axis=1)
            PI = np.where(le, p[3][:, :, t, None], p[2][:, :, t, None]).sum(axis=1)
            pf[:, t, :nw, 0] = PT ** pc
            pf[:, t, :nw, 1] = PI ** pc
        RT, RI = pf[..., 0], pf[..., 1]
        sums = np.stack([(RT * RI).sum(1), RT.sum(1), RI.sum(1), (RT * RT).sum(1), (RI * RI).sum(1)], axis=-1)
        return sums, pf
    pl, pr, a1, ae, b1, be = [v[:, k0:k1] for v in _iid_terms(XL, XR, eta, pc)]
    for t in range(T):
        sl = (slice(None), slice(None), t, None)
        a = np.where(pl[sl] <= pr[sl] + c, ae[sl], a1[sl])
        b = np.where(pr[sl] <= pl[sl] + c, be[sl], b1[sl])
        a2, b2 = a * a, b * b
        for j, v in enumerate((a, a2, a2 * a2, b, b2, b2 * b2)):
            pf[:, t, :nw, j] = v.sum(axis=1)
    return pf.sum(axis=1), pf


def stats_ambiguous(XL, XR, kind, walk, margin, k0=1, k1=None):
    """Kim / IID: (frame, candidate) pairs [S][T][nWalk] in which some bin's decision lies within the margin (see
    mask_ambiguous); FD-IID: (bin, candidate) pairs [S][K][nWalk] in which some frame's does."""
    XL, XR = np.asarray(XL, np.complex128), np.asarray(XR, np.complex128)
    S, K, T = XL.shape
    k1 = K if k1 is None else k1
    c = np.asarray(walk, np.float32).astype(np.float64)
    if kind == KIM:
        pd, w = phase_difference(XL, XR)[:, k0:k1], omega(K)[k0:k1]
        out = np.zeros((S, T, c.size), bool)
        for t in range(T):
            near = np.abs(pd[:, :, t, None] - c * w[None, :, None]) <= margin * np.pi
            near &= (w > 0)[None, :, None]                       # bin 0: x/0 is never <= anything
            out[:, t] = near.any(axis=1)
        return out
    pl, pr = np.abs(XL), np.abs(XR)
    if kind == IID:
        pl, pr = pl[:, k0:k1], pr[:, k0:k1]
    out = np.zeros((S, K, c.size) if kind == FDIID else (S, T, c.size), bool)
    for t in range(T):
        dl = (pl - pr)[:, :, t, None]
        tol = margin * ((pl + pr)[:, :, t, None] + np.abs(c))
        near = (np.abs(dl - c) <= tol) | (np.abs(-dl - c) <= tol)
        if kind == FDIID:
            out |= near
        else:
            out[:, t] = near.any(axis=1)
    if kind == FDIID:
        out[:, 0] = False
    return out


def threshold_closed_form(kind, sums, count, walk, n_cand, beta=3.0):
    """sums of ONE stream.  Kim / IID: (threshold, cost [nCand]); FD-IID: (threshold, cost [K][nCand], per-bin thresholds [K]).
    Kim and IID keep the FIRST best candidate (<), FD-IID the LAST (<=), per bin and over all bins."""
    c = np.asarray(walk, np.float32)
    nw = c.size
    n = float(count)
    with np.errstate(divide="ignore", invalid="ignore"):
        if kind == KIM:
            v = sums[:nw]
            mt, mi = v[:, 1] / n, v[:, 2] / n
            st, si = v[:, 3] / n - mt * mt, v[:, 4] / n - mi * mi
            cf = v[:, 0] / n
            rho = np.abs((cf - mt * mi) / (np.sqrt(st) * np.sqrt(si)))
        elif kind == IID:
            v = sums[:nw]
            sig2 = v[:, 1] / n + v[:, 4] / n
            cf = (v[:, 2] / n + v[:, 5] / n) - beta * sig2 * sig2
            rho = -cf
        else:
            v = sums[:, :nw]
            sigma = v[..., 2] / n
            cf = v[..., 0] / n - beta * sigma * sigma
            cf[0] = 0.0
            rho = -cf
    if kind != FDIID:
        cost = np.zeros(n_cand)
        cost[:nw] = cf
        arg, best = (c[0] if nw else np.float32(0)), 1000000.0
        for i in range(nw):
            if rho[i] < best:
                arg, best = c[i], rho[i]
        return float(arg), cost
    K = sums.shape[0]
    cost = np.zeros((K, n_cand))
    cost[:, :nw] = cf
    per_bin = np.zeros(K)
    arg, best = np.float32(0), 1000000.0
    for k in range(1, K):
        local = 1000000.0
        for i in range(nw):
            if rho[k, i] <= best:
                arg, best = c[i], rho[k, i]
            if rho[k, i] <= local:
                per_bin[k], local = float(c[i]), rho[k, i]
    return float(arg), cost, per_bin
