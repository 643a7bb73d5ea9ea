"""Float64 numpy restatement of the maximum-empirical-kurtosis beamformers' objective, gradient and statistics
(reference lib/pybeamformer.py:1548-1593, 1618-1683, 1845-1860) and of the Polak-Ribiere+ / Armijo optimiser of DESIGN.md 3.15,
vectorised over bins and frames.  Every value comes with a forward-error bound.

The bound is the classical one for float64 sums, n u sum |terms| with u = 2^-53, with the term counts of the computation:
a complex dot product of length n is 2 n real products per component (bound (2 n + 2) u sum |a||b|), N terms per frame for Y,
T per frame reduction, N for the BmH product; it is carried to first order through |Y|^2, |Y|^4, exY4 - beta exY2^2, the offset
1e6 and the products of the gradient.  It bounds the distance of ONE float64 evaluation (in any summation order, with or without
fused multiply-adds) from the exact value; a comparison of two such evaluations that both round (this file against the
reference's own numbers) takes twice the bound.
"""
import numpy as np

U = 2.0 ** -53
OFFSET = -1.0e6
DEFAULTS = dict(maxiter=40, gtol=1.0e-2, mindelta=1.0e-5, max_halvings=30, armijo_c1=1.0e-4)


def unpack(x, NS, dim):
    x = np.asarray(x, np.float64)
    return (x[..., 0::2] + 1j * x[..., 1::2]).reshape(x.shape[:-1] + (NS, dim))


def pack(w):
    w = np.asarray(w)
    out = np.zeros(w.shape[:-2] + (2 * w.shape[-2] * w.shape[-1],), np.float64)
    flat = w.reshape(w.shape[:-2] + (-1,))
    out[..., 0::2], out[..., 1::2] = flat.real, flat.imag
    return out


def evaluate(X, wuH, BmH, x, alpha, beta, gamma, normalize, mask=None, prev=None, want_grad=True):
    """X complex [K][N][T], wuH [NS][K][N], BmH [NS][K][dim][N], x float64 [K][2 NS dim] -> dict of values and bounds:
    fun, fun_err [K]; grad, grad_err [K][D]; stats, stats_err [K][2 NS + 2] (sum |Y_s|^2, sum |Y_s|^4 per source, then the sums of
    m_t and m_t^2, m_t = sum_s |Y_s|^2 / NS); kurt (calc_obj_func without the offset) and wa, woH."""
    X = np.asarray(X, np.complex128)
    wuH, BmH = np.asarray(wuH, np.complex128), np.asarray(BmH, np.complex128)
    NS, K, dim, N = BmH.shape
    if mask is not None:
        X = X[:, :, np.asarray(mask) != 0]
    T = X.shape[2]
    wa = np.moveaxis(unpack(x, NS, dim), -2, 0)                        # [NS][K][dim]
    e_wa = np.zeros(wa.shape)
    if normalize:
        nrm = np.sqrt(np.sum(np.abs(wa) ** 2, axis=-1))
        gam = np.sqrt(np.sum(np.abs(wuH) ** 2, axis=-1)) if gamma < 0 else np.full(nrm.shape, abs(gamma))
        clamp = nrm > np.abs(gam)
        scale = np.where(clamp, np.abs(gam) / np.where(nrm > 0, nrm, 1.0), 1.0)
        wa = np.where(clamp[..., None], np.abs(gam)[..., None] * wa / np.where(nrm > 0, nrm, 1.0)[..., None], wa)
        e_wa = np.where(clamp[..., None], (dim + N + 6) * U * np.abs(wa), 0.0)
        del scale
    aX, aB = np.abs(X), np.abs(BmH)
    prod = np.einsum("skj,skjn->skn", np.conj(wa), BmH)
    woH = wuH - prod
    e_w = (2 * dim + 3) * U * (np.abs(wuH) + np.einsum("skj,skjn->skn", np.abs(wa), aB)) + np.einsum("skj,skjn->skn", e_wa, aB)
    Y = np.einsum("skn,knt->skt", woH, X)
    e_Y = (2 * N + 2) * U * np.einsum("skn,knt->skt", np.abs(woH), aX) + np.einsum("skn,knt->skt", e_w, aX)
    aY = np.abs(Y)
    Y2 = aY ** 2
    e_Y2 = 2 * aY * e_Y + 3 * U * Y2
    Y4 = Y2 ** 2
    e_Y4 = 2 * Y2 * e_Y2 + U * Y4
    sum2, sum4 = Y2.sum(-1), Y4.sum(-1)                                # [NS][K]
    e_sum2 = T * U * sum2 + e_Y2.sum(-1)
    e_sum4 = T * U * sum4 + e_Y4.sum(-1)
    m = Y2.sum(0) / NS
    e_m = e_Y2.sum(0) / NS + (NS + 1) * U * m
    mix2, mix4 = m.sum(-1), (m ** 2).sum(-1)
    e_mix2 = T * U * mix2 + e_m.sum(-1)
    e_mix4 = T * U * mix4 + (2 * m * e_m + U * m ** 2).sum(-1)
    if prev is None:
        pY2 = pY4 = np.zeros((K, NS)); pN = np.zeros((K, NS), np.int64)
    else:
        pY2, pY4, pN = (np.asarray(p) for p in prev)
    pY2, pY4, pN = pY2.T, pY4.T, pN.T.astype(np.float64)              # [NS][K]
    ntot = pN + T
    ex4s = (pY4 * pN + sum4) / ntot
    ex2s = (pY2 * pN + sum2) / ntot
    e_ex4s = (e_sum4 + 2 * U * (np.abs(pY4 * pN) + sum4)) / ntot + U * np.abs(ex4s)
    e_ex2s = (e_sum2 + 2 * U * (np.abs(pY2 * pN) + sum2)) / ntot + U * np.abs(ex2s)
    ex4, ex2 = ex4s.sum(0), ex2s.sum(0)
    e_ex4 = e_ex4s.sum(0) + NS * U * np.abs(ex4s).sum(0)
    e_ex2 = e_ex2s.sum(0) + NS * U * np.abs(ex2s).sum(0)
    kurt = ex4 - beta * ex2 * ex2
    e_kurt = e_ex4 + abs(beta) * 2 * np.abs(ex2) * e_ex2 + 3 * U * (np.abs(ex4) + abs(beta) * ex2 * ex2)
    reg = np.sum(np.abs(wa) ** 2, axis=-1)                             # [NS][K]
    e_reg = (2 * dim + 2) * U * reg + 2 * np.sum(np.abs(wa) * e_wa, axis=-1)
    fun = -(kurt + OFFSET) + alpha * reg.sum(0)
    e_fun = e_kurt + 2 * U * (np.abs(kurt) + abs(OFFSET)) + abs(alpha) * (e_reg.sum(0) + (NS + 1) * U * reg.sum(0)) + U * np.abs(fun)
    out = dict(fun=fun, fun_err=e_fun, kurt=kurt, kurt_err=e_kurt, wa=wa, woH=woH, woH_err=e_w, frames=T,
               stats=np.concatenate([np.stack([sum2, sum4], -1).transpose(1, 0, 2).reshape(K, 2 * NS), mix2[:, None], mix4[:, None]], 1),
               stats_err=np.concatenate([np.stack([e_sum2, e_sum4], -1).transpose(1, 0, 2).reshape(K, 2 * NS), e_mix2[:, None], e_mix4[:, None]], 1))
    if not want_grad:
        return out
    c2 = np.conj(Y)
    c4 = 2 * Y2 * c2
    e_c2 = e_Y
    e_c4 = 2 * (e_Y2 * aY + Y2 * e_Y) + 2 * U * np.abs(c4)
    g = []
    for c, e_c in ((c4, e_c4), (c2, e_c2)):
        v = np.einsum("skt,knt->skn", c, X)
        e_v = (2 * T + 2) * U * np.einsum("skt,knt->skn", np.abs(c), aX) + np.einsum("skt,knt->skn", e_c, aX)
        p = np.einsum("skjn,skn->skj", BmH, v)
        e_p = (2 * N + 2) * U * np.einsum("skjn,skn->skj", aB, np.abs(v)) + np.einsum("skjn,skn->skj", aB, e_v)
        d = -p / ntot[..., None]
        g.append((d, e_p / ntot[..., None] + U * np.abs(d)))
    (d4, e_d4), (d2, e_d2) = g
    ex2g = (sum2 / ntot)[..., None]
    e_ex2g = (e_sum2 / ntot)[..., None] + U * ex2g
    grad = -(d4 - 2 * beta * ex2g * d2) + alpha * wa
    e_grad = (e_d4 + 2 * abs(beta) * (e_ex2g * np.abs(d2) + ex2g * e_d2)
              + 4 * U * (np.abs(d4) + 2 * abs(beta) * ex2g * np.abs(d2) + abs(alpha) * np.abs(wa)) + abs(alpha) * e_wa)
    out["grad"] = pack(np.moveaxis(grad, 0, -2))
    e = np.moveaxis(e_grad, 0, -2).reshape(K, -1)
    out["grad_err"] = np.repeat(e, 2, axis=-1)                         # the bound of a complex entry holds for both components
    return out


def store_stats(prev, stats, frames, NS):
    """store_stats (:1618-1627) as written there: prevFrameN grows first, then every frame adds Y2 / prevFrameN, Y4 / prevFrameN."""
    pY2, pY4, pN = (np.array(p) for p in prev)
    pN = pN + int(frames)
    return pY2 + stats[:, 2 * NS:2 * NS + 1] / pN, pY4 + stats[:, 2 * NS + 1:2 * NS + 2] / pN, pN


def minimize_bin(X, wuH, BmH, x0, alpha, beta, gamma, normalize, mask=None, prev=None, **options):
    """The optimiser of DESIGN.md 3.15 on ONE bin (X [1][N][T], ...): dict(x, f, iters, trace_f, trace_halvings, f0, g0norm,
    f_err, x_err, trace_f_err).  x_err / f_err: first-order propagation of the gradient bounds through the accepted steps, with
    the sensitivity of the gradient to x taken from the secant ||g' - g|| / ||x' - x|| of the iterates; trace_f_err[i] is f_err
    as it stands after iteration i (the evaluation's own bound at that point plus ||g|| times the bound of the point).

    decisions: one (iteration, kind, margin, bound) per comparison the iteration takes -- "gtol" (gnorm < gtol), "gd" (gd >= 0),
    "armijo" (one per trial), "pr" (pr > 0), "mindelta" (df < mindelta).  margin: the distance of the compared quantity from its
    threshold.  bound: what ONE run may be off by in that quantity, from fun_err of the evaluations involved, the drift of the
    point (x_err, a ed for a trial point) times the slope 2 ||g|| there (dfun_hos_bf is half the derivative), and grad_err (with
    the secant's sensitivity times the drift) through the dot products.  Two runs that both round -- the kernel and this file --
    take the same decision when margin > 2 bound: decided says so for the whole trace, decided_ratio is the smallest
    margin / (2 bound).  These three keys are returned with decisions=True only: the bound of an Armijo trial takes the
    gradient at the trial point, a second evaluation per trial that the optimiser itself never makes."""
    want_decisions = bool(options.pop("decisions", False))
    o = dict(DEFAULTS, **options)
    maxiter = int(o["maxiter"])

    def ev(x, want_grad):
        r = evaluate(X, wuH, BmH, x[None], alpha, beta, gamma, normalize, mask, prev, want_grad)
        return (r["fun"][0], r["fun_err"][0]) + ((r["grad"][0], r["grad_err"][0]) if want_grad else ())

    x = np.array(x0, np.float64)
    f, fe, g, ge = ev(x, True)
    f0, g0norm = f, float(np.sqrt(np.dot(g, g)))
    d = -g
    trace_f = np.full(maxiter, np.nan)
    trace_fe = np.full(maxiter, np.nan)
    halv = np.full(maxiter, -2, np.int32)
    step, it = 0.0, 0
    ex, ed, lip = 0.0, float(np.linalg.norm(ge)), 0.0
    decisions = []
    eg = float(np.linalg.norm(ge))                                     # bound of g as a vector: its own rounding, then the drift
    while it < maxiter:
        gg = float(np.dot(g, g))
        gd = float(np.dot(g, d))
        gnorm = np.sqrt(gg)
        decisions.append((it, "gtol", abs(gnorm - o["gtol"]), eg + 4 * U * gnorm))
        if gnorm < o["gtol"]:
            break
        e_gd = gnorm * ed + float(np.linalg.norm(d)) * eg + (len(g) + 2) * U * float(np.dot(np.abs(g), np.abs(d)))
        decisions.append((it, "gd", abs(gd), e_gd))
        if gd >= 0:
            d, gd = -g, -gg
            e_gd = 2 * gnorm * eg + (len(g) + 2) * U * gg
        f_here = fe + 2 * gnorm * ex                                   # bound of f: the evaluation's own, then the drift of x
        a = 2.0 / gnorm if it == 0 else 2.0 * step
        ok = False
        for h in range(int(o["max_halvings"]) + 1):
            xt = x + a * d
            ft, fte = ev(xt, False)
            rhs = f + o["armijo_c1"] * a * gd
            if want_decisions:
                slope = 2 * float(np.linalg.norm(ev(xt, True)[2]))     # for the bound alone: the optimiser takes no gradient here
                e_xt = ex + a * ed + 4 * U * float(np.linalg.norm(xt))
                decisions.append((it, "armijo", abs(ft - rhs), fte + slope * e_xt + f_here + o["armijo_c1"] * a * e_gd
                                  + 4 * U * (abs(f) + abs(rhs))))
            if ft <= rhs:
                ok = True
                break
            a *= 0.5
        if not ok:
            halv[it] = -1
            break
        _, _, gn, gne = ev(xt, True)
        dx = float(np.linalg.norm(xt - x))
        if dx > 0:
            lip = max(lip, float(np.linalg.norm(gn - g)) / dx)
        ex = ex + a * ed + 4 * U * float(np.linalg.norm(xt))
        pr = max(0.0, float(np.dot(gn, gn - g)) / gg)
        egn = float(np.linalg.norm(gne)) + lip * ex
        gnn, dgn = float(np.linalg.norm(gn)), float(np.linalg.norm(gn - g))
        decisions.append((it, "pr", abs(float(np.dot(gn, gn - g))), egn * dgn + gnn * (egn + eg) + (len(g) + 2) * U * gnn * dgn))
        ed = float(np.linalg.norm(gne)) + lip * ex + pr * ed
        d = -gn + pr * d
        trace_f[it], halv[it] = ft, h
        trace_fe[it] = fte + float(np.sqrt(np.dot(gn, gn))) * ex
        df = abs(f - ft)
        decisions.append((it, "mindelta", abs(df - o["mindelta"]), f_here + fte + 2 * gnn * ex + 2 * U * (abs(f) + abs(ft))))
        x, f, fe, g, step, eg = xt, ft, fte, gn, a, egn
        it += 1
        if df < o["mindelta"]:
            break
    out = dict(x=x, f=f, iters=it, trace_f=trace_f, trace_halvings=halv, f0=f0, g0norm=g0norm,
               x_err=ex, f_err=fe + float(np.sqrt(np.dot(g, g))) * ex, trace_f_err=trace_fe)
    if not want_decisions:
        return out
    # a margin or bound that is no number (an objective that overflowed) decides nothing
    ratio = min([(m / (2 * b) if b > 0 else np.inf) if np.isfinite(m) and np.isfinite(b) else 0.0 for _, _, m, b in decisions],
                default=np.inf)
    out.update(decisions=decisions, decided=bool(ratio > 1.0), decided_ratio=float(ratio))
    return out


def minimize(X, wuH, BmH, x0, alpha, beta, gamma, normalize, mask=None, prev=None, **options):
    """minimize_bin for every bin: dict of stacked arrays (decisions, with decisions=True: one list per bin)."""
    NS, K, dim, N = np.asarray(BmH).shape
    res = []
    for k in range(K):
        p = None if prev is None else tuple(np.asarray(q)[k:k + 1] for q in prev)
        x0k = np.zeros(2 * NS * dim) if x0 is None else x0[k]
        res.append(minimize_bin(X[k:k + 1], wuH[:, k:k + 1], BmH[:, k:k + 1], x0k, alpha, beta, gamma, normalize, mask, p, **options))
    out = {key: np.array([r[key] for r in res]) for key in res[0] if key != "decisions"}
    if "decisions" in res[0]:
        out["decisions"] = np.empty(K, object)                         # the lists differ in length
        out["decisions"][:] = [r["decisions"] for r in res]
    return out
