"""GPU: btk_hos_eval / btk_hos_minimize (hos_kernels.hip) where their fixtures never take them -- the cases of tests/hos_shapes.py:
2 .. 64 channels that are no multiple of the 8 a wavefront owns, 64 channels with one and two sources and one and two
constraints (D up to 252), blocks of 1 .. 1025 frames around one wavefront and around the 512-frame tile, rows in a buffer
whose every other entry is NaN, masks that select one frame, blank the first tile or select nothing, unselected frames that
hold NaN, Inf and 3e38, the NMEK clamp exactly at its threshold, and optimisations on six shapes in the MEK and NMEK forms with
every exit of the iteration.  test_hos_shapes_cpu.py holds the conditions the cases meet (coverage, decided bins, teeth).

Bounds: the forward-error bounds the float64 restatement (tests/hos_closed_form.py) carries -- fun_err, grad_err, stats_err for
an evaluation, trace_f_err, f_err, x_err for an optimisation -- taken ONCE, as tests/test_gpu_hos.py takes them; every test
prints its largest error / bound, a ratio above 1 fails.  A result that must be finite is asserted finite, and every ratio is
compared on its own with `<=`, which no NaN passes (max() of a list drops one): the NaN around the rows fails the test of any
case whose kernel reads it.  Everything else is equality of bits or of integers.  An optimisation
is compared in full on the bins whose every decision the restatement shows to be further from its threshold than twice the
bound of the compared quantity (cf.minimize_bin's decided); on the other bins up to the first iteration at which the two
halvings traces part.

Found by this file: test_unselected_frames_do_not_count failed in all six cases (N2_Nc1_NS1_T65, N17_Nc1_NS2_T65,
N9_Nc2_NS2_T511, N63_Nc1_NS2_T513, N64_Nc1_NS1_T1024, N64_Nc1_NS2_T1025) with NaN and with Inf in the masked-out frames: fun and
stats kept their bits, every entry of grad was NaN.  Phase 2 multiplied the zero coefficients of an unselected frame with that
frame's samples as loaded; it now reads the first selected frame in their place (hos_kernels.hip).  On finite data no bit of any
result of this file or of test_gpu_hos.py's shapes changed.

Measured on the MI355X (largest error / bound; no bound had to be re-derived):
  hos_eval over the 21 shapes, 3 variants, all masks:  fun 0.013, grad 0.14 (N = 3, T = 513), stats 0.12 (N = 2, T = 65);
                                                       at 64 channels fun <= 0.0011, grad <= 0.046, stats <= 0.0036
  clamp boundary:                                      grad 0.002, stats 0.007
  hos_minimize over the 30 runs:                       f 0.018, x 0.011, accepted f 0.018; all 113 decided bins take the
                                                       restatement's trace, and so do the 7 undecided ones
Every test of this file takes less than 0.2 s.
"""
import numpy as np
import pytest

from tests import hos_closed_form as cf
from tests import hos_shapes as hs
from tests.test_gpu_hos import _merge, _ratios, _state, _t, _vs_restatement

pytestmark = pytest.mark.gpu


def _rows(dev, obs, stride, fill=np.nan):
    """the observations as a [..., :T] view of rows in a buffer that holds `fill` wherever it holds no sample"""
    import torch
    K, N, T = obs.shape
    flat, front = hs.padded_rows(obs, stride, fill)
    return torch.from_numpy(flat).to(dev)[front:front + K * N * stride].view(K, N, stride)[..., :T]


def _eval(dev, c, normalize, gamma, mask=None, with_prev=False, grad=True, obs=None, x=None):
    """numpy (fun, grad or None, stats) of hos_eval on a case of hs.eval_case, rows NaN-padded"""
    from distant_speech_recognition_amd import engine as eng
    X = _rows(dev, c["obs"] if obs is None else obs, c["stride"])
    f, g, s = eng.hos_eval(X, _t(dev, c["wuH"]), _t(dev, c["BmH"]), _t(dev, c["x"] if x is None else x), Nc=c["Nc"], alpha=hs.ALPHA,
                           beta=hs.BETA, gamma=gamma, normalize=normalize, mask=None if mask is None else _t(dev, mask),
                           state=_state(dev, c["prev"] if with_prev else None, hs.K_EVAL, c["NS"]), grad=grad)
    return f.cpu().numpy(), None if g is None else g.cpu().numpy(), s.cpu().numpy()


def _held(gpu, r, what):
    """error / bound of a result that must be finite throughout.  Every ratio is compared with `<=`, which no NaN passes
    (max() of a list and _merge both drop a NaN): a read of the NaN padding or of a masked-out frame fails here."""
    for name, a in zip(("fun", "grad", "stats"), gpu):
        assert np.all(np.isfinite(a)), "%s: %d entries of %s are not finite" % (what, int((~np.isfinite(a)).sum()), name)
    ratios = _ratios(gpu, r)
    assert all(v <= 1.0 for v in ratios.values()), (what, ratios)
    return ratios


def _same_bits(a, b):
    return all((u is None and v is None) or np.array_equal(u, v, equal_nan=True) for u, v in zip(a, b))


@pytest.mark.parametrize("shape", hs.EVAL_SHAPES, ids=hs.name_of)
def test_eval_on_the_shape_cases(dev, shape):
    """every variant and mask kind of the case against the restatement; two runs give equal bits; a mask of ones is no mask;
    grad=False returns the bits grad=True returns; no frame selected: statistics exactly 0, fun and grad within the bounds with
    previous statistics and NaN without"""
    c = hs.eval_case(shape)
    T = c["T"]
    worst = {}
    for normalize, gamma in hs.VARIANTS:
        for kind in hs.eval_masks(T):
            mask, with_prev = hs.mask_of(kind, T)
            gpu = _eval(dev, c, normalize, gamma, mask, with_prev)
            assert _same_bits(gpu, _eval(dev, c, normalize, gamma, mask, with_prev)), ("two runs differ", kind)
            nograd = _eval(dev, c, normalize, gamma, mask, with_prev, grad=False)
            assert nograd[1] is None and _same_bits((gpu[0], gpu[2]), (nograd[0], nograd[2])), ("grad=False differs", kind)
            if kind == "empty_noprev":
                assert np.all(np.isnan(gpu[0])) and np.all(np.isnan(gpu[1])) and np.all(gpu[2] == 0), kind
                continue
            with np.errstate(all="ignore"):
                r = hs.evaluate(c, normalize, gamma, mask, with_prev)
            if kind == "empty_prev":
                assert np.all(gpu[2] == 0) and np.all(r["stats"] == 0)
            _merge(worst, _held(gpu, r, (c["name"], kind, normalize, gamma)))
        ones = _eval(dev, c, normalize, gamma, np.ones(T, np.float32))
        assert _same_bits(ones, _eval(dev, c, normalize, gamma)), "a mask of ones differs from no mask"
    print("hos_eval %-20s masks %s: error / bound %s" % (c["name"], list(hs.eval_masks(T)), {k: "%.3g" % v for k, v in worst.items()}))
    assert set(worst) == {"fun", "grad", "stats"} and all(v <= 1.0 for v in worst.values())


UNSELECTED_SHAPES = ((2, 1, 1, 65), (17, 1, 2, 65), (9, 2, 2, 511), (63, 1, 2, 513), (64, 1, 1, 1024), (64, 1, 2, 1025))


@pytest.mark.parametrize("shape", UNSELECTED_SHAPES, ids=hs.name_of)
def test_unselected_frames_do_not_count(dev, shape):
    """what a masked-out frame holds -- NaN, +Inf, 3e38 -- changes no bit of fun, grad and stats against the same frames set
    to 0; frame T - 1, which the lanes beyond T read, is among them"""
    c = hs.eval_case(shape)
    T = c["T"]
    mask = hs.random_mask(T)
    out = mask == 0
    assert out[T - 1] and out.sum() > T // 5
    for normalize, gamma in hs.VARIANTS:
        base = None
        for fill in (0.0, np.nan, np.inf, 3e38):
            obs = c["obs"].copy()
            obs[:, :, out] = complex(fill, fill)
            got = _eval(dev, c, normalize, gamma, mask, True, obs=obs)
            fun_only = _eval(dev, c, normalize, gamma, mask, True, grad=False, obs=obs)
            if base is None:
                base = got
                _held(base, hs.evaluate(c, normalize, gamma, mask, True), (c["name"], normalize, gamma))
            for name, a, b in zip(("fun", "grad", "stats"), got, base):
                assert np.array_equal(a, b), \
                    "%s changes with masked-out frames of %r (normalize %s, gamma %g): %d entries not finite" % (
                        name, fill, normalize, gamma, int((~np.isfinite(a)).sum()))
            assert np.array_equal(fun_only[0], base[0]) and np.array_equal(fun_only[2], base[2])


@pytest.mark.parametrize("NS", [1, 2])
def test_clamp_boundary(dev, NS):
    """NMEK with gamma = 0.625: ||wa|| = 0.625 exactly (one entry (0.375, 0.5)) is not clamped (`>`) and has the bits of the
    normalize=False run; (0.375, 0.5 + 2^-40) is clamped and lies within the bounds of the restatement"""
    shape = (9, 2, 2, 511) if NS == 2 else (9, 2, 1, 1025)
    c = hs.eval_case(shape)
    dim = c["N"] - c["Nc"]
    x = np.zeros_like(c["x"])
    for s in range(NS):
        j = (3 + 2 * s) % dim
        x[:2, 2 * (s * dim + j)] = 0.375
        x[0, 2 * (s * dim + j) + 1] = 0.5
        x[1, 2 * (s * dim + j) + 1] = 0.5 + 2.0 ** -40
    x[2] = c["x"][1]
    nrm = np.sqrt(np.sum(np.abs(cf.unpack(x, NS, dim)) ** 2, axis=-1))
    assert np.all(nrm[0] == 0.625) and np.all(nrm[1] > 0.625) and np.all(nrm[2] > 0.625)
    nmek = _eval(dev, c, True, 0.625, x=x)
    mek = _eval(dev, c, False, 0.625, x=x)
    assert all(np.array_equal(a[0], b[0]) for a, b in zip(nmek, mek)), "a norm equal to gamma was clamped"
    assert not np.array_equal(nmek[0][1:], mek[0][1:])
    r = hs.evaluate(c, True, 0.625, x=x)
    assert np.all(np.abs(np.sqrt(np.sum(np.abs(r["wa"][:, 1]) ** 2, axis=-1)) - 0.625) < 1e-15)      # the restatement clamps bin 1
    ratios = _held(nmek, r, "clamp boundary")
    print("clamp boundary NS = %d: error / bound %s" % (NS, ratios))


# ------------------------------------------------------------------------------------------------ hos_minimize
def _minimize(dev, run):
    from distant_speech_recognition_amd import engine as eng
    K, NS = hs.K_MIN, run["NS"]
    X = _t(dev, run["obs"].astype(np.complex64)) if run["stride"] is None else _rows(dev, run["obs"], run["stride"])
    args = dict(Nc=run["Nc"], alpha=hs.ALPHA, beta=hs.BETA, gamma=run["opts"]["gamma"], normalize=run["opts"]["normalize"],
                mask=None if run["mask"] is None else _t(dev, run["mask"]))
    opts = {k: v for k, v in run["opts"].items() if k not in ("gamma", "normalize")}
    wuH, BmH = _t(dev, run["wuH"]), _t(dev, run["BmH"])
    res = eng.hos_minimize(X, wuH, BmH, None if run["x0"] is None else _t(dev, run["x0"]), state=_state(dev, run["prev"], K, NS),
                           **args, **opts)
    out = {k: getattr(res, k).cpu().numpy() for k in res._fields}
    f_at_x, _, _ = eng.hos_eval(X, wuH, BmH, res.x, state=_state(dev, run["prev"], K, NS), **args)
    return out, f_at_x.cpu().numpy()


@pytest.mark.parametrize("name", list(hs.min_runs()))
def test_minimize_on_the_shape_runs(dev, name):
    """decided bins: the restatement's halvings trace and iteration count, trace_f, f and x within the bounds; the other bins:
    the common prefix within trace_f_err; every bin: trace_f falls over [:iters] and is NaN behind, halvings are -2 past the
    stop, two runs give equal bits, f has the bits of hos_eval at the returned x; the gtol, mindelta and max_halvings runs stop
    where they must"""
    run = hs.min_runs()[name]
    c = hs.restated(name)
    r, f_at_x = _minimize(dev, run)
    again, _ = _minimize(dev, run)
    assert all(np.array_equal(r[k], again[k], equal_nan=True) for k in r), "two runs differ"
    assert np.all(np.isfinite(r["x"])) and np.all(np.isfinite(r["f"])), "x or f is not finite"
    assert np.array_equal(r["f"], f_at_x), "f is not hos_eval at the returned x"
    worst = {"f": 0.0, "x": 0.0, "trace_f": 0.0}
    undecided_split = []
    for k in range(hs.K_MIN):
        n = int(r["iters"][k])
        tf, th = r["trace_f"][k], r["trace_halvings"][k]
        assert 0 <= n <= hs.MIN_MAXITER and np.all(np.isnan(tf[n:])) and np.all(np.isfinite(tf[:n])) and np.all(np.diff(tf[:n]) <= 0)
        assert np.all(th[:n] >= 0) and np.all(th[n + 1:] == -2) and (n == hs.MIN_MAXITER or th[n] in (-1, -2))
        if n:
            assert tf[n - 1] == r["f"][k]
        same, rf, rx, pre = _vs_restatement(r, {key: c[key][k] for key in c}, k)
        assert pre <= 1.0, (name, k, "accepted f", pre)                 # `<=` on each ratio: a NaN fails, max() would drop it
        worst["trace_f"] = max(worst["trace_f"], pre)
        if c["decided"][k]:
            assert same, "%s bin %d is decided (margin / (2 bound) %.3g) and differs: %s against %s" % (
                name, k, c["decided_ratio"][k], th.tolist(), c["trace_halvings"][k].tolist())
        if same:
            assert rf <= 1.0 and rx <= 1.0, (name, k, "f, x", rf, rx)
            worst["f"], worst["x"] = max(worst["f"], rf), max(worst["x"], rx)
        else:
            undecided_split.append(k)
    x0 = np.zeros_like(r["x"]) if run["x0"] is None else run["x0"]
    if name.endswith("_gtol"):
        assert np.all(r["iters"] == 0) and np.array_equal(r["x"], x0) and np.all(r["trace_halvings"] == -2)
    if name.endswith("_mindelta"):
        assert np.array_equal(r["iters"], (r["trace_halvings"][:, 0] >= 0).astype(r["iters"].dtype)) and r["iters"].any()
    if name.endswith("_halvings0"):
        assert np.all(r["trace_halvings"] <= 0) and (r["trace_halvings"] == -1).any()
    print("hos_minimize %-28s decided %d of %d, undecided bins that part %s, iterations %s: error / bound %s" % (
        name, c["decided"].sum(), hs.K_MIN, undecided_split, r["iters"].tolist(), {k: "%.3g" % v for k, v in worst.items()}))
    assert all(v <= 1.0 for v in worst.values())
