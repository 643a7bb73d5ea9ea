"""Shape cases for the maximum-kurtosis kernels beyond their fixtures (no test in here; imported by test_hos_shapes_cpu.py and
test_gpu_hos_shapes.py): channel counts that are no multiple of the 8 a wavefront owns, block lengths around one wavefront and
around the 512-frame tile, both sources at 64 channels, masks that select one frame, blank a tile or select nothing, rows in a
buffer whose padding is NaN, and optimisations whose every decision is away from its threshold.

Nothing is stored: the problems are drawn as _random_problem of test_gpu_hos.py draws them (complex64-representable
observations, wuH / N, blocking matrices of engine.weights_blocking_matrix, x inside and outside the NMEK clamp, previous
statistics) from fixed seeds; the yardstick is the float64 restatement tests/hos_closed_form.py with the bounds it carries.

  * EVAL_SHAPES: (N, Nc, NS, T), K = 3 bins each; eval_case(shape) -> the problem; eval_masks(T) -> the mask kinds of a case;
    mask_of(kind, T) -> (mask or None, with previous statistics).
  * padded_rows(obs, stride, fill): the observations as rows of a flat buffer, everything that is no sample set to `fill`.
  * MIN_SHAPES: (N, T, NS, Nc), K = 4 bins each, observations drawn as cubed normals; min_runs() -> name -> run, each with the
    arguments of hos_minimize; restated(name) -> cf.minimize of a run with its decisions, once per process.
  * mutations(case, ...): the restatement on inputs changed in one place (the teeth of test_hos_shapes_cpu.py).
"""
import functools

import numpy as np

from tests import hos_closed_form as cf

ALPHA, BETA = 0.01, 3.0
VARIANTS = ((False, -1.0), (True, -1.0), (True, 0.4))                  # (normalize, gamma): MEK, NMEK gamma = ||wuH||, NMEK gamma > 0
K_EVAL, K_MIN, MIN_MAXITER = 3, 4, 8
TILE, CPW = 512, 8                                                     # frames per tile, channels per wavefront

# ---- evaluation ----------------------------------------------------------------------------------------------------------------
EVAL_PAIRS = ((2, 1), (3, 2), (7, 1), (9, 2), (17, 1), (33, 2), (63, 1), (63, 2), (64, 1), (64, 2))
EVAL_T = (1, 63, 64, 65, 511, 512, 513, 1024, 1025)
EVAL_SHAPES = (
    # NS = 2: every T with an N that is no multiple of 8                  NS = 1
    (3, 2, 2, 1), (7, 1, 2, 63), (2, 1, 2, 64), (17, 1, 2, 65),          (2, 1, 1, 65), (3, 2, 1, 513), (7, 1, 1, 512),
    (9, 2, 2, 511), (33, 2, 2, 512), (63, 1, 2, 513), (63, 2, 2, 1024),  (9, 2, 1, 1025), (17, 1, 1, 1), (33, 2, 1, 63),
    (7, 1, 2, 1025),                                                     (63, 1, 1, 1024), (63, 2, 1, 511),
    # 64 channels: D = 252 and 248 with two sources, 126 and 124 with one
    (64, 1, 2, 1025), (64, 2, 2, 513), (64, 1, 1, 1024), (64, 2, 1, 65),
)
MASK_KINDS = ("none", "random", "first", "last", "tile0_blank", "empty_prev", "empty_noprev")


def name_of(shape):
    return "N%d_Nc%d_NS%d_T%d" % tuple(shape)


def random_problem(seed, K, N, T, NS, Nc, cubed=False):
    """_random_problem of test_gpu_hos.py; cubed=True draws the observations as cubed normals (heavy tails: the kurtosis has
    something to move) and keeps every previous frame count above zero"""
    from distant_speech_recognition_amd import engine as eng
    rng = np.random.default_rng(seed)
    re, im = rng.normal(size=(K, N, T)), rng.normal(size=(K, N, T))
    if cubed:
        re, im = re ** 3, im ** 3
    obs = (re + 1j * im).astype(np.complex64).astype(np.complex128)
    wuH = (rng.normal(size=(NS, K, N)) + 1j * rng.normal(size=(NS, K, N))) / N
    BmH = np.zeros((NS, K, N - Nc, N), complex)
    for s in range(NS):
        for k in range(K):
            BmH[s, k] = eng.weights_blocking_matrix(np.conjugate(wuH[s, k]), Nc).T
    D = 2 * NS * (N - Nc)
    x = rng.normal(size=(K, D)) * np.where(rng.random((K, 1)) < 0.5, 0.02, 1.0)       # inside and outside the clamp
    prev = (rng.random((K, NS)) * 2.0, rng.random((K, NS)) * 8.0, rng.integers(1, 500, size=(K, NS)))
    return obs, wuH, BmH, x, prev


@functools.lru_cache(maxsize=None)
def eval_case(shape):
    """dict(name, N, Nc, NS, T, stride, obs, wuH, BmH, x, prev); x: bin 0 inside the clamp, bin 1 outside, bin 2 as drawn"""
    N, Nc, NS, T = shape
    obs, wuH, BmH, x, prev = random_problem(1000 + 97 * N + 13 * T + 5 * NS + Nc, K_EVAL, N, T, NS, Nc)
    rng = np.random.default_rng(7 + N + T)
    x[0] = 0.02 / np.sqrt(x.shape[1]) * rng.normal(size=x.shape[1])
    x[1] = (2.0 + np.abs(rng.normal(size=x.shape[1]))) * np.where(rng.random(x.shape[1]) < 0.5, -1.0, 1.0)
    return dict(name=name_of(shape), N=N, Nc=Nc, NS=NS, T=T, stride=T + 1 + (N + T) % 5, obs=obs, wuH=wuH, BmH=BmH, x=x, prev=prev)


def eval_masks(T):
    if T < 65:
        return ("none",)
    return tuple(k for k in MASK_KINDS if k != "tile0_blank" or T > TILE)


def random_mask(T, seed=5, keep=0.6):
    """0/1 with frame 0 selected and frame T - 1 not (the lanes beyond T read that one)"""
    m = (np.random.default_rng(seed + T).random(T) < keep).astype(np.float32)
    m[0], m[T - 1] = 1.0, 0.0
    return m


def mask_of(kind, T):
    """(mask float32 [T] or None, with previous statistics)"""
    m = np.zeros(T, np.float32)
    if kind == "none":
        return None, False
    if kind == "random":
        return random_mask(T), True
    if kind == "first":
        m[0] = 1.0
        return m, False
    if kind == "last":
        m[T - 1] = 1.0
        return m, True
    if kind == "tile0_blank":
        m[TILE:] = 1.0
        return m, False
    if kind == "empty_prev":
        return m, True
    if kind == "empty_noprev":
        return m, False
    raise KeyError(kind)


def padded_rows(obs, stride, fill=np.nan, front=37, back=41):
    """(flat complex64 buffer, offset of the first row): the K N rows of `stride` samples each, `front` samples in front of the
    first and `back` behind the last; every entry that is no sample -- behind T in each row, in front, behind -- is `fill`"""
    K, N, T = obs.shape
    assert stride > T
    flat = np.full(front + K * N * stride + back, complex(fill, fill), np.complex64)
    flat[front:front + K * N * stride].reshape(K, N, stride)[..., :T] = obs.astype(np.complex64)
    return flat, front


def evaluate(case, normalize, gamma, mask=None, with_prev=False, want_grad=True, **over):
    """the restatement on a case; over: obs, wuH, BmH or x replaced"""
    g = dict(case, **over)
    return cf.evaluate(g["obs"], g["wuH"], g["BmH"], g["x"], ALPHA, BETA, gamma, normalize, mask=mask,
                       prev=case["prev"] if with_prev else None, want_grad=want_grad)


# ---- teeth ---------------------------------------------------------------------------------------------------------------------
def from_woH(case, r, wt, hole=False, v_from=None):
    """fun and grad in the formulas of cf.evaluate (no previous statistics) with the frames weighted by wt [T] in every sum over
    frames while the frame count stays the number of non-zero entries of the mask the caller compares under: wt = that mask
    restates cf.evaluate.  hole: channel N - 1 is left out of Y = woH . X, and so of everything that follows from Y.  v_from:
    the source whose sums over the frames every source's gradient uses."""
    X, BmH = case["obs"], case["BmH"]
    woH, wa = r["woH"].copy(), r["wa"]
    if hole:
        woH[:, :, -1] = 0.0
    n = float(r["frames"])
    Y = np.einsum("skn,knt->skt", woH, X)
    Y2 = np.abs(Y) ** 2
    sum2, sum4 = (wt * Y2).sum(-1), (wt * Y2 ** 2).sum(-1)
    kurt = (sum4 / n).sum(0) - BETA * (sum2 / n).sum(0) ** 2
    fun = -(kurt + cf.OFFSET) + ALPHA * np.sum(np.abs(wa) ** 2, axis=-1).sum(0)
    g = []
    for c in (2 * Y2 * np.conj(Y), np.conj(Y)):
        v = np.einsum("skt,knt->skn", wt * c, X)
        if v_from is not None:
            v = np.broadcast_to(v[v_from], v.shape)
        g.append(-np.einsum("skjn,skn->skj", BmH, v) / n)
    grad = -(g[0] - 2 * BETA * (sum2 / n)[..., None] * g[1]) + ALPHA * wa
    return dict(fun=fun, grad=cf.pack(np.moveaxis(grad, 0, -2)))


def mutations(case, normalize, gamma):
    """name -> (fun and grad of a kernel that is wrong in one place, the mask it runs under, the restatement under that mask):
    channel N - 1 lost in phase 1, frame T - 1 lost, frame T - 1 counted twice, source 0's sums used for source 1, one
    masked-out frame let through.  "none" is from_woH unchanged: it has to restate cf.evaluate."""
    T = case["T"]
    ones = np.ones(T)
    r = evaluate(case, normalize, gamma)
    last0, last2 = ones.copy(), ones.copy()
    last0[T - 1], last2[T - 1] = 0.0, 2.0
    out = {"none": (from_woH(case, r, ones), None, r),
           "drop_channel": (from_woH(case, r, ones, hole=True), None, r),
           "drop_frame": (from_woH(case, r, last0), None, r),
           "double_frame": (from_woH(case, r, last2), None, r)}
    if case["NS"] == 2:
        out["source0_v"] = (from_woH(case, r, ones, v_from=0), None, r)
    m = random_mask(T)
    rm = evaluate(case, normalize, gamma, mask=m)
    leak = m.astype(np.float64)
    gone = np.flatnonzero(m == 0)
    leak[gone[len(gone) // 2]] = 1.0
    out["none_masked"] = (from_woH(case, rm, m.astype(np.float64)), m, rm)
    out["mask_leak"] = (from_woH(case, rm, leak), m, rm)
    return out


# ---- minimisation --------------------------------------------------------------------------------------------------------------
MIN_SHAPES = ((2, 65, 1, 1), (3, 513, 2, 2), (9, 511, 1, 1), (17, 512, 2, 1), (63, 130, 1, 2), (64, 1025, 2, 1))     # (N, T, NS, Nc)
MIN_KINDS = ("plain", "mek", "gamma", "busy")
MIN_EXTRA_SHAPES = ((9, 511, 1, 1), (17, 512, 2, 1))                   # one with NS = 1, one with NS = 2
MIN_EXTRAS = {"halvings0": dict(max_halvings=0), "gtol": dict(gtol=1e30), "mindelta": dict(mindelta=1e30)}
MEK_SCALE = 0.005
# seeds per run (3 where none is given), picked so that the conditions of tests/test_hos_shapes_cpu.py hold: at least three of
# the four bins decided
MIN_SEED = {
    "N2_T65_NS1_Nc1_plain": 28, "N2_T65_NS1_Nc1_gamma": 28, "N2_T65_NS1_Nc1_busy": 8, "N3_T513_NS2_Nc2_plain": 4,
    "N3_T513_NS2_Nc2_busy": 39, "N9_T511_NS1_Nc1_plain": 18, "N9_T511_NS1_Nc1_gamma": 39, "N17_T512_NS2_Nc1_plain": 26,
    "N17_T512_NS2_Nc1_gamma": 26, "N17_T512_NS2_Nc1_busy": 15, "N63_T130_NS1_Nc2_plain": 9, "N63_T130_NS1_Nc2_gamma": 1,
    "N63_T130_NS1_Nc2_busy": 30, "N64_T1025_NS2_Nc1_plain": 11, "N64_T1025_NS2_Nc1_gamma": 4, "N64_T1025_NS2_Nc1_busy": 30,
    "N9_T511_NS1_Nc1_halvings0": 3, "N9_T511_NS1_Nc1_gtol": 1, "N9_T511_NS1_Nc1_mindelta": 1, "N17_T512_NS2_Nc1_halvings0": 1,
    "N17_T512_NS2_Nc1_gtol": 1, "N17_T512_NS2_Nc1_mindelta": 1, "N3_T513_NS2_Nc2_gamma": 93, "N2_T65_NS1_Nc1_mek": 5, "N9_T511_NS1_Nc1_busy": 303,
}


def min_name(shape, kind):
    return "N%d_T%d_NS%d_Nc%d_%s" % (tuple(shape) + (kind,))


@functools.lru_cache(maxsize=None)
def min_run(shape, kind):
    """dict(name, N, T, NS, Nc, obs, wuH, BmH, x0 (None: zeros), mask, prev, stride (None: contiguous), opts: normalize, gamma and
    the optimiser's options)"""
    N, T, NS, Nc = shape
    name = min_name(shape, kind)
    seed = MIN_SEED.get(name, 3)
    obs, wuH, BmH, x, prev = random_problem(seed, K_MIN, N, T, NS, Nc, cubed=True)
    run = dict(name=name, N=N, T=T, NS=NS, Nc=Nc, obs=obs, wuH=wuH, BmH=BmH, x0=None, mask=None, prev=None, stride=None,
               opts=dict(normalize=True, gamma=-1.0, maxiter=MIN_MAXITER))
    if kind == "mek":
        # Without the clamp the objective is unbounded below (-|w|^4): at unit scale the iteration leaves every basin and
        # overflows within four iterations.  At MEK_SCALE times the scale the regulariser holds it: from a start of norm 6 it
        # takes two or three steps towards the origin and stops at gtol, every value finite.
        rng = np.random.default_rng(seed + 1)
        run["obs"] = (MEK_SCALE * obs).astype(np.complex64).astype(np.complex128)
        run["x0"] = 6.0 / np.sqrt(x.shape[1]) * rng.normal(size=x.shape)
        run["opts"]["normalize"] = False
    elif kind == "gamma":
        run["opts"]["gamma"] = 0.4
    elif kind == "busy":
        run.update(x0=0.05 * x, mask=random_mask(T), prev=prev, stride=T + 3)
    elif kind in MIN_EXTRAS:
        run["opts"].update(MIN_EXTRAS[kind])
    elif kind != "plain":
        raise KeyError(kind)
    return run


def min_runs():
    out = {}
    for shape in MIN_SHAPES:
        for kind in MIN_KINDS:
            out[min_name(shape, kind)] = min_run(shape, kind)
    for shape in MIN_EXTRA_SHAPES:
        for kind in MIN_EXTRAS:
            out[min_name(shape, kind)] = min_run(shape, kind)
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """cf.minimize of a run, once per process"""
    r = min_runs()[name]
    return cf.minimize(r["obs"], r["wuH"], r["BmH"], r["x0"], ALPHA, BETA, r["opts"]["gamma"], r["opts"]["normalize"],
                       mask=r["mask"], prev=r["prev"], decisions=True, **{k: v for k, v in r["opts"].items() if k not in ("gamma", "normalize")})
