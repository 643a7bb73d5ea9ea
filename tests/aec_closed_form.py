"""Float64 (or longdouble) restatement of the four subband echo cancellers of the reference's aec/aec.cc, written from the source
and loop-faithful in frame and bin order.  Not a port of the engine: it shares no code with csrc/aec_kernels.hip.

    kind 0  NLMSAcousticEchoCancellationFeature::next            aec.cc:34-80
    kind 1  KalmanFilterEchoCancellationFeature::next            aec.cc:85-165
    kind 2  BlockKalmanFilterEchoCancellationFeature::next       aec.cc:172-307
    kind 3  DTDBlockKalmanFilterEchoCancellationFeature::next    aec.cc:801-942

V (played) and A (recorded) are [Kb][T] arrays of the bins 0..M/2 that the reference computes (any number of rows: the kind-3
scalars pass from row to row in order).  run() returns the residual E [Kb][T], the update flags [Kb][T], the final state and the
smallest margin of every gate decision, so that a test can assert its inputs sit away from every branch:

    kinds 0-2   | |v_0|^2 - threshold | / threshold                            (update_, strict >)
    kind 3      | snr_ - snr_threshold | / snr_threshold, | SkEnergy_ - energy_threshold | / energy_threshold   past frame 100
                | snr_ |  where sf = 2 / (1 + exp(-snr_)) - 1 decides by its sign (exact zeros excluded: with zero weights Sk is
                exactly 0, snr_ = 0 and sf = 0 on any arithmetic)
"""
import numpy as np

DEFAULTS = (
    dict(delta=100.0, epsilon=1.0e-4, threshold=100.0),
    dict(beta=0.95, sigma2=100.0, threshold=100.0),
    dict(beta=0.95, sigmau2=10e-4, sigmak2=5.0, threshold=100.0, amp4play=1.0),
    dict(beta=0.95, sigmau2=10e-4, sigmak2=5.0, snr_threshold=2.0, energy_threshold=100.0, smooth=0.9, amp4play=1.0),
)


def _ctype(dtype):
    return np.clongdouble if np.dtype(dtype) == np.dtype(np.longdouble) else np.complex128


def new_state(kind, Kb, P=1, dtype=np.float64, **kw):
    """The constructors' values (aec.cc:85-99, 172-204, 801-807); the NLMS filter starts at zero (stated deviation)."""
    p = dict(DEFAULTS[kind]); p.update(kw)
    f, c = np.dtype(dtype).type, _ctype(dtype)
    st = dict(kind=kind, P=P, p=p, R=np.zeros((Kb, P), c), hist=np.zeros((Kb, P), c), frames=0,
              dtd=np.zeros(3, f))                      # EkEnergy_, SkEnergy_, snr_
    if kind == 1:
        st["sig"] = np.full(Kb, f(p["sigma2"])); st["K"] = np.full((Kb, 1, 1), c(p["sigma2"]))
    elif kind >= 2:
        st["sig"] = np.full(Kb, f(p["sigmau2"]))
        st["K"] = np.zeros((Kb, P, P), c)
        for n in range(P):
            st["K"][:, n, n] = f(p["sigmak2"])
    else:
        st["sig"] = np.zeros(Kb, f); st["K"] = np.zeros((Kb, 1, 1), c)
    return st


def reset(st):
    """reset() of the nodes (aec.h:41,78,111-114)"""
    if st["kind"] < 2:
        st["R"][...] = 0


def _abs2(z):
    return z.real * z.real + z.imag * z.imag


def _dotu(a, b, c):
    acc = c(0)
    for i in range(len(a)):
        acc = acc + a[i] * b[i]
    return acc


class Margins:
    def __init__(self):
        self.energy = np.inf     # kinds 0-2
        self.snr = np.inf        # kind 3, relative to snr_threshold
        self.sk = np.inf         # kind 3, relative to energy_threshold
        self.sign = np.inf       # kind 3, |snr_| where the sign of sf decides

    def smallest(self):
        return float(min(self.energy, self.snr, self.sk, self.sign))


def run(kind, V, A, st, frame_no0=None, dtype=np.float64, trace=None):
    """One block.  frame_no0 (kind 3): None = explicit frame numbers continuing from the state's count; an int >= 0 = explicit
    from there; a negative int = that value on every frame (aec.cc:902 passes next()'s argument, not frame_no_).
    trace (kind 3): a list that receives (t, m, snr_, sf) of every update_band_ call."""
    f, c = np.dtype(dtype).type, _ctype(dtype)
    p, P = st["p"], st["P"]
    V = np.asarray(V).astype(c); A = np.asarray(A).astype(c)
    Kb, T = V.shape
    E = np.zeros((Kb, T), c)
    flags = np.zeros((Kb, T), np.uint8)
    mg = Margins()
    R, Km, sig, hist, dtd = st["R"], st["K"], st["sig"], st["hist"], st["dtd"]
    one = f(1.0)
    if frame_no0 is None:
        frame_no0 = st["frames"]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for t in range(T):
            fn = frame_no0 + t if frame_no0 >= 0 else frame_no0
            if kind < 2:
                thr = f(p["threshold"])
                for m in range(Kb):
                    Vk, Ak, Rk = V[m, t], A[m, t], R[m, 0]
                    Ek = Ak - Rk * Vk
                    E[m, t] = Ek
                    Vk2 = _abs2(Vk)
                    mg.energy = min(mg.energy, abs(Vk2 - thr) / thr)
                    if not Vk2 > thr:
                        continue
                    flags[m, t] = 1
                    if kind == 0:                                                      # aec.cc:63-74
                        dC = Rk - Ak / Vk
                        R[m, 0] = Rk - dC * (f(p["epsilon"]) * Vk2 / (f(p["delta"]) + _abs2(Ak)))
                    else:                                                              # aec.cc:140-160
                        beta = f(p["beta"])
                        s2v = beta * sig[m] + (one - beta) * _abs2(Ek)
                        sig[m] = s2v
                        Kp = Km[m, 0, 0].real + f(p["sigma2"])
                        s2s = Vk2 * Kp + s2v
                        Gk = np.conj(Vk) * (Kp / s2s)
                        R[m, 0] = Rk + Gk * Ek
                        Km[m, 0, 0] = (one - Kp * Vk2 / s2s) * Kp
                continue
            # ---- kinds 2, 3: ComplexBuffer_::next_sample, then the loop(s) over the bins
            amp = f(p["amp4play"])
            hist[:, 1:] = hist[:, :-1].copy()
            hist[:, 0] = V[:, t] * amp if amp != one else V[:, t]
            beta, su2 = f(p["beta"]), f(p["sigmau2"])
            if kind == 2:
                thr = f(p["threshold"])
                for m in range(Kb):
                    v = hist[m]
                    Ek = A[m, t] - _dotu(R[m], v, c)
                    E[m, t] = Ek
                    e0 = _abs2(v[0])
                    mg.energy = min(mg.energy, abs(e0 - thr) / thr)
                    if not e0 > thr:
                        continue
                    flags[m, t] = 1
                    _block_update(R, Km, sig, m, v, Ek, one, beta, su2, one, c)
                continue
            for m in range(Kb):                                                        # aec.cc:878-890
                E[m, t] = A[m, t] - _dotu(R[m], hist[m], c)
            sm = f(p["smooth"])
            if fn < 100:                                                               # aec.cc:825-831
                smth = one - f(fn) * (one - sm) / f(100.0)
            else:
                smth = sm
            sth, eth = f(p["snr_threshold"]), f(p["energy_threshold"])
            for m in range(Kb):                                                        # aec.cc:892-938
                Ak, Ek = A[m, t], E[m, t]
                Sk = Ak - Ek
                ce, cs = _abs2(Ek), _abs2(Sk)
                dtd[0] = ce * smth + dtd[0] * (one - smth)
                dtd[1] = cs * smth + dtd[1] * (one - smth)
                csnr = cs / (ce + f(1.0e-15))
                dtd[2] = csnr * smth + dtd[2] * (one - smth)
                snr = dtd[2]
                if fn >= 100:
                    mg.snr = min(mg.snr, abs(snr - sth) / sth)
                    mg.sk = min(mg.sk, abs(dtd[1] - eth) / eth)
                if fn < 100 or (snr > sth and dtd[1] > eth):
                    sf = f(2.0) / (one + np.exp(-snr)) - one
                    if snr != 0:
                        mg.sign = min(mg.sign, abs(snr))
                else:
                    sf = -one
                if trace is not None:
                    trace.append((t, m, float(snr), float(sf)))
                if sf < 0:
                    continue
                flags[m, t] = 1
                _block_update(R, Km, sig, m, hist[m], Ek, sf, beta, su2, one, c)
    st["frames"] += T
    return E, flags, mg


def _block_update(R, Km, sig, m, v, Ek, sf, beta, su2, one, c):
    """aec.cc:270-302 resp. :906-937 (sf scales Sigma_u in the DTD variant)"""
    P = len(v)
    s2v = beta * sig[m] + (one - beta) * _abs2(Ek)
    sig[m] = s2v
    Kp = Km[m].copy()
    for n in range(P):
        Kp[n, n] = Kp[n, n] + c(sf * su2)
    s = Kp @ np.conj(v)                                                                # zgemv
    s2s = _dotu(v, s, c).real + s2v
    G = s * (one / s2s)
    R[m] = R[m] + Ek * G
    Mx = -np.outer(G, v)                                                               # I - G v^T, then zgemm
    for n in range(P):
        Mx[n, n] = one + Mx[n, n]
    Km[m] = Mx @ Kp


# ---------------------------------------------------------------------------- the test inputs (shared by the CPU and GPU tests)
def make_inputs(seed, Kb, T, P, pause=(110, 125), quiet_until=60, scale=3000.0, noise=300.0):
    """Played V: complex Gaussian at the scale an int16 filter bank delivers, with a short pause (x 1e-4) that closes the energy
    gate.  Recorded A: a decaying (P+2)-tap echo of V plus near-end noise that is 100 x weaker before `quiet_until` (double talk
    afterwards).  Rounded to complex64: exactly what the GPU reads."""
    rng = np.random.default_rng(seed)
    V = (rng.normal(size=(Kb, T)) + 1j * rng.normal(size=(Kb, T))) * scale
    V[:, pause[0]:pause[1]] *= 1.0e-4
    taps = P + 2
    h = (rng.normal(size=(Kb, taps)) + 1j * rng.normal(size=(Kb, taps))) * (0.6 ** np.arange(taps))[None, :] * 0.5
    A = np.zeros((Kb, T), complex)
    for i in range(taps):
        A[:, i:] += h[:, i:i + 1] * V[:, :T - i]
    N = (rng.normal(size=(Kb, T)) + 1j * rng.normal(size=(Kb, T))) * noise
    N[:, :quiet_until] *= 0.01
    A += N
    return V.astype(np.complex64), A.astype(np.complex64)


DTD_GATE = dict(snr_threshold=2.0, energy_threshold=100.0)

# (name, kind, S, M, P, T, T_stride, frame_no0, parameters): the shapes of tests/test_gpu_aec.py.  M = 32 keeps the closed form
# quick; P covers 1, 2, 5, 36 and both sides of every variant boundary of the kernel (kind 2: register tiles of 4, 8, 16, 32, 64
# rows; kind 3: K in LDS up to P = 24 at M = 32, in the exported state above).
CASES = [
    ("nlms", 0, 1, 32, 1, 180, 180, None, dict()),
    ("kalman", 1, 3, 32, 1, 180, 200, None, dict(sigma2=50.0)),
    ("kalman_m256", 1, 1, 256, 1, 40, 40, None, dict()),
    ("bk_p1", 2, 1, 32, 1, 180, 180, None, dict()),
    ("bk_p2", 2, 3, 32, 2, 180, 200, None, dict(amp4play=0.5)),
    ("bk_p4", 2, 1, 32, 4, 180, 180, None, dict()),
    ("bk_p5", 2, 1, 32, 5, 180, 180, None, dict(amp4play=0.5)),
    ("bk_p8", 2, 1, 32, 8, 180, 180, None, dict()),
    ("bk_p9", 2, 1, 32, 9, 180, 180, None, dict()),
    ("bk_p16", 2, 1, 32, 16, 180, 180, None, dict()),
    ("bk_p17", 2, 1, 32, 17, 180, 180, None, dict()),
    ("bk_p32", 2, 1, 32, 32, 180, 180, None, dict()),
    ("bk_p33", 2, 1, 32, 33, 180, 180, None, dict()),
    ("bk_p36", 2, 1, 32, 36, 180, 192, None, dict(amp4play=0.5)),
    ("bk_m256_p5", 2, 1, 256, 5, 40, 40, None, dict()),
    ("dtd_p1", 3, 1, 32, 1, 180, 180, None, dict(DTD_GATE)),
    ("dtd_p2", 3, 3, 32, 2, 180, 200, None, dict(DTD_GATE, amp4play=0.5)),
    ("dtd_p5", 3, 1, 32, 5, 180, 180, None, dict(DTD_GATE)),
    ("dtd_p5_neg", 3, 3, 32, 5, 120, 120, -5, dict(DTD_GATE)),
    ("dtd_p24", 3, 1, 32, 24, 180, 180, None, dict(DTD_GATE)),
    ("dtd_p25", 3, 1, 32, 25, 180, 180, None, dict(DTD_GATE)),
    ("dtd_p36", 3, 1, 32, 36, 180, 192, None, dict(DTD_GATE, amp4play=0.5)),
    ("dtd_p36_neg", 3, 1, 32, 36, 120, 120, -5, dict(DTD_GATE)),
    ("dtd_m256_p5", 3, 1, 256, 5, 40, 40, 90, dict(DTD_GATE)),
]


# a case whose first seed left a gate decision closer than 1e-8 to its branch point gets another seed, never a looser condition
SEED_SHIFT = {}


def case_inputs(case):
    """(V, A) complex64 [S][Kb][T] of a case; the seed is the case's index, stream by stream"""
    name, kind, S, M, P, T, ts, fn0, kw = case
    idx = [c[0] for c in CASES].index(name)
    Kb = M // 2 + 1
    short = T < 180
    # (with one constant negative frame number the smoothing factor exceeds 1 and snr_ alternates in sign while it decays through
    # a pause, bin after bin: the pause is two frames there, so that |snr_| stays away from zero)
    pause = (30, 32) if (fn0 is not None and fn0 < 0) else ((20, 28) if short else (110, 125))
    outs = [make_inputs(1000 * idx + SEED_SHIFT.get(name, 0) + s, Kb, T, P, pause=pause, quiet_until=12 if short else 60)
            for s in range(S)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])


_cache = {}


def case_reference(case, dtype=np.float64):
    """Closed form of a case, computed once per process and shared: list over streams of (E, flags, margins, state)."""
    key = (case[0], np.dtype(dtype).name)
    if key not in _cache:
        name, kind, S, M, P, T, ts, fn0, kw = case
        V, A = case_inputs(case)
        res = []
        for s in range(S):
            st = new_state(kind, M // 2 + 1, P, dtype=dtype, **kw)
            E, fl, mg = run(kind, V[s], A[s], st, frame_no0=fn0, dtype=dtype)
            res.append((E, fl, mg, st))
        _cache[key] = res
    return _cache[key]
