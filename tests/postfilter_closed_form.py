"""Closed forms of the Zelinski, McCowan and Lefkimmiatis post-filters in float64 numpy: a statement of the reference's
equations (postfilter/postfilter.cc), pair by pair.  No GPU, no oracle, none of the sums the kernels collapse the pairs into:
every pair i < j keeps its own cross spectral density, vectorised over streams, bins and pairs, with a loop over the frames.

Rules (file:line of postfilter/postfilter.cc), g = index of a frame in its stream, frame_no_ = g - 1 while it is processed:

  alignment     x'_i = conj(d_i) x_i                                                                    (:30-43)
  densities     phi_ij <- a phi_ij + (1 - a) x'_i conj(x'_j) for i < j, phi_ii <- a phi_ii + (1 - a) |x'_i|^2     (:8-21, :100-116, :696-736)
                a = alpha when frame_no_ > 0, i.e. from the third frame of the stream on (:460-463, :865-868, :1113-1116), and
                only if alpha > 0 (:13, :106, :723); otherwise the densities are the current products (no memory)
  Zelinski      W = f(sum_{i<j} phi_ij) / sum_i phi_ii * 2 / (N - 1)                                      (:76-118)
                f = max(Re ., 0) if type & 1, else |.| (:90-98); while frame_no_ < min_frames the filter is called with type 0:
                f = |.| and no gain is applied (:468-473, :197-199); type 0 never applies the gain
                W >= 1 -> 1, then W < 1e-4 -> 1e-4                                                       (:120-121)
  McCowan       clean PSD  s = sum_{i<j} (phi_ij - R_ij (phi_ii + phi_jj) / 2) / (1 - R_ij)               (:809-825)
                R_ij = upper triangle of the coherence matrix, replaced by float32(threshold) when Re R_ij > threshold and
                Im R_ij <= 0 (:816-818); avg = Re s if type & 1, else |s|, in EVERY frame (:827-832)
                W = (2 avg / (N (N - 1))) / (sum_i phi_ii / N)  (:834, :735, :882);  W > 1 -> 1, W < 1e-4 -> 1e-4 (:883-884)
                the gain is applied whenever frame_no_ >= min_frames, whatever the type (:889-894)
  Lefkimmiatis  ss = the clean PSD above (2 avg / (N (N - 1)))                                            (:1127)
                noise PSD  v = sum_{i<j} ((phi_ii + phi_jj) / 2 - phi_ij) / (1 - R_ij), R_ij replaced by float32(threshold)
                when Re R_ij > threshold (imaginary part dropped), else by 0.99 when Re R_ij == 1 (:1061-1079);
                vv = 2 (Re v or |v|) / (N (N - 1)) (:1081-1088)
                W = ss / (ss + vv / L_k), L_k = 1 for k < fbin_x1, else Re Lambda_k if type & 1, else |Lambda_k|  (:1130-1140)
                same clamps and the same min_frames rule as McCowan                                       (:1142-1155)

The arithmetic is IEEE, literally: a bin whose snapshots are all zero while it has no memory gives 0 / 0 = NaN, which passes both
clamps, as in the reference's C.

Every function takes dtype: np.float64 is the closed form; np.float32 evaluates the same per-pair sums in float32 / complex64,
the straightforward way, and is the YARDSTICK for closed_forms.accept (what float32 arithmetic achieves on these inputs).
"""
import numpy as np

SPECTRAL_FLOOR = 1.0e-4
MUTANTS = ("memory_from_second_frame", "drop_pair", "clean_clip_ignores_imag", "noise_clip_keeps_imag", "no_gain_for_type0")


def _types(dtype):
    rt = np.dtype(dtype)
    assert rt in (np.dtype(np.float64), np.dtype(np.float32))
    return rt.type, (np.complex128 if rt == np.dtype(np.float64) else np.complex64)


def new_state(lead, K, N, dtype=np.float64):
    """Zeroed densities of the streams `lead` (a tuple, () for one stream): phi [..][K][N (N-1) / 2], psd [..][K][N]."""
    rt, ct = _types(dtype)
    return {"phi": np.zeros(tuple(lead) + (K, N * (N - 1) // 2), ct), "psd": np.zeros(tuple(lead) + (K, N), rt)}


def applied(T, min_frames, frame_base=0):
    """bool [T]: frames with frame_no_ >= min_frames."""
    return (frame_base + np.arange(T) - 1) >= min_frames


def _run(kind, X, d, y, alpha, type_, min_frames, frame_base, resets, state, R, threshold, lam, fbin_x1, dtype, mutant):
    assert mutant is None or mutant in MUTANTS
    rt, ct = _types(dtype)
    X, d, y = np.asarray(X).astype(ct), np.asarray(d).astype(ct), np.asarray(y).astype(ct)
    K, N, T = X.shape[-3:]
    lead = X.shape[:-3]
    assert N > 1 and d.shape[-2:] == (K, N) and y.shape == lead + (K, T)
    I, J = np.triu_indices(N, 1)                               # i < j in the reference's loop order
    if mutant == "drop_pair":
        keep = np.arange(len(I)) != len(I) // 2
        I, J = I[keep], J[keep]
    st = new_state(lead, K, N, dtype) if state is None else {k: v.copy() for k, v in state.items()}
    assert st["phi"].dtype == ct and st["psd"].dtype == rt
    if mutant == "drop_pair" and state is None:
        st["phi"] = st["phi"][..., :len(I)]
    a, one, half, two = rt(alpha), rt(1.0), rt(0.5), rt(2.0)
    thr = rt(np.float32(threshold))                            # a float member in the reference
    if kind != "zelinski":
        Rp = np.asarray(R).astype(ct)[..., I, J]               # [K][P]
        clip = Rp.real > thr
        if mutant != "clean_clip_ignores_imag":
            clip = clip & (Rp.imag <= 0)
        one_minus_Rs = one - np.where(clip, ct(thr), Rp)
        Rs = np.where(clip, ct(thr), Rp)
    if kind == "lefkimmiatis":
        Rn = np.where(Rp.real > thr, (thr + 1j * Rp.imag).astype(ct) if mutant == "noise_clip_keeps_imag" else ct(thr),
                      np.where(Rp.real == 1, ct(0.99), Rp)).astype(ct)
        L = np.asarray(lam).astype(ct)
        Lk = (L.real if type_ & 1 else np.abs(L)).astype(rt)
        Lk = np.where(np.arange(K) < fbin_x1, one, Lk).astype(rt)
    npairs = rt(N * (N - 1))
    W = np.zeros(lead + (K, T), rt)
    out = y.copy()
    first_memory = 1 if mutant == "memory_from_second_frame" else 2
    with np.errstate(all="ignore"):
        for t in range(T):
            g = frame_base + t
            if g in resets:
                st["phi"][...] = 0
                st["psd"][...] = 0
            xp = np.conj(d) * X[..., t]                        # [..][K][N]
            cross = xp[..., I] * np.conj(xp[..., J])
            power = xp.real * xp.real + xp.imag * xp.imag
            if g >= first_memory and alpha > 0:
                st["phi"] = a * st["phi"] + (one - a) * cross
                st["psd"] = a * st["psd"] + (one - a) * power
            else:
                st["phi"], st["psd"] = cross, power
            phi, psd = st["phi"], st["psd"]
            assert phi.dtype == ct and psd.dtype == rt
            use = (g - 1) >= min_frames
            if kind == "zelinski":
                s = phi.sum(axis=-1)
                pft = type_ if use else 0
                num = np.maximum(s.real, rt(0)) if pft & 1 else np.abs(s)     # (np.maximum keeps a NaN, as `if (x < 0) x = 0` does)
                w = (num / psd.sum(axis=-1)) * (two / (rt(N) - one))
                w = np.where(w >= 1, one, w)
                use = use and type_ != 0
            else:
                mean_psd = half * (psd[..., I] + psd[..., J])
                s = ((phi - Rs * mean_psd) / one_minus_Rs).sum(axis=-1)
                ss = two * (s.real if type_ & 1 else np.abs(s)) / npairs
                if kind == "mccowan":
                    w = ss / (psd.sum(axis=-1) / rt(N))
                    if mutant == "no_gain_for_type0":
                        use = use and (type_ & 3) != 0
                else:
                    v = ((mean_psd - phi) / (one - Rn)).sum(axis=-1)
                    vv = two * (v.real if type_ & 1 else np.abs(v)) / npairs
                    w = ss / (ss + vv / Lk)
                w = np.where(w > 1, one, w)
            w = np.where(w < rt(SPECTRAL_FLOOR), rt(SPECTRAL_FLOOR), w).astype(rt)
            W[..., t] = w
            if use:
                out[..., t] = w * y[..., t]
    assert W.dtype == rt and out.dtype == ct
    return W, out, st


def zelinski(X, d, y, alpha, type_, min_frames, frame_base=0, resets=(), state=None, dtype=np.float64, mutant=None):
    """X [..][K][N][T], d [..|1][K][N], y [..][K][T] -> (W [..][K][T] real, filtered y, state after the last frame).
    frame_base = frames of the stream before X[..., 0]; resets = stream frame indices at which the history is zeroed first
    (the frame counter keeps counting); state = what an earlier call returned (None: zero)."""
    return _run("zelinski", X, d, y, alpha, type_, min_frames, frame_base, resets, state, None, 0.0, None, 0, dtype, mutant)


def mccowan(X, d, y, R, alpha, type_, min_frames, threshold=0.99, frame_base=0, resets=(), state=None, dtype=np.float64,
            mutant=None):
    """As zelinski(), with the noise coherence R [K][N][N] (only i < j is read)."""
    return _run("mccowan", X, d, y, alpha, type_, min_frames, frame_base, resets, state, R, threshold, None, 0, dtype, mutant)


def lefkimmiatis(X, d, y, R, lam, fbin_x1, alpha, type_, min_frames, threshold=0.99, frame_base=0, resets=(), state=None,
                 dtype=np.float64, mutant=None):
    """As mccowan(), with Lambda [K] complex (d^H pinv(R_k) d as calcLambda forms it, :982-994) and fbin_x1."""
    return _run("lefkimmiatis", X, d, y, alpha, type_, min_frames, frame_base, resets, state, R, threshold, lam, fbin_x1, dtype,
                mutant)


def beamform(W, X, dtype=np.float64):
    """y[..][k][t] = sum_n conj(W[..][k][n]) X[..][k][n][t]; float32: channel after channel into a complex64 sum."""
    rt, ct = _types(dtype)
    W, X = np.asarray(W).astype(ct), np.asarray(X).astype(ct)
    if rt == np.float64:
        return np.einsum("...kn,...knt->...kt", np.conj(W), X)
    y = np.zeros(X.shape[:-2] + X.shape[-1:], ct)
    for n in range(X.shape[-2]):
        y = y + np.conj(W[..., n])[..., None] * X[..., n, :]
    assert y.dtype == ct
    return y


def clamp_share(W):
    """Share of the finite gains that sit at 1 or at the spectral floor."""
    W = np.asarray(W)
    ok = np.isfinite(W)
    return float(np.mean((W[ok] >= 1.0) | (W[ok] <= SPECTRAL_FLOOR))) if ok.any() else 0.0


# --------------------------------------------------------------------------- inputs
def alignment(S, K, N, seed=0):
    """Unit-modulus alignment vectors exp(j phi), complex64 [S][K][N]."""
    rng = np.random.default_rng(seed + 31)
    return np.exp(1j * rng.uniform(0.0, 2.0 * np.pi, (S, K, N))).astype(np.complex64)


def coherence(K, N, threshold, seed=0, real=False):
    """A Hermitian positive definite R [K][N][N] with unit diagonal (complex64) and, per bin, its list of `twin` pairs
    (i, j, phase).

    R is the Gram matrix of N unit vectors per bin.  A twin pair's vectors are almost parallel, turned against each other by
    +-theta: Re R_ij above the threshold, Im R_ij of either sign (zero for real=True).  All other pairs are nearly orthogonal:
    real parts of both signs, far below the threshold.  snapshots() makes the aligned signals of a twin pair equal up to the small
    rotation `phase` = +-0.3 (1 - threshold): a coherence near one then states what the data do, the pair weights
    1 / (1 - R_ij) of up to 100 do not swamp the other pairs, and the rotation keeps the pair's term sensitive to R_ij and to
    either clip rule (for exactly equal signals the term is (phi - R phi) / (1 - R) = phi whatever R is)."""
    rng = np.random.default_rng(1009 * N + 17 * K + seed)
    thr = float(np.float32(threshold))
    dim = max(4 * N, 64)
    c = 1.0 - 0.1 * (1.0 - thr)                                # |R_ij| of a twin pair
    theta = 0.9 * np.arccos(min(1.0, (thr + 0.5 * (c - thr)) / c))
    R = np.zeros((K, N, N), np.complex128)
    twins = []
    sign = 1
    for k in range(K):
        v = rng.normal(size=(N, dim)) + (0 if real else 1j) * rng.normal(size=(N, dim))
        v /= np.linalg.norm(v, axis=1, keepdims=True)
        nt = 0 if k % 3 else max(1, N // 4)
        order = rng.permutation(N)
        tw = []
        for q in range(nt):
            i, j = sorted((int(order[2 * q]), int(order[2 * q + 1])))
            w = v[j] - np.vdot(v[i], v[j]) * v[i]
            w /= np.linalg.norm(w)
            ph = 1.0 if real else np.exp(1j * sign * theta)
            v[j] = c * ph * v[i] + np.sqrt(1.0 - c * c) * w     # R_ij = v_i^H v_j = c exp(+-j theta)
            tw.append((i, j, sign * 0.3 * (1.0 - thr)))
            sign = -sign
        R[k] = np.conj(v) @ v.T
        if N == 2 and not tw and not real and (R[k][0, 1].imag > 0) != (k % 2 == 1):
            R[k] = np.conj(R[k])                               # one pair per bin: its imaginary part alternates over the bins
        R[k][np.arange(N), np.arange(N)] = 1.0
        twins.append(tw)
    R = R.astype(np.complex64)
    I, J = np.triu_indices(N, 1)
    up = R[:, I, J]
    hi, neg = up.real > thr, up.imag <= 0
    assert hi.any() and (~hi).any()                            # real parts on both sides of the threshold
    if not real:                                               # all four branches of the two clip rules occur
        assert (hi & neg).any() and (hi & ~neg).any() and (~hi & neg).any() and (~hi & ~neg).any()
    else:
        assert not np.any(R.imag)
    for k in range(K):                                         # above the threshold <=> a twin pair
        assert sorted((int(i), int(j)) for i, j in zip(I[hi[k]], J[hi[k]])) == sorted(t[:2] for t in twins[k])
    assert np.all(np.linalg.eigvalsh(R.astype(np.complex128)) > 0)
    return R, twins


def snapshots(d, T, twins=None, seed=0, noise=1500.0, target=2500.0):
    """complex64 [S][K][N][T]: x_n = d_n (s + v_n), s a target of scale `target` common to all channels (coherent after the
    alignment), v_n Gaussian noise of scale `noise`; channel j of a twin pair (i, j, phase) of the bin is channel i turned by
    `phase` (see coherence()).  d [S][K][N]."""
    d = np.asarray(d)
    S, K, N = d.shape
    rng = np.random.default_rng(seed + 7 * N + T)
    v = (rng.normal(size=(S, K, N, T)) + 1j * rng.normal(size=(S, K, N, T))) * noise
    s = (rng.normal(size=(S, K, 1, T)) + 1j * rng.normal(size=(S, K, 1, T))) * target
    z = s + v
    if twins is not None:
        for k, tw in enumerate(twins):
            for i, j, phase in tw:
                z[:, k, j] = z[:, k, i] * np.exp(1j * phase)
    return (d[..., None] * z).astype(np.complex64)
