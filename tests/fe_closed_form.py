"""numpy restatement of the recogniser's front end, stage by stage (helper of the front-end tests, not a test).

Written from the reference's feature/feature.cc (PreemphasisFeature :1128-1144, HammingFeature :1177-1200, FFTFeature
:1205-1258, SpectralPowerFeature :1291-1314, VTLNFeature :1672-1792, MelFeature :1892-2122 and :2199-2242, LogFeature
:2326-2362, CepstralFeature :2370-2415) and matrix/gslmatrix.cc:107-131: float32 where the reference declares `float`,
float64 elsewhere.  The scalar functions the reference takes from libm (log10, pow, cos, floor, ceil) come from `math`, which
calls the same library.  The transform is numpy.fft.rfft of the float32-rounded windowed frame in float64.
"""
import math

import numpy as np

f32 = np.float32
U = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------- frames
def hamming(D):
    temp = 2.0 * math.pi / float(D - 1)
    return np.array([0.54 - 0.46 * math.cos(temp * i) for i in range(D)], np.float64)


def frames(x, D, shift, T, mu=None, prior0=0.0, window=True):
    """x float32 [len] -> float32 [T][D]: frame t = samples t shift .. t shift + D - 1 (zero at and beyond len), pre-emphasised
    (mu not None; the prior of a frame's first sample is the LAST sample of the frame before, prior0 for frame 0), windowed."""
    x = np.asarray(x, np.float32)
    pad = np.zeros(max((T - 1) * shift + D, len(x)), np.float32)
    pad[:len(x)] = x
    fr = np.stack([pad[t * shift:t * shift + D] for t in range(T)])
    if mu is not None:
        prior = np.empty_like(fr)
        prior[:, 1:] = fr[:, :-1]
        prior[1:, 0] = fr[:-1, -1]
        prior[0, 0] = f32(prior0)
        fr = (fr.astype(np.float64) - float(mu) * prior.astype(np.float64)).astype(np.float32)
    if window:
        fr = (hamming(D)[None, :] * fr.astype(np.float64)).astype(np.float32)
    return fr


def spectrum64(fr, L):
    """float32 [T][D] frames -> complex128 [T][L/2+1]: zero padding to L, forward transform, unnormalised."""
    return np.fft.rfft(fr.astype(np.float64), n=L, axis=-1)


def power64(X, powN):
    """|X_k|^2, k < powN, powN = L/2+1 or L (the conjugate mirror above L/2)."""
    K = X.shape[-1]
    L = 2 * (K - 1)
    P = X.real ** 2 + X.imag ** 2
    if powN == K:
        return P
    assert powN == L
    return np.concatenate([P, P[..., L // 2 - 1:0:-1]], axis=-1)


# ---------------------------------------------------------------------------------------------------------------- mel
def _mel(hz):
    hz = f32(hz)
    return f32(2595.0 * math.log10(1.0 + float(hz) / 700.0)) if hz >= 0 else f32(0.0)


def _hertz(m):
    d = float(f32(m)) / 2595.0
    return f32(700.0 * (math.pow(10.0, d) - 1.0))


def mel_table(powN, rate, low, up, filterN, version):
    """-> (offset [filterN], count [filterN], list of float32 coefficient rows)."""
    rate, low, up = f32(rate), f32(low), f32(up)
    if up <= 0:
        up = f32(float(rate) / 2.0)
    df = f32(float(rate) / (4.0 * (powN // 2)))
    mlow, mup = _mel(low), _mel(up)
    dm = f32(f32(mup - mlow) / f32(filterN + 1))
    if float(low) < 0.0 or 2.0 * float(up) > float(rate) or low > up:
        raise ValueError("mel: something wrong with the band edges")
    offset, count, rows = [], [], []
    for x in range(filterN):
        left = _hertz(f32(f32(f32(x) * dm) + mlow))
        center = _hertz(f32((x + 1.0) * float(dm) + float(mlow)))
        right = _hertz(f32((x + 2.0) * float(dm) + float(mlow)))
        height = f32(2.0 / float(f32(right - left)))
        slope1 = f32(height / f32(center - left))
        slope2 = f32(height / f32(center - right))
        start = int(math.ceil(f32(left / df)))
        end = int(math.floor(f32(right / df)))
        n = end - start + 1
        freq = f32(f32(start) * df)
        row = np.zeros(n, np.float32)
        for i in range(n):
            if version == 1:
                freq = f32(freq + df)
            row[i] = f32(slope1 * f32(freq - left)) if freq <= center else f32(slope2 * f32(freq - right))
            if version == 2:
                freq = f32(freq + df)
        offset.append(start)
        count.append(n)
        rows.append(row)
    return np.array(offset), np.array(count), rows


def mel_apply(v, offset, count, rows):
    """v float [..., n] -> float64 [..., filterN]: float64 sums of float32 coefficient times value."""
    v = np.asarray(v, np.float64)
    out = np.zeros(v.shape[:-1] + (len(rows),), np.float64)
    for j, r in enumerate(rows):
        out[..., j] = (v[..., offset[j]:offset[j] + count[j]] * r.astype(np.float64)).sum(axis=-1)
    return out


def mel_abs(v, offset, count, rows):
    """sum |w| |in| per output, the scale of the stage's rounding bound."""
    return mel_apply(np.abs(v), offset, count, [np.abs(r) for r in rows])


# ---------------------------------------------------------------------------------------------------------------- VTLN
def vtln_org(p, N, ratio, edge):
    """VTLNFeature::nextOrg on power vectors p (float64 [inN] or [inN][batch]) -> float64 [N] or [N][batch]."""
    p = np.asarray(p, np.float64)
    inN = len(p)
    yedge = (edge / ratio) if edge < ratio else 1.0
    b = (1.0 - edge) / (1.0 - yedge) if yedge < 1.0 else 0.0
    out = np.zeros((N,) + p.shape[1:])
    for c in range(N):
        Y0, Y1 = float(c) / float(N), float(c + 1) / float(N)
        X0 = ((ratio * Y0) if Y0 < yedge else (b * Y0 + 1.0 - b)) * N
        X1 = ((ratio * Y1) if Y1 < yedge else (b * Y1 + 1.0 - b)) * N
        l1 = int(X1)
        alpha1 = X1 - l1
        l0 = int(X0)
        alpha0 = int(X0) + 1 - X0
        z = np.zeros(p.shape[1:])
        if l0 >= inN:
            l0 = inN - 1
        if l1 > inN:
            l1 = inN
        if l0 == l1:
            z = z + (X1 - X0) * p[l0]
        else:
            z = z + alpha0 * p[l0]
            for i in range(l0 + 1, l1):
                z = z + p[i]
            if l1 < inN:
                z = z + alpha1 * p[l1]
        out[c] = z
    return out


def vtln_ff(p, N, ratio, edge):
    """VTLNFeature::nextFF on power vectors p, [inN] or [inN][batch] (the values pass through a float, the reference's `float v`)."""
    p = np.asarray(p, np.float64)
    b = f32(N * edge)
    slope1 = f32(ratio)
    slope2 = f32(ratio)
    if slope1 < 1.0:
        with np.errstate(divide="ignore", invalid="ignore"):       # edge = 1: b = N, as in the reference
            slope2 = f32(f32(f32(N) - f32(slope1 * b)) / f32(f32(N) - b))
    vec, aux = np.zeros((N,) + p.shape[1:]), np.zeros(N)
    for s in range(N):
        s1, s2 = f32(s - 0.5), f32(s + 0.5)
        v = np.asarray(p[s]).astype(np.float32).astype(np.float64)
        d1 = f32(s1 * slope1)
        if s1 > b:
            d1 = f32(f32(b * slope1) + f32(f32(s1 - b) * slope2))
        d2 = f32(s2 * slope1)
        if s2 > b:
            d2 = f32(f32(b * slope1) + f32(f32(s2 - b) * slope2))
        i1, i2 = int(math.floor(d1)), int(math.ceil(d2))
        if i1 <= N - 1:
            alpha1 = 1.0 - float(f32(d1 - f32(i1)))
            alpha2 = float(f32(f32(i2) - d2))
            for j in range(i1, i2 + 1):
                k = max(j, 0)
                if k >= N:
                    break
                a = 1.0
                if j == i1:
                    a = alpha1
                if j == i2:
                    a = alpha2
                vec[k] = vec[k] + a * v
                aux[k] += a
    nz = aux > 1e-20
    vec[nz] = vec[nz] / aux[nz].reshape((-1,) + (1,) * (vec.ndim - 1))
    return vec


def vtln_matrix(N, inN, ratio, edge, version):
    """The closed form applied to the unit vectors: float64 [N][inN]."""
    fn = vtln_org if version == 1 else vtln_ff
    return fn(np.eye(inN), N, ratio, edge)                         # column s of the batch is the unit vector s


# ---------------------------------------------------------------------------------------------------------------- log, cepstra
def log_feature(v, m=1.0, a=1.0, floor=False):
    """LogFeature::next on float values -> float32."""
    val = np.asarray(v, np.float64).copy()
    if floor:
        val[val < 1.0e-5] = 1.0e-5
    else:
        val += a
        val[val <= 0.0] = 1.0
    return (m * np.vectorize(math.log10, otypes=[np.float64])(val)).astype(np.float32)


def dct_table(type, cepN, filterN):
    """-> float32 [cepN][filterN]"""
    m = np.zeros((cepN, filterN), np.float32)
    for k in range(cepN):
        if type == 0:
            fac = k * math.pi / float(filterN - 1)
            m[k, 0] = 1.0
            for l in range(1, filterN - 1):
                m[k, l] = 2.0 * math.cos(fac * l)
            m[k, filterN - 1] = math.cos(k * math.pi)
        elif type == 1:
            fac = k * math.pi / float(filterN)
            for l in range(filterN):
                m[k, l] = math.cos(fac * (l + 0.5))
        elif type == 2:
            deltaF = math.pi * float(f32(k)) / filterN
            for l in range(filterN):
                c = math.cos(deltaF * (l + 0.5)) / filterN
                if l == 0:
                    c *= 0.5
                m[k, l] = c
        else:
            raise IndexError("Unknown DCT type")
    return m


# ---------------------------------------------------------------------------------------------------------------- LDS placement
LDS_TABLE_LIMIT = 64 * 1024


def pcm_kernel_lds(L, vtln=None, mel=None, dct=None):
    """(bytes of the frames' buffers, bytes of the tables) of the kernel that starts from PCM, by the size rule of its launch:
    NF = L/2 complex points, NT = clamp(NF/4, 64, 512) threads per frame, G = 1 frame per workgroup from NT = 256, else 256/NT;
    frames = G (8 NF + 4 (NF + 2)); tables = 8 (VTLN weights) + 4 (mel weights + cosine table) + 12 (VTLN rows + mel rows).
    The tables are staged in LDS where frames + tables <= 64 KiB and read from global memory otherwise.  The arguments are the
    FeTables handed to fe_process (their own counts)."""
    NF = L // 2
    NT = min(max(NF // 4, 64), 512)
    G = 1 if NT >= 256 else 256 // NT
    frames = G * (8 * NF + 4 * (NF + 2))
    tabs = 0
    if vtln is not None:
        tabs += 8 * len(vtln.coef) + 12 * vtln.rows
    if mel is not None:
        tabs += 4 * len(mel.coef) + 12 * mel.rows
    if dct is not None:
        tabs += 4 * len(dct.coef)
    return frames, tabs


def tables_in_lds(L, vtln=None, mel=None, dct=None):
    frames, tabs = pcm_kernel_lds(L, vtln, mel, dct)
    return frames + tabs <= LDS_TABLE_LIMIT
