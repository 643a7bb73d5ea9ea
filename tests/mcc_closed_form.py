"""numpy float64 restatement of the multichannel cross-correlation localiser (reference localization/mcc_localizer.cc,
localization.cc:107-118): the sample window and its wrap into the block's own tail, tau truncated through float32, the cost
from eigvalsh with |lambda|, the N-best insertion, and the far-field grid walk of SGB4LinearArray in float32.

Nothing here touches the product; the tests compare the product with it."""
import math

import numpy as np

F32 = np.float32
SSPEED = 343740.0
TPI = 6.28318530717958647692
RESET_COST = 100000.0


def max_sample_delay(fs, max_time_delay):
    """(size_t)(fs * maxTimeDelay): unsigned x float is a float product (:273)."""
    return int(F32(fs) * F32(max_time_delay))


def sample_delays(fs, delays):
    """(int)(float)(fs * d): the double product rounded to float, truncated toward zero (:333-335)."""
    d = np.asarray(delays, np.float64)
    return np.trunc((float(fs) * d).astype(F32)).astype(np.int64)


def shifted(block, tau, D):
    """xt [N][nS] float64: xt_c[f] = x_c[f + tau_c], or x_c[L + f + tau_c] where f + tau_c < 0 (:343-353 with :336)."""
    block = np.asarray(block)
    N, L = block.shape
    nS = L - D
    assert L >= 2 * D and np.all(np.abs(tau) <= D)
    f = np.arange(nS)
    out = np.empty((N, nS), np.float64)
    for c in range(N):
        idx = f + int(tau[c])
        idx = np.where(idx < 0, idx + L, idx)
        out[c] = block[c, idx]
    return out


def corr_matrix(block, tau, D):
    """R = (1 / nS) sum xt xt^T in float64; the sum itself exactly rounded once per entry (math.fsum over exact products)."""
    xt = shifted(block, tau, D)
    N, nS = xt.shape
    inv = 1.0 / float(nS)
    if np.all(xt == np.rint(xt)) and float(np.max(np.abs(xt), initial=0.0)) ** 2 * nS < 2.0 ** 53:
        xi = xt.astype(np.int64)                         # integer samples: the sums are exact in int64 and fit a float64
        return (xi @ xi.T).astype(np.float64) * inv
    R = np.empty((N, N), np.float64)
    for i in range(N):
        for j in range(i + 1):
            R[i, j] = R[j, i] = math.fsum((xt[i] * xt[j]).tolist()) * inv
    return R


def abs_sum_matrix(block, tau, D):
    """(1 / nS) sum |xt_i xt_j|: what the rounding bound of R scales with."""
    xt = np.abs(shifted(block, tau, D))
    return (xt @ xt.T) / float(xt.shape[1])


def cost_of(R, normalize=True):
    """calcObjectiveFunction (:368-411), log form: sum log |lambda_i| - sum log R_ii; 0.0 at a zero eigenvalue.  A dead channel
    (R_ii <= 0) has a zero eigenvalue in exact arithmetic: 0.0 as well (the stated rule of the product)."""
    if np.any(np.diag(R) <= 0):
        return 0.0, True
    lam = np.linalg.eigvalsh(R)
    if np.any(lam == 0):
        return 0.0, True
    ld = float(np.sum(np.log(np.abs(lam))))
    ln = float(np.sum(np.log(np.diag(R)))) if normalize else 0.0
    return ld - ln, False


def costs(x, taus, L, D, normalize=True):
    """x [N][samples] -> cost float64 [B][G], flag bool [B][G] over the B = samples // L blocks."""
    x = np.asarray(x)
    B = x.shape[1] // L
    taus = np.asarray(taus)
    out = np.zeros((B, len(taus)))
    flag = np.zeros((B, len(taus)), bool)
    for b in range(B):
        blk = x[:, b * L:(b + 1) * L]
        seen = {}
        for g, tau in enumerate(taus):
            key = tuple(int(t) for t in tau)
            if key not in seen:
                seen[key] = cost_of(corr_matrix(blk, tau, D), normalize)
            out[b, g], flag[b, g] = seen[key]
    return out, flag


def nbest(cost_row, n):
    """The insertion of search() (:431-443): grid order, strict <, entries start at 100000 -> (costs [n], indices [n], -1 empty)."""
    best, idx = [RESET_COST] * n, [-1] * n
    for g, c in enumerate(np.asarray(cost_row, np.float64)):
        if c < best[n - 1]:
            for i in range(n):
                if c < best[i]:
                    best[i + 1:] = best[i:n - 1]
                    idx[i + 1:] = idx[i:n - 1]
                    best[i], idx[i] = float(c), g
                    break
    return np.array(best), np.array(idx, np.int64)


def linear_geometry(fs, N, spacing=None, positions=None):
    """(ypos float64 [N], constV float32, maxTimeDelay float32) of setDistanceBtwMicrophones / setPositionsOfMicrophones
    (:54-100); microphone 0 is pos0 (the stated deviation from the reference's loop from 1)."""
    if positions is None:
        d = F32(spacing)
        ypos = np.array([float(F32(m) * d) for m in range(N)])
        span = F32(N - 1) * d
        const_v = F32(0.99 * SSPEED / float(span * F32(fs)))
        return ypos, const_v, F32(float(span) / SSPEED)
    pos = np.asarray(positions, np.float64)
    if pos.ndim == 1:
        pos = np.stack([np.zeros_like(pos), pos, np.zeros_like(pos)], axis=1)
    p32 = pos.astype(F32)
    max_dist = F32(-1)
    for m in range(1, N):
        dx, dy, dz = (p32[0] - p32[m])
        dist = np.sqrt(F32(F32(dx * dx + dy * dy) + dz * dz))
        max_dist = max(max_dist, F32(dist))
    const_v = F32(0.99 * SSPEED / float(max_dist * F32(fs)))
    return pos[:, 1].copy(), const_v, F32(float(max_dist) / SSPEED)


def linear_walk(const_v, numpy_f32=False, limit=100000):
    """Azimuths (float32) of reset() followed by nextSearchGridFF until it returns NULL (:119-148).  Every value is a float32;
    sinf / asinf are the correctly rounded float32 functions (the float64 function rounded once), or with numpy_f32 numpy's own
    float32 loops, which are a few units less exact: the walk feeds sin(asin(.)) back into itself and asin near 1 magnifies
    what the sine lost, so the two walks drift apart towards pi/2 (44 float32 ulp at the last of 60 steps of 63 x 20 mm)."""
    const_v = F32(const_v)
    if numpy_f32:
        sinf, asinf = (lambda v: np.sin(v, dtype=F32)), (lambda v: np.arcsin(v, dtype=F32))
    else:
        sinf, asinf = (lambda v: F32(math.sin(float(v)))), (lambda v: F32(math.asin(float(v))))
    az = F32(0.0)
    out = [az]
    while len(out) < limit:
        old_sin = sinf(az)
        if float(az) < math.pi / 2:
            new_sin = F32(old_sin + const_v)
            new_az = F32(math.pi / 2) if new_sin >= 1 else asinf(new_sin)
        elif float(az) < 3 * (math.pi / 2):
            new_az = F32(3 * (math.pi / 2))
        else:
            new_sin = F32(old_sin + const_v)
            if float(new_sin) + float(const_v) / 2.0 >= 0:
                return np.array(out, F32)
            new_az = F32(TPI + float(asinf(new_sin)))
        az = F32(new_az)
        out.append(az)
    raise RuntimeError("the walk does not end")


def linear_delays(ypos, azimuth):
    """calcDelaysOfLinearMicrophoneArray (localization.cc:107-118): float azimuth, float distance, the rest double."""
    d = np.zeros(len(ypos))
    for i in range(1, len(ypos)):
        dist = F32(abs(ypos[i] - ypos[0]))
        d[i] = -float(dist) * math.sin(float(F32(azimuth))) / SSPEED
    return d


def linear_grid(fs, N, spacing=None, positions=None, numpy_f32=False):
    ypos, const_v, mtd = linear_geometry(fs, N, spacing, positions)
    az = linear_walk(const_v, numpy_f32)
    delays = np.stack([linear_delays(ypos, a) for a in az])
    return dict(azimuths=az, delays=delays, tau=sample_delays(fs, delays), D=max_sample_delay(fs, mtd), max_time_delay=mtd,
                const_v=const_v, prod=float(fs) * delays)


def synthetic(rng, N, nsamp, true_tau, amp=3000.0, noise_db=-10.0, smooth=8):
    """A smoothed common source with per-channel integer delays plus independent noise `noise_db` below it, rounded to integers
    at PCM scale -> float32 [N][nsamp].  Channel c carries the source delayed so that x_c[f + true_tau_c] lines up over c."""
    true_tau = np.asarray(true_tau, np.int64)
    pad = int(np.max(np.abs(true_tau))) + smooth
    src = rng.normal(size=nsamp + 2 * pad + smooth)
    src = np.convolve(src, np.ones(smooth) / math.sqrt(smooth), mode="valid")
    src *= amp / src.std()
    x = np.empty((N, nsamp))
    for c in range(N):
        o = pad - int(true_tau[c])
        x[c] = src[o:o + nsamp] + rng.normal(size=nsamp) * amp * 10.0 ** (noise_db / 20.0)
    return np.rint(x).astype(F32)
