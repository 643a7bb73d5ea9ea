"""Yardstick of the block-convolution tests (a helper, not a test): the direct sums in float64 on float32-valued inputs, a
loop-for-loop numpy restatement of OverlapAdd::next / OverlapSave::next (convolution/convolution.cc:83-131, :196-230: float64
transform, float32 buffer, shift), and the derived error bound of the device's tile kernel.

Bound of a tile (derived in tests/test_gpu_conv.py, evaluated here).  u = 2^-24, B = (log2 N + 1) eta of DESIGN 3.17.  With x_q
the span partition q of the tile transforms (N samples, zero where the kernel reads zero) and h_q its taps:

    d_q   = B |x_q|_2 |h_q|_1 + B |x_q|_1 |h_q|_2 + B^2 sqrt(N) |x_q|_2 |h_q|_2
    e_G   = sum_q [(1 + c) d_q + c |x_q|_2 |h_q|_1],      c = sqrt(2) gamma_2 + (Q - 1) u
    bound = e_G + B (sum_q |x_q|_2 |h_q|_1 + e_G)         on the 2-norm of the tile's error
"""
import math

import numpy as np

U = 2.0 ** -24
MU = 2.0 ** -24
G4 = 4 * U / (1 - 4 * U)
ETA = MU + G4 * (math.sqrt(2.0) + MU)
G2 = 2 * U / (1 - 2 * U)


# (name, (N, Lk, Bp, Q), P, S_h, rule): the plans of tests/test_gpu_conv.py's test_every_length, two per transform length the
# other tests leave out.  "full": Q = 1 and Lk + P - 1 == N, the section exactly full.  "part": Q = 3, P = 2 Bp + r with
# 0 < r < Bp (a short last partition) and Lk + Bp - 1 == N.  S_h: 1 = filters shared by the streams, 0 = one set per stream.
# rule: (P, n_max) where the plan is the one btk_conv_plan picks for that call, else None.  S = 2, C = 2 everywhere; the row
# ends inside the third tile (case_len).
CASES = [
    ("n1024_full", (1024, 600, 425, 1), 425, 1, None),
    ("n1024_part", (1024, 725, 300, 3), 730, 1, None),
    ("n2048_full", (2048, 1100, 949, 1), 949, 1, None),
    ("n2048_part", (2048, 1349, 700, 3), 1733, 0, None),
    ("n4096_full", (4096, 2500, 1597, 1), 1597, 1, None),
    ("n4096_part", (4096, 2597, 1500, 3), 3700, 1, None),
    ("n8192_full", (8192, 5000, 3193, 1), 3193, 1, None),
    ("n8192_part", (8192, 5193, 3000, 3), 7111, 0, None),
    ("n8192_rule_p500", (8192, 7693, 500, 1), 500, 1, (500, 16384)),
    ("n8192_rule_p5000", (8192, 4097, 4096, 2), 5000, 1, (5000, 8192)),
]
CASE_S, CASE_C = 2, 2


def case_len(plan):
    """samples of a case's rows: two whole tiles and an odd part of the third"""
    Lk = plan[1]
    return 2 * Lk + Lk // 3 + 1


def b_n(N):
    return (math.log2(N) + 1) * ETA


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def direct(x, h, out_len=None, hist=0):
    """y[n] = sum_p h[p] x[hist + n - p] in float64; x holds `hist` samples of the past in front, zeros before them."""
    x = np.asarray(x, np.float32).astype(np.float64)
    h = np.asarray(h, np.float32).astype(np.float64)
    full = np.convolve(x, h)[hist:]
    out_len = len(x) - hist if out_len is None else out_len
    y = np.zeros(out_len)
    m = min(out_len, len(full))
    y[:m] = full[:m]
    return y


def direct_abs(x, h, out_len=None, hist=0):
    """sum_p |h[p]| |x[n - p]|: what every rounding of a running sum is relative to."""
    return direct(np.abs(np.asarray(x, np.float32)), np.abs(np.asarray(h, np.float32)), out_len, hist)


def blocks_direct(x, h, L, step):
    """OverlapSave's block form by explicit loops: out[t][j] = sum_{p < P} h[p] x[t step + j + P - p], j < L - P."""
    x = np.asarray(x, np.float32).astype(np.float64)
    h = np.asarray(h, np.float32).astype(np.float64)
    P = len(h)
    T = (len(x) - L) // step + 1 if len(x) >= L else 0
    out = np.zeros((T, L - P))
    for t in range(T):
        for j in range(L - P):
            acc = 0.0
            for p in range(P):
                acc += h[p] * x[t * step + j + P - p]
            out[t, j] = acc
    return out


def next_pow2(n):
    v = 1
    while v < n:
        v *= 2
    return v


def overlap_add_restated(blocks, h, fft_len=0):
    """OverlapAdd::next over `blocks` ([T][L], as the source serves them): float64 transform of the zero-padded block, product
    with the frequency response (bins 0 and N/2 real times real), inverse, the L + P - 1 results added into a FLOAT32 buffer,
    its first L values handed out, the buffer shifted down by L."""
    blocks = np.asarray(blocks, np.float32)
    h = np.asarray(h, np.float64)
    T, L = blocks.shape
    P = len(h)
    if fft_len == 0:
        N = next_pow2(L + P - 1)
    else:
        if fft_len < L + P - 1:
            raise ValueError("Section (%d) and impulse response (%d) lengths inconsistent with FFT length (%d)." % (L, P, fft_len))
        N = fft_len
    sec = np.zeros(N)
    sec[:P] = h
    H = np.fft.rfft(sec)
    H[0] = H[0].real
    H[N // 2] = H[N // 2].real
    buf = np.zeros(L + P - 1, np.float32)
    out = np.zeros((T, L), np.float32)
    for t in range(T):
        sec = np.zeros(N)
        sec[:L] = blocks[t].astype(np.float64)
        X = np.fft.rfft(sec)
        Y = X * H
        Y[0] = X[0].real * H[0].real
        Y[N // 2] = X[N // 2].real * H[N // 2].real
        sec = np.fft.irfft(Y, N)
        for i in range(L + P - 1):
            buf[i] = np.float32(np.float64(buf[i]) + sec[i])
        out[t] = buf[:L]
        for i in range(P - 1):
            buf[i] = buf[i + L] if i + L < L + P - 1 else np.float32(0)
        for i in range(P - 1, L + P - 1):
            buf[i] = 0
    return out


def overlap_save_restated(blocks, h):
    """OverlapSave::next: every block alone, an L-point circular convolution, samples P .. L - 1 handed out."""
    blocks = np.asarray(blocks, np.float32)
    h = np.asarray(h, np.float64)
    T, L = blocks.shape
    P = len(h)
    if P >= L:
        raise ValueError("Cannot have P = %d and L = %d" % (P, L))
    sec = np.zeros(L)
    sec[:P] = h
    H = np.fft.rfft(sec)
    out = np.zeros((T, L - P), np.float32)
    for t in range(T):
        X = np.fft.rfft(blocks[t].astype(np.float64))
        Y = X * H
        Y[0] = X[0].real * H[0].real
        Y[L // 2] = X[L // 2].real * H[L // 2].real
        sec = np.fft.irfft(Y, L)
        for i in range(P, L):
            out[t, i - P] = sec[i]
    return out


def _transforms64(blocks, h, N):
    """what the float64 transforms of one section leave on each of its samples: three transforms (block, response, inverse), each
    within (log2 N + 1) eta_64 of its operand's 2-norm: 3 (log2 N + 1) eta_64 |block|_2 |h|_1 (eta_64: eta at u = 2^-53)"""
    blocks = np.asarray(blocks, np.float64)
    u64 = 2.0 ** -53
    eta64 = u64 + 4 * u64 / (1 - 4 * u64) * (math.sqrt(2.0) + u64)
    return 3 * (math.log2(N) + 1) * eta64 * math.sqrt(float(np.max(np.sum(blocks * blocks, axis=1)))) * float(np.abs(h).sum())


def running_sum_bound(blocks, x, h, out_len):
    """(k + 1) 2^-24 sum_p |h[p]| |x[n - p]|, k = sections that reach one buffer cell = ceil((P - 1) / L) + 1, plus what the
    float64 transforms of those k sections leave."""
    L, P = np.shape(blocks)[1], len(h)
    k = -(-(P - 1) // L) + 1
    return (k + 1) * U * direct_abs(x, h, out_len) + k * _transforms64(blocks, h, next_pow2(L + P - 1))


def block_rounding_bound(blocks, h, mag):
    """OverlapSave: one float32 rounding of a float64 result whose terms' magnitudes sum to `mag`, and one section's transforms"""
    return U * np.asarray(mag) + _transforms64(blocks, h, np.shape(blocks)[1])


def _span(x, hist, at, N, i0, i1):
    """span elements i0 .. i1 - 1 of the N samples from stream index `at` on (x[hist + n] is sample n; zero outside x)"""
    s = np.zeros(N)
    lo = max(i0, 0, -hist - at)
    hi = min(i1, N, len(x) - hist - at)
    if hi > lo:
        s[lo:hi] = x[hist + at + lo:hist + at + hi]
    return s


def _tile_bound(spans, taps, N, Q):
    B = b_n(N)
    c = math.sqrt(2.0) * G2 + (Q - 1) * U
    eG = sx = 0.0
    for xq, hq in zip(spans, taps):
        x1, x2, h1, h2 = np.abs(xq).sum(), math.sqrt((xq * xq).sum()), np.abs(hq).sum(), math.sqrt((hq * hq).sum())
        d = B * x2 * h1 + B * x1 * h2 + B * B * math.sqrt(N) * x2 * h2
        eG += (1 + c) * d + c * x2 * h1
        sx += x2 * h1
    return eG + B * (sx + eG)


def apply_tile_bounds(x, h, plan, out_len, hist=0):
    """[(first output, outputs stored, 2-norm bound)] for every tile of btk_conv_apply on one row."""
    N, Lk, Bp, Q = plan
    x = np.asarray(x, np.float32).astype(np.float64)
    h = np.asarray(h, np.float32).astype(np.float64)
    P = len(h)
    o = Bp - 1
    res = []
    for j in range(-(-out_len // Lk)):
        n = min(Lk, out_len - j * Lk)
        spans, taps = [], []
        for q in range(Q):
            hq = h[q * Bp:min((q + 1) * Bp, P)]
            spans.append(_span(x, hist, j * Lk - o - q * Bp, N, o - (len(hq) - 1), o + n))
            taps.append(hq)
        res.append((j * Lk, n, _tile_bound(spans, taps, N, Q)))
    return res


def blocks_tile_bounds(x, h, L, step):
    x = np.asarray(x, np.float32).astype(np.float64)
    h = np.asarray(h, np.float32).astype(np.float64)
    T = (len(x) - L) // step + 1 if len(x) >= L else 0
    return [_tile_bound([_span(x, 0, t * step, L, 1, L)], [h], L, 1) for t in range(T)]


def worst_ratio(y, ref, tiles):
    """largest (2-norm of a tile's error) / (its bound) over the tiles of one output row; a tile whose bound is 0 must be exact"""
    worst = 0.0
    for first, n, bound in tiles:
        err = math.sqrt(float(np.sum((np.asarray(y[first:first + n], np.float64) - ref[first:first + n]) ** 2)))
        if bound == 0.0:
            assert err == 0.0, "a tile with nothing in its span holds %g" % err
        else:
            worst = max(worst, err / bound)
    return worst
