"""CPU: the float64 closed form of WPE (tests/wpe_closed_form.py) against the oracle's restatement of
dereverberation.cc:312-698 -- both float64, only the summation order differs -- on every axis the GPU tests of
tests/test_gpu_wpe_stages.py lean on: band limiting, delayed prediction, lower >= L, loading and diagonal bias.  Also the inputs,
the condition-number guard and the float32-against-float64 figure of the heavy-loading cases of that file."""
import functools

import numpy as np
import pytest

from tests import wpe_closed_form as cf
from tests.test_gpu_wpe import _reverberant

FS = 16000.0


def rounded_input(seed, S, C, M, T):
    """reverberant subband signals, one independent draw per stream, rounded to complex64 ("what the GPU saw") -> [S][K][C][T]"""
    K = M // 2 + 1
    X = np.zeros((S, K, C, T), np.complex64)
    for s in range(S):
        Y = _reverberant(np.random.default_rng(seed + 7919 * s), T, C, M)
        X[s] = np.transpose(Y[:, :, :K], (2, 1, 0))
    return X


def oracle_frames(Xs, M):
    """one stream [K][C][T] complex64 -> the oracle's [T][C][M] complex128 with the conjugate-symmetric upper half"""
    K = M // 2 + 1
    Y = np.zeros((Xs.shape[2], Xs.shape[1], M), np.complex128)
    Y[:, :, :K] = np.transpose(Xs.astype(np.complex128), (2, 1, 0))
    Y[:, :, K:] = np.conj(Y[:, :, M // 2 - 1:0:-1])
    return Y


def oracle_taps(orc, Xs, M, lower, upper, iters, load_db, band_width, bias):
    """-> (G [C][K][P] on the engine's layout, the oracle's own G [C][M][P])"""
    G = orc.wpe_estimate(oracle_frames(Xs, M), lower, upper, iters, load_db, band_width, bias, FS)
    return G[:, :M // 2 + 1], G


def oracle_output(orc, Xs, Gfull, M, lower, upper, band_width):
    out = orc.wpe_apply(oracle_frames(Xs, M), Gfull, lower, upper, band_width, FS)
    return np.transpose(out[:, :, :M // 2 + 1], (2, 1, 0))                  # [K][C][T]


# (C, lower, upper, band_width, load_db, diagonal_bias, iterations, T)
CASES = [(1, 0, 3, 0.0, -18.0, 1e-4, 2, 120), (1, 2, 6, 3000.0, -40.0, 0.0, 2, 150), (3, 0, 4, 3000.0, -18.0, 1e-4, 2, 200),
         (3, 1, 5, 8000.0, 0.0, 10.0, 1, 160), (3, 3, 5, 0.0, -18.0, 1e-4, 2, 130), (3, 5, 6, 3000.0, -40.0, 10.0, 2, 90),
         (8, 0, 3, 3000.0, -18.0, 0.0, 2, 200), (8, 1, 4, 0.0, 0.0, 1e-4, 1, 140), (8, 2, 3, 8000.0, -40.0, 1e-4, 2, 170),
         (8, 0, 5, 3000.0, 0.0, 0.0, 2, 111), (1, 4, 4, 8000.0, -18.0, 10.0, 1, 64), (3, 0, 0, 3000.0, -18.0, 0.0, 2, 50)]


@pytest.mark.parametrize("C,lower,upper,bw,load_db,bias,iters,T", CASES)
def test_closed_form_matches_the_oracle(orc, C, lower, upper, bw, load_db, bias, iters, T):
    M, K = 16, 9
    X = rounded_input(1000 + 10 * C + lower + upper, 1, C, M, T)
    lo, up = cf.band(M, bw, FS)
    assert lo == {0.0: 8, 3000.0: 3, 8000.0: 8}[bw] and (lo, up) == tuple(orc.wpe_band(M, bw, FS))
    Gref, Gfull = oracle_taps(orc, X[0], M, lower, upper, iters, load_db, bw, bias)
    G = cf.estimate(X.astype(np.complex128), lower, upper, iters, load_db, bias, lo, up)
    gs = np.max(np.abs(Gref))
    assert gs > 1e-4
    assert np.max(np.abs(G[0] - Gref)) <= 1e-9 * gs
    inactive = [k for k in range(K) if not cf.active(k, lo, up)]
    assert len(inactive) == (5 if bw == 3000.0 else 0)
    assert np.all(G[0][:, inactive] == 0) and np.all(Gref[:, inactive] == 0)
    # apply with the oracle's taps on both sides: prediction alone, the ring rule included
    ref = oracle_output(orc, X[0], Gfull, M, lower, upper, bw)
    X = X.astype(np.complex128)
    out, mag = cf.predict(X, Gref[None], lower, upper, lo, up, apply=True)
    assert np.array_equal(out, cf.apply(X, Gref[None], lower, upper, lo, up))
    assert np.max(np.abs(out[0] - ref)) <= 1e-9 * np.max(np.abs(ref))
    assert np.all(mag >= np.abs(X)) and np.all(np.abs(out) <= mag * (1 + 1e-12))
    assert np.array_equal(out[0][:, :, :lower], X[0][:, :, :lower]) and np.array_equal(out[0][inactive], X[0][inactive])
    if lower >= upper - lower + 1:                                         # no tap reaches a frame of the ring
        assert np.array_equal(out, X) and np.array_equal(ref, X[0])
    else:
        assert np.max(np.abs(out - X)) > 1e-3 * np.max(np.abs(X))


def test_stages_compose(orc):
    """weights, normal_equations and load_and_solve chained by hand give estimate(); several streams are independent"""
    M, C, lower, upper, T = 16, 3, 1, 4, 100
    X = rounded_input(5, 2, C, M, T).astype(np.complex128)
    lo, up = cf.band(M, 0.0, FS)
    G1 = cf.estimate(X, lower, upper, 1, -18.0, 1e-4, lo, up)
    W = cf.weights(X)
    assert np.array_equal(W, 1.0 / np.maximum(np.abs(X), 1e-3) ** 2)
    R, r = cf.normal_equations(X, W, lower, upper)
    assert np.max(np.abs(R - np.conj(np.swapaxes(R, -1, -2)))) <= 1e-12 * np.max(np.abs(R))
    assert np.array_equal(cf.load_and_solve(R, r, -18.0, 1e-4), G1)
    e, _ = cf.predict(X, G1, lower, upper, lo, up, apply=False)
    R2, r2 = cf.normal_equations(X, cf.weights(e), lower, upper)
    G2 = cf.load_and_solve(R2, r2, -18.0, 1e-4)
    assert np.array_equal(G2, cf.estimate(X, lower, upper, 2, -18.0, 1e-4, lo, up))
    for s in range(2):
        Gref, _ = oracle_taps(orc, X[s].astype(np.complex64), M, lower, upper, 2, -18.0, 0.0, 1e-4)
        assert np.max(np.abs(G2[s] - Gref)) <= 1e-9 * np.max(np.abs(Gref))
    assert np.max(np.abs(G2[0] - G2[1])) > 1e-2 * np.max(np.abs(G2))


def test_band_matches_the_engine():
    from distant_speech_recognition_amd import engine as eng, _lib
    for M in (16, 64, 256, 512):
        for bw in (0.0, 1.0, 2000.0, 2999.9, 3000.0, 3000.1, 7999.0, 8000.0):
            assert cf.band(M, bw, FS) == tuple(eng.wpe_band(M, bw, FS))
    assert cf.band(16, 3000.0, FS) == (3, 13) and cf.band(64, 2000.0, FS) == (8, 56) and cf.band(16, 8000.0, FS) == (8, 8)
    assert [cf.active(k, 3, 13) for k in range(9)] == [True] * 4 + [False] * 5
    with pytest.raises(_lib.BtkError):
        eng.wpe_band(16, 8001.0, FS)
    with pytest.raises(ValueError):
        cf.band(16, 8001.0, FS)


# ---- the heavy-loading cases of tests/test_gpu_wpe_stages.py (e): inputs, the guard on their conditioning and the rounding level of
# float32 arithmetic on them, all from the closed form alone.
E_SHAPES = [(8, 1, 10, 300), (4, 0, 15, 300), (5, 1, 9, 300), (6, 0, 6, 200)]          # (C, lower, upper, T) of (c) and (d), M = 16
E_LOADS = [(0.0, 0.0), (10.0, 0.0), (-40.0, 1e-2), (-18.0, 10.0)]                       # (load_db, diagonal_bias)
# (C, lower, upper, T, load_db, diagonal_bias, iterations)
E_CASES = [s + l + (1,) for s in E_SHAPES for l in E_LOADS] + [(8, 1, 10, 300, 0.0, 0.0, 2)]
# largest tap difference of estimate(complex64) from estimate(complex128), relative to the largest tap, as measured by
# test_float32_ratio_of_the_heavy_loading_cases (numpy 2, OpenBLAS), in the order of E_CASES:
#   C=8 (1,10): 2.4e-7, 2.0e-7, 2.0e-3, 6.8e-6;   C=4 (0,15): 2.3e-7, 2.6e-7, 4.5e-4, 4.9e-6;   C=5 (1,9): 2.1e-7, 2.1e-7, 2.6e-3, 6.5e-6
#   C=6 (0,6): 1.9e-7, 1.7e-7, 8.2e-4, 6.8e-6;   C=8 (1,10), two iterations at 0 dB: 5.6e-7
# (condition numbers of the loaded matrices: 10..20 at 0 dB, 2..3 at +10 dB, 1e5..2e5 at -40 dB / 1e-2, 570..1200 at -18 dB / 10)
E_FLOOR = 1.0e-6


def e_input(C, lower, upper, T):
    return rounded_input(31000 + 100 * C + upper, 1, C, 16, T)


@functools.lru_cache(maxsize=None)
def e_reference(case):
    """-> (G float64 [1][C][K][P], largest tap, float32 ratio, largest condition number of the loaded matrices)"""
    C, lower, upper, T, load_db, bias, iters = case
    X = e_input(C, lower, upper, T)
    G64, Rl = cf.estimate(X.astype(np.complex128), lower, upper, iters, load_db, bias, 8, 8, np.complex128, return_loaded=True)
    G32 = cf.estimate(X, lower, upper, iters, load_db, bias, 8, 8, np.complex64)
    assert G32.dtype == np.complex64 and G64.dtype == np.complex128
    gs = float(np.max(np.abs(G64)))
    Rl = np.tril(Rl) + np.conj(np.swapaxes(np.tril(Rl, -1), -1, -2))
    return G64, gs, float(np.max(np.abs(G32 - G64))) / gs, float(np.max(np.linalg.cond(Rl)))


def e_tolerance(case):
    """4 x the float32 figure of the closed form, floor 1e-6, relative to the largest tap"""
    return max(4.0 * e_reference(case)[2], E_FLOOR)


@pytest.mark.parametrize("case", E_CASES, ids=lambda c: "C%d-%d_%d-%gdB-%g-it%d" % (c[0], c[1], c[2], c[4], c[5], c[6]))
def test_float32_ratio_of_the_heavy_loading_cases(orc, case):
    C, lower, upper, T, load_db, bias, iters = case
    G64, gs, ratio, cond = e_reference(case)
    print("WPE heavy loading %s: largest tap %.3g, float32/float64 %.3g, cond %.3g" % (case, gs, ratio, cond))
    assert gs > 1e-3                                                       # taps that carry information
    if load_db >= 0:
        assert cond < 50
    # float32 rounding, not a blunder of the float32 path: eps = 6e-8 times the conditioning, far below the 2e-3 of the end-to-end tests
    assert 0 < ratio < 2e-7 * max(cond, 10.0)
    Gref, _ = oracle_taps(orc, e_input(C, lower, upper, T)[0], 16, lower, upper, iters, load_db, 0.0, bias)
    assert np.max(np.abs(G64[0] - Gref)) <= 1e-9 * gs
