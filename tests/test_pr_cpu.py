"""The closed forms of the PR banks and the windowed FFT bank (pr_closed_form.py) against the literal restatement of the
reference's ring buffers and next() loops; frame counts, windows, and the sine-window known answer.  No GPU, no library."""
import numpy as np
import pytest

import pr_closed_form as pcf

GEOMETRIES = [(8, 1, 0), (8, 2, 0), (8, 3, 1), (16, 4, 2), (8, 2, 1)]           # (M, m, r)


def _case(M, m, r, L):
    h = pcf.random_prototype(M, m, seed=3)
    x = pcf.int_signal(L, seed=M + 10 * m + r)
    return h, x


@pytest.mark.parametrize("M,m,r", GEOMETRIES)
def test_analysis_closed_form_is_the_literal_bank(M, m, r):
    D = M >> r
    for L in (5 * D, 7 * D + max(D - 1, 1) // 2 + (D > 1)):                       # whole blocks, and a short last block
        h, x = _case(M, m, r, L)
        lit, cf = pcf.pr_analysis_literal(h, M, m, r, x), pcf.pr_analysis_cf(h, M, m, r, x)
        assert lit.shape == cf.shape == (-(-L // D) + 2 * m - 1, 2 * M)
        # integer samples times float32 taps: every product and sum is exact in float64, and the transform is the same routine
        assert np.max(np.abs(lit - cf)) == 0.0


@pytest.mark.parametrize("M,m,r", GEOMETRIES)
def test_synthesis_closed_form_is_the_literal_bank(M, m, r):
    D = M >> r
    h, x = _case(M, m, r, 9 * D + (1 if D > 1 else 0))
    Y = pcf.pr_analysis_cf(h, M, m, r, x)
    rng = np.random.default_rng(5)
    Y = Y + (rng.normal(size=Y.shape) + 1j * rng.normal(size=Y.shape)) * 10.0    # not a real signal's spectrum: all M2 bins count
    lit, bound = pcf.pr_synthesis_literal(h, M, m, r, Y)
    cf = pcf.pr_synthesis_cf(h, M, m, r, Y)
    assert lit.shape == cf.shape == ((Y.shape[0] - (2 * m - 1)) * D,)
    # the literal bank adds 2R terms into a float32 vector: each add rounds by at most 2^-24 of the partial sum, which is at most
    # sum |terms|; the float64 sums on both sides are 2^-29 finer and get a thousandth of the bound
    err = np.abs(lit.astype(np.float64) - cf)
    assert np.all(err <= bound * 1.001 + 1e-300), float(np.max(err / np.maximum(bound, 1e-300)))
    assert np.max(err) > 0 or np.max(np.abs(cf)) == 0                            # the float32 sum is really there


def test_frame_and_block_counts():
    for M, m, r in GEOMETRIES:
        D = M >> r
        for L in (0, 1, D, 3 * D, 3 * D + 1):
            T = pcf.pr_num_frames(L, M, m, r)
            assert T == -(-L // D) + 2 * m - 1
            assert pcf.pr_analysis_cf(pcf.random_prototype(M, m), M, m, r, np.zeros(L, np.float32)).shape[0] == T
            assert pcf.pr_num_blocks(T, m) == -(-L // D)
    assert pcf.pr_num_blocks(2, 2) == 0
    assert pcf.stft_num_frames(17, 8, 1) == 5 + 1


@pytest.mark.parametrize("M,r,lag", [(8, 0, 0), (16, 0, 0), (8, 1, 8)])
def test_sine_window_round_trip(M, r, lag):
    """m = 1 with h[n] = sin(pi (n + 1/2) / M2): analysis -> synthesis returns the input, gain 1, at lag 0 (r = 0) or M (r = 1).
    The first 2R - 1 blocks lack the overlap partners the bank leaves at zero while it primes its ring, so they are not compared."""
    h = pcf.sine_prototype(M)
    L = 12 * M
    x = np.random.default_rng(1).normal(size=L)
    out = pcf.pr_synthesis_cf(h, M, 1, r, pcf.pr_analysis_cf(h, M, 1, r, x))
    assert out.shape == (L,)
    ref = np.concatenate([np.zeros(lag), x])[:L]
    skip = (2 * (1 << r) - 1) * (M >> r)
    assert np.max(np.abs(out - ref)[skip:]) <= 1e-13 * np.max(np.abs(x))
    assert np.max(np.abs(out - ref)[:skip]) > 1e-3                               # (and the primed blocks really differ)


@pytest.mark.parametrize("M,r,wt", [(8, 0, 0), (8, 1, 1), (16, 2, 2)])
def test_stft_closed_form_is_the_literal_bank(M, r, wt):
    D = M >> r
    x = pcf.int_signal(6 * D + 1, seed=2)
    lit, cf = pcf.stft_literal(M, r, wt, x), pcf.stft_cf(M, r, wt, x)
    assert lit.shape == cf.shape == (7 + 1, M)
    assert np.max(np.abs(lit - cf)) == 0.0


def test_windows_at_length_8():
    i = np.arange(8)
    assert np.array_equal(pcf.get_window_cf(0, 8), np.ones(8))
    np.testing.assert_allclose(pcf.get_window_cf(2, 8), 0.5 - 0.5 * np.cos(2 * np.pi * i / 7), rtol=0, atol=1e-15)
    np.testing.assert_allclose(pcf.get_window_cf(1, 8), 0.54 - 0.46 * np.cos(2 * np.pi * i / 7), rtol=0, atol=1e-15)
    np.testing.assert_array_equal(pcf.get_window_cf(7, 8), pcf.get_window_cf(1, 8))       # anything else is Hamming
    assert pcf.get_window_cf(2, 8)[0] == 0.0 and abs(pcf.get_window_cf(1, 8)[0] - 0.08) < 1e-15
