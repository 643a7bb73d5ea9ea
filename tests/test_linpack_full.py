"""CPU checks of svd_rule = "linpack_full" (csrc/linpack_f32.h): csvdc with job = 11 -- U and V rotation for rotation -- and
pseudoinverse()'s assembly A+ = V S^-1 U^H (beamformer/beamformer.cc:262-280), the kernel bodies compiled by g++ as serial code
(tests/cpp/linpack_full_host.cc), against what the reference's own compiled csvdc returned
(tests/golden/csvdc_full_test_matrices.npz, oracle/_ref itself where built) -- bit for bit.  The GPU build of the same bodies is
checked in tests/test_gpu_linpack_full.py."""
import os
import zlib

import numpy as np
import pytest

from tests import linpack_full_host as lf
from tests import linpack_host as lh

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "csvdc_full_test_matrices.npz")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _colmajor_bytes(a):
    return np.ascontiguousarray(np.asarray(a, np.complex64).T).tobytes()


def dead_channel_matrices(N):
    """The matrices of test_dead_channel_in_the_middle_of_the_array_is_a_stated_deviation (tests/test_gpu_postfilter_cov_mvdr.py):
    R [3][N][N] -- no dead channel, one in the middle, one at the end -- and d [3][N]."""
    rng = np.random.default_rng(N)
    X = rng.normal(size=(N, 3 * N)) + 1j * rng.normal(size=(N, 3 * N))
    R0 = (X @ X.conj().T / (3 * N) + 0.01 * np.eye(N)).astype(np.complex64)
    d = (np.exp(-2j * np.pi * rng.uniform(size=(3, N))) / N).astype(np.complex64)
    R = np.stack([R0, R0, R0]).copy()
    mid = N // 2
    R[1][:, mid] = 0; R[1][mid, :] = 0
    R[2][:, N - 1] = 0; R[2][N - 1, :] = 0
    return R, d


def test_host_csvdc_full_matches_reference_bit_for_bit(orc):
    """s, e, INFO and the singular vectors U, V of all 64 matrices -- tall, wide, rank deficient, zero column -- equal the
    fixture (full matrices up to 40 x 40, CRC of the bytes beyond) and oracle/_ref itself where it is built."""
    z = np.load(GOLDEN)
    mats = lh.test_matrices()
    assert [tuple(A.shape) for A in mats] == [tuple(sh) for sh in z["shape"]]
    full = set(int(i) for i in z["full"])
    assert len(full) >= 40
    for i, A in enumerate(mats):
        s, e, U, V, info = lf.csvdc_full(A)
        m = len(s)
        assert info == int(z["info"][i]), (A.shape, info)
        assert np.array_equal(_bits(s), _bits(z["s"][i, :m])) and np.array_equal(_bits(e), _bits(z["e"][i, :m])), A.shape
        assert zlib.crc32(_colmajor_bytes(U)) == int(z["u_crc"][i]) and zlib.crc32(_colmajor_bytes(V)) == int(z["v_crc"][i]), A.shape
        if i in full:
            assert np.array_equal(_bits(U), _bits(z["u_%d" % i])) and np.array_equal(_bits(V), _bits(z["v_%d" % i])), A.shape
        if orc.ref_lib() is not None:
            sr, er, ur, vr, ir = lf.ref_csvdc_full(orc, A)
            assert info == ir and np.array_equal(_bits(s), _bits(sr)) and np.array_equal(_bits(e), _bits(er)), A.shape
            assert np.array_equal(_bits(U), _bits(ur)) and np.array_equal(_bits(V), _bits(vr)), A.shape


def test_vectors_do_not_feed_back():
    """s, e and INFO of the job = 11 body equal the job = 0 body's (lh.csvdc_values): the compile-time switch changes nothing there."""
    for A in lh.test_matrices():
        s, e, _, _, info = lf.csvdc_full(A)
        s0, e0, info0 = lh.csvdc_values(A)
        assert info == info0 and np.array_equal(_bits(s), _bits(s0)) and np.array_equal(_bits(e), _bits(e0)), A.shape


def test_host_pinv_assemble_equals_the_numpy_restatement():
    """pinv_assemble on the reference's U, V, s (fixture) against the numpy restatement of beamformer.cc:262-280 -- separate
    float32 real / imaginary arrays, one ufunc per operation, k serial -- value for value, and the same `ok`."""
    z = np.load(GOLDEN)
    done = 0
    for i in (int(i) for i in z["full"]):
        n, p = (int(v) for v in z["shape"][i])
        if n < p:
            continue
        s, U, V, info = z["s"][i, :p], z["u_%d" % i], z["v_%d" % i], int(z["info"][i])
        inv, below = lf.pinv_assemble(s, U, V, 1.0e-8)
        want, ok = lf.pinv_restated(s, U, V, info, 1.0e-8)
        assert np.all(inv == want), (n, p, float(np.max(np.abs(inv - want))))
        assert (info == 0 and below == 0) == ok
        done += 1
    assert done >= 36


def test_restated_inverse_against_oracle_summation_order(orc):
    """orc.pseudoinverse sums the N terms of an element with np.sum (pairwise), the source left to right: two float32 summation
    orders of the same terms plus two complex products per term differ by at most 2 (N + 8) 2^-24 sum_k |v[j,k]| |sinv[k]| |u[i,k]|."""
    if orc.ref_lib() is None:
        pytest.skip("oracle/_ref not built: the oracle's pseudoinverse() then uses another SVD")
    worst = 0.0
    for A in lh.test_matrices():
        n, p = A.shape
        if n != p or n > 64:
            continue
        s, e, U, V, info = lf.csvdc_full(A)
        inv, below = lf.pinv_assemble(s, U, V, 1.0e-8)
        ref, ok, iref = orc.pseudoinverse(A.astype(np.complex128), 1.0e-8, return_info=True)
        assert iref == info and ok == (info == 0 and below == 0)
        sinv = np.array([0.0 if abs(x) < np.float32(1.0e-8) else 1.0 / float(x) for x in s[:p]])
        terms = np.abs(V.astype(np.complex128)) @ np.diag(np.abs(sinv)) @ np.abs(U.astype(np.complex128)).T      # [j, i]
        bound = 2.0 * (p + 8) * 2.0 ** -24 * terms
        diff = np.abs(inv.astype(np.complex128) - ref)
        assert np.all(diff <= bound), (n, float(np.max(diff / np.maximum(bound, 1e-300))))
        worst = max(worst, float(np.max(diff / np.maximum(terms, 1e-300))) * 2.0 ** 24)
    print("\nworst |A+ - A+_oracle| = %.2f x 2^-24 x sum |terms|" % worst)


@pytest.mark.parametrize("N", [8, 64])
def test_dead_channel_gets_the_reference_inverse(orc, N):
    """The matrices of the stated deviation of the default rule: with the dead channel in the middle pseudoinverse() returns true
    and inverts sigma ~ 5e-8 (max |A+| > 1e6); at the end sigma = 0 and it returns false.  The weights of the float64 formula on
    the host build's inverse agree with calc_mvdr_weights on the oracle's pseudoinverse() to 1e-6."""
    from tests.test_gpu_postfilter_cov_mvdr import _oracle_mvdr_bin
    R, d = dead_channel_matrices(N)
    res = []
    for k in range(3):
        s, e, U, V, info = lf.csvdc_full(R[k])
        inv, below = lf.pinv_assemble(s, U, V, 1.0e-8)
        res.append((inv, info == 0 and below == 0))
    assert res[0][1] and res[1][1] and not res[2][1]
    assert np.max(np.abs(res[1][0])) > 1e6
    if orc.ref_lib() is None:
        return                                                  # (the oracle's stand-in SVD finds the exact zero: nothing to compare)
    for k in range(3):
        w, _ = lf.mvdr_from_inverse(res[k][0], res[k][1], d[k])
        ref = _oracle_mvdr_bin(orc, R[k].astype(np.complex128), d[k].astype(np.complex128))
        rel = np.linalg.norm(w - ref) / np.linalg.norm(ref)
        print("N = %d bin %d: || w - w_oracle || / || w_oracle || = %.3g" % (N, k, rel))
        assert rel <= 1e-6, (N, k, rel)
