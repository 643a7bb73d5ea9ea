"""Golden data for tests/test_linpack_full.py: what the REFERENCE's OWN compiled LINPACK csvdc (oracle/_ref, built in the dev
container) returns with job = 11 -- singular vectors included -- for the fixed matrix family tests/linpack_host.test_matrices().
Stored -> tests/golden/csvdc_full_test_matrices.npz:
  shape        int32 [64][2]       (n, p) of each matrix, to catch a changed family
  info         int32 [64]          csvdc's INFO
  s, e         float32 [64][150]   the first m = min(n + 1, p) entries of s and e (real parts), zero beyond m
  u_crc, v_crc uint32 [64]         crc32 of u's (n x n) and v's (p x p) bytes in the reference's memory order (column-major)
  full         int32 [*]           the matrices with max(n, p) <= 40, whose vectors are stored in full:
  u_<i>, v_<i> complex64           U [n][n], V [p][p] of matrix i (element [r, c] is the reference's u[r + c * ldu])
Only numbers are stored.

Run:  python tests/golden/gen_csvdc_full_test_matrices.py"""
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
FULL_MAX = 40


def colmajor_bytes(a):
    return np.ascontiguousarray(np.asarray(a, np.complex64).T).tobytes()


def main():
    from oracle import oracle as orc
    from tests import linpack_full_host as lf
    from tests import linpack_host as lh
    orc.build(ref=True)
    assert orc.ref_lib() is not None, "oracle/_ref (the reference's compiled LINPACK) is needed"
    mats = lh.test_matrices()
    width = max(min(A.shape[0] + 1, A.shape[1]) for A in mats)
    out = dict(shape=np.array([A.shape for A in mats], np.int32), info=np.zeros(len(mats), np.int32),
               s=np.zeros((len(mats), width), np.float32), e=np.zeros((len(mats), width), np.float32),
               u_crc=np.zeros(len(mats), np.uint32), v_crc=np.zeros(len(mats), np.uint32))
    full = []
    for i, A in enumerate(mats):
        sr, er, u, v, out["info"][i] = lf.ref_csvdc_full(orc, A)
        out["s"][i, :len(sr)], out["e"][i, :len(er)] = sr, er
        out["u_crc"][i], out["v_crc"][i] = zlib.crc32(colmajor_bytes(u)), zlib.crc32(colmajor_bytes(v))
        if max(A.shape) <= FULL_MAX:
            full.append(i)
            out["u_%d" % i], out["v_%d" % i] = np.ascontiguousarray(u), np.ascontiguousarray(v)
    out["full"] = np.array(full, np.int32)
    np.savez_compressed(os.path.join(HERE, "csvdc_full_test_matrices.npz"), **out)


if __name__ == "__main__":
    main()
