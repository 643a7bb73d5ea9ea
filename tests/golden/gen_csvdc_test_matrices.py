"""Golden data for tests/test_linpack_f32.py: what the REFERENCE's OWN compiled LINPACK csvdc (oracle/_ref, built in the dev
container) returns for the fixed matrix family tests/linpack_host.test_matrices(), with job = 11 (what pseudoinverse() calls)
and job = 0 (no vectors).  Stored -> tests/golden/csvdc_test_matrices.npz:
  shape  int32 [64][2]         (n, p) of each matrix, to catch a changed family
  info   int32 [64][2]         csvdc's INFO per matrix and job (11, 0)
  s, e   float32 [64][2][150]  the first m = min(n + 1, p) entries of s and e (real parts), zero beyond m
Only numbers are stored.

Run:  python tests/golden/gen_csvdc_test_matrices.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))


def main():
    from oracle import oracle as orc
    from tests import linpack_host as lh
    orc.build(ref=True)
    assert orc.ref_lib() is not None, "oracle/_ref (the reference's compiled LINPACK) is needed"
    mats = lh.test_matrices()
    width = max(min(A.shape[0] + 1, A.shape[1]) for A in mats)
    shape = np.array([A.shape for A in mats], np.int32)
    info = np.zeros((len(mats), 2), np.int32)
    s = np.zeros((len(mats), 2, width), np.float32)
    e = np.zeros((len(mats), 2, width), np.float32)
    for i, A in enumerate(mats):
        for j, job in enumerate((11, 0)):
            sr, er, info[i, j] = lh.ref_csvdc(orc, A, job)
            s[i, j, :len(sr)], e[i, j, :len(er)] = sr, er
    np.savez_compressed(os.path.join(HERE, "csvdc_test_matrices.npz"), shape=shape, info=info, s=s, e=e)


if __name__ == "__main__":
    main()
