#!/usr/bin/env python3
"""The Hestenes column of the table in DESIGN.md section 4.2 for the groups whose inputs are too large for the suite
(iv, vi, vii at 200 to 300 rows; iii at 2049 columns): the float64 reference solver of tests/jacobi_cases.py on the
inputs of tests/test_gpu_jacobi_rows.py, through the same `check_rows_result`.  CPU only, 30 to 100 s per case (one
process each):

    python tests/jacobi_reference_table.py

The reference always converges all rows, so it is held to the full contract (no drop_below, no subspace split); for the
subspace cases the two sides of its answer are compared with the spectrum as the GPU test compares the device's.
TEST INFRASTRUCTURE — never imported by the product, not part of the suite."""
import multiprocessing
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import jacobi_cases as jc  # noqa: E402

CASES = [("iv full rank", "smooth_deficient", (300, 320, 15, 300), None, None),
         ("iv rank 150", "smooth_deficient", (300, 320, 15, 150), None, None),
         ("vi", "smooth_deficient", (200, 240, 16, 200), None, None),
         ("vii cut 1e-10", "gapped", (300, 320, 1e-10, 2), None, (1e-10, 3.2e5)),
         ("vii cut 1e-4", "gapped", (300, 320, 1e-4, 2), None, (1e-4, 100.0)),
         ("iii 2049 columns", "graded", (40, 2009, 2, 2049), 64, None)]


def one(case):
    name, family, args, gc1, split = case
    A = jc.make(family, args)
    t0 = time.time()
    Zin, probs = jc.pack([dict(A=A, row0=1, ldx=1, gc1=gc1)])
    Zout, sig, sweeps = jc.simulate(Zin, probs)
    r = jc.check_rows_result(A, Zin, Zout, sig[0], probs[0], sweeps)
    line = "%-18s sweeps %2d  " % (name, sweeps) + "  ".join("%s %.3g" % (k, r[k]) for k in "abcde")
    if split:
        cut, margin = split
        s_np = np.linalg.svd(A, compute_uv=False)
        k = int((s_np > cut * s_np[0]).sum())
        YG = jc.region(Zout, probs[0])[:, :A.shape[1]]
        up, lo = np.linalg.svd(YG[:k], compute_uv=False), np.linalg.svd(YG[k:], compute_uv=False)
        line += "  split: upper %.3g, lower %.3g" % (np.abs(up - s_np[:k]).max() / (1e-12 * s_np[0]),
                                                     np.abs(lo - s_np[k:]).max() / ((1e-12 * margin * cut + 1e-16) * s_np[0]))
    return line + "  (%.0f s)" % (time.time() - t0)


if __name__ == "__main__":
    with multiprocessing.Pool(min(len(CASES), os.cpu_count() or 1)) as pool:
        for ln in pool.imap(one, CASES):
            print(ln, flush=True)
