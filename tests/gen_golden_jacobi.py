#!/usr/bin/env python3
"""Generate tests/golden/jacobi_exact.npz: the singular values of the `jacobi_cases.EXACT_CASES` (at most 96 rows), rounded
to float64 from a 60-digit mpmath evaluation, and numpy's own worst error against them.  CPU only:

    python tests/gen_golden_jacobi.py            # write the file
    python tests/gen_golden_jacobi.py --check    # recompute and compare with the committed file, bit by bit

Route: the entries of A are binary fractions, so the Gram matrix A A^H over the Gram columns is formed EXACTLY in Python
integers (every entry scaled by one power of two); mpmath's Hermitian eigensolver at 60 digits then resolves eigenvalues
down to 1e-60 sigma_0^2, thirty decades below the smallest singular value of any case; s = sqrt(max(lambda, 0)).
Self-check before anything is written: numpy.linalg.svd of the same matrix agrees to 1e-14 sigma_0 on every case.

Layout: keys (n) the `case_key` of every case (the generator's arguments, nothing else is needed to rebuild the input),
off (n + 1) offsets into s_ref (float64, descending, min(rows, Gram columns) values per case), e_case (n) numpy's
max |s_numpy - s_ref| / sigma_0 per case, e_ref their maximum — the yardstick of condition e in `check_rows_result`.
TEST INFRASTRUCTURE — never imported by the product."""
import multiprocessing
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mpmath as mp  # noqa: E402

import jacobi_cases as jc  # noqa: E402

OUT = jc.GOLDEN
DIGITS = 60


def exact_gram(X):
    """X X^H of a complex128 matrix as exact integers: (re, im, shift) with X X^H = (re + i im) / 4^shift."""
    parts = []
    shift = 0
    for P in (X.real, X.imag):
        ratios = [[float(v).as_integer_ratio() for v in row] for row in P]
        shift = max([shift] + [d.bit_length() - 1 for row in ratios for _, d in row])
        parts.append(ratios)
    re, im = [np.array([[n << (shift - (d.bit_length() - 1)) for n, d in row] for row in ratios], dtype=object)
              for ratios in parts]
    return re @ re.T + im @ im.T, im @ re.T - re @ im.T, shift


def exact_singular_values(X):
    mp.mp.dps = DIGITS
    n, k = X.shape[0], min(X.shape)
    if k == 0:
        return np.zeros(0)
    gre, gim, shift = exact_gram(X)
    scale = mp.mpf(2) ** (-2 * shift)
    G = mp.matrix(n, n)
    for i in range(n):
        for j in range(n):
            G[i, j] = mp.mpc(mp.mpf(int(gre[i, j])) * scale, mp.mpf(int(gim[i, j])) * scale)
    ev = mp.eigh(G, eigvals_only=True)
    s = sorted((mp.sqrt(max(ev[i], mp.mpf(0))) for i in range(n)), reverse=True)
    return np.array([float(v) for v in s[:k]], dtype=np.float64)


def one_case(case):
    family, args, gc0, gc1 = case
    t0 = time.time()
    X = jc.make(family, args)[:, gc0:gc1]
    s = exact_singular_values(X)
    s_np = np.linalg.svd(X, compute_uv=False)
    e = float(np.abs(s_np - s).max() / s[0])
    assert e < 1e-14, ("numpy and the exact spectrum disagree", case, e)
    assert (np.diff(s) <= 0).all()
    return jc.case_key(*case), s, e, time.time() - t0


def generate():
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(one_case, jc.EXACT_CASES, chunksize=1)
    for key, s, e, dt in res:
        print("%-44s %3d values, numpy off by %.2e sigma_0, %.1f s" % (key, s.size, e, dt), flush=True)
    n = np.array([r[1].size for r in res], dtype=np.int64)
    e_case = np.array([r[2] for r in res])
    return dict(keys=np.array([r[0] for r in res]), off=np.concatenate([[0], np.cumsum(n)]),
                s_ref=np.concatenate([r[1] for r in res]), e_case=e_case, e_ref=e_case.max())


def main():
    t0 = time.time()
    d = generate()
    print("e_ref = %.3e" % d["e_ref"])
    if "--check" in sys.argv[1:]:
        g = np.load(OUT)
        for k, v in d.items():
            assert np.asarray(v).dtype == g[k].dtype and np.asarray(v).tobytes() == g[k].tobytes(), k
        print(os.path.basename(OUT), "reproduced bit for bit")
    else:
        np.savez_compressed(OUT, **d)
        print(os.path.basename(OUT), os.path.getsize(OUT), "bytes,", len(d["keys"]), "cases")
    print("%.0f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
