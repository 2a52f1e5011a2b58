#!/usr/bin/env python3
"""Generate tests/golden/legendre_exact.npz and legendre_exact_underflow.npz: lambda_lm, W_lm, X_lm on HEALPix rings,
rounded to float64 from a 77-digit (256-bit) mpmath evaluation that shares nothing with the package's recurrence.  CPU only:

    python tests/gen_golden_legendre.py            # write both files
    python tests/gen_golden_legendre.py --check    # recompute and compare with the committed files, bit by bit

Route: the UNNORMALISED associated Legendre functions by their own upward recurrence from P_mm = (-1)^m (2m-1)!! sin^m,
    (l - m) P_lm = (2l - 1) z P_{l-1,m} - (l + m - 1) P_{l-2,m},
then lambda_lm = sqrt((2l + 1) / (4 pi) (l - m)! / (l + m)!) P_lm with the factorial ratio carried as an exact running
product.  mpmath numbers have an unbounded exponent: nothing underflows.  W and X are the HEALPix closed forms in
lambda_lm and lambda_{l-1,m} (Kamionkowski, Kosowsky & Stebbins 1997, eq. 2.25 for normalised functions), in mpmath.
z is `healpix.ring_z` taken as the exact binary number it is; 1 - z^2 is formed exactly.

Self-checks before anything is written: every value with l <= 40 against scipy.special.sph_harm_y, every W, X with
l <= 9 against the Goldberg closed form of the spin-weighted harmonics (tests/test_oracle_btgen.py::spin_ylm), and the
parity rule below against a direct evaluation on southern rings.

Layout of each file: cols (n, 4) = (nside, lmax, m, ring), off (n + 1) offsets into the flat float64 arrays lam, W, X
(l = m .. lmax per column).  Only rings down to the equator are stored: ring_z is exactly antisymmetric and
    lambda_lm(-z) = (-1)^(l+m) lambda_lm(z),  W_lm(-z) = (-1)^(l+m) W_lm(z),  X_lm(-z) = -(-1)^(l+m) X_lm(z)
hold bit for bit after rounding, so tests/legendre_cases.py serves the southern rings from their mirrors; `south`
(k, 4) lists the southern columns the cases ask for.  The columns of lmax >= 2047 are in the second file: a committed
file stays below 1 MB.
TEST INFRASTRUCTURE — never imported by the product."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import mpmath as mp  # noqa: E402

from driftscan_amd import healpix  # noqa: E402
from legendre_cases import seed_is_normal  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
FILES = ("legendre_exact.npz", "legendre_exact_underflow.npz")
mp.mp.prec = 256


def cases():
    """[(nside, lmax, [m], [ring])]: the columns of the fixture (0-based rings, north to south)."""
    out = []
    for nside, lmaxes in ((2, (5, 11)), (8, (23, 35))):                 # small, complete
        for lmax in lmaxes:
            out.append((nside, lmax, list(range(lmax + 1)), list(range(4 * nside - 1))))
    n = 32                                                              # medium
    # first ring, last north-cap ring, first belt ring, equator, mirror of the last cap ring, last ring
    out.append((n, 95, [0, 1, 2, 3, 31, 47, 94, 95], [0, n - 2, n - 1, 2 * n - 1, 4 * n - 2 - (n - 2), 4 * n - 2]))
    out.append((512, 1024, [0, 2, 300, 700] + list(range(1017, 1025)), [0, 5, 100, 511, 700, 1023, 2046]))   # production
    # underflow regime: a cap ring, its mirror, and a belt ring whose seed is a normal double
    out.append((1024, 2047, list(range(696, 704)), [438, 4094 - 438, 1500]))
    # host-only underflow rows, each with the largest m below it whose seed is still a normal double ON THE SAME RING: the
    # group's base figure.  (The error of the recurrence over thousands of oscillating steps depends on the ring — a few
    # 1e-13 next to the pole at lmax 6143 against 5e-15 in the belt — so only the same ring says what float64 can do there.)
    for nside, lmax, m, ring in ((1024, 3071, 360, 149), (2048, 6143, 304, 183)):
        mn = max(k for k in range(m) if seed_is_normal(nside, k, ring))
        out.append((nside, lmax, [mn, m], [ring]))
    return out


def exact_column(lmax, m, z):
    """(lambda, W, X) for l = m .. lmax at the float64 z, as lists of mpf."""
    zz = mp.mpf(float(z))
    s2 = 1 - zz * zz
    p1 = (-1) ** m * mp.fac2(2 * m - 1) * mp.sqrt(s2) ** m if m > 0 else mp.mpf(1)     # P_mm
    p2 = mp.mpf(0)
    n2 = mp.mpf(2 * m + 1) / (4 * mp.pi * mp.factorial(2 * m))                         # N_mm^2
    lam = [mp.sqrt(n2) * p1]
    for l in range(m + 1, lmax + 1):
        cur = ((2 * l - 1) * zz * p1 - (l + m - 1) * p2) / (l - m)
        n2 = n2 * mp.mpf(2 * l + 1) / (2 * l - 1) * (l - m) / (l + m)
        lam.append(mp.sqrt(n2) * cur)
        p2, p1 = p1, cur
    W, X = [], []
    for l in range(m, lmax + 1):
        if l < 2:
            W.append(mp.mpf(0))
            X.append(mp.mpf(0))
            continue
        ll = mp.mpf(l)
        nl = 2 * mp.sqrt(1 / ((ll - 1) * ll * (ll + 1) * (ll + 2)))
        a = lam[l - m]
        b = lam[l - m - 1] if l > m else mp.mpf(0)
        c = mp.sqrt((2 * ll + 1) / (2 * ll - 1) * (ll * ll - m * m))
        W.append(-nl * (-((ll - m * m) / s2 + ll * (ll - 1) / 2) * a + c * zz / s2 * b))
        X.append(nl * (m / s2) * ((ll - 1) * zz * a - c * b))
    return lam, W, X


def to_f64(v):
    return np.array([float(x) for x in v], dtype=np.float64)


def self_check(nside, lmax, m, ring, z, lam, W, X):
    """scipy for l <= 40, Goldberg for l <= 9 (float64 references: the bounds are theirs, 1e-12 and 1e-11 as in
    tests/test_oracle_btgen.py)."""
    import scipy.special as sp

    from test_oracle_btgen import spin_ylm

    th = np.arccos(np.array([z]))
    for l in range(m, min(lmax, 40) + 1):
        ref = sp.sph_harm_y(l, m, th, 0.0).real[0]
        assert abs(lam[l - m] - ref) < 1e-12 * max(1.0, abs(ref)), ("scipy", nside, lmax, m, ring, l, lam[l - m], ref)
    # Goldberg's sums of cot^k(theta / 2) lose digits next to the poles: keep to the rings the existing test's range covers
    if abs(z) <= 0.9:
        for l in range(max(m, 2), min(lmax, 9) + 1):
            fp = spin_ylm(2, l, m, th, np.zeros(1)).real[0]
            fm = spin_ylm(-2, l, m, th, np.zeros(1)).real[0]
            assert abs(W[l - m] + 0.5 * (fp + fm)) < 1e-11, ("goldberg W", nside, lmax, m, ring, l)
            assert abs(X[l - m] + 0.5 * (fp - fm)) < 1e-11, ("goldberg X", nside, lmax, m, ring, l)


def generate():
    files = [dict(cols=[], lam=[], W=[], X=[], south=[]) for _ in FILES]
    nchecked = 0
    for nside, lmax, ms, rings in cases():
        z = healpix.ring_z(nside)
        nring = 4 * nside - 1
        assert np.array_equal(z, -z[::-1])                   # exact antisymmetry: what the mirror rule rests on
        f = files[1 if lmax >= 2047 else 0]
        north = sorted(set(min(r, nring - 1 - r) for r in rings))
        for r in rings:
            if r > nring - 1 - r:
                f["south"] += [(nside, lmax, m, r) for m in ms]
        for m in ms:
            for r in north:
                lam, W, X = [to_f64(v) for v in exact_column(lmax, m, z[r])]
                self_check(nside, lmax, m, r, z[r], lam, W, X)
                f["cols"].append((nside, lmax, m, r))
                f["lam"].append(lam)
                f["W"].append(W)
                f["X"].append(X)
        # the mirror rule against a direct evaluation on the southern ring (a few columns per case)
        for m in sorted(set([ms[0], ms[len(ms) // 2], ms[-1]])):
            r = north[0]
            lam, W, X = [to_f64(v) for v in exact_column(lmax, m, z[r])]
            slam, sW, sX = [to_f64(v) for v in exact_column(lmax, m, z[nring - 1 - r])]
            par = (-1.0) ** (np.arange(m, lmax + 1) + m)
            assert np.array_equal(slam, par * lam) and np.array_equal(sW, par * W) and np.array_equal(sX, -par * X)
            nchecked += 1
        print("nside %d lmax %d: %d m x %d rings (%d stored)" % (nside, lmax, len(ms), len(rings), len(north)), flush=True)
    out = []
    for f in files:
        n = np.array([a.size for a in f["lam"]], dtype=np.int64)
        out.append(dict(cols=np.array(f["cols"], dtype=np.int32), off=np.concatenate([[0], np.cumsum(n)]),
                        lam=np.concatenate(f["lam"]), W=np.concatenate(f["W"]), X=np.concatenate(f["X"]),
                        south=np.array(f["south"], dtype=np.int32).reshape(-1, 4)))
    print("mirror rule verified directly on %d columns" % nchecked)
    return out


def main():
    out = generate()
    for name, d in zip(FILES, out):
        path = os.path.join(OUT, name)
        if "--check" in sys.argv[1:]:
            g = np.load(path)
            for k, v in d.items():
                assert v.dtype == g[k].dtype and v.tobytes() == g[k].tobytes(), (name, k)
            print(name, "reproduced bit for bit")
            continue
        np.savez_compressed(path, **d)
        size = os.path.getsize(path)
        print(name, size, "bytes,", d["cols"].shape[0], "columns,", d["lam"].size, "values per table")
        assert size < 1000000, "a committed fixture file must stay below 1 MB"


if __name__ == "__main__":
    main()
