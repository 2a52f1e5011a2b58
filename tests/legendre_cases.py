"""The exact Legendre fixture (tests/golden/legendre_exact*.npz, written by tests/gen_golden_legendre.py) for
test_host_legendre.py and test_gpu_sht_exact.py: loader, the measured base figures and the bounds that follow.

BASE[lmax] is the worst absolute error, over lambda, W and X and every l, of the float64 recurrence
`oracle.btgen.lambda_lm` / `wx_lm` against the fixture on the columns of that lmax whose seed exp(logpre + m ln sin theta)
is a normal double (for lmax 2047 those are the belt-ring columns; for lmax 3071 and 6143 the column of the largest m
below the underflowing one whose seed is still normal, on the same ring).  Measured on the CPU with
`python tests/legendre_cases.py`, which prints them; the figures below are those, rounded up to two digits.  The
recurrence is unchanged on these columns by the underflow fix, so the figures are the parent commit's.
BOUND[lmax] = 8 x BASE[lmax] holds host and device to the fixture, on the normalised quantities (coefficients divided
by w nphi, maps as they are); 8 is DESIGN.md 4.3's allowance for another summation order and FMA contraction.  The
underflow columns have no allowance of their own: they are held to the bound of their lmax.
TEST INFRASTRUCTURE — never imported by the product."""
import os

import numpy as np

FILES = ("legendre_exact.npz", "legendre_exact_underflow.npz")

# measured: 4.72e-16, 5.00e-16, 9.55e-15, 9.55e-15, 2.24e-13, 6.12e-11, 6.73e-14, 3.99e-13, 4.64e-13
BASE = {5: 4.8e-16, 11: 5.0e-16, 23: 9.6e-15, 35: 9.6e-15, 95: 2.3e-13, 1024: 6.2e-11, 2047: 6.8e-14, 3071: 4.0e-13,
        6143: 4.7e-13}
BOUND = {lmax: 8.0 * v for lmax, v in BASE.items()}


class Exact(object):
    """Columns of the fixture by (nside, lmax, m, ring); southern rings come from their stored mirrors."""

    def __init__(self, golden_dir):
        self.files = [np.load(os.path.join(golden_dir, f)) for f in FILES]
        self.index = {}
        self.asked = []                                   # every column the cases ask for, southern ones included
        for fi, f in enumerate(self.files):
            for ci, key in enumerate(map(tuple, f["cols"].tolist())):
                self.index[key] = (fi, ci)
                self.asked.append(key)
            self.asked += list(map(tuple, f["south"].tolist()))
        self.tabs = [dict(off=f["off"], lam=f["lam"], W=f["W"], X=f["X"]) for f in self.files]

    def has(self, nside, lmax, m, ring):
        return (nside, lmax, m, min(ring, 4 * nside - 2 - ring)) in self.index

    def column(self, nside, lmax, m, ring):
        """(lambda, W, X), each (lmax + 1 - m,), for l = m .. lmax on the ring."""
        north = min(ring, 4 * nside - 2 - ring)
        fi, ci = self.index[(nside, lmax, m, north)]
        t = self.tabs[fi]
        a, b = int(t["off"][ci]), int(t["off"][ci + 1])
        lam, W, X = t["lam"][a:b], t["W"][a:b], t["X"][a:b]
        if ring != north:   # lambda_lm(-z) = (-1)^(l+m) lambda_lm(z); W alike; X with one more sign
            par = 1.0 - 2.0 * ((np.arange(b - a)) % 2)
            lam, W, X = par * lam, par * W, -par * X
        return lam, W, X

    def groups(self):
        """{(nside, lmax): sorted [(m, ring)]} of the columns asked for."""
        out = {}
        for nside, lmax, m, ring in self.asked:
            out.setdefault((nside, lmax), []).append((m, ring))
        return {k: sorted(v) for k, v in out.items()}


def seed_is_normal(nside, m, ring):
    """Whether the seed of the float64 recurrence, exp(logpre + m ln sin theta), is a normal double on the ring."""
    from driftscan_amd import healpix

    z = healpix.ring_z(nside)[ring]
    if m == 0:
        return True
    k = np.arange(1, m + 1)
    t = 0.5 * (np.log(2.0 * m + 1.0) - np.log(4.0 * np.pi)) + 0.5 * np.sum(np.log((2.0 * k - 1.0) / (2.0 * k)))
    t += m * np.log(np.sqrt((1.0 - z) * (1.0 + z)))
    return bool(np.exp(t) >= np.finfo(np.float64).tiny)


def worst_errors(fx, fns, keep):
    """{lmax: worst |fns - fixture| over lambda, W, X} on the columns of fx with keep(nside, m, ring); fns = (lambda_lm, wx_lm)."""
    from driftscan_amd import healpix

    lam_fn, wx_fn = fns
    out = {}
    for (nside, lmax), cols in sorted(fx.groups().items()):
        z = healpix.ring_z(nside)
        for m in sorted(set(c[0] for c in cols)):
            rings = np.array([r for mm, r in cols if mm == m and keep(nside, m, r)], dtype=np.int64)
            if not rings.size:
                continue
            lam = lam_fn(lmax, m, z[rings])
            W, X = wx_fn(lmax, m, z[rings])
            for j, r in enumerate(rings):
                el, eW, eX = fx.column(nside, lmax, m, int(r))
                err = max(np.abs(lam[:, j] - el).max(), np.abs(W[:, j] - eW).max(), np.abs(X[:, j] - eX).max())
                out[lmax] = max(out.get(lmax, 0.0), float(err))
    return out


if __name__ == "__main__":
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    from oracle import btgen as ob

    fx = Exact(os.path.join(root, "tests", "golden"))
    for lmax, e in sorted(worst_errors(fx, (ob.lambda_lm, ob.wx_lm), seed_is_normal).items()):
        print("lmax %5d  base %.3e  (BASE %.1e, bound %.1e)" % (lmax, e, BASE[lmax], BOUND[lmax]))
