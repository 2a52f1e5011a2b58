"""The host copies of the Legendre recurrence (healpix.lambda_lm / wx_lm and oracle.btgen.lambda_lm / wx_lm) against
exact values: every column of tests/golden/legendre_exact*.npz (50+ digit mpmath evaluation by another route,
tests/gen_golden_legendre.py), element by element, within BOUND[lmax] = 8 x the measured error of the float64
recurrence where nothing underflows (tests/legendre_cases.py).  The columns whose seed exp(m ln sin theta) is below the
smallest normal double — (nside 1024, lmax 2047, m 696..703, rings 438 and 3656), (1024, 3071, 360, 149) and
(2048, 6143, 304, 183) — were exact zeros before the seed was carried with its own exponent, against true values of
order one; they get the bound of their lmax like every other column."""
import numpy as np
import pytest

import legendre_cases as lc


@pytest.fixture(scope="module")
def fx(golden_dir):
    return lc.Exact(golden_dir)


def _fns(which):
    if which == "healpix":
        from driftscan_amd import healpix

        return healpix.lambda_lm, healpix.wx_lm
    from oracle import btgen as ob

    return ob.lambda_lm, ob.wx_lm


def test_fixture_holds_the_cases(fx):
    """The columns the cases name are there, the underflow columns are what they are said to be, and the largest
    true values on them are the ones the underflow was found with."""
    g = fx.groups()
    assert sorted(g) == [(2, 5), (2, 11), (8, 23), (8, 35), (32, 95), (512, 1024), (1024, 2047), (1024, 3071), (2048, 6143)]
    for nside, lmax in ((2, 5), (2, 11), (8, 23), (8, 35)):
        assert g[(nside, lmax)] == [(m, r) for m in range(lmax + 1) for r in range(4 * nside - 1)]
    assert g[(32, 95)] == [(m, r) for m in (0, 1, 2, 3, 31, 47, 94, 95) for r in (0, 30, 31, 63, 96, 126)]
    assert g[(512, 1024)] == [(m, r) for m in [0, 2, 300, 700] + list(range(1017, 1025)) for r in (0, 5, 100, 511, 700, 1023, 2046)]
    assert g[(1024, 2047)] == [(m, r) for m in range(696, 704) for r in (438, 1500, 3656)]
    for m in range(696, 704):
        assert not lc.seed_is_normal(1024, m, 438) and not lc.seed_is_normal(1024, m, 3656) and lc.seed_is_normal(1024, m, 1500)
    for nside, lmax, m, ring, peak in ((1024, 2047, 700, 438, 1.36), (1024, 3071, 360, 149, 2.09), (2048, 6143, 304, 183, 2.59)):
        assert not lc.seed_is_normal(nside, m, ring)
        assert abs(np.abs(fx.column(nside, lmax, m, ring)[0]).max() - peak) < 0.01
    for nside, lmax, ring in ((1024, 3071, 149), (2048, 6143, 183)):
        (mn, r0), (mu, r1) = g[(nside, lmax)]
        assert r0 == r1 == ring and lc.seed_is_normal(nside, mn, ring) and not lc.seed_is_normal(nside, mn + 1, ring)


@pytest.mark.parametrize("which", ["healpix", "oracle"])
@pytest.mark.parametrize("group", [(2, 5), (2, 11), (8, 23), (8, 35), (32, 95), (512, 1024), (1024, 2047), (1024, 3071),
                                   (2048, 6143)], ids=lambda g: "nside%d-lmax%d" % g)
def test_recurrence_vs_exact(fx, which, group):
    nside, lmax = group
    lam_fn, wx_fn = _fns(which)
    from driftscan_amd import healpix

    z = healpix.ring_z(nside)
    cols = fx.groups()[group]
    worst, where = {"lambda": 0.0, "W": 0.0, "X": 0.0}, {}
    for m in sorted(set(c[0] for c in cols)):
        rings = np.array([r for mm, r in cols if mm == m], dtype=np.int64)
        lam = lam_fn(lmax, m, z[rings])
        W, X = wx_fn(lmax, m, z[rings])
        assert lam.shape == W.shape == X.shape == (lmax + 1 - m, rings.size)
        for j, r in enumerate(rings):
            for name, got, ref in zip(("lambda", "W", "X"), (lam[:, j], W[:, j], X[:, j]), fx.column(nside, lmax, m, int(r))):
                assert np.isfinite(got).all(), (name, m, r)
                err = np.abs(got - ref)
                if err.max() > worst[name]:
                    worst[name], where[name] = float(err.max()), (m, int(r), m + int(err.argmax()))
    print("%s nside %d lmax %d: worst |error| %s at (m, ring, l) %s; bound %.2e" % (which, nside, lmax, worst, where, lc.BOUND[lmax]))
    assert max(worst.values()) <= lc.BOUND[lmax], (worst, where)


def test_plain_columns_keep_their_bits():
    """Where the seed is a normal double the recurrence is the plain one: a column next to an underflowing one (same m,
    another ring, in one call) has the bits it has when computed alone, and both host copies agree bit for bit."""
    from driftscan_amd import healpix
    from oracle import btgen as ob

    z = healpix.ring_z(1024)
    both = healpix.lambda_lm(2047, 700, z[[438, 1500]])
    alone = healpix.lambda_lm(2047, 700, z[[1500]])
    assert np.array_equal(both[:, 1], alone[:, 0])
    assert np.array_equal(both, ob.lambda_lm(2047, 700, z[[438, 1500]]))
    assert np.abs(both[:, 0]).max() > 1.0          # ... and the underflowing one is not zeros
    # sin(theta) = 0 keeps its zeros (m > 0 vanishes at the poles)
    assert not healpix.lambda_lm(40, 3, np.array([1.0, -1.0])).any()
