"""Inputs, the extended-precision restatement and the bound of the tests of a_lm evaluated at points (test_host_points.py,
test_gpu_points.py).

Per output element (s, f), the same for every polarisation, with eps = 2^-52, L = lmax + 1 and |a|_1 summed over the
polarisations of the case:

    bound = BOUND[lmax] sum_{l,m} fac_m |a_flm|_1 + 4 (2 L + 2) eps sum_{l,m} fac_m |a_flm|_1 max(|lambda|, |W|, |X|)_s(l, m)

The first term is the allowance of tests/legendre_cases.py for the float64 recurrence at that lmax on every coefficient,
the second that of the two nested sums (at most L terms each) with the rounding of the phase.  lmax only takes values of
that table.  The sums run over the m of the call.
TEST INFRASTRUCTURE — never imported by the product."""
import functools

import numpy as np

import legendre_cases as lc
import sources_cases as sc

EPS = 2.0 ** -52
LD = np.longdouble

NPTS = (1, 63, 64, 65, 257)
NF = (1, 3, 9)               # 9: more than one block of frequencies for both kernels (blocks of 8 and 4)
LMAX = (5, 11, 23, 95)
# (npts, nf, npol, lmax, ms): ms None = every m in order, else a tuple
CASES = [(n, nf, npol, lmax, None) for lmax in LMAX for n in NPTS for nf in NF for npol in (1, 4)]
CASES += [(65, 3, 4, 23, tuple(range(1, 24, 3))), (65, 3, 4, 23, tuple(range(23, -1, -1)))]


def case_id(c):
    n, nf, npol, lmax, ms = c
    tag = "" if ms is None else ("-desc" if ms[0] > ms[-1] else "-stride%d" % (ms[1] - ms[0]))
    return "n%d-f%d-p%d-l%d%s" % (n, nf, npol, lmax, tag)


@functools.lru_cache(maxsize=None)
def master_alm(lmax):
    """Random full coefficients (9, 4, L, L), zero above the diagonal, a_l0 real; a case takes [:nf, :npol] (npol = 1: T)."""
    rng = np.random.default_rng(77 + lmax)
    L = lmax + 1
    alm = (rng.standard_normal((9, 4, L, L)) + 1j * rng.standard_normal((9, 4, L, L))) * np.tril(np.ones((L, L)))
    alm[..., 0] = alm[..., 0].real
    alm.setflags(write=False)
    return alm


def points(npts, lmax):
    """(theta, phi) of `sources_cases.master_inputs`: random pixel centres of nside 8 with random phi offsets."""
    theta, phi, _ = sc.master_inputs(npts, lmax)
    return theta, phi


def terms_ld(alm, theta, phi, ms):
    """The formulas of `skysim.alm_at_points_host` in numpy.longdouble on the same float64 inputs: z = cos(theta), phi
    reduced to [0, 2 pi), the phase argument the float64 product m * phi.  alm (nf, 4, L, nm), column j holding ms[j].
    Per m: val (nm, nf, 4, npts) longdouble — the term fac_m Re(F_m e^{i m phi}) — and for the bound, with the |a| of T
    alone (index 0) and of all four polarisations (index 1): a1 (nm, 2, nf) = fac sum_l |a|_1 and
    at (nm, 2, nf, npts) = fac sum_l |a|_1 max(|lambda|, |W|, |X|)."""
    alm = np.asarray(alm)
    nf, npol, L, nm = alm.shape
    assert npol == 4 and len(ms) == nm
    lmax = L - 1
    z = np.cos(np.asarray(theta, dtype=np.float64))
    ph = np.mod(np.asarray(phi, dtype=np.float64), 2.0 * np.pi)
    ar, ai = alm.real.astype(LD), alm.imag.astype(LD)
    val = np.zeros((nm, nf, 4, z.size), dtype=LD)
    a1 = np.zeros((nm, 2, nf))
    at = np.zeros((nm, 2, nf, z.size))
    for j, m in enumerate(ms):
        lam, W, X = sc.lambda_wx_ld(lmax, m, z)
        arg = (m * ph).astype(LD)                                   # the float64 product, then extended precision
        c, s = np.cos(arg), np.sin(arg)
        r, i = ar[:, :, m:, j], ai[:, :, m:, j]
        Fr, Fi = np.zeros((nf, 4, z.size), dtype=LD), np.zeros((nf, 4, z.size), dtype=LD)
        for p in (0, 3):
            Fr[:, p], Fi[:, p] = r[:, p] @ lam, i[:, p] @ lam
        # Q = E W + i B X, U = B W - i E X
        Fr[:, 1], Fi[:, 1] = r[:, 1] @ W - i[:, 2] @ X, i[:, 1] @ W + r[:, 2] @ X
        Fr[:, 2], Fi[:, 2] = r[:, 2] @ W + i[:, 1] @ X, i[:, 2] @ W - r[:, 1] @ X
        fac = 1.0 if m == 0 else 2.0
        val[j] = LD(fac) * (Fr * c - Fi * s)
        tab = np.maximum(np.abs(lam), np.maximum(np.abs(W), np.abs(X))).astype(np.float64)      # (L - m, npts)
        ab = np.abs(alm[:, :, m:, j])                                                           # (nf, 4, L - m)
        for k, a in enumerate((ab[:, 0], ab.sum(axis=1))):
            a1[j, k] = fac * a.sum(axis=1)
            at[j, k] = fac * (a @ tab)
    return val, a1, at


def reference_of(terms, sel, npol, lmax):
    """(ref (npts, npol, nf) longdouble, bound (npts, nf)) of the columns `sel` of terms_ld's output."""
    val, a1, at = terms
    k = 0 if npol == 1 else 1
    pols = [0] if npol == 1 else [0, 1, 2, 3]
    ref = val[sel].sum(axis=0)[:, pols]                                                       # (nf, npol, npts)
    L = lmax + 1
    bnd = lc.BOUND[lmax] * a1[sel, k].sum(axis=0)[:, None] + 4.0 * (2 * L + 2) * EPS * at[sel, k].sum(axis=0)
    return ref.transpose(2, 1, 0), bnd.T


@functools.lru_cache(maxsize=None)
def master_terms(npts, lmax):
    """terms_ld of master_alm(lmax) at points(npts, lmax) for every m — computed once, read by every case of (npts, lmax)."""
    theta, phi = points(npts, lmax)
    out = terms_ld(master_alm(lmax), theta, phi, list(range(lmax + 1)))
    for a in out:
        a.setflags(write=False)
    return out


def case_reference(case):
    """(alm (nf, npol, L, nm), theta, phi, ms, ref (npts, npol, nf) longdouble, bound (npts, nf))."""
    npts, nf, npol, lmax, ms = case
    theta, phi = points(npts, lmax)
    ms = list(range(lmax + 1)) if ms is None else list(ms)
    val, a1, at = master_terms(npts, lmax)
    ref, bnd = reference_of((val[:, :nf], a1[:, :, :nf], at[:, :, :nf]), ms, npol, lmax)
    alm = np.ascontiguousarray(master_alm(lmax)[:nf, : (1 if npol == 1 else 4)][..., ms])
    return alm, theta, phi, ms, ref, bnd


def worst_ratio(got, ref, bnd):
    """max over elements of |got - ref| / bound, got and ref (npts, npol, nf), bound (npts, nf); a bound of 0 wants an exact 0."""
    err = np.abs(np.asarray(got).astype(LD) - ref).astype(np.float64)
    b = np.broadcast_to(bnd[:, None, :], err.shape)
    return float(np.max(np.where(b > 0.0, err / np.where(b > 0.0, b, 1.0), np.where(err > 0.0, np.inf, 0.0))))
