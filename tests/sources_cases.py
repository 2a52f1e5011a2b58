"""Inputs, the extended-precision restatement and the bound of the point-source tests (test_host_sources.py,
test_gpu_sources.py).

bound(f, l, m) = BOUND[lmax] sum_s sum_k |F_fks| + 4 (nsrc + 2) eps sum_s |F_fs| max(|lambda|, |W|, |X|)_s(l, m), the same
for every polarisation, |F_fs| = sum_k |F_fks|: the first term is the allowance of tests/legendre_cases.py for the float64
recurrence at that lmax (8 x its measured error against the exact fixture) on every source, the second the usual bound
of a sum of nsrc products with the phases' own rounding.  lmax only takes values of that table.
TEST INFRASTRUCTURE — never imported by the product."""
import functools

import numpy as np

import legendre_cases as lc

EPS = 2.0 ** -52
LD = np.longdouble

NSRC = (1, 63, 64, 65, 1024, 1025)          # 1024 = skysim.SOURCE_CHUNK (asserted by the tests)
LMAX = (5, 11, 23, 95)
# (nsrc, nf, npol, lmax, mmax, m_range)
CASES = [(n, nf, npol, lmax, None, None) for lmax in LMAX for n in NSRC for nf in (1, 3) for npol in (1, 4)]
CASES += [(65, 3, 4, 23, 9, None), (65, 3, 4, 23, None, (5, 17))]


def case_id(c):
    n, nf, npol, lmax, mmax, mr = c
    return "n%d-f%d-p%d-l%d%s%s" % (n, nf, npol, lmax, "" if mmax is None else "-mmax%d" % mmax,
                                   "" if mr is None else "-m%d_%d" % mr)


@functools.lru_cache(maxsize=None)
def master_inputs(nsrc, lmax):
    """(theta, phi, flux (3, 4, nsrc)): random pixel centres of nside 8 with random phi offsets; a case of nf frequencies
    and npol polarisations takes flux[:nf, :npol]."""
    from driftscan_amd import healpix

    rng = np.random.default_rng(1000 * nsrc + lmax)
    ang = healpix.ang_positions(8)
    pix = rng.integers(0, ang.shape[0], size=nsrc)
    theta = ang[pix, 0].copy()
    phi = ang[pix, 1] + rng.uniform(-0.2, 0.2, size=nsrc)
    flux = rng.standard_normal((3, 4, nsrc))
    for a in (theta, phi, flux):
        a.setflags(write=False)
    return theta, phi, flux


def lambda_wx_ld(lmax, m, z):
    """lambda_lm, W_lm, X_lm (lmax + 1 - m, len(z)) by the recurrences of `healpix.lambda_lm` / `wx_lm` in numpy.longdouble
    (no underflow handling: for the small lmax of these tests)."""
    z = np.asarray(z, dtype=LD)
    one, two, four, half = LD(1), LD(2), LD(4), LD(0.5)
    s2 = (one - z) * (one + z)
    st = np.sqrt(s2)
    pi = LD(np.pi) + LD(1.2246467991473532e-16)              # pi to the precision of the type
    lam = np.zeros((lmax + 1 - m, z.size), dtype=LD)
    logpre = half * (np.log(two * m + one) - np.log(four * pi))
    for k in range(1, m + 1):
        logpre += half * np.log((two * k - one) / (two * k))
    lam[0] = ((-one) ** m) * np.exp(logpre + m * np.log(st)) if m > 0 else np.exp(logpre)
    if lmax > m:
        lam[1] = np.sqrt(two * m + LD(3)) * z * lam[0]
    for l in range(m + 2, lmax + 1):
        a = np.sqrt((four * l * l - one) / LD(l * l - m * m))
        b = np.sqrt(LD((l - 1) ** 2 - m * m) / (four * (l - 1) ** 2 - one))
        lam[l - m] = a * (z * lam[l - m - 1] - b * lam[l - m - 2])
    W, X = np.zeros_like(lam), np.zeros_like(lam)
    for l in range(max(m, 2), lmax + 1):
        nl = two * np.sqrt(one / LD((l - 1) * l * (l + 1) * (l + 2)))
        lam_l = lam[l - m]
        lam_lm1 = lam[l - m - 1] if l - 1 >= m else np.zeros_like(z)
        c = np.sqrt(LD(2 * l + 1) / LD(2 * l - 1) * LD(l * l - m * m))
        W[l - m] = -nl * (-(LD(l - m * m) / s2 + half * l * (l - 1)) * lam_l + c * z / s2 * lam_lm1)
        X[l - m] = nl * (LD(m) / s2) * (LD(l - 1) * z * lam_l - c * lam_lm1)
    return lam, W, X


def alm_ld(theta, phi, flux, lmax, m_lo, m_hi):
    """The formulas of `skysim.source_alm_host` in numpy.longdouble on the same float64 inputs: z = cos(theta), phi
    reduced to [0, 2 pi) and the phase argument the float64 product m * phi, as both routes define them.  flux
    (nf, 4, nsrc).  Returns (re, im) (nf, 4, L, nm) and tabmax (nsrc, L, nm) = max(|lambda|, |W|, |X|) per source."""
    z = np.cos(np.asarray(theta, dtype=np.float64))
    phi = np.mod(np.asarray(phi, dtype=np.float64), 2.0 * np.pi)
    flux = np.asarray(flux)
    nf, npol, nsrc = flux.shape
    assert npol == 4
    L, nm = lmax + 1, m_hi - m_lo + 1
    re, im = np.zeros((nf, 4, L, nm), dtype=LD), np.zeros((nf, 4, L, nm), dtype=LD)
    tabmax = np.zeros((nsrc, L, nm))
    F = flux.astype(LD)
    for m in range(m_lo, m_hi + 1):
        arg = (m * phi).astype(LD)                                  # the float64 product, then extended precision
        c, s = np.cos(arg), -np.sin(arg)
        lam, W, X = lambda_wx_ld(lmax, m, z)
        tabmax[:, m:, m - m_lo] = np.maximum(np.abs(lam), np.maximum(np.abs(W), np.abs(X))).T.astype(np.float64)
        fc, fs = F * c, F * s                                        # (nf, 4, nsrc): real and imaginary parts of F e^{-i m phi}
        k = m - m_lo
        for p in (0, 3):
            re[:, p, m:, k], im[:, p, m:, k] = fc[:, p] @ lam.T, fs[:, p] @ lam.T
        # E = W Q + i X U, B = W U - i X Q
        re[:, 1, m:, k], im[:, 1, m:, k] = fc[:, 1] @ W.T - fs[:, 2] @ X.T, fs[:, 1] @ W.T + fc[:, 2] @ X.T
        re[:, 2, m:, k], im[:, 2, m:, k] = fc[:, 2] @ W.T + fs[:, 1] @ X.T, fs[:, 2] @ W.T - fc[:, 1] @ X.T
    return re, im, tabmax


@functools.lru_cache(maxsize=None)
def master_reference(nsrc, lmax):
    """alm_ld of master_inputs(nsrc, lmax) for every m — computed once, read by every case of that (nsrc, lmax)."""
    theta, phi, flux = master_inputs(nsrc, lmax)
    re, im, tabmax = alm_ld(theta, phi, flux, lmax, 0, lmax)
    for a in (re, im, tabmax):
        a.setflags(write=False)
    return re, im, tabmax


def bound(flux, lmax, tabmax):
    """(nf, L, nm) from flux (nf, npol, nsrc) and tabmax (nsrc, L, nm)."""
    fabs = np.abs(flux).sum(axis=1)                                  # (nf, nsrc)
    nsrc = flux.shape[2]
    return lc.BOUND[lmax] * fabs.sum(axis=1)[:, None, None] + 4.0 * (nsrc + 2) * EPS * np.einsum("fs,slm->flm", fabs, tabmax)


def case_reference(case):
    """(theta, phi, flux (nf, npol, nsrc), m_lo, m_hi, re, im (nf, npol, L, nm) longdouble, bound (nf, L, nm))."""
    nsrc, nf, npol, lmax, mmax, mr = case
    theta, phi, fm = master_inputs(nsrc, lmax)
    re, im, tabmax = master_reference(nsrc, lmax)
    m_lo, m_hi = (0, lmax if mmax is None else mmax) if mr is None else mr
    pols = [0] if npol == 1 else [0, 1, 2, 3]
    flux = np.ascontiguousarray(fm[:nf][:, pols])
    sl = slice(m_lo, m_hi + 1)
    return (theta, phi, flux, m_lo, m_hi, re[:nf][:, pols][..., sl], im[:nf][:, pols][..., sl],
            bound(flux, lmax, tabmax[..., sl]))


def worst_ratio(got, re, im, bnd):
    """max over elements of max(|Re got - re|, |Im got - im|) / bound (a bound of 0 wants an exact 0)."""
    err = np.maximum(np.abs(got.real.astype(LD) - re), np.abs(got.imag.astype(LD) - im)).astype(np.float64)
    b = np.broadcast_to(bnd[:, None], err.shape)
    return float(np.max(np.where(b > 0.0, err / np.where(b > 0.0, b, 1.0), np.where(err > 0.0, np.inf, 0.0))))


# ---- maps with five pixels ------------------------------------------------------------------------------------------------
def five_pixels(nside):
    """Pixel indices in the north cap, the belt, on the equator, in the south cap and on the last ring."""
    from driftscan_amd import healpix

    nphi, _, start = healpix.ring_layout(nside)
    rings = [max(nside // 2 - 1, 0), nside + 1, 2 * nside - 1, 3 * nside + nside // 2, 4 * nside - 2]
    return np.array([int(start[r]) + (3 * i + 1) % int(nphi[r]) for i, r in enumerate(rings)], dtype=np.int64)


def five_pixel_map(nside, npol, seed):
    """(map (1, npol, npix), pixels, values (npol, 5))."""
    rng = np.random.default_rng(seed)
    pix = five_pixels(nside)
    val = rng.standard_normal((npol, 5))
    mp = np.zeros((1, npol, 12 * nside * nside))
    mp[0][:, pix] = val
    return mp, pix, val
