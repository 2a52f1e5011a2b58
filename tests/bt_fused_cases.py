"""Cases, inputs, reference and bound for the fused ring transform of beam-transfer generation (`dm_bt_columns` /
`dm_bt_columns_c`, dm_btgen.hip): test_host_bt_fused_cases.py checks the table and the reference on the CPU,
test_gpu_bt_fused.py holds the device to it.  TEST INFRASTRUCTURE — never imported by the product.

Cases.  `CASES` lists one call each: nside, P (1 or 4 Stokes maps), real or complex field patterns, the zenith, the
columns, the band limit and the m-range, and the kernels `dm_bt_ring_plan_info` has to name for it: `fft` = pixels per
thread of the belt FFT (None: no FFT) and `dft` = (dft2, P, NMG, NCG) of the matrix-form row.  Cases that differ in the
m-range only share a `Problem` (inputs, reference, bound), remembered in `problem()`.

Inputs.  Three beams, smooth in the pixel direction n: a narrow and a wide Gaussian about the zenith times 1 + a n.d,
zero below the horizon, the two polarisation components with different widths and gradients; the complex patterns carry
a phase exp(i k n.e) that differs per beam and component, so b_i conj(b_j) is not b_i b_j.  Column c pairs the beams as
PAIRS[c mod 9] = (0,0), (0,1), (1,2), (2,1), ... and has uv = 0 for c = 0, else 2 pi |uv| <= 0.98 lmax.  No pixel may lie
within 1e-9 of the horizon (`Problem.horizon_margin`): the device asks n.z > 0, the oracle signbit(-n.z).

Reference.  The oracle's map expressions (`oracle.btgen.fringe`, `horizon`, `construct_pol_real` / `construct_pol_complex`,
for one map the product of telescope.py:1156-1176) with the solid angles summed over the whole sphere, then the ring
sums and Legendre sums of `oracle.btgen.transfer_single(..., fft=True)` and the fold of `fold_to_m`, evaluated in slabs
of rings that share a pixel count (maps of a slab, its ring sums, then the Legendre products of all rings): the maps of
four Stokes parameters at nside 1024 never exist as a whole.  test_host_bt_fused_cases.py holds this slab evaluation to
the oracle's own functions called on whole maps.

Bound, per element (m, slot, column, p, l), on the real and on the imaginary part, derived — not a fraction of a scale.
With S_p(r) = sum_j |map_p(r, j)|, w = 4 pi / npix and rw the ring weights,

    A_T = w sum_r rw_r |lambda_lm(z_r)| S_T(r),   A_V likewise with S_V,
    A_Q = w sum_r rw_r (|W_lm| S_Q + |X_lm| S_U), A_U = w sum_r rw_r (|W_lm| S_U + |X_lm| S_Q),
    bound = c A + d_tab w sum_r rw_r S + e A',    S = S_T | S_Q + S_U | S_U + S_Q | S_V,
    c = (max nphi + nring + 64) 2^-53 + 2e-14,    d_tab = legendre_cases.BOUND[lmax],    e = 8 x 2^-53.

(max nphi + nring) 2^-53 are the recursive-summation bounds of the ring sum and of the Legendre sum (any order of
summation), 64 x 2^-53 the roundings of the map value, the twiddle and the products; 2e-14 is the kernels' statement
about their twiddle rotation (drift below 1e-14 between two exact seeds), doubled for the seed; d_tab is the allowance
of the device's Legendre tables against the exact functions, which is why lmax is a key of that table (23, 35).
e A' is the rounding of the Stokes combinations themselves, which |map| does not bound where they cancel: A' is A with
S_p replaced by S'_p(r) = sum_j |tc| (|b_i0| |b_j0| + |b_i1| |b_j1|) for I and Q, |tc| (|b_i0| |b_j1| + |b_i1| |b_j0|) for U
and V, the moduli of the two terms, and e counts the roundings of the two (complex) products and their sum or
difference.  V of a real beam with itself is a0 b1 - a1 b0 = 0 in the oracle's arithmetic, while a kernel whose compiler
contracts it to fma(a0, b1, -(a1 b0)) keeps the rounding error of one product, 1e-17 of the other maps: found on the
device (the term was missing: bound 0 there), legitimate, and all this term admits.  With one map A' = A.
Elements that must be exact zeros (l < m, l > col_lmax, slot 1 of m = 0) have reference 0 and bound 0.
"""
import functools
import math
import time

import numpy as np

import legendre_cases as lc
from oracle import btgen as ob

ZENITHS = {"N": (np.pi / 2 - np.radians(49.3), 0.0), "S": (np.pi / 2 + np.radians(37.1), 0.7)}
PAIRS = ((0, 0), (0, 1), (1, 2), (2, 1), (2, 2), (1, 0), (0, 2), (1, 1), (2, 0))
NBEAM = 3
HORIZON_MIN = 1e-9
SLAB_ELEMS = 1 << 20          # (pixels x columns x P) of one slab of rings

# beam b, component k: exp(-(1 - mu) / S_NARROW) + WIDE_AMP exp(-(1 - mu) / S_WIDE), times GAIN (1 + GRAD n.d),
# times exp(i KPH n.e) for the complex patterns; mu = n.zenith, d and e fixed combinations of East, North and up
S_NARROW = ((0.006, 0.009), (0.008, 0.005), (0.004, 0.007))
S_WIDE = ((0.45, 0.6), (0.5, 0.4), (0.65, 0.55))
WIDE_AMP = ((0.30, 0.22), (0.25, 0.35), (0.28, 0.18))
GAIN = ((1.0, 0.7), (0.9, -0.8), (-0.6, 1.1))
GRAD = ((0.4, -0.3), (-0.35, 0.45), (0.25, 0.3))
GDIR = (((1.0, 0.3, 0.0), (0.2, -1.0, 0.1)), ((-0.4, 1.0, 0.0), (1.0, 0.5, -0.2)), ((0.7, 0.7, 0.1), (-1.0, 0.2, 0.0)))
KPH = ((1.3, -0.9), (-1.7, 0.8), (0.6, 2.1))
PDIR = (((0.8, -0.5, 0.2), (0.1, 1.0, 0.0)), ((-0.3, 0.9, 0.1), (1.0, 0.2, -0.3)), ((0.5, 0.5, 0.5), (-0.9, 0.4, 0.0)))


# ---- the case table ---------------------------------------------------------------------------------------------------
# matrix-form row by (P, m-range): wide calls (more than 8 m-values) and nmg = ceil(cnt / 2) >= 3 (P = 4) / >= 5 (P = 1)
# take the shared-synthesis kernels
DFT_ROW = {
    (4, (0, 23)): (True, 4, 2, 1), (4, (5, 23)): (True, 4, 2, 1), (4, (3, 22)): (True, 4, 2, 1), (4, (8, 15)): (True, 4, 2, 1),
    (4, (9, 12)): (False, 4, 2, 2), (4, (20, 21)): (False, 4, 1, 4), (4, (23, 23)): (False, 4, 1, 4),
    (4, (0, 35)): (True, 4, 2, 1),
    (1, (0, 23)): (True, 1, 2, 4), (1, (5, 23)): (True, 1, 2, 4), (1, (3, 22)): (True, 1, 2, 4), (1, (8, 15)): (False, 1, 4, 4),
    (1, (9, 12)): (False, 1, 4, 4), (1, (20, 21)): (False, 1, 1, 8), (1, (23, 23)): (False, 1, 1, 8),
}
WIDE = {(0, 23), (5, 23), (3, 22), (0, 35)}
# pixels per thread of the belt FFT of a wide call; at nside 1024 four maps exceed the LDS: no FFT there
FFT_NPT = {(1, 2): 1, (1, 4): 1, (1, 8): 1, (1, 16): 1, (1, 32): 1, (1, 64): 1, (1, 128): 2, (1, 256): 4, (1, 512): 8, (1, 1024): 16,
           (4, 2): 1, (4, 4): 1, (4, 8): 1, (4, 16): 1, (4, 32): 1, (4, 64): 1, (4, 128): 2, (4, 256): 4, (4, 512): 8}
LONG_RANGES = ((0, 23), (5, 23), (8, 15), (9, 12), (20, 21), (23, 23))


def _case(group, nside, P, cplx, ncol, rng, zen="N", lmax=23, lside=25, scatter=False, ringw=False):
    name = "%s-n%d-P%d-%s%s-c%d-m%d_%d" % (group, nside, P, "c" if cplx else "r", "" if zen == "N" else "-S", ncol, rng[0], rng[1])
    fft = FFT_NPT.get((P, nside)) if rng in WIDE else None
    return dict(name=name, group=group, nside=nside, P=P, cplx=cplx, ncol=ncol, m_range=rng, zen=zen, lmax=lmax, lside=lside,
                scatter=scatter, ringw=ringw, fft=fft, dft=DFT_ROW[(P, rng)])


def _cases():
    out = []
    for nside in (64, 128, 256, 512):
        for P in (1, 4):
            for cplx in (False, True):
                out += [_case("long", nside, P, cplx, 3 if nside == 512 else 5, r) for r in LONG_RANGES]
    for P in (1, 4):
        out += [_case("south", 128, P, False, 5, r, zen="S") for r in ((0, 23), (8, 15))]
    out += [_case("full", 1024, 1, False, 2, r) for r in ((0, 23), (8, 15))]
    out += [_case("full", 1024, 1, True, 2, (0, 23))]          # (the one input that selects fft<1,16> for complex patterns)
    out += [_case("full", 1024, 4, False, 2, (0, 23))]
    for nside in (2, 4, 8, 16, 32):
        for P in (1, 4):
            out += [_case("depth", nside, P, False, 17, r) for r in ((0, 23), (3, 22))]
    for ncol in (1, 16, 17, 130, 520):
        for P in (1, 4):
            out += [_case("ragged", 4, P, False, ncol, r) for r in ((0, 23), (8, 15), (9, 12), (20, 21))]
    for P in (1, 4):
        out += [_case("scatter", 8, P, False, 7, r, scatter=True) for r in ((0, 23), (8, 15))]
    for nside in (8, 128):
        out += [_case("ringw", nside, 4, False, 5, r, ringw=True) for r in ((0, 23), (8, 15))]
    for P in (1, 4):
        for cplx in (False, True):
            out += [_case("belt", 48, P, cplx, 5, (0, 23))]
    out += [_case("lmax35", 128, 4, True, 5, (0, 35), lmax=35, lside=37)]
    return out


CASES = _cases()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
# (f, b) rows and band limits of the scatter cases: a gap (b = 2 of f = 0), an out-of-order pair (b = 5, 4): B = ncol + 3
SCATTER_F = (0, 0, 0, 1, 1, 1, 1)
SCATTER_B = (0, 1, 3, 5, 4, 6, 7)
SCATTER_LMAX = (23, 10, 0, 23, 17, 5, 23)


def layout(case):
    """(F, B, col_f, col_b, col_lmax) of a case."""
    n = case["ncol"]
    if case["scatter"]:
        return 2, n + 3, np.array(SCATTER_F), np.array(SCATTER_B), np.array(SCATTER_LMAX)
    return 1, n, np.zeros(n, dtype=np.int64), np.arange(n), np.full(n, case["lmax"], dtype=np.int64)


def pkey(case):
    return (case["nside"], case["P"], case["cplx"], case["zen"], case["ncol"], case["lmax"], case["ringw"], case["scatter"])


def columns(ncol, lmax):
    """(uv (ncol, 2), bi, bj): uv = 0 for column 0, else |uv| = f lmax / (2 pi) with f in [0.15, 0.98]."""
    c = np.arange(ncol)
    f = np.where(c == 0, 0.0, 0.15 + 0.83 * ((c * 0.381966) % 1.0))
    ang = 2.4 * c + 0.3
    uv = (f * lmax / (2.0 * np.pi))[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=-1)
    assert (2.0 * np.pi * np.hypot(uv[:, 0], uv[:, 1]) <= lmax).all()
    pr = np.array([PAIRS[i % len(PAIRS)] for i in c])
    return uv, pr[:, 0].copy(), pr[:, 1].copy()


def ring_weights(nside):
    return 1.0 + 1e-3 * np.random.default_rng(1000 + nside).random(4 * nside - 1)


def c_const(nside):
    return (4 * nside + 4 * nside - 1 + 64) * 2.0 ** -53 + 2e-14


# ---- inputs -------------------------------------------------------------------------------------------------------------
def slabs(nside, width):
    """Lists of rings that share a pixel count, at most SLAB_ELEMS / width pixels each (one ring at least)."""
    nphi = ob.ring_info(nside)[1]
    nring = nphi.size
    out = []
    for i in range(nside - 1):                       # a cap ring and its mirror
        out.append([i, nring - 1 - i])
    per = max(1, SLAB_ELEMS // (width * 4 * nside))
    belt = list(range(nside - 1, 3 * nside))
    out += [belt[i : i + per] for i in range(0, len(belt), per)]
    assert sorted(r for s in out for r in s) == list(range(nring))
    return out


def slab_angpos(nside, rings):
    """(k n, 2) pixel centres (theta, phi) of the rings, as `oracle.btgen.ang_positions`."""
    z, nphi, phi0, _ = ob.ring_info(nside)
    n = int(nphi[rings[0]])
    ap = np.empty((len(rings), n, 2))
    for i, r in enumerate(rings):
        ap[i, :, 0] = np.arccos(z[r])
        ap[i, :, 1] = phi0[r] + 2.0 * np.pi * np.arange(n) / n
    return ap.reshape(-1, 2)


def patterns(angpos, frame, P, cplx):
    """(NBEAM, npx, ncomp) field patterns on the given pixel centres, zero below the horizon (as the beams of the
    package: the solid angles are plain sums of |b|^2); also n.zenith."""
    n = ob.sph_to_cart(angpos)
    xh, yh, zh = frame[0:3], frame[3:6], frame[6:9]
    mu = n @ zh
    e, no = n @ xh, n @ yh
    hz = (mu > 0.0).astype(np.float64)
    ncomp = 2 if P == 4 else 1
    out = np.empty((NBEAM, n.shape[0], ncomp), dtype=np.complex128 if cplx else np.float64)
    for b in range(NBEAM):
        for k in range(ncomp):
            g = np.exp(-(1.0 - mu) / S_NARROW[b][k]) + WIDE_AMP[b][k] * np.exp(-(1.0 - mu) / S_WIDE[b][k])
            d = GDIR[b][k]
            v = hz * GAIN[b][k] * g * (1.0 + GRAD[b][k] * (d[0] * e + d[1] * no + d[2] * mu))
            if cplx:
                q = PDIR[b][k]
                ph = KPH[b][k] * (q[0] * e + q[1] * no + q[2] * mu)
                v = v * (np.cos(ph) + 1j * np.sin(ph))
            out[b, :, k] = v
    return out, mu


def stokes_maps(bi, bj, tc, P, cplx):
    """(P, npx) map values from the patterns of the two feeds (npx, ncomp) and tc = fringe horizon / sqrt(O_i O_j): the
    expressions of `oracle.btgen.construct_pol_real` / `construct_pol_complex` and, for one map, of `beam_transfer_m`."""
    cj = bj.conj() if cplx else bj
    if P == 1:
        return (tc * bi[:, 0] * cj[:, 0])[None]
    out = np.empty((4, bi.shape[0]), dtype=np.complex128)
    out[0] = tc * (bi[:, 0] * cj[:, 0] + bi[:, 1] * cj[:, 1])
    out[1] = tc * (bi[:, 0] * cj[:, 0] - bi[:, 1] * cj[:, 1])
    out[2] = tc * (bi[:, 0] * cj[:, 1] + bi[:, 1] * cj[:, 0])
    out[3] = 1j * tc * (bi[:, 0] * cj[:, 1] - bi[:, 1] * cj[:, 0])
    return out


def stokes_moduli(bi, bj, atc, P):
    """(P, npx) sums of the moduli of the terms of `stokes_maps` (atc = |tc|): what the roundings of a map value scale with."""
    ai, aj = np.abs(bi), np.abs(bj)
    if P == 1:
        return (atc * ai[:, 0] * aj[:, 0])[None]
    d = atc * (ai[:, 0] * aj[:, 0] + ai[:, 1] * aj[:, 1])
    x = atc * (ai[:, 0] * aj[:, 1] + ai[:, 1] * aj[:, 0])
    return np.stack([d, d, x, x])


E_TERMS = 8.0 * 2.0 ** -53
# mistakes a kernel could make, restated on the reference (Problem.ring_sums(mutant=...)): test_host_bt_fused_cases.py shows
# that each one leaves the bound on a named case.  lastpixel: the last pixel of every belt ring is lost; wrap: the output
# phase exp(i m phi0) of a belt ring is formed from m mod N (seen only where m reaches N: nside 2 and 4); ringw: a belt ring takes the weight of the ring above; conj: the second
# complex pattern is not conjugated; vsign: V with the other sign
MUTANTS = ("lastpixel", "wrap", "ringw", "conj", "vsign")


def _rmat(tab, v):
    """real (a, nring) @ complex (nring, k) as one real product."""
    v = np.ascontiguousarray(v)
    return (tab @ v.view(np.float64).reshape(v.shape[0], -1)).view(np.complex128)


class Problem(object):
    """Inputs, reference and bound of the cases that share everything but the m-range.

    beams (NBEAM, npix[, 2]) float64 or complex128; uv, bi, bj; frame (9); ring_w or None; F, B, col_f, col_b, col_lmax;
    G (2, lmax + 1, nring, ncol, P): ring sums sum_j f_j exp(i m phi_j) for +m, and conj of those of -m; S (nring, ncol, P);
    ref (lmax + 1, 2, ncol, P, lside + 1), bound and A (lmax + 1, ncol, P, lside + 1) for m = 0 .. lmax; seconds."""

    def __init__(self, case):
        t0 = time.time()
        nside, P, cplx, lmax = case["nside"], case["P"], case["cplx"], case["lmax"]
        self.case = dict(case)
        self.nside, self.P, self.cplx, self.lmax, self.lside, self.ncol = nside, P, cplx, lmax, case["lside"], case["ncol"]
        self.zenith = np.array(ZENITHS[case["zen"]])
        from driftscan_amd import btgen

        self.frame = btgen.telescope_frame(self.zenith)
        self.uv, self.bi, self.bj = columns(self.ncol, lmax)
        self.ring_w = ring_weights(nside) if case["ringw"] else None
        self.F, self.B, self.col_f, self.col_b, self.col_lmax = layout(case)
        z, nphi, phi0, start = ob.ring_info(nside)
        self.z, self.nphi, self.phi0, self.start = z, nphi, phi0, start
        nring, npix, ncol = z.size, 12 * nside * nside, self.ncol
        ncomp = 2 if P == 4 else 1
        self.slabs = slabs(nside, ncol * P)
        # pass 1: the patterns, their solid angles, the distance of the nearest pixel to the horizon
        beams = np.empty((NBEAM, npix, ncomp), dtype=np.complex128 if cplx else np.float64)
        part = [[] for _ in range(NBEAM)]
        margin = np.inf
        for rings in self.slabs:
            n = int(nphi[rings[0]])
            bs, mu = patterns(slab_angpos(nside, rings), self.frame, P, cplx)
            margin = min(margin, float(np.abs(mu).min()))
            for i, r in enumerate(rings):
                beams[:, start[r] : start[r] + n] = bs[:, i * n : (i + 1) * n]
            for b in range(NBEAM):
                part[b].append(float(np.sum(np.abs(bs[b]) ** 2)))
        self.horizon_margin = margin
        self.omega = np.array([math.fsum(p) for p in part]) * (4.0 * np.pi / npix)
        self.beams = beams if P == 4 else beams[:, :, 0]
        # pass 2: maps of a slab, their ring sums (one FFT per ring, as ring_dft_fft) and absolute sums
        self.G, self.S, self.S2 = self.ring_sums()
        self._legendre()
        self.seconds = time.time() - t0

    def ring_sums(self, mutant=None):
        """G (2, lmax + 1, nring, ncol, P), S and S' (nring, ncol, P) of all rings; `mutant` names a mistake (MUTANTS)."""
        lmax, ncol, P, nside = self.lmax, self.ncol, self.P, self.nside
        nring, phi0 = self.z.size, self.phi0
        ms = np.arange(lmax + 1)
        G = np.zeros((2, lmax + 1, nring, ncol, P), dtype=np.complex128)
        S = np.zeros((nring, ncol, P))
        S2 = np.zeros((nring, ncol, P))
        for rings in self.slabs:
            mp, mod = self.slab_maps(rings, moduli=True, mutant=mutant)       # (ncol, P, k, n)
            n = mp.shape[-1]
            if mutant == "lastpixel" and n == 4 * nside:
                mp = mp.copy()
                mp[..., -1] = 0.0
            spec = np.fft.ifft(mp, axis=-1) * n
            mph = np.mod(ms, n) if mutant == "wrap" and n == 4 * nside else ms
            php = np.exp(1j * np.outer(phi0[rings], mph))                     # (k, nm)
            gp = spec[..., np.mod(ms, n)] * php                               # (ncol, P, k, nm)
            gn = (spec[..., np.mod(-ms, n)] * php.conj()).conj()
            G[0][:, rings] = np.moveaxis(gp, (3, 2), (0, 1))
            G[1][:, rings] = np.moveaxis(gn, (3, 2), (0, 1))
            S[rings] = np.moveaxis(np.abs(mp).sum(axis=-1), 2, 0)
            S2[rings] = np.moveaxis(mod.sum(axis=-1), 2, 0)
        if mutant == "ringw" and self.ring_w is not None:                     # the belt takes the weight of the ring above
            belt = np.arange(nside - 1, 3 * nside)
            G[:, :, belt] *= (self.ring_w[belt - 1] / self.ring_w[belt])[None, None, :, None, None]
        return G, S, S2

    def slab_maps(self, rings, moduli=False, mutant=None):
        """(ncol, P, k, n) map values of the rings of a slab; with `moduli` also their `stokes_moduli`."""
        nside, P, cplx = self.nside, self.P, self.cplx
        n = int(self.nphi[rings[0]])
        ap = slab_angpos(nside, rings)
        hz = ob.horizon(ap, self.zenith).astype(np.float64)
        idx = np.concatenate([np.arange(self.start[r], self.start[r] + n) for r in rings])
        bs = self.beams[:, idx].reshape(NBEAM, idx.size, -1)
        out = np.empty((self.ncol, P, len(rings) * n), dtype=np.complex128)
        mod = np.empty((self.ncol, P, len(rings) * n)) if moduli else None
        for c in range(self.ncol):
            i, j = int(self.bi[c]), int(self.bj[c])
            tc = ob.fringe(ap, self.zenith, self.uv[c]) * hz / np.sqrt(self.omega[i] * self.omega[j])
            out[c] = stokes_maps(bs[i], bs[j].conj() if mutant == "conj" else bs[j], tc, P, cplx)
            if mutant == "vsign" and P == 4:
                out[c, 3] = -out[c, 3]
            if moduli:
                mod[c] = stokes_moduli(bs[i], bs[j], hz / np.sqrt(self.omega[i] * self.omega[j]), P)
        out = out.reshape(self.ncol, P, len(rings), n)
        return (out, mod.reshape(out.shape)) if moduli else out

    def tables(self, m):
        """(lambda, W, X), each (lmax + 1 - m, nring); W = X = None for one map."""
        lam = ob.lambda_lm(self.lmax, m, self.z)
        W, X = ob.wx_lm(self.lmax, m, self.z) if self.P == 4 else (None, None)
        return lam, W, X

    def coefficients(self, G):
        """(lmax + 1, 2, ncol, P, lside + 1) blocks from ring sums G: the Legendre sums of `transfer_single` and the fold."""
        lmax, P, ncol, L = self.lmax, self.P, self.ncol, self.lside + 1
        nring = self.z.size
        wr = (4.0 * np.pi / (12 * self.nside**2)) * (np.ones(nring) if self.ring_w is None else self.ring_w)
        ref = np.zeros((lmax + 1, 2, ncol, P, L), dtype=np.complex128)
        for m in range(lmax + 1):
            lam, W, X = self.tables(m)
            sl = slice(m, lmax + 1)
            for s in range(2):
                if m == 0 and s == 1:
                    continue
                g = G[s, m] * wr[:, None, None]                          # (nring, ncol, P)
                n_l = lmax + 1 - m
                if P == 1:
                    ref[m, s, :, 0, sl] = _rmat(lam, g[:, :, 0]).T
                else:
                    tv = _rmat(lam, g[:, :, [0, 3]].reshape(nring, -1)).reshape(n_l, ncol, 2)
                    wq = _rmat(W, g[:, :, [1, 2]].reshape(nring, -1)).reshape(n_l, ncol, 2)
                    xq = _rmat(X, g[:, :, [1, 2]].reshape(nring, -1)).reshape(n_l, ncol, 2)
                    ref[m, s, :, 0, sl] = tv[:, :, 0].T
                    ref[m, s, :, 3, sl] = tv[:, :, 1].T
                    ref[m, s, :, 1, sl] = (wq[:, :, 0] - 1j * xq[:, :, 1]).T
                    ref[m, s, :, 2, sl] = (wq[:, :, 1] + 1j * xq[:, :, 0]).T
        for c in range(ncol):                                                 # the column's own band limit
            ref[:, :, c, :, self.col_lmax[c] + 1 :] = 0.0
        return ref

    def _legendre(self):
        lmax, P, ncol, L = self.lmax, self.P, self.ncol, self.lside + 1
        nring = self.z.size
        w = 4.0 * np.pi / (12 * self.nside**2)
        wr = w * (np.ones(nring) if self.ring_w is None else self.ring_w)
        self.wr = wr
        ref = self.coefficients(self.G)
        bound = np.zeros((lmax + 1, ncol, P, L))
        amp = np.zeros((lmax + 1, ncol, P, L))
        cc, dtab = c_const(self.nside), lc.BOUND[lmax]
        Sw = self.S * wr[:, None, None]                                       # (nring, ncol, P)
        Sw2 = self.S2 * wr[:, None, None]
        for m in range(lmax + 1):
            lam, W, X = self.tables(m)
            sl = slice(m, lmax + 1)
            al = np.abs(lam)
            if P == 1:
                A = (al @ Sw[:, :, 0])[:, :, None]                            # (n_l, ncol, 1)
                A2 = (al @ Sw2[:, :, 0])[:, :, None]
                St = Sw.sum(axis=0)[None]                                     # (1, ncol, 1)
            else:
                aW, aX = np.abs(W), np.abs(X)
                A, A2 = [np.stack([al @ q[:, :, 0], aW @ q[:, :, 1] + aX @ q[:, :, 2], aW @ q[:, :, 2] + aX @ q[:, :, 1],
                                   al @ q[:, :, 3]], axis=-1) for q in (Sw, Sw2)]
                s1 = Sw.sum(axis=0)                                           # (ncol, P)
                St = np.stack([s1[:, 0], s1[:, 1] + s1[:, 2], s1[:, 1] + s1[:, 2], s1[:, 3]], axis=-1)[None]
            amp[m, :, :, sl] = np.moveaxis(A, 0, -1)
            bound[m, :, :, sl] = np.moveaxis(cc * A + dtab * St + E_TERMS * A2, 0, -1)
        # the column's own band limit
        for c in range(ncol):
            bound[:, c, :, self.col_lmax[c] + 1 :] = 0.0
            amp[:, c, :, self.col_lmax[c] + 1 :] = 0.0
        self.ref, self.bound, self.A = ref, bound, amp

    def expected(self, m_range):
        """(ref (nm, 2, ncol, P, L), bound (nm, 1, ncol, P, L)) of the blocks m_lo .. m_hi."""
        m_lo, m_hi = m_range
        return self.ref[m_lo : m_hi + 1], self.bound[m_lo : m_hi + 1, None]


@functools.lru_cache(maxsize=2)
def _problem(key, name):
    return Problem(BY_NAME[name])


def problem(case):
    """The Problem of a case, remembered for the cases that share it (the two most recent ones are kept)."""
    key = pkey(case)
    first = next(c["name"] for c in CASES if pkey(c) == key)
    return _problem(key, first)


def gather(bm, prob):
    """(nm, F, 2, B, P, L) blocks as the device wrote them -> (nm, 2, ncol, P, L) of the call's columns."""
    return bm[:, prob.col_f, :, prob.col_b].transpose(1, 2, 0, 3, 4)


def worst_ratio(got, ref, bound):
    """Largest |got - ref| / bound over the real and imaginary parts of the elements with bound > 0, and whether every
    element is within its bound (elements with bound 0 have to be equal)."""
    d = got - ref
    err = np.maximum(np.abs(d.real), np.abs(d.imag))
    b = np.broadcast_to(bound, err.shape)
    ok = bool((err <= b).all())
    pos = b > 0
    return (float((err[pos] / b[pos]).max()) if pos.any() else 0.0), ok
