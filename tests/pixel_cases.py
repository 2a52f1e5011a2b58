"""Cases, long-double reference and bound for the pixel stage of beam-transfer generation (dm_btgen.hip: `bt_beam_pixel`
behind `dm_bt_beam_cyl` / `dm_bt_beams_cyl`, and the solid-angle and map kernels behind `dm_bt_maps` / `dm_bt_maps_c`):
test_host_pixel_cases.py checks the cases, the reference and the bound on the CPU, test_gpu_bt_pixels.py holds the
device to them pixel by pixel.  TEST INFRASTRUCTURE — never imported by the product.

Reference.  `oracle.btgen` (`beam_amp`, `beam_exptan`, `spline_eval`, `polpattern`, `fringe`, `construct_pol_real`,
`construct_pol_complex`) restated in np.longdouble.  Its inputs are what the device receives, taken as exact numbers:
the float64 ring cos / sin of `healpix.ring_trig`, the float64 frame of `btgen.telescope_frame`, the float64 spline
knots, `fwhm_ns`, `uv`, and for the maps the float64 (complex128) field patterns that the test uploads.  The pixel
azimuth is formed in long double, phi = phi0 + 2 pi j / nphi with phi0 the exact multiple of pi of `healpix.ring_layout`;
the solid angles are long-double sums over the whole sphere.

Bound, per pixel and per real component — not a fraction of a scale.  Every output is a smooth function of the pixel
direction n apart from the horizon step, so a float64 evaluation carries the rounding of the evaluation itself and the
rounding of n (of phi: up to 2 pi 2^-53, hence 1 + 2 pi), carried by the gradient:

    bound(pix) = k 2^-53 (T(pix) + (1 + 2 pi) |grad_n f|(pix)) + (N_above + 8) 2^-53 |f(pix)| + 2^-1022

T is the sum of the moduli of the terms that make up the value: the four spline terms times the N-S factor times the
modulus of the polarisation component; for maps |tc| times the moduli of the beam products (A' of bt_fused_cases.py).
grad_n f is the reference's gradient along thetahat and phihat by central differences with step 2^-20 (with the horizon
factor of the pixel itself; for a map the field patterns are data, the fringe is what moves: this is where 2 pi |uv| of
the phase rounding enters).  The (N_above + 8) term is the rounding of the two solid-angle sums in any order, maps only.
2^-1022 is the smallest normal double: with fwhm_ns = 0.05 the N-S factor runs down to exp(-3e4) and most of the sphere
is denormal or zero in float64, where no relative statement holds (the term is 1e-292 of the peak).

k was measured on the CPU, never on the device: `python tests/pixel_cases.py` evaluates the float64 oracle
(`oracle.btgen`'s own functions on the same inputs) against this reference on every case and prints the worst
error / (2^-53 (T + (1 + 2 pi) |grad f|)) over the compared pixels whose value is not in underflow (MEASURE_MIN).
Rounded up to two digits that is BASE; BOUND = 8 BASE, the 8 being DESIGN.md 4.3's allowance for another order of
summation and FMA contraction, as in legendre_cases.py.  test_host_pixel_cases.py asserts that the measurement still
gives at most BASE.

Pixels left out of the comparison: |n.zhat| < 1e-9 (the device asks n.z > 0, a value that close is decided by rounding)
and, for dipole patterns, a projected dipole shorter than 1e-6 (the unit vector is ill-conditioned there).  They must
be finite and within the envelope T (taken with the horizon factor 1) plus the bound.  At most 0.1 % of a case's pixels
may be left out and none at nside <= 3: that is why nside 1 and 3 do not take the zenith "N" (phi = 0: the pixel at the
east point of the horizon is a pixel centre there, and it is the direction of the X dipole).
"""
import functools
import sys

import numpy as np

LD = np.longdouble
LD_OK = np.finfo(np.longdouble).eps < 2e-19   # 64-bit mantissa; the tests skip where long double is only a double
U = 2.0 ** -53
TINY = 2.0 ** -1022
PI = LD(4) * np.arctan(LD(1))
CGRAD = LD(1) + LD(2) * PI
HSTEP = LD(2.0 ** -20)
HORIZON_MIN = 1e-9            # bt_fused_cases.HORIZON_MIN
DIPOLE_MIN = 1e-6
LEFT_OUT_MAX = 1e-3
MEASURE_MIN = 2.0 ** -900     # BASE is measured where T + (1 + 2 pi) |grad f| is at least this

# measured by `python tests/pixel_cases.py` (float64 oracle against the long-double reference, all cases; the figures it
# printed: beams 15.67, maps 12.37), rounded up to two digits.  Both figures come from pixels where |grad f| is small by
# cancellation while the roundings it stands for are not: for the beams a pixel near the N-S axis (n.y = -0.957, nside
# 64, zenith P, Y dipole, fwhm_ns 2.5), where the slopes of the E-W factor, the N-S factor and the polarisation
# component cancel while 1 - s^2 of the N-S factor alone loses 11 x 2^-53; for the maps a pixel the baseline points at
# (|uv| = 30), where the phase 2 pi |uv| n.u is rounded at its full size while the gradient sees the tangential part of
# the baseline only.
BASE = {"beam": 16.0, "maps": 13.0}
BOUND = {k: 8.0 * v for k, v in BASE.items()}

# "N" and "S" are bt_fused_cases.ZENITHS; "E" is a northern site off phi = 0 for the smallest maps, "P" lies 0.6 degrees
# from the pole: polpattern's singular point (the pole of the coordinates) is 0.6 degrees from the beam centre
ZENITHS = {"N": (np.pi / 2 - np.radians(49.3), 0.0), "S": (np.pi / 2 + np.radians(37.1), 0.7),
           "E": (np.pi / 2 - np.radians(41.7), 1.1), "P": (np.radians(0.6), 2.1)}
NSIDES = (1, 2, 3, 16, 64)
ZEN_OF = {1: ("S", "E", "P"), 2: ("N", "S", "P"), 3: ("S", "E", "P"), 16: ("N", "S", "P"), 64: ("N", "S", "P")}
TABLES = ("fr3", "fr7", "syn2", "syn5")
FWHMS = (0.05, 2.5)
FR_FWHM = 2.0 * np.pi / 3.0
FR_WIDTH = {"fr3": 2.7, "fr7": 7.3}


# ---- geometry ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry(nside):
    """Per pixel, in long double from the float64 ring cos / sin: ct, st, cos phi, sin phi; ring, j and the layout."""
    from driftscan_amd import healpix

    cth, sth = healpix.ring_trig(nside)
    nphi, phi0, start = healpix.ring_layout(nside)
    i = np.arange(1, 4 * nside)
    north, belt = i < nside, (i >= nside) & (i <= 3 * nside)
    jj = np.where(north, i, 4 * nside - i)
    q = np.where(belt, np.where((i + nside) % 2 == 0, LD(1) / LD(4 * nside), LD(0)), LD(1) / (LD(4) * jj.astype(LD)))
    phi0_ld = PI * q
    ring = np.repeat(np.arange(nphi.size), nphi)
    j = np.arange(12 * nside * nside) - start[ring]
    phi = phi0_ld[ring] + LD(2) * PI * j.astype(LD) / nphi[ring].astype(LD)
    return dict(nside=nside, npix=12 * nside * nside, cth=cth, sth=sth, nphi=nphi, phi0=phi0, phi0_ld=phi0_ld, start=start,
                ring=ring, j=j, ct=cth.astype(LD)[ring], st=sth.astype(LD)[ring], cp=np.cos(phi), sp=np.sin(phi))


def frame_of(zen):
    from driftscan_amd import btgen

    return np.ascontiguousarray(btgen.telescope_frame(np.array(ZENITHS[zen])), dtype=np.float64).reshape(9)


def _points(geo, idx=None):
    """(ct, st, cp, sp) of the pixels and of the four points n +/- h thetahat, n +/- h phihat (renormalised)."""
    ct, st, cp, sp = (geo[k] if idx is None else geo[k][idx] for k in ("ct", "st", "cp", "sp"))
    n = np.stack([st * cp, st * sp, ct])
    e1 = np.stack([ct * cp, ct * sp, -st])
    e2 = np.stack([-sp, cp, np.zeros_like(sp)])
    out = [(ct, st, cp, sp)]
    for e in (e1, e2):
        for s in (1, -1):
            m = n + LD(s) * HSTEP * e
            m = m / np.sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2])
            s_ = np.hypot(m[0], m[1])
            out.append((m[2], s_, m[0] / s_, m[1] / s_))
    return out


def _grad(vals):
    """|grad| from the values at (n, +e1, -e1, +e2, -e2), per real component."""
    d1 = (vals[1] - vals[2]) / (LD(2) * HSTEP)
    d2 = (vals[3] - vals[4]) / (LD(2) * HSTEP)
    return np.hypot(d1, d2)


# ---- field patterns ---------------------------------------------------------------------------------------------------
def float64_dots(geo, frame):
    """n.x, n.y, n.z as numpy's float64 forms them from the float64 geometry (what the knots of the synthetic tables
    are taken from, and what the oracle sees)."""
    phi = geo["phi0"][geo["ring"]] + 2.0 * np.pi * geo["j"] / geo["nphi"][geo["ring"]]
    st, ct = geo["sth"][geo["ring"]], geo["cth"][geo["ring"]]
    n = np.stack([st * np.cos(phi), st * np.sin(phi), ct], axis=-1)
    return n @ frame[0:3], n @ frame[3:6], n @ frame[6:9]


@functools.lru_cache(maxsize=None)
def table(name, nside, zen):
    """(x, y, y'') float64 knots.  fr3 / fr7: the Fraunhofer pattern of a cylinder 2.7 / 7.3 wavelengths wide.  syn2 /
    syn5: 2 / 5 knots that ARE computed n.x values of pixels above the horizon (quantiles of the distinct values, so
    that pixels lie on the first and on the last knot and beyond both), natural-spline second derivatives for syn5;
    syn2 carries second derivatives of its own (one interval: a cubic everywhere)."""
    from oracle import btgen as ob

    if name in FR_WIDTH:
        return tuple(np.ascontiguousarray(a) for a in ob.fraunhofer_cylinder(FR_FWHM, FR_WIDTH[name]))
    dx, _, dz = float64_dots(geometry(nside), frame_of(zen))
    vals = np.unique(dx[dz > HORIZON_MIN])
    if name == "syn2":
        x = vals[[int(0.2 * (vals.size - 1)), int(np.ceil(0.8 * (vals.size - 1)))]]
        return x, np.array([0.7, -0.4]), np.array([0.9, -1.3])
    # (nside 1 has five or six distinct values above the horizon: the knots then span all of them)
    q = np.array([0.1, 0.3, 0.5, 0.7, 0.9]) * (vals.size - 1) if vals.size >= 10 else np.linspace(0, vals.size - 1, 5)
    x = vals[np.unique(np.round(q).astype(int))]
    assert x.size == 5, (name, nside, zen)
    y = np.array([0.2, -0.5, 1.0, 0.4, -0.1])
    return x, y, ob.natural_spline(x, y)


def _beam_core(pt4, frame, kind, tab, fwhm, hz=None):
    """value and T (npx, ncomp) in long double at the points (ct, st, cp, sp); also n.z and the norm of the projected
    dipole.  hz None: the horizon factor of these points."""
    ct, st, cp, sp = pt4
    fr = frame.astype(LD)
    x, y, y2 = (np.asarray(a, dtype=LD) for a in tab)
    n0, n1, n2 = st * cp, st * sp, ct
    dz = n0 * fr[6] + n1 * fr[7] + n2 * fr[8]
    dx = n0 * fr[0] + n1 * fr[1] + n2 * fr[2]
    dy = n0 * fr[3] + n1 * fr[4] + n2 * fr[5]
    if hz is None:
        hz = (dz > 0).astype(LD)
    khi = np.clip(np.searchsorted(x, dx, side="left"), 1, x.size - 1)
    klo = khi - 1
    h = x[khi] - x[klo]
    a = (x[khi] - dx) / h
    b = (dx - x[klo]) / h
    terms = (a * y[klo], b * y[khi], (a * a * a - a) * y2[klo] * (h * h) / LD(6), (b * b * b - b) * y2[khi] * (h * h) / LD(6))
    ew = terms[0] + terms[1] + (terms[2] + terms[3])
    tew = sum(np.abs(t) for t in terms)
    alpha = np.log(LD(2)) / (LD(2) * np.tan(LD(fwhm) / LD(2)) ** 2)
    s2 = dy * dy
    with np.errstate(under="ignore"):
        ns = np.exp(-alpha * s2 / (LD(1) - s2 + LD(1e-100)))
        amp, tamp = ew * ns * hz, tew * ns * hz
        if kind == 0:
            return amp[:, None], tamp[:, None], dz, None
        dip = fr[0:3] if kind == 1 else fr[3:6]
        pt = ct * cp * dip[0] + ct * sp * dip[1] - st * dip[2]
        pp = -sp * dip[0] + cp * dip[1]
        nrm = np.hypot(pt, pp)
        safe = np.where(nrm == 0, LD(1), nrm)
        comp = np.stack([pt / safe, pp / safe], axis=-1)
        return amp[:, None] * comp, tamp[:, None] * np.abs(comp), dz, nrm


def beam_cases():
    """(nside, zen, kind, table, fwhm_ns): every kind, table and width at every nside and zenith."""
    out = []
    for nside in NSIDES:
        for zen in ZEN_OF[nside]:
            for kind in (0, 1, 2):
                for tab in TABLES:
                    for fw in FWHMS:
                        out.append((nside, zen, kind, tab, fw))
    return out


BEAM_CASES = beam_cases()
BEAM_GROUPS = sorted({(c[0], c[1]) for c in BEAM_CASES})
# the patterns of one `dm_bt_beams_cyl` call (kind, table, fwhm_ns) and where it is made: all of them rows of BEAM_CASES
BATCH = ((0, "fr3", 2.5), (1, "syn2", 0.05), (2, "fr7", 2.5), (0, "syn5", 0.05), (1, "fr7", 0.05), (2, "syn2", 2.5), (0, "syn2", 2.5))
BATCH_AT = ((1, "E"), (3, "S"), (16, "P"), (64, "N"))


def to_f64(a):
    with np.errstate(under="ignore"):
        return np.asarray(a).astype(np.float64)


class Beam(object):
    """Reference of one field pattern: ref, T, G (npix, ncomp) long double; bound (npix, ncomp) float64; keep (npix,)
    pixels in the comparison; env (npix, ncomp) float64: what a left-out pixel may reach."""

    def __init__(self, case):
        nside, zen, kind, tname, fwhm = case
        self.case, self.nside, self.kind, self.fwhm = case, nside, kind, fwhm
        geo = geometry(nside)
        self.frame = frame_of(zen)
        self.tab = table(tname, nside, zen)
        pts = _points(geo)
        ref, T, dz, nrm = _beam_core(pts[0], self.frame, kind, self.tab, fwhm)
        hz = (dz > 0).astype(LD)
        with np.errstate(under="ignore"):
            G = _grad([ref] + [_beam_core(p, self.frame, kind, self.tab, fwhm, hz=hz)[0] for p in pts[1:]])
        self.ref, self.T, self.G, self.dz = ref, T, G, dz
        self.keep = np.abs(dz) >= HORIZON_MIN
        if kind:
            self.keep &= nrm >= DIPOLE_MIN
        self.n_above = int((dz > 0).sum())
        self.scale = T + CGRAD * G
        self.bound = to_f64(LD(BOUND["beam"] * U) * self.scale) + TINY
        # left-out pixels: the envelope is that of the amplitude with the horizon factor 1
        self.env = np.zeros(ref.shape)
        out = np.nonzero(~self.keep)[0]
        if out.size:
            po = _points(geo, out)
            one = np.ones(out.size, dtype=LD)
            v, t = zip(*[_beam_core(p, self.frame, 0, self.tab, fwhm, hz=one)[:2] for p in po])
            self.env[out] = to_f64(t[0] * (LD(1) + LD(BOUND["beam"] * U)) + LD(BOUND["beam"] * U) * CGRAD * _grad(list(v))) + TINY

    def input64(self):
        """The pattern as float64 data (npix, ncomp): the input of the map cases."""
        return to_f64(self.ref)

    def oracle(self):
        """The float64 oracle on the same inputs: the body of `oracle.btgen.beam_amp` / `beam_x` / `beam_y` with the table
        handed in (test_host_pixel_cases.py holds it to those functions where the table is theirs)."""
        from oracle import btgen as ob

        return oracle_beam(ob.ang_positions(self.nside), self.frame, self.kind, self.tab, self.fwhm)

    def check(self, got):
        """(worst error / bound over the compared pixels, list of complaints) for a (npix, ncomp) float64 result."""
        return _check(got.reshape(self.ref.shape), self.ref, self.bound, self.keep, self.env, str(self.case))


def oracle_beam(ap, frame, kind, tab, fwhm, spline=None):
    from oracle import btgen as ob

    cvec = ob.sph_to_cart(ap)
    xh, yh, zh = frame[0:3], frame[3:6], frame[6:9]
    hz = (cvec @ zh > 0.0).astype(np.float64)
    with np.errstate(under="ignore"):
        amp = (spline or ob.spline_eval)(tab[0], tab[1], tab[2], cvec @ xh) * ob.beam_exptan(cvec @ yh, fwhm) * hz
        if kind == 0:
            return amp[:, None]
        return amp[:, None] * ob.polpattern(ap, xh if kind == 1 else yh)


def _check(got, ref, bound, keep, env, name):
    """Compared pixels: |got - ref| <= bound per real component.  Left-out pixels: finite and within the envelope."""
    fails = []
    if not np.isfinite(got.view(np.float64)).all():
        fails.append("%s: %d values are not finite" % (name, int((~np.isfinite(got.view(np.float64))).sum())))
        return np.inf, fails
    if np.iscomplexobj(got):
        with np.errstate(under="ignore"):
            err = np.stack([to_f64(np.abs(got.real.astype(LD) - ref.real)), to_f64(np.abs(got.imag.astype(LD) - ref.imag))], axis=-1)
        mag = np.stack([np.abs(got.real), np.abs(got.imag)], axis=-1)
    else:
        err = to_f64(np.abs(got.astype(LD) - ref))
        mag = np.abs(got)
    kp = keep.reshape(keep.shape + (1,) * (err.ndim - keep.ndim)) & np.ones(err.shape, dtype=bool)
    ratio = err / bound
    worst = float(ratio[kp].max()) if kp.any() else 0.0
    bad = kp & ~(err <= bound)
    if bad.any():
        at = np.unravel_index(np.argmax(np.where(bad, ratio, 0.0)), ratio.shape)
        fails.append("%s: %d of %d compared values leave the bound; worst err %.3e bound %.3e at %s"
                     % (name, int(bad.sum()), int(kp.sum()), err[at], bound[at], at))
    over = ~kp & ~(mag <= env)
    if over.any():
        fails.append("%s: %d left-out values leave the envelope" % (name, int(over.sum())))
    return worst, fails


@functools.lru_cache(maxsize=4)
def beam(case):
    return Beam(case)


def measure(err, scale, keep):
    """Worst err / (2^-53 scale) over the compared values that are not in underflow."""
    m = keep.reshape(keep.shape + (1,) * (err.ndim - keep.ndim)) & (scale >= LD(MEASURE_MIN))
    if not m.any():
        return 0.0
    return float((err[m] / (LD(U) * scale[m])).max())


# ---- maps -------------------------------------------------------------------------------------------------------------
# three patterns per (nside, zenith): polarised X, Y, Y (kinds 1, 2, 2), unpolarised kind 0, with these tables and widths
MAP_BEAMS = (("fr3", 2.5), ("fr7", 2.5), ("syn5", 0.05))
MAP_KINDS = {True: (1, 2, 2), False: (0, 0, 0)}
UVABS = (0.0, 0.5, 30.0, 300.0, 300.0, 30.0)
UVANG = (0.0, 0.4, 2.3, 4.1, 5.6, 1.2)
MAP_BI = (0, 1, 1, 0, 2, 2)
MAP_BJ = (1, 0, 1, 2, 2, 0)
MAP_ZEN = {1: ("S",), 2: ("N",), 3: ("E",), 16: ("N", "P"), 64: ("S",)}
MODES = ("real", "cast", "phase")
# the "phase" patterns: component k of beam b times exp(i KPH n.q), so that b_i conj(b_j) is not b_i b_j and V of a beam
# with itself is not zero
KPH = ((1.3, -0.9), (-1.7, 0.8), (0.6, 2.1))
PDIR = (((0.8, -0.5, 0.2), (0.1, 1.0, 0.0)), ((-0.3, 0.9, 0.1), (1.0, 0.2, -0.3)), ((0.5, 0.5, 0.5), (-0.9, 0.4, 0.0)))
MAP_CASES = [(nside, zen, pol, mode) for nside in NSIDES for zen in MAP_ZEN[nside] for pol in (False, True) for mode in MODES]


def map_columns():
    uv = np.array(UVABS)[:, None] * np.stack([np.cos(UVANG), np.sin(UVANG)], axis=-1)
    return np.ascontiguousarray(uv), np.array(MAP_BI, dtype=np.int32), np.array(MAP_BJ, dtype=np.int32)


def stokes(bi, bj, tc, pol, out_dtype):
    """The expressions of `oracle.btgen.construct_pol_complex` (`construct_pol_real` for real bj) / of
    `beam_transfer_m` for one map: (P, npx) from patterns (npx, ncomp) and tc = fringe horizon / sqrt(O_i O_j)."""
    cj = np.conj(bj)
    if not pol:
        return (tc * bi[:, 0] * cj[:, 0])[None].astype(out_dtype)
    out = np.empty((4, bi.shape[0]), dtype=out_dtype)
    out[0] = tc * (bi[:, 0] * cj[:, 0] + bi[:, 1] * cj[:, 1])
    out[1] = tc * (bi[:, 0] * cj[:, 0] - bi[:, 1] * cj[:, 1])
    out[2] = tc * (bi[:, 0] * cj[:, 1] + bi[:, 1] * cj[:, 0])
    out[3] = 1j * tc * (bi[:, 0] * cj[:, 1] - bi[:, 1] * cj[:, 0])
    return out


def moduli(bi, bj, atc, pol):
    ai, aj = np.abs(bi), np.abs(bj)
    if not pol:
        return (atc * ai[:, 0] * aj[:, 0])[None]
    d = atc * (ai[:, 0] * aj[:, 0] + ai[:, 1] * aj[:, 1])
    x = atc * (ai[:, 0] * aj[:, 1] + ai[:, 1] * aj[:, 0])
    return np.stack([d, d, x, x])


class Maps(object):
    """Inputs, reference and bound of one `dm_bt_maps` / `dm_bt_maps_c` call.

    beams (3, npix, ncomp) float64 or complex128 (the input, exact); uv, bi, bj; ref (ncol, P, npix) complex long
    double; T (ncol, P, npix) and G, bound, env (ncol, P, npix, 2) for the real and the imaginary part; keep (npix,)."""

    def __init__(self, case):
        nside, zen, pol, mode = case
        self.case, self.nside, self.pol, self.mode, self.zen = case, nside, pol, mode, zen
        geo = geometry(nside)
        npix = geo["npix"]
        self.frame = frame_of(zen)
        fr = self.frame.astype(LD)
        self.uv, self.bi, self.bj = map_columns()
        pts = _points(geo)
        ct, st, cp, sp = pts[0]
        dirs = [np.stack([p[1] * p[2], p[1] * p[3], p[0]], axis=-1) for p in pts]       # (npix, 3) at the five points
        b64 = np.stack([beam((nside, zen, kind, tab, fw)).input64()
                        for kind, (tab, fw) in zip(MAP_KINDS[pol], MAP_BEAMS)])          # (3, npix, ncomp)
        if mode == "real":
            self.beams = b64
        elif mode == "cast":
            self.beams = b64.astype(np.complex128)
        else:
            e, no, mu = (dirs[0] @ fr[3 * k : 3 * k + 3] for k in range(3))
            self.beams = np.empty(b64.shape, dtype=np.complex128)
            for b in range(3):
                for k in range(b64.shape[2]):
                    q = PDIR[b][k]
                    ph = LD(KPH[b][k]) * (LD(q[0]) * e + LD(q[1]) * no + LD(q[2]) * mu)
                    self.beams[b, :, k] = to_f64(b64[b, :, k] * np.cos(ph)) + 1j * to_f64(b64[b, :, k] * np.sin(ph))
        cdt = np.clongdouble
        bl = self.beams.astype(cdt if np.iscomplexobj(self.beams) else LD)
        dz = dirs[0] @ fr[6:9]
        hz = (dz > 0).astype(LD)
        self.keep = np.abs(dz) >= HORIZON_MIN
        self.n_above = int((dz > 0).sum())
        with np.errstate(under="ignore"):
            omega = np.array([np.sum(hz * np.sum(np.abs(bl[b]) ** 2, axis=-1)) for b in range(3)], dtype=LD) * LD(4) * PI / LD(npix)
        self.omega = omega
        ncol, P = self.uv.shape[0], 4 if pol else 1
        self.ref = np.empty((ncol, P, npix), dtype=cdt)
        self.T = np.empty((ncol, P, npix), dtype=LD)
        self.Tenv = np.empty((ncol, P, npix), dtype=LD)
        self.G = np.empty((ncol, P, npix, 2), dtype=LD)
        for c in range(ncol):
            i, j = int(self.bi[c]), int(self.bj[c])
            uv3 = LD(self.uv[c, 0]) * fr[0:3] + LD(self.uv[c, 1]) * fr[3:6]
            pre = LD(1) / np.sqrt(omega[i] * omega[j])
            vals = []
            with np.errstate(under="ignore"):
                for d in dirs:
                    ph = LD(2) * PI * (d @ uv3)
                    tc = (np.cos(ph) + 1j * np.sin(ph)).astype(cdt) * (hz * pre)
                    vals.append(stokes(bl[i], bl[j], tc, pol, cdt))
                self.ref[c] = vals[0]
                self.G[c, ..., 0] = _grad([v.real for v in vals])
                self.G[c, ..., 1] = _grad([v.imag for v in vals])
                self.Tenv[c] = moduli(bl[i], bl[j], pre, pol)
                self.T[c] = self.Tenv[c] * hz
        with np.errstate(under="ignore"):
            self.scale = self.T[..., None] + CGRAD * self.G
            parts = np.stack([np.abs(self.ref.real), np.abs(self.ref.imag)], axis=-1)
            self.bound = to_f64(LD(BOUND["maps"] * U) * self.scale + LD((self.n_above + 8) * U) * parts) + TINY
            # a left-out pixel (the horizon): the device may decide the horizon factor either way
            k = LD(BOUND["maps"] * U)
            gmax = LD(2) * PI * LD(np.hypot(self.uv[:, 0], self.uv[:, 1]))[:, None, None]
            self.env = to_f64(self.Tenv * (LD(1) + k * (LD(1) + CGRAD * gmax) + LD((self.n_above + 8) * U)))[..., None] + TINY
            self.env = np.broadcast_to(self.env, self.bound.shape)

    def oracle(self):
        """The float64 oracle on the same inputs: `fringe`, `horizon` and `construct_pol_real` / `construct_pol_complex`
        of oracle.btgen, for one map the product of `beam_transfer_m`."""
        from oracle import btgen as ob

        ap = ob.ang_positions(self.nside)
        zen = np.array(ZENITHS[self.zen])
        hz = ob.horizon(ap, zen).astype(np.float64)
        out = np.empty(self.ref.shape, dtype=np.complex128)
        with np.errstate(under="ignore"):
            for c in range(self.uv.shape[0]):
                bi, bj = self.beams[self.bi[c]], self.beams[self.bj[c]]
                fr = ob.fringe(ap, zen, self.uv[c])
                if self.pol:
                    out[c] = (ob.construct_pol_complex if np.iscomplexobj(bi) else ob.construct_pol_real)(bi, bj, fr, hz)
                else:
                    pxarea = 4 * np.pi / ap.shape[0]
                    om_i = np.sum(np.abs(bi[:, 0]) ** 2 * hz) * pxarea
                    om_j = np.sum(np.abs(bj[:, 0]) ** 2 * hz) * pxarea
                    out[c, 0] = hz * fr * bi[:, 0] * bj[:, 0].conjugate() / np.sqrt(om_i * om_j)
        return out

    def check(self, got):
        keep = np.broadcast_to(self.keep, self.ref.shape)
        return _check(got.reshape(self.ref.shape), self.ref, self.bound, keep, self.env, str(self.case))

    def errors(self, got):
        """|got - ref| (ncol, P, npix, 2) in long double."""
        with np.errstate(under="ignore"):
            return np.stack([np.abs(got.real.astype(LD) - self.ref.real), np.abs(got.imag.astype(LD) - self.ref.imag)], axis=-1)


@functools.lru_cache(maxsize=2)
def maps(case):
    return Maps(case)


def measure_base(out=None):
    """The worst error / (2^-53 (T + (1 + 2 pi) |grad f|)) of the float64 oracle over all cases: (beams, maps)."""
    wb = wm = 0.0
    for case in BEAM_CASES:
        b = beam(case)
        with np.errstate(under="ignore"):
            r = measure(np.abs(b.oracle().astype(LD) - b.ref), b.scale, b.keep)
        wb = max(wb, r)
        if out:
            out.write("beam %-34s %6.2f\n" % (case, r))
    for case in MAP_CASES:
        m = maps(case)
        r = measure(m.errors(m.oracle()), m.scale, np.broadcast_to(m.keep, m.ref.shape))
        wm = max(wm, r)
        if out:
            out.write("maps %-34s %6.2f\n" % (case, r))
    return wb, wm


if __name__ == "__main__":
    import os

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    wb, wm = measure_base(sys.stdout)
    print("worst float64 oracle error / (2^-53 (T + (1 + 2 pi) |grad f|)): beams %.2f, maps %.2f" % (wb, wm))
    print("in the file: BASE = %r" % (BASE,))
