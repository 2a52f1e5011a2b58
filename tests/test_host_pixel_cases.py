"""CPU checks of tests/pixel_cases.py, the cases, long-double reference and bound that test_gpu_bt_pixels.py holds the
pixel kernels of beam-transfer generation to: the cap on left-out pixels, from the reference alone; the float64 oracle
inside BOUND everywhere and its measured figure still at most BASE; and the reason for the per-pixel bound, kept as a
test — four damaged evaluations that a tolerance of 1e-12 of the largest value cannot see where the pattern is in its
sidelobes, each of which leaves the bound there."""
import numpy as np
import pytest

import pixel_cases as pc
from oracle import btgen as ob

pytestmark = pytest.mark.skipif(not pc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")
LD = pc.LD
OLD_TOL = 1e-12          # times the largest value: what test_gpu_btgen.py / test_gpu_telescopes.py ask
SIDELOBE = 1e-3          # of the peak and below


def test_case_table():
    import bt_fused_cases as bf

    assert pc.ZENITHS["N"] == bf.ZENITHS["N"] and pc.ZENITHS["S"] == bf.ZENITHS["S"] and pc.HORIZON_MIN == bf.HORIZON_MIN
    assert pc.ZENITHS["S"][1] != 0.0 and pc.ZENITHS["P"][0] < np.radians(1.0)
    assert {c[0] for c in pc.BEAM_CASES} == set(pc.NSIDES) == {c[0] for c in pc.MAP_CASES} == {1, 2, 3, 16, 64}
    for nside in pc.NSIDES:
        sub = [c for c in pc.BEAM_CASES if c[0] == nside]
        assert {c[2] for c in sub} == {0, 1, 2} and {c[3] for c in sub} == set(pc.TABLES) and {c[4] for c in sub} == set(pc.FWHMS)
        if nside >= 16:
            assert {"N", "S"} <= {c[1] for c in sub}
    for kind in (0, 1, 2):     # every kind meets every table and both widths
        assert {(c[3], c[4]) for c in pc.BEAM_CASES if c[2] == kind and c[0] == 16} == {(t, f) for t in pc.TABLES for f in pc.FWHMS}
    assert {g + b for g in pc.BATCH_AT for b in pc.BATCH} <= set(pc.BEAM_CASES) and len(pc.BATCH) >= 5
    assert {b[0] for b in pc.BATCH} == {0, 1, 2} and len({b[1] for b in pc.BATCH}) == 4
    uv, bi, bj = pc.map_columns()
    assert sorted(set(np.round(np.hypot(uv[:, 0], uv[:, 1]), 9))) == [0.0, 0.5, 30.0, 300.0]
    pairs = set(zip(bi.tolist(), bj.tolist()))
    assert {(0, 1), (1, 0)} <= pairs and any(i == j for i, j in pairs)
    for name in pc.BASE:
        assert pc.BOUND[name] == 8.0 * pc.BASE[name]
        assert round(pc.BASE[name], 1 if pc.BASE[name] < 10 else 0) == pc.BASE[name]      # two digits


@pytest.mark.parametrize("nside", pc.NSIDES)
def test_geometry_is_what_the_device_receives(nside):
    from driftscan_amd import healpix

    g = pc.geometry(nside)
    p0 = healpix.ring_layout(nside)[1]                       # (float64 pi / (4 i) is not always the rounded exact value)
    assert (np.abs(g["phi0_ld"].astype(np.float64) - p0) <= 2.0 ** -52 * p0).all() and ((p0 == 0.0) == (g["phi0_ld"] == 0)).all()
    assert np.array_equal(g["phi0"], ob.ring_info(nside)[2]) and np.array_equal(g["start"], ob.ring_info(nside)[3])
    ap = ob.ang_positions(nside)
    assert np.array_equal(np.cos(ap[:, 0]), g["cth"][g["ring"]]) and np.array_equal(np.sin(ap[:, 0]), g["sth"][g["ring"]])
    n = np.stack([g["st"] * g["cp"], g["st"] * g["sp"], g["ct"]], axis=-1).astype(np.float64)
    assert np.abs(n - ob.sph_to_cart(ap)).max() < (1.0 + 2.0 * np.pi) * 2.0 ** -52     # the rounding of phi and one of n
    for zen in pc.ZEN_OF[nside]:
        assert np.array_equal(pc.frame_of(zen), np.concatenate(ob.telescope_frame(np.array(pc.ZENITHS[zen]))))


def test_oracle_composition_is_the_oracle():
    """`pixel_cases.oracle_beam` with a Fraunhofer table is `oracle.btgen.beam_amp` / `beam_x` / `beam_y`."""
    ap = ob.ang_positions(16)
    zen = np.array(pc.ZENITHS["S"])
    w = pc.FR_WIDTH["fr3"]
    assert np.array_equal(pc.beam((16, "S", 0, "fr3", 2.5)).oracle()[:, 0], ob.beam_amp(ap, zen, w, pc.FR_FWHM, 2.5))
    assert np.array_equal(pc.beam((16, "S", 1, "fr3", 2.5)).oracle(), ob.beam_x(ap, zen, w, pc.FR_FWHM, 2.5))
    assert np.array_equal(pc.beam((16, "S", 2, "fr3", 0.05)).oracle(), ob.beam_y(ap, zen, w, 0.05, pc.FR_FWHM))


def _cap(keep, nside, name):
    out = int((~keep).sum())
    assert out <= pc.LEFT_OUT_MAX * keep.size, (name, out)
    if nside <= 3:
        assert out == 0, (name, out)


@pytest.mark.parametrize("group", pc.BEAM_GROUPS, ids=lambda g: "n%d-%s" % g)
def test_beam_cases(group):
    """Per case: the cap on left-out pixels; every ring's first and last pixel compared; pixels on the knots of the
    synthetic tables, the first and the last included, and beyond them; the float64 oracle within BOUND, its measured
    figure at most BASE."""
    nside, zen = group
    geo = pc.geometry(nside)
    ends = np.concatenate([geo["start"], geo["start"] + geo["nphi"] - 1])
    dx, _, dz = pc.float64_dots(geo, pc.frame_of(zen))
    worst = 0.0
    for case in [c for c in pc.BEAM_CASES if c[:2] == group]:
        b = pc.beam(case)
        _cap(b.keep, nside, case)
        assert b.keep[ends].all(), case
        assert b.ref.shape == (geo["npix"], 2 if case[2] else 1)
        assert (pc.to_f64(b.ref)[b.dz < 0] == 0.0).all() and (b.bound[b.dz < 0] == pc.TINY).all()
        if case[3].startswith("syn"):
            x = b.tab[0]
            on = [int(((dx == k) & (dz > 0)).sum()) for k in x]
            assert min(on) >= 1, (case, on)
            if nside > 1:
                assert ((dx < x[0]) & (dz > 0)).any() and ((dx > x[-1]) & (dz > 0)).any(), case
        o = b.oracle()
        ratio, fails = b.check(o)
        assert not fails, fails
        with np.errstate(under="ignore"):
            r = pc.measure(np.abs(o.astype(LD) - b.ref), b.scale, b.keep)
        worst = max(worst, r)
        assert r <= pc.BASE["beam"], (case, r)
    print("beams nside %d zenith %s: float64 oracle at most %.2f x 2^-53 (T + (1 + 2 pi) |grad|), BASE %.1f" % (nside, zen, worst, pc.BASE["beam"]))


@pytest.mark.parametrize("group", sorted({c[:3] for c in pc.MAP_CASES}), ids=lambda g: "n%d-%s-%s" % (g[0], g[1], "pol" if g[2] else "unpol"))
def test_map_cases(group):
    nside = group[0]
    worst = 0.0
    for mode in pc.MODES:
        m = pc.maps(group + (mode,))
        _cap(m.keep, nside, m.case)
        geo = pc.geometry(nside)
        assert m.keep[geo["start"]].all() and m.keep[geo["start"] + geo["nphi"] - 1].all()
        assert m.beams.dtype == (np.float64 if mode == "real" else np.complex128)
        o = m.oracle()
        ratio, fails = m.check(o)
        assert not fails, fails
        r = pc.measure(m.errors(o), m.scale, np.broadcast_to(m.keep, m.ref.shape))
        worst = max(worst, r)
        assert r <= pc.BASE["maps"], (m.case, r)
        if mode == "cast":       # the same numbers as the real patterns
            assert np.array_equal(pc.to_f64(m.ref.real), pc.to_f64(pc.maps(group + ("real",)).ref.real))
        if mode == "phase" and group[2]:   # V of a beam with itself: zero for real patterns, not for these
            c = [k for k in range(len(pc.MAP_BI)) if pc.MAP_BI[k] == pc.MAP_BJ[k]][0]
            assert np.abs(pc.to_f64(np.abs(m.ref[c, 3]))).max() > 0.0
            assert np.abs(pc.to_f64(np.abs(pc.maps(group + ("real",)).ref[c, 3]))).max() == 0.0
    print("maps nside %d zenith %s pol %s: float64 oracle at most %.2f, BASE %.1f" % (group + (worst, pc.BASE["maps"])))


# ---- damaged evaluations ------------------------------------------------------------------------------------------------
# Each mistake is made on the pixels where a tolerance of 1e-12 of the largest value cannot see it (all of them in the
# sidelobes, 1e-3 of the peak and below); everywhere else the evaluation is the oracle's.  The old tolerance passes the
# result, the per-pixel bound does not.
def _invisible(err, ref_abs):
    peak = ref_abs.max()
    return (err <= 0.5 * OLD_TOL * peak) & (ref_abs <= SIDELOBE * peak)


def _beam_mutant(case, damaged):
    b = pc.beam(case)
    good = b.oracle()
    ref64 = pc.to_f64(b.ref)
    amp = np.sqrt((ref64 ** 2).sum(axis=-1))
    hide = _invisible(np.abs(damaged - good).max(axis=-1), amp) & b.keep
    dam = np.where(hide[:, None], damaged, good)
    assert np.abs(dam - ref64).max() <= OLD_TOL * np.abs(ref64).max()          # today's tolerance is met
    assert not b.check(good)[1]
    ratio, fails = b.check(dam)
    caught = int(((np.abs(dam - ref64) > b.bound).any(axis=-1)).sum())
    print("%s: %d pixels hidden from 1e-12 of the peak, %d of them leave the bound, worst err / bound %.3g" % (case, int(hide.sum()), caught, ratio))
    assert fails and ratio > 8.0 and caught >= 10


def test_damage_spline_interval_shifted_at_a_knot():
    """The interval below the right one (khi - 1): exact on the shared knot, the neighbouring cubic beyond it."""
    case = (16, "N", 1, "fr3", 0.05)
    b = pc.beam(case)

    def shifted(x, y, y2, xv):
        khi = np.clip(np.clip(np.searchsorted(x, xv, side="left"), 1, x.size - 1) - 1, 1, x.size - 1)
        klo = khi - 1
        h = x[khi] - x[klo]
        a, bb = (x[khi] - xv) / h, (xv - x[klo]) / h
        return a * y[klo] + bb * y[khi] + ((a**3 - a) * y2[klo] + (bb**3 - bb) * y2[khi]) * (h * h) / 6.0

    _beam_mutant(case, pc.oracle_beam(ob.ang_positions(16), b.frame, 1, b.tab, 0.05, spline=shifted))


def test_damage_phi0_of_one_ring_dropped():
    """A ring whose pixels start at phi = 0 instead of phi0: the ring with the most hidden pixels."""
    case = (16, "N", 2, "fr7", 0.05)
    b = pc.beam(case)
    geo = pc.geometry(16)
    ap = ob.ang_positions(16)
    ap0 = ap.copy()
    ap0[:, 1] -= geo["phi0"][geo["ring"]]
    all_rings = pc.oracle_beam(ap0, b.frame, 2, b.tab, 0.05)
    good = b.oracle()
    amp = np.sqrt((pc.to_f64(b.ref) ** 2).sum(axis=-1))
    hide = _invisible(np.abs(all_rings - good).max(axis=-1), amp) & b.keep & (np.abs(all_rings - good) > b.bound).any(axis=-1)
    ring = int(np.argmax(np.bincount(geo["ring"][hide], minlength=geo["nphi"].size)))
    assert geo["phi0"][ring] != 0.0
    _beam_mutant(case, np.where((geo["ring"] == ring)[:, None], all_rings, good))


def _map_mutant(case, damage):
    m = pc.maps(case)
    good = m.oracle()
    damaged = damage(m, good)
    ref64 = pc.to_f64(m.ref.real) + 1j * pc.to_f64(m.ref.imag)
    peak = np.abs(ref64).max(axis=(1, 2), keepdims=True)                        # per column, as test_gpu_btgen.py
    hide = (np.abs(damaged - good) <= 0.5 * OLD_TOL * peak) & (np.abs(ref64) <= SIDELOBE * peak) & m.keep
    dam = np.where(hide, damaged, good)
    assert (np.abs(dam - ref64).max(axis=(1, 2)) <= OLD_TOL * peak[:, 0, 0]).all()
    assert not m.check(good)[1]
    ratio, fails = m.check(dam)
    caught = int((pc.to_f64(m.errors(dam)) > m.bound).any(axis=-1).sum())
    print("%s: %d values hidden from 1e-12 of the column's peak, %d of them leave the bound, worst err / bound %.3g"
          % (case, int(hide.sum()), caught, ratio))
    assert fails and ratio > 8.0 and caught >= 10


def test_damage_v_sign_flipped():
    def damage(m, good):
        d = good.copy()
        d[:, 3] = -d[:, 3]
        return d

    _map_mutant((16, "N", True, "real"), damage)


def test_damage_phase_in_float32():
    def damage(m, good):
        ap = ob.ang_positions(m.nside)
        zen = np.array(pc.ZENITHS[m.zen])
        d = np.empty_like(good)
        for c in range(m.uv.shape[0]):
            that, phat = ob.thetaphi_plane_cart(zen)
            ph = (2.0 * np.pi * (ob.sph_to_cart(ap) @ (m.uv[c, 0] * phat - m.uv[c, 1] * that))).astype(np.float32).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
                d[c] = good[c] * (np.cos(ph) + 1j * np.sin(ph)) / ob.fringe(ap, zen, m.uv[c])
        return np.where(np.isfinite(d), d, good)

    _map_mutant((16, "N", False, "real"), damage)
