"""GPU: the pixel stage of beam-transfer generation pixel by pixel — the cylinder field patterns of `dm_bt_beam_cyl` and
of the batched `dm_bt_beams_cyl` that production calls, the solid angles and response maps of `dm_bt_maps` and
`dm_bt_maps_c` — against the long-double reference and the derived per-pixel bound of tests/pixel_cases.py (cases, bound
and what is left out are described there; test_host_pixel_cases.py checks them on the CPU).  Every output buffer is
filled with NaN and wrapped in guards first.  Each test prints the worst error / bound per case: the float64 oracle sits
at 1/8 at most, by construction of the bound."""
import ctypes

import numpy as np
import pytest

import pixel_cases as pc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not pc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")]
PAD = 64
c_dbl_p, c_int_p = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 30)
    yield c
    c.close()


def _poisoned(ctx, n, dtype=np.float64):
    """A NaN-filled device vector of n + 2 PAD elements; the payload is [PAD, PAD + n)."""
    t = ctx.empty((n + 2 * PAD,), dtype)
    t.fill_(complex(np.nan, np.nan) if np.dtype(dtype).kind == "c" else np.nan)
    return t


def _host(t):
    return t.cpu().numpy()


def _all_nan(a):
    return bool(np.isnan(a.view(np.float64)).all())


def _single(ctx, case):
    """`dm_bt_beam_cyl` of one case: (npix, ncomp) float64, the guards checked."""
    nside, zen, kind, tname, fwhm = case
    geo = pc.geometry(nside)
    n = geo["npix"] * (2 if kind else 1)
    buf = _poisoned(ctx, n)
    ctx.bt_beam_cyl(nside, geo["cth"], geo["sth"], pc.frame_of(zen), kind, pc.table(tname, nside, zen), fwhm, buf[PAD : PAD + n])
    ctx.sync()
    h = _host(buf)
    assert _all_nan(h[:PAD]) and _all_nan(h[PAD + n :]), case
    return h[PAD : PAD + n].reshape(geo["npix"], -1)


@pytest.mark.parametrize("group", pc.BEAM_GROUPS, ids=lambda g: "n%d-%s" % g)
def test_beam_cyl(ctx, group):
    fails, worst = [], {}
    for case in [c for c in pc.BEAM_CASES if c[:2] == group]:
        r, f = pc.beam(case).check(_single(ctx, case))
        fails += f
        worst[case] = r
        print("dm_bt_beam_cyl %-32s worst err / bound %.3f" % (case, r))
    assert not fails, "\n".join(fails)


BATCH = pc.BATCH


@pytest.mark.parametrize("nside,zen", pc.BATCH_AT)
def test_beams_cyl_batched(ctx, nside, zen):
    """One call for seven patterns of mixed kinds, tables of 2, 5 and some hundred knots, rows further apart than the
    longest: every row has the bits of `dm_bt_beam_cyl`, what lies between and around the rows is untouched."""
    geo = pc.geometry(nside)
    npix = geo["npix"]
    stride = 2 * npix + 37
    nb = len(BATCH)
    buf = _poisoned(ctx, nb * stride)
    out = buf[PAD : PAD + nb * stride].view(nb, stride)
    specs = [(kind, pc.table(t, nside, zen), fw) for kind, t, fw in BATCH]
    assert len({len(s[1][0]) for s in specs}) >= 4
    ctx.bt_beams_cyl(nside, geo["cth"], geo["sth"], pc.frame_of(zen), specs, out, list(range(nb)))
    ctx.sync()
    h = _host(buf)
    assert _all_nan(h[:PAD]) and _all_nan(h[PAD + nb * stride :])
    rows = h[PAD : PAD + nb * stride].reshape(nb, stride)
    fails = []
    for b, (kind, t, fw) in enumerate(BATCH):
        n = npix * (2 if kind else 1)
        case = (nside, zen, kind, t, fw)
        one = _single(ctx, case)
        assert np.array_equal(rows[b, :n].view(np.uint64), one.reshape(-1).view(np.uint64)), case
        assert _all_nan(rows[b, n:]), case
        r, f = pc.beam(case).check(rows[b, :n].reshape(npix, -1))
        fails += f
        print("dm_bt_beams_cyl row %d %-30s worst err / bound %.3f" % (b, case, r))
    assert not fails, "\n".join(fails)


def _geo_ptrs(nside, zen):
    geo = pc.geometry(nside)
    keep = [np.ascontiguousarray(geo["cth"]), np.ascontiguousarray(geo["sth"]), pc.frame_of(zen)]
    return keep, [a.ctypes.data_as(c_dbl_p) for a in keep]


@pytest.mark.parametrize("group", sorted({c[:3] for c in pc.MAP_CASES}), ids=lambda g: "n%d-%s-%s" % (g[0], g[1], "pol" if g[2] else "unpol"))
def test_maps(ctx, group):
    """`dm_bt_maps` on float64 patterns, `dm_bt_maps_c` on the same patterns cast to complex128 (the same bound) and on
    patterns with a phase per component (the conjugate of the second pattern, the sign of V); `ncol = 0` writes nothing."""
    nside, zen, pol = group
    geo = pc.geometry(nside)
    fails = []
    for mode in pc.MODES:
        m = pc.maps(group + (mode,))
        ncol, P, npix = m.ref.shape
        buf = _poisoned(ctx, ncol * P * npix, np.complex128)
        out = buf[PAD : PAD + ncol * P * npix].view(ncol, P, npix)
        beams = ctx.to_device(m.beams.reshape(3, -1))
        assert beams.is_complex() == (mode != "real")
        ctx.bt_maps(nside, geo["cth"], geo["sth"], m.frame, pol, beams, m.uv, m.bi, m.bj, out)
        ctx.sync()
        h = _host(buf)
        assert _all_nan(h[:PAD]) and _all_nan(h[PAD + ncol * P * npix :]), m.case
        r, f = m.check(h[PAD : PAD + ncol * P * npix].reshape(ncol, P, npix))
        fails += f
        print("%s %-28s worst err / bound %.3f" % ("dm_bt_maps  " if mode == "real" else "dm_bt_maps_c", m.case, r))
        # no columns: nothing is written
        buf = _poisoned(ctx, P * npix, np.complex128)
        keep, (cp, sp, fp) = _geo_ptrs(nside, zen)
        uv, bi, bj = np.ascontiguousarray(m.uv), np.ascontiguousarray(m.bi, dtype=np.int32), np.ascontiguousarray(m.bj, dtype=np.int32)
        fn = ctx.lib.dm_bt_maps if mode == "real" else ctx.lib.dm_bt_maps_c
        rc = fn(ctx.h, nside, cp, sp, fp, int(pol), 3, ctx.ptr(beams), 0, uv.ctypes.data_as(c_dbl_p), bi.ctypes.data_as(c_int_p),
                bj.ctypes.data_as(c_int_p), ctx.ptr(buf[PAD:]))
        ctx.sync()
        assert rc == 0 and _all_nan(_host(buf)), m.case
    assert not fails, "\n".join(fails)


def test_refusals(ctx):
    """Each of these calls returns an error whose text names the entry point, and writes nothing."""
    nside, zen = 3, "S"
    geo = pc.geometry(nside)
    npix = geo["npix"]
    keep, (cp, sp, fp) = _geo_ptrs(nside, zen)
    lib, h = ctx.lib, ctx.h
    tab = [np.ascontiguousarray(a) for a in pc.table("syn5", nside, zen)]
    tx, ty, t2 = (a.ctypes.data_as(c_dbl_p) for a in tab)
    null_d, null_i, null_v = c_dbl_p(), c_int_p(), ctypes.c_void_p(0)
    out = _poisoned(ctx, 4 * npix)
    op = ctx.ptr(out[PAD:])
    seen = []

    def refused(name, rc):
        msg = lib.dm_last_error(h).decode()
        assert rc < 0 and name in msg, (name, rc, msg)
        seen.append(name)

    # dm_bt_beam_cyl: one knot, an unknown kind, null pointers
    refused("dm_bt_beam_cyl", lib.dm_bt_beam_cyl(h, nside, cp, sp, fp, 1, tx, ty, t2, 1, 0.5, op))
    refused("dm_bt_beam_cyl", lib.dm_bt_beam_cyl(h, nside, cp, sp, fp, 3, tx, ty, t2, 5, 0.5, op))
    refused("dm_bt_beam_cyl", lib.dm_bt_beam_cyl(h, nside, cp, sp, fp, -1, tx, ty, t2, 5, 0.5, op))
    refused("dm_bt_beam_cyl", lib.dm_bt_beam_cyl(h, nside, cp, sp, fp, 1, tx, ty, t2, 5, 0.5, null_v))
    refused("dm_bt_beam_cyl", lib.dm_bt_beam_cyl(h, nside, cp, sp, fp, 1, null_d, ty, t2, 5, 0.5, op))
    refused("dm_bt_beam_cyl", lib.dm_bt_beam_cyl(h, nside, null_d, sp, fp, 1, tx, ty, t2, 5, 0.5, op))
    refused("dm_bt_beam_cyl", lib.dm_bt_beam_cyl(h, nside, cp, sp, null_d, 1, tx, ty, t2, 5, 0.5, op))
    # dm_bt_beams_cyl: two beams sharing the table; the second one with an unknown kind, with one knot, in rows too short
    fw = np.array([0.5, 0.7])
    fwp = fw.ctypes.data_as(c_dbl_p)

    def beams(kinds, offs, stride, o=op, k_null=False, t_null=False):
        k, of = np.array(kinds, dtype=np.int32), np.array(offs, dtype=np.int32)
        return lib.dm_bt_beams_cyl(h, nside, cp, sp, fp, 2, null_i if k_null else k.ctypes.data_as(c_int_p), null_d if t_null else tx,
                                   ty, t2, of.ctypes.data_as(c_int_p), fwp, o, stride)

    refused("dm_bt_beams_cyl", beams([0, 3], [0, 2, 5], 2 * npix))
    refused("dm_bt_beams_cyl", beams([0, 1], [0, 4, 5], 2 * npix))
    refused("dm_bt_beams_cyl", beams([0, 1], [0, 2, 5], 2 * npix - 1))
    refused("dm_bt_beams_cyl", beams([0, 0], [0, 2, 5], npix - 1))
    refused("dm_bt_beams_cyl", beams([0, 1], [0, 2, 5], 2 * npix, o=null_v))
    refused("dm_bt_beams_cyl", beams([0, 1], [0, 2, 5], 2 * npix, k_null=True))
    refused("dm_bt_beams_cyl", beams([0, 1], [0, 2, 5], 2 * npix, t_null=True))
    ctx.sync()
    assert _all_nan(_host(out))
    assert beams([0, 1], [0, 2, 5], 2 * npix) == 0            # (the same call is accepted with nothing wrong)
    ctx.sync()
    good = _host(out)
    assert _all_nan(good[:PAD]) and np.isfinite(good[PAD : PAD + npix]).all() and np.isfinite(good[PAD + 2 * npix : PAD + 4 * npix]).all()
    assert _all_nan(good[PAD + npix : PAD + 2 * npix]) and _all_nan(good[PAD + 4 * npix :])
    # dm_bt_maps / dm_bt_maps_c: a beam index out of range in either list, null pointers
    uv = np.ascontiguousarray(pc.map_columns()[0][:2])
    uvp = uv.ctypes.data_as(c_dbl_p)
    for name, dt in (("dm_bt_maps", np.float64), ("dm_bt_maps_c", np.complex128)):
        fn = getattr(lib, name)
        bdev = ctx.zeros((2, npix), dt)
        mout = _poisoned(ctx, 2 * npix, np.complex128)
        mp = ctx.ptr(mout[PAD:])

        def call(bi, bj, b=None, o=mp, u=uvp, i_null=False):
            i_, j_ = np.array(bi, dtype=np.int32), np.array(bj, dtype=np.int32)
            return fn(h, nside, cp, sp, fp, 0, 2, ctx.ptr(bdev) if b is None else b, 2, u, null_i if i_null else i_.ctypes.data_as(c_int_p),
                      j_.ctypes.data_as(c_int_p), o)

        refused(name, call([0, 2], [1, 1]))
        refused(name, call([0, 1], [1, -1]))
        refused(name, call([-1, 1], [1, 0]))
        refused(name, call([0, 1], [2, 0]))
        refused(name, call([0, 1], [1, 0], b=null_v))
        refused(name, call([0, 1], [1, 0], o=null_v))
        refused(name, call([0, 1], [1, 0], u=null_d))
        refused(name, call([0, 1], [1, 0], i_null=True))
        ctx.sync()
        assert _all_nan(_host(mout)), name
    assert set(seen) == {"dm_bt_beam_cyl", "dm_bt_beams_cyl", "dm_bt_maps", "dm_bt_maps_c"}
    # a null context has no message to carry
    assert lib.dm_bt_beam_cyl(ctypes.c_void_p(0), nside, cp, sp, fp, 1, tx, ty, t2, 5, 0.5, op) < 0
