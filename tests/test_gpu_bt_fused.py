"""The fused ring transform of beam-transfer generation (`Context.bt_columns`: dm_bt_columns / dm_bt_columns_c) against
the reference and the per-element bound of tests/bt_fused_cases.py, one call per case: every instantiation that
`bt_ring_fused` can pick (six matrix-form rows, nine FFT rows, each for real and complex patterns — held to the table
by test_host_bt_fused_cases.py) on rings of up to 4096 pixels, ragged column counts, scattered (f, b) rows with ragged
band limits in a NaN-filled destination, ring weights, a ring length that is no power of two, and lmax 35.

`reference`: |got - ref| <= bound on the real and the imaginary part of EVERY element (m, slot, column, p, l); the
elements that must be exact zeros (l < m, l > col_lmax, slot 1 of m = 0, l > lmax_grp up to lside) have bound 0; rows of
(f, b) pairs that are not columns of the call keep their NaN, everything else is finite.
`routes` (the all-m case of a problem): two wide partitions of m give the bits of the all-m call; a narrow call differs
by at most 2e-13 of the largest coefficient (the figure of test_sht_m_range_matches_full); DM_BT_RING_SKIP=0 by at most
2e-16 (test_ring_skip_is_below_rounding); a repeated call gives the same bits.
`twocall` (complex patterns, four maps, nside 256): the same columns through bt_maps + bt_sht within the same bound.
DM_BT_FFT, DM_BT_FOLD and DM_BT_NARROW are read once per process and are not touched here.

Worst |got - ref| / bound of any element per group of cases, measured on an MI355X (no kernel had to be changed):

    long (nside 64 .. 512, P 1 / 4, real / complex, six m-ranges)   0.0087  (nside 256, one map, real, m 0..23)
    south (second zenith)                                           0.0031
    full (nside 1024: fft<1,16> real and complex; four maps, no FFT) 0.0025  (four maps)
    depth (nside 2 .. 32, 17 columns)                               0.0222  (nside 2, four maps, m 3..22)
    ragged (nside 4, 1 .. 520 columns)                              0.0165  (520 columns, four maps, m 8..15)
    scatter / ringw (nside 8; ringw also nside 128)                 0.0115
    belt (nside 48) / lmax35                                        0.0032 / 0.0028
    twocall (bt_maps + bt_sht, nside 256, complex, four maps)       0.0048
    routes: narrow against wide <= 8.7e-16, ring skip off <= 3.4e-19 of the largest coefficient; partitions and repeats bit-equal
"""
import numpy as np
import pytest

import bt_fused_cases as bc

pytestmark = pytest.mark.gpu

ROUTE_GROUPS = ("long", "south", "full", "depth", "ringw", "belt", "lmax35", "scatter")
TWOCALL = "long-n256-P4-c-c5-m0_23"


def _params():
    out = []
    for case in bc.CASES:
        out.append((case["name"], "reference"))
        if case["m_range"] == (0, case["lmax"]):
            if case["group"] in ROUTE_GROUPS or case["ncol"] == 520:
                out.append((case["name"], "routes"))
            if case["name"] == TWOCALL:
                out.append((case["name"], "twocall"))
    return out


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=2 << 30)
    yield c
    c.close()


_DEV = {}


def _device_beams(ctx, prob):
    """The patterns of a problem on the device, kept for the cases that share the problem."""
    if _DEV.get("prob") is not prob:
        _DEV.clear()
        _DEV.update(prob=prob, beams=ctx.to_device(np.ascontiguousarray(prob.beams)))
    return _DEV["beams"]


def _trig(nside):
    from driftscan_amd import healpix

    return healpix.ring_trig(nside)


def _run(ctx, prob, m_range):
    """One call: (nm, F, 2, B, P, L) on the host, from a destination filled with NaN."""
    cth, sth = _trig(prob.nside)
    m_lo, m_hi = m_range
    shape = (m_hi - m_lo + 1, prob.F, 2, prob.B, prob.P, prob.lside + 1)
    bm = ctx.to_device(np.full(shape, complex(np.nan, np.nan)))
    ctx.bt_columns(prob.nside, cth, sth, prob.frame, prob.P == 4, _device_beams(ctx, prob), prob.uv, prob.bi, prob.bj, prob.lside,
                   prob.lmax, prob.lmax, prob.F, prob.B, prob.col_f, prob.col_b, prob.col_lmax, bm, m_range=m_range,
                   ring_w=prob.ring_w)
    ctx.sync()
    return bm.cpu().numpy()


def _check_layout(bm, prob, m_lo):
    """The exact conditions of a block array as the device left it."""
    used = np.zeros((prob.F, prob.B), dtype=bool)
    used[prob.col_f, prob.col_b] = True
    rest = bm.transpose(0, 1, 3, 2, 4, 5)[:, ~used]            # (nm, pairs, 2, P, L): never touched
    assert np.isnan(rest.real).all() and np.isnan(rest.imag).all(), "rows that are no columns of the call must keep their NaN"
    got = bc.gather(bm, prob)                                  # (nm, 2, ncol, P, L)
    assert np.isfinite(got.view(np.float64)).all()
    l = np.arange(prob.lside + 1)
    for i in range(got.shape[0]):
        assert not got[i][..., l < m_lo + i].any(), "l < m must be exact zeros"
    assert not got[..., prob.lmax + 1 :].any(), "l > lmax_grp must be exact zeros"
    for c in range(prob.ncol):
        assert not got[:, :, c, :, prob.col_lmax[c] + 1 :].any(), "l > col_lmax must be exact zeros"
    if m_lo == 0:
        assert not got[0, 1].any(), "slot 1 of m = 0 must be exact zeros"
    return got


def _against_reference(got, prob, m_range, what):
    ref, bound = prob.expected(m_range)
    ratio, ok = bc.worst_ratio(got, ref, bound)
    print("%s: worst |got - ref| / bound = %.4f (%d elements, largest bound %.2e of the largest coefficient; reference %.1f s)"
          % (what, ratio, got.size, bound.max() / np.abs(ref).max(), prob.seconds))
    assert ok, (what, ratio)


@pytest.mark.parametrize("name,check", _params())
def test_case(ctx, name, check, monkeypatch):
    case = bc.BY_NAME[name]
    prob = bc.problem(case)
    m_range = case["m_range"]
    assert prob.horizon_margin >= bc.HORIZON_MIN
    if check == "reference":
        got = _check_layout(_run(ctx, prob, m_range), prob, m_range[0])
        _against_reference(got, prob, m_range, name)
        return
    if check == "twocall":
        cth, sth = _trig(prob.nside)
        beams = _device_beams(ctx, prob)
        maps = ctx.empty((prob.ncol, prob.P, 12 * prob.nside**2), np.complex128)
        ctx.bt_maps(prob.nside, cth, sth, prob.frame, prob.P == 4, beams, prob.uv, prob.bi, prob.bj, maps)
        bm = ctx.to_device(np.full((m_range[1] - m_range[0] + 1, prob.F, 2, prob.B, prob.P, prob.lside + 1), complex(np.nan, np.nan)))
        ctx.bt_sht(prob.nside, cth, sth, prob.P == 4, prob.lside, prob.lmax, prob.lmax, prob.F, prob.B, prob.col_f, prob.col_b,
                   prob.col_lmax, maps, bm, m_range=m_range)
        ctx.sync()
        got = _check_layout(bm.cpu().numpy(), prob, m_range[0])
        _against_reference(got, prob, m_range, name + " through bt_maps + bt_sht")
        return
    # routes: the same inputs through other calls
    lmax = prob.lmax
    full = _run(ctx, prob, (0, lmax))
    scale = np.abs(bc.gather(full, prob)).max()
    again = _run(ctx, prob, (0, lmax))
    assert np.array_equal(full, again, equal_nan=True), "a repeated call must give the same bits"
    cut = (lmax + 1) // 2
    for lo, hi in ((0, cut - 1), (cut, lmax)):
        assert hi - lo + 1 > 8
        part = _run(ctx, prob, (lo, hi))
        assert np.array_equal(part, full[lo : hi + 1], equal_nan=True), ("wide partitions must give the bits of the all-m call", lo, hi)
    worst = 0.0
    for lo, hi in ((8, 15), (9, 12), (20, 21), (lmax, lmax)):
        part = bc.gather(_run(ctx, prob, (lo, hi)), prob)
        d = np.abs(part - bc.gather(full[lo : hi + 1], prob)).max() / scale
        worst = max(worst, d)
        assert d <= 2e-13, ("narrow against wide", lo, hi, d)
    monkeypatch.setenv("DM_BT_RING_SKIP", "0")
    every = _run(ctx, prob, (0, lmax))
    monkeypatch.delenv("DM_BT_RING_SKIP")
    dskip = np.abs(bc.gather(every, prob) - bc.gather(full, prob)).max() / scale
    print("%s: narrow against wide %.2e, ring skip off %.2e of the largest coefficient" % (name, worst, dskip))
    assert dskip <= 2e-16, dskip
