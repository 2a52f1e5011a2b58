"""The spherical-harmonic transforms on the device against exact lambda_lm, W_lm, X_lm (tests/golden/legendre_exact*.npz:
a 50+ digit mpmath evaluation by another route than the package's recurrence, tests/gen_golden_legendre.py) — every
other SHT test compares the device with a host copy of the same recurrence.

Analysis: a map that is sum_m exp(-i m phi_j) on the pixels of ONE ring and zero elsewhere has the coefficients
c_lm' = w G_m' lambda_lm'(z_ring), G_m' = sum_j f_j exp(i m' phi_j) — N_ring where m' is one of the m, and on rings with
N_ring <= m + m' also where m' = +-m (mod N_ring), nothing elsewhere; the same pattern in Q and U gives W and X through
[[W, -iX], [iX, W]].  Each coefficient is divided by w G_m' (by w N_ring where G_m' = 0) and its real and imaginary parts
are held to the fixture within BOUND[lmax] (tests/legendre_cases.py: 8 x the measured error of the float64 recurrence
where nothing underflows).  Both m-slots of a block are checked (slot 1 holds (-1)^m conj(c_l,-m)), and the entries with
l < m' or l > col_lmax must be exact zeros.  Synthesis: one unit coefficient per map.  No magnitude decides what is compared.

The columns of (nside 1024, lmax 2047, m 696..703) on rings 438 and 3656 are the ones whose seed exp(m ln sin theta)
underflows: the tables held exact zeros there before the seed was carried with its own exponent, against true values
up to 1.36.  They are held to the bound of lmax 2047, measured on the belt ring 1500."""
import numpy as np
import pytest

import legendre_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fx(golden_dir):
    return lc.Exact(golden_dir)


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    # nside 1024, 16 m-values: twiddles 2 x 16 x 12.6 M pixels (6.4 GB) + one table of 0.7 GB; 8 m-values polarised:
    # 3.2 GB + three tables of 0.35 GB
    c = Context(0, workspace_bytes=10 << 30)
    yield c
    c.close()


# ---- ring patterns with exactly reduced phases: phi_j = pi (k0 + 2 j) / N with k0 = 0 or 1 on every HEALPix ring -------
def _layout(nside):
    from driftscan_amd import healpix

    nphi, phi0, start = healpix.ring_layout(nside)
    k0 = (phi0 != 0.0).astype(np.int64)
    assert np.array_equal(phi0, k0 * (np.pi / nphi))
    return nphi, k0, start


def _cis(mm, n, k0):
    """exp(i mm phi_j), j < n: the phase pi (mm (k0 + 2 j) mod 2 n) / n is formed from an exact integer."""
    q = (int(mm) * (k0 + 2 * np.arange(n, dtype=np.int64))) % (2 * n)
    a = np.pi * q / n
    return np.cos(a) + 1j * np.sin(a)


def _pattern(ms, n, k0):
    return sum(_cis(-m, n, k0) for m in ms)


def _ring_sum(ms, mp, n, k0, sign):
    """G = sum_j f_j exp(sign i mp phi_j) of the pattern of `ms`: exactly zero unless some m = sign mp (mod n)."""
    if not any((sign * mp - m) % n == 0 for m in ms):
        return None
    return complex(np.sum(_pattern(ms, n, k0) * _cis(sign * mp, n, k0)))


def _expected(fx, nside, lfix, mp, ring, cl, amp, pol):
    """Normalised coefficients (P, cl + 1 - mp) of a column with Stokes amplitudes amp = (T, Q, U, V) — the same for both
    m-slots: slot 1 = (-1)^m conj(c_l,-m) = w conj(G_-m) (lambda | aQ W - i aU X | aU W + i aQ X)."""
    lam, W, X = [t[: cl + 1 - mp] for t in fx.column(nside, lfix, mp, ring)]
    if not pol:
        return (amp[0] * lam)[None].astype(np.complex128)
    return np.stack([amp[0] * lam, amp[1] * W - 1j * amp[2] * X, amp[2] * W + 1j * amp[1] * X, amp[3] * lam])


def _check_blocks(fx, bm, nside, cols, pol, m_lo, scale=None, need_all=True):
    """bm (nm, ncol, 2, 1, P, L) from the device against the fixture.  cols: [(ring, ms, col_lmax, lfix, amp)];
    scale[c]: what the maps of column c were multiplied by.  Returns the number of (column, m', slot) rows with G != 0 compared."""
    nphi, k0, _ = _layout(nside)
    w = 4.0 * np.pi / (12 * nside * nside)
    nm, ncol, _, _, P, L = bm.shape
    div = np.empty((nm, ncol, 2), dtype=np.complex128)
    exp_ = np.zeros(bm.shape, dtype=np.complex128)
    known = np.ones((nm, ncol, 2), dtype=bool)
    nrows = 0
    bound = np.empty(ncol)
    keep = np.zeros((nm, ncol, L), dtype=bool)             # l in [m', col_lmax]
    for c, (ring, ms, cl, lfix, amp) in enumerate(cols):
        n, k = int(nphi[ring]), int(k0[ring])
        sc = w * (1.0 if scale is None else scale[c])
        div[:, c, :] = sc * n
        bound[c] = lc.BOUND[lfix]
        for i in range(nm):
            mp = m_lo + i
            if mp > cl:
                continue
            keep[i, c, mp : cl + 1] = True
            for s, sign in ((0, +1), (1, -1)):
                G = _ring_sum(ms, mp, n, k, sign)
                if G is None or (s == 1 and mp == 0):       # (the m = 0 block has no second slot)
                    continue
                if not fx.has(nside, lfix, mp, ring):
                    assert not need_all, (nside, lfix, mp, ring)
                    known[i, c, s] = False
                    continue
                div[i, c, s] = sc * (G if s == 0 else np.conj(G))
                exp_[i, c, s, 0, :, mp : cl + 1] = _expected(fx, nside, lfix, mp, ring, cl, amp, pol)
                nrows += 1
    assert np.isfinite(bm.view(np.float64)).all()
    # exact zeros below l = m' and above the column's band limit, in every block and slot
    out = ~keep[:, :, None, None, None, :]
    assert not (bm * out).any(), "coefficients outside l in [m', col_lmax] must be exact zeros"
    err = bm / div[:, :, :, None, None, None] - exp_
    err = np.maximum(np.abs(err.real), np.abs(err.imag)) * known[:, :, :, None, None, None]
    per_col = err.max(axis=(0, 2, 3, 4, 5))
    worst = int(np.argmax(per_col / bound))
    print("nside %d, %d columns, m' %d..%d, pol %s: worst normalised error %.3e (column ring %d, m %s; bound %.2e)"
          % (nside, ncol, m_lo, m_lo + nm - 1, pol, per_col[worst], cols[worst][0], list(cols[worst][1])[:3], bound[worst]))
    assert (per_col <= bound).all(), (per_col[worst], bound[worst], cols[worst][:4])
    return nrows


def _run_analysis(ctx, nside, lside, maps, col_lmax, pol, m_range):
    from driftscan_amd import healpix

    cth, sth = healpix.ring_trig(nside)
    ncol = len(col_lmax)
    P = 4 if pol else 1
    m_lo, m_hi = (0, lside) if m_range is None else m_range
    bm = ctx.zeros((m_hi - m_lo + 1, ncol, 2, 1, P, lside + 1), np.complex128)
    ctx.bt_sht(nside, cth, sth, pol, lside, lside, int(max(col_lmax)), ncol, 1, np.arange(ncol), np.zeros(ncol, dtype=np.int64),
               np.asarray(col_lmax), maps, bm, m_range=m_range)
    ctx.sync()
    return bm.cpu().numpy(), m_lo


# ---- a. small and medium sizes: every (ring, m) of the fixture as a column -----------------------------------------------
AMPS = {"unpol": (1.0, 0.0, 0.0, 0.0), "Q": (1.0, 1.0, 0.0, 0.5), "U": (1.0, 0.0, 1.0, 0.5), "QU": (1.0, 1.0, 1.0, 0.5)}
# (nside, lside, [(col_lmax = fixture lmax)], narrow range (<= 8 m), wide range (> 8 m))
SMALL = {2: (11, (5, 11), (3, 8), (1, 11)), 8: (35, (23, 35), (20, 27), (5, 30)), 32: (95, (95,), (0, 3), (30, 50))}


@pytest.mark.parametrize("stokes", ["unpol", "Q", "U", "QU"])
@pytest.mark.parametrize("nside,route", [(n, r) for n in (2, 8, 32) for r in ("all", "narrow", "wide")] + [(32, "top")])
def test_ring_delta_analysis(ctx, fx, nside, route, stokes):
    """Context.bt_sht over all m, a narrow m-range (at most 8 values) and a wide one; at nside 32 also the last two m."""
    lside, lfixes, narrow, wide = SMALL[nside]
    m_range = {"all": None, "narrow": narrow, "wide": wide, "top": (94, 95)}[route]
    pol = stokes != "unpol"
    amp = AMPS[stokes]
    nphi, k0, start = _layout(nside)
    groups = fx.groups()
    cols = [(ring, (m,), lfix, lfix, amp) for lfix in lfixes for m, ring in groups[(nside, lfix)]]
    P = 4 if pol else 1
    maps = np.zeros((len(cols), P, 12 * nside * nside), dtype=np.complex128)
    for c, (ring, ms, cl, lfix, a) in enumerate(cols):
        f = _pattern(ms, int(nphi[ring]), int(k0[ring]))
        for p in range(P):
            maps[c, p, start[ring] : start[ring] + nphi[ring]] = a[p] * f
    bm, m_lo = _run_analysis(ctx, nside, lside, ctx.to_device(maps), [c[2] for c in cols], pol, m_range)
    # nside 32 holds a few m only: a polar ring aliases its pattern onto m' the fixture does not have
    n = _check_blocks(fx, bm, nside, cols, pol, m_lo, need_all=nside != 32)
    assert n >= (2 if route == "top" else len(cols) // 8)


# ---- b, c. production scale and the underflow regime: one ring per column, the maps built on the device ------------------
def _device_ring_maps(ctx, nside, cols, pol):
    """(ncol, P, npix) c128 on the device, column c = amp[p] x the pattern of its m on its ring."""
    torch = ctx.torch
    nphi, k0, start = _layout(nside)
    P = 4 if pol else 1
    maps = ctx.zeros((len(cols), P, 12 * nside * nside), np.complex128)
    for c, (ring, ms, cl, lfix, amp) in enumerate(cols):
        n, k = int(nphi[ring]), int(k0[ring])
        j = torch.arange(n, dtype=torch.int64, device=maps.device)
        f = torch.zeros(n, dtype=torch.complex128, device=maps.device)
        for m in ms:
            a = (np.pi / n) * ((-int(m) * (k + 2 * j)) % (2 * n)).to(torch.float64)
            f += torch.complex(torch.cos(a), torch.sin(a))
        # the pattern the expectation is formed from is numpy's: the two differ by an ulp of the phase at most
        assert float((f.cpu() - torch.from_numpy(_pattern(ms, n, k))).abs().max()) < 1e-14 * len(ms)
        for p in range(P):
            maps[c, p, int(start[ring]) : int(start[ring]) + n] = amp[p] * f
    return maps


@pytest.mark.parametrize("case", [("narrow-0", (0, 7), (0, 2), "unpol"), ("wide-300", (292, 307), (300,), "unpol"),
                                  ("narrow-700", (696, 703), (700,), "unpol"),
                                  ("narrow-top", (1017, 1024), tuple(range(1017, 1025)), "unpol"),
                                  ("narrow-top-pol", (1017, 1024), tuple(range(1017, 1025)), "QU"),
                                  ("wide-top", (1005, 1024), tuple(range(1017, 1025)), "unpol")], ids=lambda c: c[0])
def test_production_scale_analysis(ctx, fx, case):
    """nside 512, lmax 1024: the listed m of a range on one ring per column (rings 0, 5, 100, 511, 700, 1023, 2046)."""
    _, m_range, ms, stokes = case
    nside, lmax = 512, 1024
    pol = stokes != "unpol"
    cols = [(ring, ms, lmax, lmax, AMPS[stokes]) for ring in (0, 5, 100, 511, 700, 1023, 2046)]
    maps = _device_ring_maps(ctx, nside, cols, pol)
    bm, m_lo = _run_analysis(ctx, nside, lmax, maps, [lmax] * len(cols), pol, m_range)
    del maps
    n = _check_blocks(fx, bm, nside, cols, pol, m_lo, need_all=False)
    assert n >= len(cols) * len(ms)


@pytest.mark.parametrize("case", [("narrow", (696, 703), "unpol"), ("narrow-pol", (696, 703), "QU"), ("wide", (688, 703), "unpol")],
                         ids=lambda c: c[0])
def test_underflow_regime_analysis(ctx, fx, case):
    """nside 1024, lmax 2047, m 696..703 on rings 438 and 3656 (seed below the smallest normal double) and 1500 (belt)."""
    _, m_range, stokes = case
    nside, lmax = 1024, 2047
    pol = stokes != "unpol"
    cols = [(ring, tuple(range(696, 704)), lmax, lmax, AMPS[stokes]) for ring in (438, 3656, 1500)]
    maps = _device_ring_maps(ctx, nside, cols, pol)
    bm, m_lo = _run_analysis(ctx, nside, lmax, maps, [lmax] * len(cols), pol, m_range)
    del maps
    n = _check_blocks(fx, bm, nside, cols, pol, m_lo)
    assert n == 3 * 8          # slot 0 of each m on each ring; m + m' < N_ring on all three: nothing aliases
    # the true functions are of order one on the two rings that used to be zeros
    i = 700 - m_lo
    assert np.abs(bm[i, 0, 0, 0, 0]).max() > 1.3 * (4.0 * np.pi / (12 * nside * nside)) * 1756


@pytest.mark.parametrize("wide", [False, True], ids=["narrow", "wide"])
@pytest.mark.parametrize("south", [False, True], ids=["north", "south"])
def test_underflow_regime_fused_path_with_ring_skip(ctx, fx, wide, south):
    """dm_bt_columns (maps formed inside the ring transform) with ring skipping on: bt_ring_skip_lookup drops the (m, ring)
    pairs whose table peak, from the host copy of the recurrence (bt_table_peak), is below 1e-18 — with an underflowed
    seed that peak was 0 and ring 438 was dropped for m 696..703.  Complex field patterns b_i = the ring pattern,
    b_j = 1 on the ring, no baseline, zenith at the pole of the ring's hemisphere: the map is the pattern over
    sqrt(Omega_i Omega_j).  Narrow call: matrix-form belt; wide call: FFT belt."""
    nside, lmax = 1024, 2047
    ms = tuple(range(696, 704))
    rings = (3656,) if south else (438, 1500)
    m_range = (688, 703) if wide else (696, 703)
    from driftscan_amd import healpix

    cth, sth = healpix.ring_trig(nside)
    nphi, k0, start = _layout(nside)
    npx = 12 * nside * nside
    w = 4.0 * np.pi / npx
    cols = [(ring, ms, lmax, lmax, AMPS["unpol"]) for ring in rings]
    pat = _device_ring_maps(ctx, nside, cols, False)[:, 0]            # (nring, npix)
    one = ctx.zeros((len(rings), npx), np.complex128)
    scale = []
    for c, ring in enumerate(rings):
        n = int(nphi[ring])
        one[c, int(start[ring]) : int(start[ring]) + n] = 1.0
        om_i = w * float(np.sum(np.abs(_pattern(ms, n, int(k0[ring]))) ** 2))
        scale.append(1.0 / np.sqrt(om_i * w * n))
    beams = ctx.torch.cat([pat, one]).contiguous()
    frame = np.array([0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, -1.0] if south else [0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    nc = len(rings)
    bm = ctx.zeros((m_range[1] - m_range[0] + 1, nc, 2, 1, 1, lmax + 1), np.complex128)
    ctx.bt_columns(nside, cth, sth, frame, False, beams, np.zeros((nc, 2)), np.arange(nc), nc + np.arange(nc), lmax, lmax, lmax,
                   nc, 1, np.arange(nc), np.zeros(nc, dtype=np.int64), np.full(nc, lmax), bm, m_range=m_range)
    ctx.sync()
    n = _check_blocks(fx, bm.cpu().numpy(), nside, cols, False, m_range[0], scale=scale)
    assert n == nc * 8


# ---- d. synthesis: one unit coefficient per map -------------------------------------------------------------------------
@pytest.mark.parametrize("pol", [False, True], ids=["T", "TEBV"])
@pytest.mark.parametrize("case", [(2, 5), (2, 11), (8, 23), (8, 35), (32, 95)], ids=lambda c: "nside%d-lmax%d" % c)
def test_unit_coefficient_synthesis(fx, case, pol):
    """healpix.sphtrans_inv_sky (dm_sht_synth) with a single coefficient per map, every (l, m) of the case batched as the
    frequency axis: T = c_m Re(a lambda_lm e^{i m phi}) (a = 1) and V the same with a = i; a unit E gives
    Q = c_m W cos(m phi), U = c_m X sin(m phi), a unit B gives Q = -c_m X sin(m phi), U = c_m W cos(m phi)
    (F_Q = W a_E + i X a_B, F_U = W a_B - i X a_E); c_0 = 1, c_m = 2.  lmax 11 and 35 exceed 3 nside - 1, and on the polar
    rings m reaches past the number of pixels."""
    from driftscan_amd import healpix

    nside, lmax = case
    nphi, k0, start = _layout(nside)
    cols = fx.groups()[case]
    msel = sorted(set(m for m, _ in cols))
    rings = sorted(set(r for _, r in cols))
    pairs = [(l, m) for m in msel for l in range(m, lmax + 1)]
    kinds = ("E", "B") if pol else ("T",)
    L = lmax + 1
    alm = np.zeros((len(pairs) * len(kinds), 4 if pol else 1, L, L), dtype=np.complex128)
    for k, kind in enumerate(kinds):
        for i, (l, m) in enumerate(pairs):
            f = k * len(pairs) + i
            alm[f, 0, l, m] = 1.0
            if pol:
                alm[f, 3, l, m] = 1.0j
                alm[f, 1 if kind == "E" else 2, l, m] = 1.0
    maps = healpix.sphtrans_inv_sky(alm, nside)
    assert maps.shape == (alm.shape[0], alm.shape[1], 12 * nside * nside) and np.isfinite(maps).all()
    worst = 0.0
    for ring in rings:
        n, k = int(nphi[ring]), int(k0[ring])
        seg = maps[:, :, start[ring] : start[ring] + n]
        for m in msel:
            e = _cis(m, n, k)
            cm = 1.0 if m == 0 else 2.0
            lam, W, X = fx.column(nside, lmax, m, ring)
            i0 = pairs.index((m, m))
            sl = slice(i0, i0 + L - m)
            ref_t = cm * lam[:, None] * e.real[None, :]
            for kk, kind in enumerate(kinds):
                got = seg[kk * len(pairs) :][sl]
                err = [np.abs(got[:, 0] - ref_t).max()]
                if pol:
                    wc, xs = cm * W[:, None] * e.real[None, :], cm * X[:, None] * e.imag[None, :]
                    q, u = (wc, xs) if kind == "E" else (-xs, wc)
                    err += [np.abs(got[:, 1] - q).max(), np.abs(got[:, 2] - u).max(),
                            np.abs(got[:, 3] + cm * lam[:, None] * e.imag[None, :]).max()]
                worst = max(worst, max(err))
                assert max(err) <= lc.BOUND[lmax], (ring, m, kind, err, lc.BOUND[lmax])
    print("synthesis nside %d lmax %d pol %s: worst |map - exact| %.3e, bound %.2e" % (nside, lmax, pol, worst, lc.BOUND[lmax]))
