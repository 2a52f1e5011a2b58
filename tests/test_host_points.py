"""CPU: a_lm evaluated at points (skysim.alm_at_points_host) against the extended-precision
restatement of tests/points_cases.py, the host synthesis at pixel centres and the adjoint identity with source_alm_host;
`stack_spectra` against a loop written out per source; the optional `redshift` of a catalogue; and the checker itself
against doctored answers."""
import numpy as np
import pytest

import points_cases as pc


# ---- the oracle against extended precision ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_oracle_against_extended_precision(case):
    from driftscan_amd import skysim

    npts, nf, npol, lmax, _ = case
    alm, theta, phi, ms, ref, bnd = pc.case_reference(case)
    got = skysim.alm_at_points_host(alm, theta, phi, ms=ms)
    assert got.shape == (npts, npol, nf) and got.dtype == np.float64
    r = pc.worst_ratio(got, ref, bnd)
    print("host %s: worst error / bound = %.3g" % (pc.case_id(case), r))
    assert r <= 0.05


@pytest.mark.parametrize("npol", [1, 4])
@pytest.mark.parametrize("nside,lmax", [(4, 11), (8, 23)])
def test_oracle_is_the_synthesis_at_pixel_centres(nside, lmax, npol):
    """`healpix.sphtrans_inv_sky_host` at every pixel centre: twice the bound (each route within it)."""
    from driftscan_amd import healpix, skysim

    ang = healpix.ang_positions(nside)
    alm = np.ascontiguousarray(pc.master_alm(lmax)[:2, : (1 if npol == 1 else 4)])
    mp = healpix.sphtrans_inv_sky_host(alm, nside)                       # (nf, npol, npix)
    got = skysim.alm_at_points_host(alm, ang[:, 0], ang[:, 1])
    a4 = pc.master_alm(lmax)[:2]
    _, bnd = pc.reference_of(pc.terms_ld(a4, ang[:, 0], ang[:, 1], list(range(lmax + 1))), list(range(lmax + 1)), npol, lmax)
    r = pc.worst_ratio(got, mp.transpose(2, 1, 0).astype(pc.LD), bnd)
    print("synthesis nside %d lmax %d npol %d: worst |delta| / bound = %.3g" % (nside, lmax, npol, r))
    assert r <= 2.0


@pytest.mark.parametrize("npol", [1, 4])
def test_adjoint_of_source_alm(npol):
    """sum_s F_s value(s) = sum_pol sum_l [Re(a_l0 b*_l0) + 2 sum_{m > 0} Re(a_lm b*_lm)] with b = source_alm_host(F)."""
    from driftscan_amd import skysim

    lmax, npts = 23, 65
    theta, phi = pc.points(npts, lmax)
    a = np.ascontiguousarray(pc.master_alm(lmax)[:3, : (1 if npol == 1 else 4)])   # (E, B at l < 2 meet W = X = 0 on both sides)
    rng = np.random.default_rng(5)
    F = rng.standard_normal((3, npol, npts))
    val = skysim.alm_at_points_host(a, theta, phi)                       # (npts, npol, nf)
    b = skysim.source_alm_host(theta, phi, F, lmax)
    lhs = np.einsum("fps,spf->", F, val)
    w = np.full(lmax + 1, 2.0)
    w[0] = 1.0
    rhs = np.sum((a * b.conj()).real * w)
    tol = 1e-12 * np.einsum("fps,spf->", np.abs(F), np.abs(val))
    print("adjoint npol %d: |lhs - rhs| = %.3g (tolerance %.3g)" % (npol, abs(lhs - rhs), tol))
    assert abs(lhs - rhs) <= tol


def test_partial_sums_add_up():
    from driftscan_amd import skysim

    case = (65, 3, 4, 23, None)
    alm, theta, phi, ms, ref, bnd = pc.case_reference(case)
    split = [list(range(0, 24, 3)), list(range(1, 24, 3)), list(range(23, 1, -3))]
    assert sorted(sum(split, [])) == ms
    tot = sum(skysim.alm_at_points_host(np.ascontiguousarray(alm[..., s]), theta, phi, ms=s) for s in split)
    assert pc.worst_ratio(tot, ref, bnd) <= 1.0
    whole = skysim.alm_at_points_host(alm, theta, phi)
    assert pc.worst_ratio(tot, whole.astype(pc.LD), bnd) <= 1.0


def test_oracle_refusals_and_edges():
    from driftscan_amd import skysim

    a = np.ones((2, 4, 6, 6), dtype=complex)
    with pytest.raises(ValueError, match="pole"):
        skysim.alm_at_points_host(a, [0.0, 1.0], [0.0, 0.0])
    with pytest.raises(ValueError, match="distinct"):
        skysim.alm_at_points_host(a[..., :2], [1.0], [0.0], ms=[1, 1])
    with pytest.raises(ValueError, match="distinct"):
        skysim.alm_at_points_host(a[..., :2], [1.0], [0.0], ms=[1, 6])
    with pytest.raises(ValueError, match="1 or 4"):
        skysim.alm_at_points_host(a[:, :2], [1.0], [0.0])
    # unpolarised at a pole: only m = 0 contributes, lambda_l0(1) = sqrt((2 l + 1) / 4 pi)
    v = skysim.alm_at_points_host(a[:, :1], [0.0], [0.3])
    assert np.allclose(v[0, 0], np.sqrt((2 * np.arange(6) + 1) / (4 * np.pi)).sum(), rtol=1e-14)
    assert skysim.alm_at_points_host(a, np.zeros(0), np.zeros(0)).shape == (0, 4, 2)
    # phi is reduced to [0, 2 pi)
    assert np.array_equal(skysim.alm_at_points_host(a, [1.0], [0.5 - 2 * np.pi]),
                          skysim.alm_at_points_host(a, [1.0], [np.mod(0.5 - 2 * np.pi, 2 * np.pi)]))


# ---- the checker ------------------------------------------------------------------------------------------------------------
def test_checker_rejects_doctored_answers():
    """A dropped m = 0 factor (m = 0 doubled like the others), a sign flip on X and a conjugated phase all leave the bound
    by orders of magnitude."""
    from driftscan_amd import healpix

    case = (65, 3, 4, 23, None)
    alm, theta, phi, ms, ref, bnd = pc.case_reference(case)
    z, ph = np.cos(theta), np.mod(phi, 2 * np.pi)

    def doctored(fac0=1.0, xsign=1.0, phsign=1.0):
        out = np.zeros((3, 4, z.size))
        for m in ms:
            lam = healpix.lambda_lm(23, m, z)
            W, X = healpix.wx_lm(23, m, z)
            X = xsign * X
            a = alm[:, :, m:, m]
            F = np.zeros((3, 4, z.size), dtype=complex)
            F[:, 0], F[:, 3] = a[:, 0] @ lam, a[:, 3] @ lam
            F[:, 1] = a[:, 1] @ W + 1j * (a[:, 2] @ X)
            F[:, 2] = a[:, 2] @ W - 1j * (a[:, 1] @ X)
            out += (fac0 if m == 0 else 2.0) * (F * np.exp(phsign * 1j * m * ph)).real
        return out.transpose(2, 1, 0)

    assert pc.worst_ratio(doctored(), ref, bnd) <= 0.05
    for kw in (dict(fac0=2.0), dict(xsign=-1.0), dict(phsign=-1.0)):
        r = pc.worst_ratio(doctored(**kw), ref, bnd)
        print("doctored %s: worst error / bound = %.3g" % (kw, r))
        assert r > 100.0


# ---- catalogues with redshifts ----------------------------------------------------------------------------------------------
def test_catalogue_redshift_is_optional(tmp_path):
    from driftscan_amd import skysim, storage

    cat = skysim.random_catalogue(7, 3)
    plain = str(tmp_path / "plain.hdf5")
    skysim.write_catalogue(plain, cat)
    back = skysim.read_catalogue(plain)
    assert sorted(back) == sorted(skysim._CAT_KEYS) and "redshift" not in back
    with storage.File(plain, "r") as f:
        assert "redshift" not in f
    assert skysim.read_positions(plain)[2] is None
    cat["redshift"] = np.linspace(0.8, 2.5, 7)
    withz = str(tmp_path / "withz.hdf5")
    skysim.write_catalogue(withz, cat)
    back = skysim.read_catalogue(withz)
    assert np.array_equal(back["redshift"], cat["redshift"])
    th, ph, red = skysim.read_positions(withz)
    assert np.array_equal(th, cat["theta"]) and np.array_equal(ph, cat["phi"]) and np.array_equal(red, cat["redshift"])
    assert skysim.read_positions((th, ph))[2] is None
    with pytest.raises(ValueError, match="redshift"):
        skysim.read_catalogue(dict(cat, redshift=np.zeros(3)))
    # the spectra of the simulations do not look at it
    nu = np.array([400.0, 500.0])
    assert np.array_equal(skysim.source_spectra(cat, nu), skysim.source_spectra(plain, nu))


# ---- the stack ----------------------------------------------------------------------------------------------------------------
def _stack_loop(T, nu, line, K, w=None, om=None):
    """stack_spectra written out per source."""
    nsrc, npol, nf = T.shape
    w = np.ones(nsrc) if w is None else w
    om = np.ones(nf) if om is None else om
    num, den, hits = np.zeros((npol, 2 * K + 1)), np.zeros(2 * K + 1), np.zeros(2 * K + 1, dtype=np.int64)
    chan = np.full(nsrc, -1)
    lo, hi = (0, nf - 1) if nu[1] > nu[0] else (nf - 1, 0)
    for s in range(nsrc):
        if line[s] < nu[lo] - 0.5 * abs(nu[1] - nu[0] if lo == 0 else nu[-1] - nu[-2]):
            continue
        if line[s] > nu[hi] + 0.5 * abs(nu[-1] - nu[-2] if hi == nf - 1 else nu[1] - nu[0]):
            continue
        c = int(np.argmin(np.abs(nu - line[s])))
        chan[s] = c
        for k in range(-K, K + 1):
            if 0 <= c + k < nf and w[s] * om[c + k] > 0.0:
                num[:, k + K] += w[s] * om[c + k] * T[s, :, c + k]
                den[k + K] += w[s] * om[c + k]
                hits[k + K] += 1
    return np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0), hits, den, chan


@pytest.mark.parametrize("descending", [False, True])
def test_stack_against_the_loop(descending):
    from driftscan_amd import skysim

    rng = np.random.default_rng(8 + descending)
    nf, nsrc, K = 16, 40, 3
    nu = 400.0 + 2.0 * np.arange(nf) + 0.1 * rng.uniform(-1, 1, nf)      # channels of slightly uneven width
    if descending:
        nu = nu[::-1].copy()
    line = rng.uniform(nu.min() - 3.0, nu.max() + 3.0, nsrc)
    half_lo = 0.5 * abs(nu[1] - nu[0]) if not descending else 0.5 * abs(nu[-1] - nu[-2])
    half_hi = 0.5 * abs(nu[-1] - nu[-2]) if not descending else 0.5 * abs(nu[1] - nu[0])
    # at the edges of the band: just inside and just outside, both ends
    line[:4] = [nu.min() - half_lo * 0.999, nu.min() - half_lo * 1.001, nu.max() + half_hi * 0.999, nu.max() + half_hi * 1.001]
    T = rng.standard_normal((nsrc, 4, nf))
    w = rng.uniform(0.0, 2.0, nsrc)
    w[5] = 0.0
    om = rng.uniform(0.5, 1.5, nf)
    om[[3, 9]] = 0.0
    for kw in (dict(), dict(source_weight=w), dict(channel_weight=om), dict(source_weight=w, channel_weight=om)):
        got = skysim.stack_spectra(T, nu, line, K, **kw)
        st, hits, den, chan = _stack_loop(T, nu, line, K, kw.get("source_weight"), kw.get("channel_weight"))
        assert np.array_equal(got["channel"], chan) and np.array_equal(got["hits"], hits)
        assert np.array_equal(got["offsets"], np.arange(-K, K + 1))
        assert np.allclose(got["weight"], den, rtol=1e-13, atol=0) and np.allclose(got["stack"], st, rtol=1e-12, atol=1e-14)
    assert list(chan[:4] >= 0) == [True, False, True, False]
    assert (chan < 0).sum() > 2 and (chan >= 0).sum() > 20


def test_stack_of_planted_lines():
    """A unit line planted in the channel of every source on top of nothing comes back as 1 at k = 0 and 0 elsewhere;
    channels without weight and sources outside the band do not enter."""
    from driftscan_amd import skysim

    rng = np.random.default_rng(2)
    nf, nsrc, K = 32, 200, 4
    nu = np.linspace(800.0, 400.0, nf)                                    # descending, as CHIME-like bands are stored
    red = rng.uniform(0.7, 2.7, nsrc)
    line = skysim.LINE_21CM_MHZ / (1.0 + red)
    chan = np.argmin(np.abs(nu[None] - line[:, None]), axis=1)
    inside = (line >= 400.0 - 0.5 * abs(nu[1] - nu[0])) & (line <= 800.0 + 0.5 * abs(nu[1] - nu[0]))
    assert inside.sum() > 50 and (~inside).sum() > 5
    T = np.zeros((nsrc, 1, nf))
    T[np.arange(nsrc), 0, chan] = 1.0
    T[~inside] = 1e6                                                       # dropped sources must not leak in
    om = np.ones(nf)
    om[10] = 0.0
    T[:, :, 10] = np.where(T[:, :, 10] == 0.0, 5e5, T[:, :, 10])           # neither must a channel without weight
    got = skysim.stack_spectra(T, nu, line, K, channel_weight=om)
    want = np.zeros(2 * K + 1)
    want[K] = 1.0
    assert np.array_equal(got["stack"][0], want)
    assert got["hits"][K] == np.count_nonzero(inside & (chan != 10))
    assert np.array_equal(got["channel"] >= 0, inside)
    # nothing kept: zeros, no division by zero
    none = skysim.stack_spectra(T, nu, np.full(nsrc, 100.0), K)
    assert not none["stack"].any() and not none["hits"].any() and not none["weight"].any()


def test_stack_refusals():
    from driftscan_amd import skysim

    T = np.zeros((2, 1, 4))
    nu = np.array([1.0, 2.0, 3.0, 4.0])
    for bad in (dict(freqs_mhz=np.array([1.0, 3.0, 2.0, 4.0])), dict(halfwidth=-1), dict(line_mhz=np.zeros(3)),
                dict(source_weight=np.array([1.0, -1.0])), dict(channel_weight=np.ones(3)), dict(freqs_mhz=np.ones(1), spectra=T[..., :1])):
        kw = dict(spectra=T, freqs_mhz=nu, line_mhz=np.array([2.0, 3.0]), halfwidth=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            skysim.stack_spectra(**kw)
