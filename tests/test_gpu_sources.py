"""GPU: exact a_lm of point sources (dm_source_alm through driftscan_amd/skysim.py) — the tables
and the E / B signs against the exact Legendre fixture, the sums against the host oracle within the bound of
tests/sources_cases.py, against the ring analysis of single pixels, bits independent of the memory budget, refusals, and
the `sources=` keyword of the timestream simulations on the products of a small polarised cylinder."""
import numpy as np
import pytest

import legendre_cases as lc
import sources_cases as sc

pytestmark = pytest.mark.gpu


def _ctx():
    from driftscan_amd import device

    return device.get_context()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return lc.Exact(golden_dir)


# ---- exact values ---------------------------------------------------------------------------------------------------------
GROUPS = [(2, 5), (2, 11), (8, 23), (8, 35), (32, 95), (512, 1024), (1024, 2047)]


@pytest.mark.parametrize("nside,lmax", GROUPS, ids=lambda v: str(v))
def test_exact_tables_and_signs(fx, nside, lmax):
    """Sources at the fixture's rings (phi = 0), "frequency" f holding source f alone with unit I, then unit Q, then unit U
    (3 n frequencies of one call per m): T = lambda; Q gives E = W, B = -i X; U gives B = W, E = i X — within BOUND[lmax],
    absolute, against values no code of this package produced.  The columns of lmax 2047 with m 696..703 on rings 438 and
    3656 are those whose seed underflows."""
    from driftscan_amd import healpix, skysim

    cols = fx.groups()[(nside, lmax)]
    z = healpix.ring_z(nside)
    bound = lc.BOUND[lmax]
    worst, ncol = 0.0, 0
    for m in sorted(set(c[0] for c in cols)):
        rings = [r for mm, r in cols if mm == m]
        n = len(rings)
        theta = np.arccos(z[rings])                           # as pix2ang and `healpix.ring_trig` place a ring
        flux = np.zeros((3 * n, 4, n))
        for k, p in enumerate((0, 1, 2)):
            flux[k * n + np.arange(n), p, np.arange(n)] = 1.0
        a = skysim.source_alm((theta, np.zeros(n), flux), lmax, m_range=(m, m))
        assert a.shape == (3 * n, 4, lmax + 1, 1) and np.isfinite(a.view(np.float64)).all()
        assert not a[:, :, :m].any() and not a[:, 3].any()
        # the unpolarised entry on the same sources
        t = skysim.source_alm((theta, np.zeros(n), np.ascontiguousarray(flux[:n, :1])), lmax, m_range=(m, m))
        assert np.array_equal(t[:, 0], a[:n, 0])
        a = a[:, :, m:, 0]
        zero = np.zeros(lmax + 1 - m)
        for s, ring in enumerate(rings):
            lam, W, X = fx.column(nside, lmax, m, ring)
            want = {0: (lam, zero, zero), 1: (zero, W, -1j * X), 2: (zero, 1j * X, W)}
            for k in range(3):
                for p in range(3):
                    d = a[k * n + s, p] - want[k][p]
                    worst = max(worst, float(np.abs(d.real).max()), float(np.abs(d.imag).max()))
            ncol += 1
    print("exact nside %d lmax %d: %d columns, worst |delta| = %.3e (bound %.2e)" % (nside, lmax, ncol, worst, bound))
    assert ncol == len(cols) and worst <= bound
    if lmax == 2047:   # the underflow columns are of order one, not zeros
        theta = np.arccos(z[[438]])
        a = skysim.source_alm((theta, np.zeros(1), np.ones((1, 1, 1))), lmax, m_range=(700, 700))
        assert np.abs(a).max() > 1.3


# ---- against the host oracle ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sc.CASES, ids=sc.case_id)
def test_against_the_host_oracle(case):
    """Random pixel centres of nside 8 with phi offsets: per element within the bound of sources_cases.py of the host
    oracle, and of the extended-precision restatement the host oracle is held to by test_host_sources.py."""
    from driftscan_amd import skysim

    assert skysim.SOURCE_CHUNK == 1024
    nsrc, nf, npol, lmax, mmax, mr = case
    theta, phi, flux, m_lo, m_hi, re, im, bnd = sc.case_reference(case)
    got = skysim.source_alm((theta, phi, flux), lmax, mmax=mmax, m_range=mr)
    assert got.shape == (nf, npol, lmax + 1, m_hi - m_lo + 1)
    r = sc.worst_ratio(got, re, im, bnd)
    host = skysim.source_alm_host(theta, phi, flux, lmax, mmax=mmax, m_range=mr)
    rh = sc.worst_ratio(got, host.real.astype(sc.LD), host.imag.astype(sc.LD), bnd)
    print("device %s: worst error / bound = %.3g (against the host oracle %.3g)" % (sc.case_id(case), r, rh))
    assert rh <= 1.0 and r <= 1.0
    for m in range(m_lo, m_hi + 1):   # l < m: exact zeros
        assert not got[:, :, :m, m - m_lo].any()
    if npol == 4:
        assert not got[:, 1:3, :2].any()


def test_device_tensor_and_frequency_rows():
    """to_host=False hands back the device tensor; `freqs` computes those rows, with the bits of the full call."""
    from driftscan_amd import skysim

    theta, phi, flux, *_ = sc.case_reference((65, 3, 4, 23, None, None))
    full = skysim.source_alm((theta, phi, flux), 23)
    d = skysim.source_alm((theta, phi, flux), 23, freqs=[0, 2], to_host=False)
    assert d.is_cuda and tuple(d.shape) == (2, 4, 24, 24)
    assert np.array_equal(d.cpu().numpy(), full[[0, 2]])
    cat = skysim.random_catalogue(40, 3, pol_frac=0.1)
    nu = np.array([400.0, 410.0, 420.0])
    a = skysim.source_alm(cat, 11, frequencies=nu, mmax=7)
    b = skysim.source_alm((cat["theta"], cat["phi"], skysim.source_spectra(cat, nu)), 11, mmax=7)
    assert a.shape == (3, 4, 12, 8) and np.array_equal(a, b)
    assert not skysim.source_alm((np.zeros(0), np.zeros(0), np.zeros((2, 4, 0))), 5).any()


# ---- independent device route --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npol", [1, 4])
@pytest.mark.parametrize("nside,lmax", [(4, 11), (8, 23)])
def test_ring_analysis_of_single_pixels(nside, lmax, npol):
    """`healpix.sphtrans_sky` (the ring analysis with plain quadrature) of a map with 5 non-zero pixels is `source_alm` of
    their centres with flux f 4 pi / npix: twice the bound (each route within it)."""
    from driftscan_amd import healpix, skysim

    mp, pix, val = sc.five_pixel_map(nside, npol, 11 * nside + npol)
    ang = healpix.ang_positions(nside)
    w = 4.0 * np.pi / (12 * nside * nside)
    flux = np.ascontiguousarray((w * val)[None])
    got = skysim.source_alm((ang[pix, 0], ang[pix, 1], flux), lmax)
    ring = healpix.sphtrans_sky(mp, lmax)
    assert ring.shape == got.shape == (1, npol, lmax + 1, lmax + 1)
    f4 = flux if npol == 4 else np.concatenate([flux, np.zeros((1, 3, 5))], axis=1)
    _, _, tabmax = sc.alm_ld(ang[pix, 0], ang[pix, 1], f4, lmax, 0, lmax)
    bnd = sc.bound(flux, lmax, tabmax)
    r = sc.worst_ratio(got, ring.real.astype(sc.LD), ring.imag.astype(sc.LD), bnd)
    print("ring analysis nside %d lmax %d npol %d: worst |delta| / bound = %.3g" % (nside, lmax, npol, r))
    assert r <= 2.0


# ---- bits and the memory budget ------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_memory_budget():
    """nsrc = chunk + 1, lmax 23, polarised: a budget that allows one block of 8 m-values at a time (three passes) gives the
    bits of the single pass; so does the same call again."""
    from driftscan_amd import skysim

    theta, phi, flux, *_ = sc.case_reference((skysim.SOURCE_CHUNK + 1, 3, 4, 23, None, None))
    one = skysim.source_alm((theta, phi, flux), 23)
    for mb in (1, 3 << 20):   # 8 m-values of 1024 polarised sources take 3.9 to 5 MB of tables
        assert np.array_equal(skysim.source_alm((theta, phi, flux), 23, max_bytes=mb), one), mb
    assert np.array_equal(skysim.source_alm((theta, phi, flux), 23), one)
    assert np.array_equal(skysim.source_alm((theta, phi, flux), 23, m_range=(9, 20)), one[..., 9:21])


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """The C entry refuses with an error text before anything is written: the output keeps its NaNs."""
    from driftscan_amd._lib import DriftMIError

    ctx = _ctx()
    z, sth, phi = np.array([0.5, 1.0]), np.array([np.sqrt(0.75), 0.0]), np.array([0.1, 0.2])

    def call(flux, lmax, m_lo, m_hi, match):
        nf, npol = flux.shape[:2]
        out = ctx.empty((nf, npol, lmax + 1, m_hi - m_lo + 1), np.complex128)
        out.fill_(float("nan"))
        with pytest.raises(DriftMIError, match=match):
            ctx.source_alm(z, sth, phi, flux, lmax, m_lo, m_hi, out=out)
        ctx.sync()
        assert bool(ctx.torch.isnan(out.real).all())

    call(np.ones((1, 3, 2)), 5, 0, 5, "1 .I. or 4")
    call(np.ones((1, 2, 2)), 5, 0, 5, "1 .I. or 4")
    call(np.ones((1, 1, 2)), 5, 0, 6, "above lmax")
    f = np.ones((2, 4, 2))
    call(f, 5, 0, 5, "pole")
    f[:, 1:3, 1] = 0.0
    f[1, 2, 1] = 1e-300                                   # U at one frequency only
    call(f, 5, 0, 5, "pole")
    # an unpolarised source at the pole is fine, alone and among four Stokes parameters
    f[1, 2, 1] = 0.0
    a = ctx.to_host(ctx.source_alm(z, sth, phi, f, 5, 0, 5))
    assert np.isfinite(a.view(np.float64)).all()
    b = ctx.to_host(ctx.source_alm(z, sth, phi, np.ascontiguousarray(f[:, :1]), 5, 0, 5))
    assert np.array_equal(a[:, 0], b[:, 0])
    # the polar source adds sqrt((2 l + 1) / 4 pi) to m = 0 and nothing elsewhere
    c = ctx.to_host(ctx.source_alm(z[1:], sth[1:], phi[1:], np.ones((1, 1, 1)), 5, 0, 5))
    assert np.allclose(c[0, 0, :, 0], np.sqrt((2 * np.arange(6) + 1) / (4 * np.pi)), rtol=1e-14) and not c[0, 0, :, 1:].any()


# ---- through the simulation ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    """The products of tests/test_gpu_tsim.py: 2 cylinders, 3 feeds, 3 frequencies, polarised."""
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("srcsim")
    conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, inverse=True, use_foregrounds=False)])
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    return pm, d


@pytest.fixture(scope="module")
def catalogue(prod):
    from driftscan_amd import skysim

    _, d = prod
    cat = skysim.random_catalogue(6, 12, 1.0, 50.0, 2.0, -0.7, 0.2, pol_frac=0.2, nu0=415.0)
    cat["flux"][:, 3] = 0.01 * cat["flux"][:, 0]
    fname = str(d / "sources.hdf5")
    skysim.write_catalogue(fname, cat)
    return cat, fname


@pytest.fixture(scope="module")
def per_m_route(prod, catalogue):
    """source_alm_host -> project_vector_sky_to_telescope per m -> ifft x ntime: (npairs, nfreq, ntime)."""
    from driftscan_amd import skysim

    pm, _ = prod
    bt, tel = pm.beamtransfer, pm.telescope
    cat, _ = catalogue
    ntime = 2 * tel.mmax + 1
    alm = skysim.source_alm_host(cat["theta"], cat["phi"], skysim.source_spectra(cat, tel.frequencies), tel.lmax, mmax=tel.mmax)
    col = np.zeros((tel.npairs, tel.nfreq, ntime), dtype=np.complex128)
    for mi in range(tel.mmax + 1):
        vis = bt.project_vector_sky_to_telescope(mi, np.ascontiguousarray(alm[..., mi])).reshape(tel.nfreq, 2, tel.npairs)
        col[..., mi] = vis[:, 0].T
        if mi:
            col[..., -mi] = vis[:, 1].T.conj()
    want = np.fft.ifft(col, axis=-1) * ntime
    want.setflags(write=False)
    return want


def test_simulate_with_sources(prod, catalogue, per_m_route):
    from driftscan_amd import timestream

    pm, d = prod
    tel = pm.telescope
    cat, fname = catalogue
    assert tel.num_pol_sky == 4
    scale = np.abs(per_m_route).max()
    assert scale > 0
    for key, src in (("file", [fname]), ("dict", cat)):
        ts = timestream.simulate(pm, str(d / ("ts_src_" + key)), sources=src, ndays=0)
        for fi in range(tel.nfreq):
            v = ts.timestream_f(fi)
            err = np.abs(v - per_m_route[:, fi]).max()
            print("simulate(sources=%s), frequency %d: max |delta| / max |v| = %.3g" % (key, fi, err / scale))
            assert err <= 1e-10 * scale


def test_simulate_visibilities_with_sources(prod, catalogue, per_m_route):
    from driftscan_amd import timestream

    pm, _ = prod
    _, fname = catalogue
    ctx = _ctx()
    scale = np.abs(per_m_route).max()
    X = ctx.to_host(timestream.simulate_visibilities(pm, 2, sources=[fname], ndays=0))
    assert X.shape == (2,) + per_m_route.transpose(1, 0, 2).shape
    for r in range(2):
        err = np.abs(X[r] - per_m_route.transpose(1, 0, 2)).max()
        print("simulate_visibilities(sources), realisation %d: max |delta| / max |v| = %.3g" % (r, err / scale))
        assert err <= 1e-10 * scale
    # a rank's share of the frequencies
    one = ctx.to_host(timestream.simulate_visibilities(pm, 1, sources=[fname], ndays=0, freqs=[1]))
    assert np.abs(one[0, 0] - per_m_route[:, 1]).max() <= 1e-10 * scale
    tss = timestream.simulate_ensemble(pm, str(prod[1] / "ens_src"), 1, sources=[fname], ndays=0)
    assert np.abs(tss[0].timestream_f(2) - per_m_route[:, 2]).max() <= 1e-10 * scale


def test_sources_add_to_maps(prod, catalogue):
    from driftscan_amd import healpix, skysim, timestream

    pm, d = prod
    tel = pm.telescope
    _, fname = catalogue
    rng = np.random.default_rng(4)
    L = tel.lmax + 1
    alm = (rng.standard_normal((tel.nfreq, 4, L, L)) + 1j * rng.standard_normal((tel.nfreq, 4, L, L))) * np.tril(np.ones((L, L)))
    alm[..., 0].imag = 0.0
    alm[:, 1:3, :2] = 0.0
    sky = str(d / "sky.hdf5")
    skysim.write_sky(sky, 1e-3 * healpix.sphtrans_inv_sky(alm, 32))
    both = timestream.simulate(pm, str(d / "ts_both"), maps=[sky], sources=[fname], ndays=0)
    m_only = timestream.simulate(pm, str(d / "ts_maps"), maps=[sky], ndays=0)
    s_only = timestream.simulate(pm, str(d / "ts_srcs"), sources=[fname], ndays=0)
    for fi in range(tel.nfreq):
        a, b, c = both.timestream_f(fi), m_only.timestream_f(fi), s_only.timestream_f(fi)
        scale = max(np.abs(b).max(), np.abs(c).max())
        assert np.abs(b).max() > 0 and np.abs(c).max() > 0
        print("maps + sources, frequency %d: max |delta| / max |v| = %.3g" % (fi, np.abs(a - (b + c)).max() / scale))
        assert np.abs(a - (b + c)).max() <= 1e-10 * scale


def test_pipeline_yaml_sources_reach_simulate(prod, catalogue, per_m_route, tmp_path):
    import yaml

    from driftscan_amd import pipeline

    pm, d = prod
    _, fname = catalogue
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=False, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=False),
                timestreams=[dict(name="pts", directory=str(tmp_path / "ts_pipe"), simulate=dict(ndays=0, sources=[fname]))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = pipeline.PipelineManager.from_configfile(str(cfile))
    p.simulate()
    v = p.timestreams["pts"].timestream_f(1)
    assert np.abs(v - per_m_route[:, 1]).max() <= 1e-10 * np.abs(per_m_route).max()
