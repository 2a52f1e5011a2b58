"""GPU: a_lm evaluated at points (dm_alm_at_points through driftscan_amd/skysim.py) — every case of
tests/points_cases.py against the extended-precision restatement within its bound, one-hot coefficients against the exact
Legendre fixture (the scaled seeds included), the device synthesis at its pixel centres, bits independent of chunking and
of the memory budget, refusals that leave the output untouched, and the route `Timestream.catalogue_spectra` / the
`catalogues:` list of the pipeline on the products of a small polarised cylinder."""
import os

import numpy as np
import pytest

import legendre_cases as lc
import points_cases as pc

pytestmark = pytest.mark.gpu


def _ctx():
    from driftscan_amd import device

    return device.get_context()


# ---- against extended precision -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.CASES, ids=pc.case_id)
def test_against_extended_precision(case):
    from driftscan_amd import skysim

    npts, nf, npol, lmax, _ = case
    alm, theta, phi, ms, ref, bnd = pc.case_reference(case)
    got = skysim.alm_at_points(alm, (theta, phi), ms=ms)
    assert got.shape == (npts, npol, nf) and got.dtype == np.float64
    r = pc.worst_ratio(got, ref, bnd)
    host = skysim.alm_at_points_host(alm, theta, phi, ms=ms)
    rh = pc.worst_ratio(got, host.astype(pc.LD), bnd)
    print("device %s: worst error / bound = %.3g (against the host oracle %.3g)" % (pc.case_id(case), r, rh))
    assert r <= 1.0 and rh <= 1.0


# ---- exact values -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fx(golden_dir):
    return lc.Exact(golden_dir)


GROUPS = [(2, 5), (2, 11), (8, 23), (8, 35), (32, 95), (512, 1024), (1024, 2047)]


@pytest.mark.parametrize("nside,lmax", GROUPS, ids=lambda v: str(v))
def test_one_hot_coefficients_against_exact_values(fx, nside, lmax):
    """Points on the fixture's rings, one m per call, "frequency" k < n holding a^T = a^E = 1 at l = m + k alone and
    frequency n + k holding a^B = -i there (n = lmax + 1 - m): T = fac lambda cos(m phi), Q = fac W cos(m phi) for the
    first n and Q = fac X cos(m phi) for the others (U = fac X, W sin(m phi) = 0), at phi = 0 and phi = pi / m — within
    BOUND[lmax], absolute, against values no code of this package produced.  The columns of lmax 2047 with m 696..703 on
    rings 438 and 3656 are those whose seed underflows.

    A point is put on a ring by the ring's own z and sin theta = sqrt((1 - z)(1 + z)) (`Context.alm_at_points` takes the
    two directly), the values the fixture is defined at and `healpix.lambda_lm` works with.  Going through
    theta = arccos(z) moves z and sin theta by an ulp, which lambda_mm ~ sin^m theta amplifies m-fold: on the underflow
    columns that input error alone is 3.5e-13 in lambda (the float64 recurrence on the CPU shows the same), and fac = 2
    doubles it to 6.98e-13, measured on the MI355X — beyond BOUND[2047] = 5.44e-13 with a kernel that has no part in it.
    Measured on the MI355X, worst |delta| with the ring's z (through theta): lmax 5 6.7e-16 (9.6e-16), 11 1.2e-15
    (2.9e-15), 23 1.1e-14 (1.3e-14), 35 1.6e-14 (1.8e-14), 95 2.5e-13 (2.7e-13), 1024 5.0e-11 (5.2e-11), 2047 1.27e-13
    (6.98e-13)."""
    import torch

    from driftscan_amd import healpix

    ctx = _ctx()
    cols = fx.groups()[(nside, lmax)]
    z = healpix.ring_z(nside)
    bound = lc.BOUND[lmax]
    worst, ncol = 0.0, 0
    L = lmax + 1

    def values(a, zr, phi, m, nf, npol):
        out = ctx.alm_at_points(zr, np.sqrt((1.0 - zr) * (1.0 + zr)), np.full(zr.size, phi), [m], a, lmax, nf, npol,
                                (npol * L, L, 1, 1))
        return ctx.to_host(out)

    for m in sorted(set(c[0] for c in cols)):
        rings = [r for mm, r in cols if mm == m]
        n = L - m
        k = torch.arange(n, device="cuda")
        a = torch.zeros((2 * n, 4, L, 1), dtype=torch.complex128, device="cuda")
        a[k, 0, m + k, 0] = 1.0
        a[k, 1, m + k, 0] = 1.0
        a[n + k, 2, m + k, 0] = -1j
        fac = 1.0 if m == 0 else 2.0
        for phi, sign in ((0.0, 1.0),) + (((np.pi / m, -1.0),) if m else ()):
            got = values(a, z[rings], phi, m, 2 * n, 4)                                   # (nring, 4, 2 n)
            assert got.shape == (len(rings), 4, 2 * n) and np.isfinite(got).all()
            assert not got[:, 3].any() and not got[:, 0, n:].any()
            for s, ring in enumerate(rings):
                lam, W, X = fx.column(nside, lmax, m, ring)
                c = np.cos(m * phi)                            # the phase the kernel forms: -1 up to the rounding of pi
                for g, want in ((got[s, 0, :n], lam), (got[s, 1, :n], W), (got[s, 1, n:], X)):
                    worst = max(worst, float(np.abs(g - fac * c * want).max()))
                # U = fac (X, W) sin(m phi): sin of the rounded multiple of pi, below 1e-15
                assert np.abs(got[s, 2]).max() <= bound + 1e-15 * fac * max(np.abs(W).max(), np.abs(X).max())
                assert sign * c > 0.999
            ncol += len(rings) if phi == 0.0 else 0
        del a
    print("exact nside %d lmax %d: %d columns, worst |delta| = %.3e (bound %.2e)" % (nside, lmax, ncol, worst, bound))
    assert ncol == len(cols) and worst <= bound
    if lmax == 2047:   # the underflow columns are of order one, not zeros
        a = torch.zeros((1, 1, L, 1), dtype=torch.complex128, device="cuda")
        a[0, 0, 700:, 0] = 1.0
        v = values(a, z[[438]], 0.0, 700, 1, 1)
        lam = fx.column(nside, lmax, 700, 438)[0]
        assert np.abs(lam).max() > 0.5 and abs(v[0, 0, 0] - 2.0 * lam.sum()) <= 2.0 * (L - 700) * bound


# ---- the device synthesis ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npol", [1, 4])
def test_device_synthesis_at_its_pixel_centres(npol):
    """`healpix.sphtrans_inv_sky` (Legendre products + ring FFT) at nside 8, lmax 23: twice the bound (each route within it)."""
    from driftscan_amd import healpix, skysim

    nside, lmax = 8, 23
    ang = healpix.ang_positions(nside)
    alm = np.ascontiguousarray(pc.master_alm(lmax)[:2, : (1 if npol == 1 else 4)])
    mp = healpix.sphtrans_inv_sky(alm, nside)
    got = skysim.alm_at_points(alm, (ang[:, 0], ang[:, 1]))
    allm = list(range(lmax + 1))
    _, bnd = pc.reference_of(pc.terms_ld(pc.master_alm(lmax)[:2], ang[:, 0], ang[:, 1], allm), allm, npol, lmax)
    r = pc.worst_ratio(got, mp.transpose(2, 1, 0).astype(pc.LD), bnd)
    print("device synthesis nside %d npol %d: worst |delta| / bound = %.3g" % (nside, npol, r))
    assert r <= 2.0


# ---- bits -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("npol", [1, 4])
def test_bits_do_not_depend_on_chunks_or_budget(npol):
    from driftscan_amd import skysim

    alm, theta, phi, ms, _, _ = pc.case_reference((257, 9, npol, 23, None))
    one = skysim.alm_at_points(alm, (theta, phi))
    assert np.array_equal(skysim.alm_at_points(alm, (theta, phi)), one)
    # (a) the same points in chunks of 1 and of 64
    for step in (1, 64):
        parts = [skysim.alm_at_points(alm, (theta[i : i + step], phi[i : i + step])) for i in range(0, 257, step)]
        assert np.array_equal(np.concatenate(parts), one), step
    # (b) a budget of one block of frequencies per pass, for the host input (uploaded in runs of 8) and a device tensor
    assert np.array_equal(skysim.alm_at_points(alm, (theta, phi), max_bytes=1), one)
    dev = _ctx().to_device(alm)
    assert np.array_equal(skysim.alm_at_points(dev, (theta, phi), max_bytes=1), one)
    assert np.array_equal(skysim.alm_at_points(dev, (theta, phi), max_bytes=64 << 30), one)
    # (c) a point alone and inside the batch (above: chunks of 1), and in another order of points
    perm = np.random.default_rng(0).permutation(257)
    assert np.array_equal(skysim.alm_at_points(alm, (theta[perm], phi[perm])), one[perm])
    # frequencies cut in multiples of the block
    assert np.array_equal(skysim.alm_at_points(alm[:8], (theta, phi)), one[:, :, :8])


def test_device_tensor_accumulate_and_partial_sums():
    from driftscan_amd import skysim

    alm, theta, phi, ms, ref, bnd = pc.case_reference((65, 3, 4, 23, None))
    ctx = _ctx()
    dev = ctx.to_device(alm)
    d = skysim.alm_at_points(dev, (theta, phi), to_host=False)
    assert d.is_cuda and tuple(d.shape) == (65, 4, 3) and d.dtype == ctx.torch.float64
    assert np.array_equal(d.cpu().numpy(), skysim.alm_at_points(alm, (theta, phi)))
    with pytest.raises(ValueError, match="complex128"):
        skysim.alm_at_points(dev.to(ctx.torch.complex64), (theta, phi))
    # partial sums over disjoint subsets of m, added on the device, give the whole within the bound
    acc = ctx.zeros((65, 4, 3), np.float64)
    for sub in (list(range(0, 24, 2)), list(range(23, 0, -2))):
        skysim.alm_at_points(np.ascontiguousarray(alm[..., sub]), (theta, phi), ms=sub, out=acc, accumulate=True, to_host=False)
    assert pc.worst_ratio(acc.cpu().numpy(), ref, bnd) <= 1.0
    # no m at all: zeros, or the output as it was
    assert not skysim.alm_at_points(alm[..., :0], (theta, phi), ms=[]).any()
    assert skysim.alm_at_points(alm, (np.zeros(0), np.zeros(0))).shape == (0, 4, 3)
    # unpolarised at the poles: only m = 0 contributes
    one = np.ones((1, 1, 6, 6), dtype=complex)
    v = skysim.alm_at_points(one, ([0.0, np.pi], [0.3, 0.4]))
    lam = np.sqrt((2 * np.arange(6) + 1) / (4 * np.pi))
    assert np.allclose(v[:, 0, 0], [lam.sum(), (lam * (-1.0) ** np.arange(6)).sum()], rtol=1e-13)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing():
    """The C entry refuses with an error text before anything is written: the output keeps its NaNs."""
    from driftscan_amd._lib import DriftMIError

    ctx = _ctx()
    z, sth, phi = np.array([0.5, 1.0]), np.array([np.sqrt(0.75), 0.0]), np.array([0.1, 0.2])

    def call(npts, nf, npol, lmax, ms, match):
        alm = ctx.zeros((max(nf, 1), max(npol, 1), lmax + 1, max(len(ms), 1)), np.complex128)
        out = ctx.empty((npts, npol, nf), np.float64)
        out.fill_(float("nan"))
        with pytest.raises(DriftMIError, match=match):
            ctx.alm_at_points(z[:npts], sth[:npts], phi[:npts], ms, alm, lmax, nf, npol,
                              (npol * (lmax + 1) * len(ms), (lmax + 1) * len(ms), len(ms), 1), out=out)
        ctx.sync()
        assert bool(ctx.torch.isnan(out).all())

    call(1, 2, 3, 5, [0, 1], "1 .T. or 4")
    call(1, 2, 2, 5, [0, 1], "1 .T. or 4")
    call(1, 2, 1, 5, [0, 6], "outside 0 .. lmax")
    call(1, 2, 1, 5, [0, -1], "outside 0 .. lmax")
    call(1, 2, 4, 5, [2, 3, 2], "repeated")
    call(2, 2, 4, 5, [0, 1], "pole")
    call(0, 2, 1, 5, [0, 1], "one point and one frequency")
    call(1, 0, 1, 5, [0, 1], "one point and one frequency")
    # the wrapper refuses strides that leave the tensor before the library sees them
    alm = ctx.zeros((2, 1, 6, 2), np.complex128)
    with pytest.raises(ValueError, match="outside its coefficients"):
        ctx.alm_at_points(z[:1], sth[:1], phi[:1], [0, 1], alm, 5, 2, 1, (13, 12, 2, 1))
    # the same polar point is fine without polarisation
    v = ctx.to_host(ctx.alm_at_points(z, sth, phi, [0, 1], alm, 5, 2, 1, (12, 12, 2, 1)))
    assert v.shape == (2, 1, 2) and not v.any()


# ---- through the timestream and the pipeline ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    """The products of tests/test_gpu_sources.py moved down to 370 .. 400 MHz, where the band limit is a value of the bound's
    table: 2 cylinders, 3 feeds, 3 frequencies, polarised, lmax 35 and mmax 34; and a timestream of six sources."""
    import yaml

    from driftscan_amd import device, manager, skysim, timestream

    device.reset_context()
    d = tmp_path_factory.mktemp("ptsroute")
    conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=370.0, freq_end=400.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, inverse=True, use_foregrounds=False)])
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    assert pm.telescope.lmax == 35 and pm.telescope.mmax == 34 and pm.telescope.num_pol_sky == 4
    srcs = skysim.random_catalogue(6, 12, 1.0, 50.0, 2.0, -0.7, 0.2, pol_frac=0.2, nu0=385.0)
    ts = timestream.simulate(pm, str(d / "ts"), sources=srcs, ndays=0)
    # the objects to look at: the sources themselves and a few other places, with redshifts inside and outside the band
    rng = np.random.default_rng(3)
    cat = dict(theta=np.concatenate([srcs["theta"], np.arccos(rng.uniform(-0.9, 0.9, 5))]),
               phi=np.concatenate([srcs["phi"], rng.uniform(0, 2 * np.pi, 5)]),
               redshift=skysim.LINE_21CM_MHZ / np.array([375.0, 385.0, 395.0, 374.0, 386.0, 396.0, 300.0, 500.0, 379.9, 390.1, 385.0]) - 1.0)
    return pm, d, ts, cat


def test_catalogue_spectra_svd(prod):
    from driftscan_amd import skysim, storage

    pm, d, ts, cat = prod
    tel = pm.telescope
    fname = ts.catalogue_spectra(cat, source="svd", name="objects")
    assert fname == ts.output_directory + "/spectra_objects.hdf5" and os.path.exists(fname)
    parts = ts.alm_svd_batched()
    ms = [mi for mi, _ in parts]
    alm = np.stack([a for _, a in parts], axis=-1)                       # (nfreq, npol, L, nm)
    assert alm.shape == (3, 4, 36, 35) and np.abs(alm).max() > 0
    want = skysim.alm_at_points_host(alm, cat["theta"], cat["phi"], ms=ms)
    _, bnd = pc.reference_of(pc.terms_ld(alm, cat["theta"], cat["phi"], ms), list(range(len(ms))), 4, 35)
    with storage.File(fname, "r") as f:
        assert {"spectra", "theta", "phi", "freq", "ms_used", "stack", "hits", "offsets"} <= set(f.keys())
        got = f["spectra"][:]
        assert got.shape == (11, 4, 3)
        r = pc.worst_ratio(got, want.astype(pc.LD), bnd)
        print("catalogue_spectra(svd): worst |delta| / bound = %.3g, max |T| = %.3g" % (r, np.abs(got).max()))
        assert r <= 1.0 and np.abs(got).max() > 0
        assert np.array_equal(f["theta"][:], cat["theta"]) and np.array_equal(f["phi"][:], cat["phi"])
        assert np.array_equal(f["freq"][:], tel.frequencies) and list(f["ms_used"][:]) == sorted(ms)
        line = skysim.LINE_21CM_MHZ / (1.0 + cat["redshift"])
        st = skysim.stack_spectra(got, tel.frequencies, line, 2)
        assert np.array_equal(f["stack"][:], st["stack"]) and np.array_equal(f["hits"][:], st["hits"])
        assert list(f["offsets"][:]) == [-2, -1, 0, 1, 2] and st["hits"][2] == 9 and f["stack"].shape == (4, 5)
    # a second call returns without rewriting
    stamp = os.stat(fname).st_mtime_ns
    assert ts.catalogue_spectra(cat, source="svd", name="objects") == fname and os.stat(fname).st_mtime_ns == stamp
    # without redshifts there is no stack, and asking for one is refused before anything is computed
    plain = ts.catalogue_spectra((cat["theta"], cat["phi"]), name="plain")
    with storage.File(plain, "r") as f:
        assert "stack" not in f and np.array_equal(f["spectra"][:], got)
    with pytest.raises(ValueError, match="redshifts"):
        ts.catalogue_spectra((cat["theta"], cat["phi"]), name="refused", stack=dict(halfwidth=1))
    with pytest.raises(ValueError, match="unknown stack"):
        ts.catalogue_spectra(cat, name="refused", stack=dict(width=1))
    assert not os.path.exists(ts.output_directory + "/spectra_refused.hdf5")


def test_pipeline_catalogues(prod, tmp_path):
    import yaml

    from driftscan_amd import pipeline, skysim, storage

    pm, d, ts, cat = prod
    cfile_cat = str(tmp_path / "objects.hdf5")
    with storage.File(cfile_cat, "w") as f:
        for k, v in cat.items():
            f.create_dataset(k, data=v)
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_powerspectra=False, klmodes=["kl"], nside=16,
                            collect_klmodes=False,
                            catalogues=[dict(name="a", file=cfile_cat, source="svd"),
                                        dict(name="b", file=cfile_cat, source="kl", wiener=True, stack=dict(halfwidth=1))]),
                timestreams=[dict(name="pts", directory=ts.directory, output_directory=str(tmp_path / "out"))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = pipeline.PipelineManager.from_configfile(str(cfile))
    assert [c["name"] for c in p.catalogues] == ["a", "b"]
    p.generate()
    out = str(tmp_path / "out")
    with storage.File(ts.catalogue_spectra(cat, source="svd", name="objects"), "r") as f:
        direct = f["spectra"][:]
    with storage.File(out + "/spectra_a.hdf5", "r") as f:
        a = f["spectra"][:]
        assert f["stack"].shape == (4, 5)
    assert np.abs(a - direct).max() <= 1e-10 * np.abs(direct).max()
    with storage.File(out + "/spectra_b.hdf5", "r") as f:
        b = f["spectra"][:]
        assert b.shape == (11, 4, 3) and np.isfinite(b).all() and np.abs(b).max() > 0
        assert f["stack"].shape == (4, 3) and list(f["offsets"][:]) == [-1, 0, 1]
        assert 0 not in list(f["ms_used"][:])                               # no_m_zero
    # the default list is empty and an entry without the batched route is refused
    assert pipeline.PipelineManager().catalogues == []
    p.batched = False
    with pytest.raises(ValueError, match="batched"):
        p._catalogue("pts", p.timestreams["pts"], dict(name="c", file=cfile_cat))
