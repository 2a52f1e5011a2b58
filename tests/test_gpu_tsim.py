"""Timestream ensembles on the device: the noise kernel against its numpy restatement, the
m -> time synthesis against the FFT `simulate` uses, the batched sky -> telescope projection against extended precision
and the per-m route, and `simulate_visibilities` / `simulate_ensemble` against `simulate` on the products of a small
polarised cylinder (the fixture of tests/test_gpu_timestream.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("tsim")
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
def skyfile(prod):
    """One fixed polarised sky as the `map` file `simulate(maps=[...])` reads."""
    from driftscan_amd import healpix, storage

    pm, d = prod
    tel = pm.telescope
    rng = np.random.default_rng(4)
    lmax = tel.lmax
    alm = np.zeros((tel.nfreq, 4, lmax + 1, lmax + 1), dtype=np.complex128)
    for l in range(lmax + 1):
        for m in range(l + 1):
            alm[:, :, l, m] = rng.standard_normal((tel.nfreq, 4)) + (1j * rng.standard_normal((tel.nfreq, 4)) if m else 0)
    alm[:, 1:3, :2] = 0.0
    fname = str(d / "sky.hdf5")
    with storage.File(fname, "w") as f:
        f.create_dataset("map", data=healpix.sphtrans_inv_sky(alm, 32))
    return fname


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def noise_statistics(z):
    """[(max |d|, rms d)] of the normalised deviations over the (f, pair) cells of unit noise z (nreal, nf, npairs, ntime):
    the sample variance, the lag-1 product (real and imaginary parts) and the mean (real and imaginary parts)."""
    nreal, ntime = z.shape[0], z.shape[-1]
    N, N1 = nreal * ntime, nreal * (ntime - 1)
    var = ((np.abs(z) ** 2).mean(axis=(0, 3)) - 1.0) * np.sqrt(N)
    lag = (z[..., :-1] * z[..., 1:].conj()).sum(axis=(0, 3)) * np.sqrt(2.0 / N1)
    mean = z.sum(axis=(0, 3)) * np.sqrt(2.0 / N)
    out = []
    for d in (var.ravel(), np.concatenate([lag.real.ravel(), lag.imag.ravel()]),
              np.concatenate([mean.real.ravel(), mean.imag.ravel()])):
        out.append((float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))))
    return out


# ---- ts_noise -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (3, 2, 5, 17), (2, 3, 7, 257), (1, 2, 3, 1025)])
def test_ts_noise_matches_the_host_stream(shape):
    """|device - noise_host| <= 1e-13 sigma: the figure DESIGN.md section 4.12 uses for the same map from a Philox block
    to a normal draw (device log / sincos against numpy's)."""
    from driftscan_amd import skysim

    ctx = _ctx()
    nreal, nf, npairs, ntime = shape
    rng = np.random.default_rng(sum(shape))
    sigma = rng.uniform(0.25, 4.0, size=(nf, npairs))
    fg = np.sort(rng.choice(11, size=nf, replace=False))
    got = ctx.to_host(ctx.ts_noise(sigma, fg, ntime, nreal, seed=7, first=1))
    want = skysim.noise_host(sigma, fg, ntime, nreal, seed=7, first=1)
    assert got.shape == shape
    err = np.abs(got - want) / sigma[None, :, :, None]
    print("ts_noise %s: max |delta| / sigma = %.3g" % (shape, err.max()))
    assert err.max() <= 1e-13


def test_ts_noise_invariance_and_statistics():
    from driftscan_amd import _lib

    ctx = _ctx()
    rng = np.random.default_rng(9)
    sigma = rng.uniform(0.5, 2.0, size=(4, 5))
    fg = np.array([0, 1, 2, 5])
    full = ctx.to_host(ctx.ts_noise(sigma, fg, 17, 4, seed=3))
    sub = ctx.to_host(ctx.ts_noise(sigma[[1, 3]], fg[[1, 3]], 17, 4, seed=3))
    assert np.array_equal(sub, full[:, [1, 3]])
    part = ctx.to_host(ctx.ts_noise(sigma, fg, 17, 2, seed=3, first=2))
    assert np.array_equal(part, full[2:4])
    assert not np.any(full[0] == full[1])
    # into a buffer of the caller: every element is written
    buf = ctx.empty((4, 4, 5, 17), np.complex128)
    buf.fill_(float("nan"))
    assert ctx.ts_noise(sigma, fg, 17, 4, seed=3, out=buf) is buf
    assert np.array_equal(ctx.to_host(buf), full)
    # the three statistics of the host test on the device result
    z = ctx.to_host(ctx.ts_noise(np.ones((4, 16)), np.arange(4), 257, 4, seed=11))
    stats = noise_statistics(z)
    print("ts_noise statistics (max |d|, rms):", stats)
    for dmax, rms in stats:
        assert dmax < 5.0 and 0.6 < rms < 1.4, stats
    # a realisation that does not fit the counter word is refused, nothing is launched
    with pytest.raises(_lib.DriftMIError, match="24 bits"):
        ctx.ts_noise(np.ones((1, 1)), [0], 1, 2, seed=0, first=(1 << 24) - 1)
    with pytest.raises(ValueError):
        ctx.ts_noise(np.ones((2, 3)), [0], 5, 1, seed=0)
    assert tuple(ctx.ts_noise(np.ones((0, 3)), [], 5, 2, seed=0).shape) == (2, 0, 3, 5)


def test_ts_noise_indexes_past_2_to_31():
    """(2, 2, 2, 2^28 + 3): 2^31 + 24 elements, the last 24 lie past element 2^31 (the size of one chunk of the largest
    configuration).  The ends of the first and last rows against the generator evaluated at those counters."""
    from driftscan_amd import skysim

    ctx = _ctx()
    ntime = (1 << 28) + 3
    sigma = np.array([[1.0, 2.0], [3.0, 4.0]])
    fg = [3, 7]
    out = ctx.ts_noise(sigma, fg, ntime, 2, seed=5, first=6)
    assert out.numel() == (1 << 31) + 24

    def draws(r, i, p, t):
        t = np.asarray(t, dtype=np.uint64)
        c = [np.full_like(t, p), np.full_like(t, fg[i]), t, np.full_like(t, ((6 + r) << 8) | skysim.STREAM_TS_NOISE)]
        w = skysim._philox4x32_10(c, (5, 0))
        rad = np.sqrt(-np.log(skysim._u53(w[0], w[1]))) * sigma[i, p]
        th = 6.283185307179586 * skysim._u53(w[2], w[3])
        return rad * np.cos(th) + 1j * (rad * np.sin(th))

    for (r, i, p) in ((0, 0, 0), (0, 1, 1), (1, 1, 0), (1, 1, 1)):
        for t0 in (0, ntime - 64):
            got = ctx.to_host(out[r, i, p, t0 : t0 + 64])
            want = draws(r, i, p, np.arange(t0, t0 + 64))
            assert np.abs(got - want).max() <= 1e-13 * sigma[i, p], (r, i, p, t0)
    del out


# ---- mmode_synthesis ------------------------------------------------------------------------------------------------------
def _col_vis(V, ntime):
    """The Fourier bins `simulate` fills from m-modes V (mmax + 1, nf, 2, npairs): (npairs, nf, ntime)."""
    nm, nf, _, npairs = V.shape
    col = np.zeros((npairs, nf, ntime), dtype=np.complex128)
    for mi in range(nm):
        col[..., mi] = V[mi, :, 0].T
        if mi:
            col[..., -mi] = V[mi, :, 1].T.conj()
    return col


def _synthesis_case(mmax, ntime, nf, npairs):
    rng = np.random.default_rng(1000 * mmax + 10 * ntime + nf + npairs)
    V = _crandn(rng, mmax + 1, nf, 2, npairs)
    col = _col_vis(V, ntime)
    want = (np.fft.ifft(col, axis=-1) * ntime).transpose(1, 0, 2)                       # (nf, npairs, ntime)
    bound = 4 * (2 * mmax + 3) * EPS * np.abs(col).sum(axis=-1).T[:, :, None]           # 4 (K + 2) eps sum_m |c_m|
    return V, want, bound


@pytest.mark.parametrize("npairs", [1, 7])
@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("mmax,ntime", [(0, 1), (0, 5), (3, 7), (8, 17), (8, 64), (20, 257)])
def test_mmode_synthesis_against_the_fft(mmax, ntime, nf, npairs):
    ctx = _ctx()
    V, want, bound = _synthesis_case(mmax, ntime, nf, npairs)
    got = ctx.to_host(ctx.mmode_synthesis(ctx.to_device(V), ntime))
    assert got.shape == (nf, npairs, ntime)
    print("synthesis (%d, %d, %d, %d): max err / bound = %.3g" % (mmax, ntime, nf, npairs, (np.abs(got - want) / bound).max()))
    assert np.all(np.abs(got - want) <= bound)


def test_mmode_synthesis_round_trip_accumulate_and_columns():
    ctx = _ctx()
    mmax, ntime, nf, npairs = 8, 17, 3, 7
    V, want, bound = _synthesis_case(mmax, ntime, nf, npairs)
    dV = ctx.to_device(V)
    X = ctx.mmode_synthesis(dV, ntime)
    # back through the time -> m transform: V with slot 1 of m = 0 zeroed.  The transform sums ntime products
    # x_t W[t, m], |W| = 1 / ntime: 4 (ntime + 2) eps mean_t |x_t|; the synthesis error of x reaches a bin through the
    # same mean, so it adds at most its own bound (constant along t).
    back = ctx.to_host(ctx.mmode_transform(X, mmax))
    Vz = V.copy()
    Vz[0, :, 1] = 0.0
    xh = ctx.to_host(X)
    b2 = bound[:, :, 0] + 4 * (ntime + 2) * EPS * np.abs(xh).mean(axis=-1)                  # (nf, npairs)
    assert np.all(np.abs(back - Vz) <= b2[None, :, None, :])
    # accumulate on a non-zero buffer adds
    rng = np.random.default_rng(8)
    base = _crandn(rng, nf, npairs, ntime)
    buf = ctx.to_device(base)
    assert ctx.mmode_synthesis(dV, ntime, out=buf, accumulate=True) is buf
    assert np.all(np.abs(ctx.to_host(buf) - (base + want)) <= bound)
    # one column of an (mmax + 1, nf, 2, npairs, R) array, as the batched projection leaves it: read in place
    cols = ctx.to_device(np.ascontiguousarray(np.stack([V, 2.0 * V, -V], axis=-1)))
    got = ctx.to_host(ctx.mmode_synthesis(cols[..., 1], ntime))
    assert np.all(np.abs(got - 2.0 * want) <= 2.0 * bound)
    # too few time samples for the m
    with pytest.raises(ValueError):
        ctx.mmode_synthesis(dV, 2 * mmax)
    with pytest.raises(ValueError):
        ctx.mmode_synthesis(dV, ntime, accumulate=True)


# ---- the batched projection -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def projection_reference(prod):
    """Beam blocks of every m on the host, a_lm for 8 skies, their products in extended precision and the bound
    4 (nsky + 2) eps (|B| |a|) of DESIGN.md section 4.11 — computed once, read by the tests below."""
    pm, _ = prod
    bt, tel = pm.beamtransfer, pm.telescope
    ms = list(range(tel.mmax + 1))
    rng = np.random.default_rng(21)
    beam = np.stack([bt.beam_m(mi).reshape(bt.nfreq, bt.ntel, bt.nsky) for mi in ms])       # (nm, nf, ntel, nsky)
    alm = _crandn(rng, len(ms), bt.nfreq, tel.num_pol_sky, tel.lmax + 1, 8)
    a = alm.reshape(len(ms), bt.nfreq, bt.nsky, 8)
    want = np.einsum("mftk,mfkr->mftr", beam.astype(np.clongdouble), a.astype(np.clongdouble))
    bound = 4 * (bt.nsky + 2) * EPS * np.einsum("mftk,mfkr->mftr", np.abs(beam), np.abs(a))
    for arr in (beam, alm, want, bound):
        arr.setflags(write=False)
    return ms, beam, alm, want, bound


@pytest.mark.parametrize("R", [1, 3, 8])
def test_batched_projection(prod, projection_reference, R):
    pm, _ = prod
    bt = pm.beamtransfer
    ctx = _ctx()
    ms, beam, alm, want, bound = projection_reference
    dalm = ctx.to_device(np.ascontiguousarray(alm[..., :R]))
    one = ctx.to_host(bt.project_vectors_sky_to_telescope_device(ms, dalm))
    assert one.shape == (len(ms), bt.nfreq, bt.ntel, R)
    print("projection R = %d: max err / bound = %.3g" % (R, float((np.abs(one - want[..., :R]) / np.maximum(bound[..., :R], 1e-300)).max())))
    assert np.all(np.abs(one - want[..., :R]) <= bound[..., :R])
    # the same m in two batches
    h = len(ms) // 2
    two = np.concatenate([ctx.to_host(bt.project_vectors_sky_to_telescope_device(ms[:h], dalm[:h].contiguous())),
                          ctx.to_host(bt.project_vectors_sky_to_telescope_device(ms[h:], dalm[h:].contiguous()))])
    assert np.all(np.abs(two - want[..., :R]) <= bound[..., :R])
    # a frequency subset reads and multiplies those slices only
    freqs = [0, 2]
    sub = ctx.to_host(bt.project_vectors_sky_to_telescope_device(ms, dalm[:, freqs].contiguous(), freqs=freqs))
    assert sub.shape == (len(ms), 2, bt.ntel, R)
    assert np.all(np.abs(sub - want[:, freqs, :, :R]) <= bound[:, freqs, :, :R])
    # from products resident on the device: the same blocks, the same bits
    bt._beam_all, bt._beam_all_m0 = ctx.to_device(beam.reshape((len(ms),) + bt.beam_m(0).shape).copy()), 0
    try:
        res = ctx.to_host(bt.project_vectors_sky_to_telescope_device(ms, dalm))
        res_sub = ctx.to_host(bt.project_vectors_sky_to_telescope_device(ms, dalm[:, freqs].contiguous(), freqs=freqs))
    finally:
        bt._beam_all = None
    assert np.array_equal(res, one) and np.array_equal(res_sub, sub)
    with pytest.raises(ValueError):
        bt.project_vectors_sky_to_telescope_device(ms[:2], dalm)


def test_batched_projection_against_the_per_m_route(prod, projection_reference):
    pm, _ = prod
    bt = pm.beamtransfer
    ctx = _ctx()
    ms, beam, alm, want, bound = projection_reference
    got = ctx.to_host(bt.project_vectors_sky_to_telescope_device(ms, ctx.to_device(np.ascontiguousarray(alm[..., :1]))))[..., 0]
    for i, mi in enumerate(ms):
        per_m = bt.project_vector_sky_to_telescope(mi, np.ascontiguousarray(alm[i, ..., 0]))
        assert np.all(np.abs(got[i] - per_m) <= 2 * bound[i, ..., 0]), mi       # each route within the bound


# ---- end to end -----------------------------------------------------------------------------------------------------------
def test_ensemble_without_noise_is_simulate(prod, skyfile):
    from driftscan_amd import storage, timestream

    pm, d = prod
    tel = pm.telescope
    first = 2
    tss = timestream.simulate_ensemble(pm, str(d / "ens"), 1, maps=[skyfile], skymodels=("signal",), ndays=0, first=first)
    ref = timestream.simulate(pm, str(d / "ens_ref"), maps=[skyfile], skymodels=("signal",), sky_realisation=first, ndays=0)
    assert len(tss) == 1 and tss[0].directory.endswith("real_%04d" % first)
    ts = tss[0]
    assert ts.ntime == ref.ntime == 2 * tel.mmax + 1
    for fi in range(tel.nfreq):
        v, w = ts.timestream_f(fi), ref.timestream_f(fi)
        assert v.shape == w.shape == (tel.npairs, ts.ntime) and v.dtype == np.complex128
        print("ensemble vs simulate, frequency %d: max |delta| / max |v| = %.3g" % (fi, np.abs(v - w).max() / np.abs(w).max()))
        assert np.abs(v - w).max() <= 1e-10 * np.abs(w).max(), fi
        with storage.File(ts._ffile(fi), "r") as f, storage.File(ref._ffile(fi), "r") as g:
            assert sorted(f.keys()) == sorted(g.keys())
            assert int(f.attrs["ntime"]) == int(g.attrs["ntime"])
            assert f.attrs["beamtransfer_path"] == g.attrs["beamtransfer_path"]
            assert np.array_equal(f["phi"][:], g["phi"][:])
    again = timestream.Timestream.load(ts.directory)
    assert again.ntime == ts.ntime
    again.generate_modes_batched()
    ref.generate_mmodes()
    for mi in (0, 1, tel.mmax):
        a, b = again.mmode(mi), ref.mmode(mi)
        assert a.shape == (tel.nfreq, 2, tel.npairs)
        assert np.abs(a - b).max() <= 1e-10 * max(np.abs(b).max(), 1e-300), mi
    assert again.mmode_svd(1).shape == (int(pm.beamtransfer.ndof(1)),)


def test_noise_only_visibilities(prod):
    from driftscan_amd import timestream

    pm, _ = prod
    tel = pm.telescope
    ctx = _ctx()
    mmax, nf, npairs = tel.mmax, tel.nfreq, tel.npairs
    X = timestream.simulate_visibilities(pm, 8, ndays=10, seed=11)
    assert tuple(X.shape) == (8, nf, npairs, 2 * mmax + 1)
    # the noise level the KL stage assumes: m-modes of variance noisepower in every bin of both slots
    npower = np.asarray(tel.noisepower(np.arange(npairs)[None, :], np.arange(nf)[:, None], ndays=10)).reshape(nf, npairs)
    p2 = np.zeros((nf, npairs))
    for r in range(8):
        v = ctx.to_host(ctx.mmode_transform(X[r], mmax))                    # (mmax + 1, nf, 2, npairs), [0, :, 1] zero
        p2 += (np.abs(v) ** 2).sum(axis=(0, 2))
    nbin = 8 * (2 * mmax + 1)
    dev = (p2 / nbin / npower - 1.0) * np.sqrt(nbin)
    stats = (float(np.abs(dev).max()), float(np.sqrt((dev ** 2).mean())))
    print("noise-only m-modes: max |d| = %.3g, rms = %.3g over %d cells" % (stats + (dev.size,)))
    assert stats[0] < 5.0 and 0.6 < stats[1] < 1.4
    Xh = ctx.to_host(X)
    # one frequency alone, the same call again, a range of realisations
    one = ctx.to_host(timestream.simulate_visibilities(pm, 8, ndays=10, seed=11, freqs=[1]))
    assert one.shape == (8, 1, npairs, 2 * mmax + 1) and np.array_equal(one[:, 0], Xh[:, 1])
    assert np.array_equal(ctx.to_host(timestream.simulate_visibilities(pm, 8, ndays=10, seed=11)), Xh)
    assert np.array_equal(ctx.to_host(timestream.simulate_visibilities(pm, 2, ndays=10, seed=11, first=3)), Xh[3:5])
    assert not np.any(ctx.to_host(timestream.simulate_visibilities(pm, 1, ndays=10, seed=12)) == Xh[:1])
    # nothing at all: zeros
    assert not ctx.to_host(timestream.simulate_visibilities(pm, 1, ndays=0)).any()


def test_sky_and_noise_split_by_frequency(prod, skyfile):
    """The union of the ranks' results is the single-process result: the frequencies [0, 2] and [1] computed apart
    reproduce the full call within the synthesis bound.  Every stage works per frequency in an order that does not
    depend on the other rows (the draws are counter based, a block of the projection and a frequency of the synthesis
    are summed by themselves), so the same bits are expected; whether they are is printed, not asserted."""
    from driftscan_amd import timestream

    pm, _ = prod
    tel = pm.telescope
    ctx = _ctx()
    mmax = tel.mmax
    kw = dict(maps=[skyfile], skymodels=("signal",), ndays=10, seed=5, sky_seed=3, first=1)
    full = ctx.to_host(timestream.simulate_visibilities(pm, 2, **kw))
    a = ctx.to_host(timestream.simulate_visibilities(pm, 2, freqs=[0, 2], **kw))
    b = ctx.to_host(timestream.simulate_visibilities(pm, 2, freqs=[1], **kw))
    split = np.empty_like(full)
    split[:, [0, 2]] = a
    split[:, [1]] = b
    # sum_m |c_m| of the noise-free m-modes, per realisation, frequency and pair
    sky = timestream.simulate_visibilities(pm, 2, **dict(kw, ndays=0))
    csum = np.stack([np.abs(ctx.to_host(ctx.mmode_transform(sky[r], mmax))).sum(axis=(0, 2)) for r in range(2)])
    bound = 4 * (2 * mmax + 3) * EPS * csum[..., None]
    print("frequency split: max |delta| / bound = %.3g, identical bits: %s"
          % (float((np.abs(split - full) / bound).max()), np.array_equal(split, full)))
    assert np.all(np.abs(split - full) <= bound)
    # the sky is in there: with the noise taken off, what is left is the noise-free result
    noise = ctx.to_host(timestream.simulate_visibilities(pm, 2, ndays=10, seed=5, first=1))
    resid = np.abs((full - noise) - ctx.to_host(sky))
    assert np.all(resid <= bound + 4 * EPS * (np.abs(full) + np.abs(noise)))
    assert np.abs(ctx.to_host(sky)).max() > 0


def test_ensemble_files_are_the_visibilities_with_everything_on(prod, skyfile):
    """`simulate_ensemble` writes what `simulate_visibilities` returns with every option at once: maps and a model, noise,
    a GainModel, weights with zeros and 9 realisations (one more than BLOCKVEC_MAX_R, so a second group reuses the
    ensemble's one buffer), stacked and unstacked, the latter also in chunks of one frequency.  Bit for bit: two
    identical calls agreed in every bit, sky part included, in three runs of the commit before the simulators were
    staged, so equality is what is asserted, not the synthesis bound of `test_sky_and_noise_split_by_frequency`."""
    from driftscan_amd import _lib, skysim, storage, timestream

    pm, d = prod
    tel = pm.telescope
    ctx = _ctx()
    nreal, nf, nfeed, ntime, first = _lib.BLOCKVEC_MAX_R + 1, tel.nfreq, tel.nfeed, 2 * tel.mmax + 1, 1
    class_off, members = tel.redundant_pairs()
    rng = np.random.default_rng(17)
    gains = skysim.GainModel(sigma_amp=0.05, sigma_phase=0.05, corr_time=3600.0, seed=2)
    kw = dict(maps=[skyfile], skymodels=("signal",), ndays=10, seed=5, sky_seed=3, first=first, gains=gains)
    ref = timestream.simulate(pm, str(d / "all_ref"), maps=[skyfile], gains=gains, ndays=10, seed=1,
                              weights=np.ones((nf, tel.npairs, ntime)))
    with storage.File(ref._ffile(0), "r") as f:
        names = set(f.keys())
    assert {"timestream", "phi", "gain", "weight"} <= names
    for tag, extra in (("stacked", {}), ("unstacked", dict(unstacked=True)),
                       ("unstacked_chunks", dict(unstacked=True, chunk_gb=1e-9))):
        nrow = int(class_off[-1]) if extra else tel.npairs
        w = (rng.uniform(size=(nf, nrow, ntime)) > 0.2) * rng.uniform(0.5, 2.0, size=(nf, nrow, ntime))
        assert (w == 0).any()
        X = ctx.to_host(timestream.simulate_visibilities(pm, nreal, weights=w, **kw, **extra))
        assert X.shape == (nreal, nf, nrow, ntime) and not X[w[None].repeat(nreal, 0) == 0].any()
        tss = timestream.simulate_ensemble(pm, str(d / ("all_" + tag)), nreal, weights=w, **kw, **extra)
        assert len(tss) == nreal
        worst = 0.0
        for i, ts in enumerate(tss):
            assert ts.directory.endswith("real_%04d" % (first + i)) and ts.is_unstacked() == bool(extra)
            for fi in range(nf):
                with storage.File(ts._ffile(fi), "r") as f:
                    v = f["timestream"][:]
                    worst = max(worst, float(np.abs(v - X[i, fi]).max()))
                    assert np.array_equal(v, X[i, fi]), (tag, i, fi)
                    assert np.array_equal(f["weight"][:], w[fi])
                    assert f["gain"].shape == (nfeed, ntime) and f["gain"].dtype == np.complex128
                    assert int(f.attrs["ntime"]) == ntime
                    if extra:
                        assert set(f.keys()) == names | {"class_off", "members"} and int(f.attrs["unstacked"]) == 1
                        assert np.array_equal(f["class_off"][:], class_off) and np.array_equal(f["members"][:], members)
                    else:
                        assert set(f.keys()) == names and "unstacked" not in f.attrs
        print("ensemble files vs simulate_visibilities (%s): max |delta| = %.3g" % (tag, worst))
