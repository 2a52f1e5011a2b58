"""Per-feed gain errors on the device: the coefficient draws and the series against their numpy
restatement, `ts_gain_compose` against numpy, `ts_gain_apply` against extended precision on hand-made pair tables
(tests/gains_cases.py), and the routes `simulate_visibilities` / `simulate_ensemble` with gains against the per-m
`simulate` on the products of the small polarised cylinder of tests/test_gpu_tsim.py."""
import numpy as np
import pytest

import gains_cases as gc

pytestmark = pytest.mark.gpu

EPS = gc.EPS


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _model(ntime, freq_corr="none", seed=7):
    """Equal weights for the short days, a correlation time for the longer ones: 7200 s caps K at 16 (31 uncapped at 64
    samples) and leaves the 8 of 17 samples with unequal weights."""
    from driftscan_amd import skysim

    return skysim.GainModel(0.05, 0.3, corr_time=7200.0 if ntime >= 17 else 0.0, freq_corr=freq_corr, seed=seed)


# ---- coefficients, series, gains ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("freq_corr", ["none", "full"])
@pytest.mark.parametrize("nreal", [1, 3])
@pytest.mark.parametrize("ntime", [1, 5, 17, 64])
@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("nfeed", [1, 3])
def test_gain_draws_and_series_match_the_host(nfeed, nf, ntime, nreal, freq_corr):
    """Coefficients within the draw figure 1e-13 of sigma sum c_k, series within that plus the synthesis bound
    4 (2 K + 3) eps sum_k |coeff_k| (gains_cases.series_bound), gains within the sum of the two series bounds times
    (1 + |x_amp|) plus 4 eps for the sine, cosine and product."""
    from driftscan_amd import skysim

    ctx = _ctx()
    model = _model(ntime, freq_corr)
    assert model.kmax(ntime) == {1: 0, 5: 2, 17: 8, 64: 16}[ntime]
    fg = np.array([4] if nf == 1 else [1, 4, 9])
    first = 2
    bounds = {}
    for stream, sigma in ((skysim.STREAM_TS_GAIN_AMP, model.sigma_amp), (skysim.STREAM_TS_GAIN_PHASE, model.sigma_phase)):
        want_c = skysim.gain_coeff_host(model, nfeed, fg, ntime, nreal, first, stream)
        want_x = skysim.gain_series_host(want_c, ntime)
        coeff, x = skysim.gain_series_device(model, nfeed, fg, ntime, nreal, first, stream)
        got_c, got_x = ctx.to_host(coeff), ctx.to_host(x)
        assert got_c.shape == want_c.shape == (nreal, nf, nfeed, model.kmax(ntime) + 1) and got_x.shape == want_x.shape
        draw = 1e-13 * sigma * model.weights(ntime).sum()
        bound = gc.series_bound(model, want_c, ntime, sigma)[..., None]
        print("stream %d: coefficients max |delta| / bound = %.3g, series %.3g"
              % (stream, np.abs(got_c - want_c).max() / draw, (np.abs(got_x.real - want_x) / bound).max()))
        assert np.abs(got_c - want_c).max() <= draw
        assert np.all(np.abs(got_x.real - want_x) <= bound)
        bounds[stream] = (bound, want_x)
    g = ctx.to_host(skysim.gains_device(model, nfeed, fg, ntime, nreal, first))
    want = skysim.gains_host(model, nfeed, fg, ntime, nreal, first)
    amp = 1.0 + np.abs(bounds[skysim.STREAM_TS_GAIN_AMP][1])
    bound = (bounds[skysim.STREAM_TS_GAIN_AMP][0] + bounds[skysim.STREAM_TS_GAIN_PHASE][0]) * amp + 4 * EPS
    print("gains: max |delta| / bound = %.3g" % (np.abs(g - want) / bound).max())
    assert np.all(np.abs(g - want) <= bound)
    if freq_corr == "full" and nf > 1:
        assert np.array_equal(g, np.broadcast_to(g[:, :1], g.shape))


def test_gain_draws_of_subsets_and_refusals():
    from driftscan_amd import _lib, skysim

    ctx = _ctx()
    model = _model(17)
    fg = np.array([0, 1, 2, 5])
    full = ctx.to_host(skysim.gains_device(model, 5, fg, 17, 4))
    sub = ctx.to_host(skysim.gains_device(model, 5, fg[[1, 3]], 17, 4))
    part = ctx.to_host(skysim.gains_device(model, 5, fg, 17, 2, first=2))
    # the bound of the test above, here between two device calls
    c = {s: skysim.gain_coeff_host(model, 5, fg, 17, 4, 0, s) for s in (skysim.STREAM_TS_GAIN_AMP, skysim.STREAM_TS_GAIN_PHASE)}
    amp = 1.0 + np.abs(skysim.gain_series_host(c[skysim.STREAM_TS_GAIN_AMP], 17))
    bound = (gc.series_bound(model, c[skysim.STREAM_TS_GAIN_AMP], 17, model.sigma_amp)
             + gc.series_bound(model, c[skysim.STREAM_TS_GAIN_PHASE], 17, model.sigma_phase))[..., None] * amp + 4 * EPS
    print("frequency subset: identical bits: %s; realisation range: identical bits: %s"
          % (np.array_equal(sub, full[:, [1, 3]]), np.array_equal(part, full[2:4])))
    assert np.all(np.abs(sub - full[:, [1, 3]]) <= bound[:, [1, 3]])
    assert np.all(np.abs(part - full[2:4]) <= bound[2:4])
    assert not np.any(full[0] == full[1])
    # every element of a caller's buffer is written
    buf = ctx.empty((4, 4, 5, 9), np.complex128)
    buf.fill_(float("nan"))
    ck = model.weights(17)
    assert ctx.ts_gain_coeff(4, fg, 5, ck, 0.05, 7, out=buf) is buf
    assert not np.isnan(ctx.to_host(buf)).any()
    # a realisation that does not fit the counter word, a stream that is not a gain stream: refused, nothing launched
    with pytest.raises(_lib.DriftMIError, match="24 bits"):
        ctx.ts_gain_coeff(2, [0], 1, ck, 0.05, 0, first=(1 << 24) - 1)
    with pytest.raises(_lib.DriftMIError):
        ctx.ts_gain_coeff(1, [0], 1, ck, 0.05, 0, stream=skysim.STREAM_TS_NOISE)
    assert tuple(ctx.ts_gain_coeff(2, [], 3, ck, 0.05, 0).shape) == (2, 0, 3, 9)


def test_ts_gain_compose_against_numpy():
    ctx = _ctx()
    rng = np.random.default_rng(12)
    for shape in ((1,), (2, 3, 5, 17), (1, 1, 7, 257)):
        xa, xp = 0.2 * gc.crandn(rng, *shape), 3.0 * gc.crandn(rng, *shape)
        got = ctx.to_host(ctx.ts_gain_compose(ctx.to_device(xa), ctx.to_device(xp)))
        # the same inputs on both sides, so no series bound: what is left is the sine, the cosine and the product, 4 eps
        # (numpy in extended precision, so that the reference adds no rounding of its own)
        xl = xp.real.astype(np.longdouble)
        want = (1 + xa.real.astype(np.longdouble)) * (np.cos(xl) + 1j * np.sin(xl))
        err = np.abs(got - want).astype(np.float64)
        print("ts_gain_compose %s: max |delta| / (4 eps) = %.3g" % (shape, err.max() / (4 * EPS)))
        assert got.shape == shape and np.all(err <= 4 * EPS)
    with pytest.raises(ValueError):
        ctx.ts_gain_compose(ctx.to_device(xa), ctx.to_device(xp[:, :, :3]))


# ---- ts_gain_apply --------------------------------------------------------------------------------------------------------
def _apply_case(rng, ctx, nfeed, off, mem, nreal, g_nreal, nf, ntime, accumulate):
    """One call inside guard rows; returns (max err / bound, device result)."""
    npairs = off.shape[0] - 1
    g = gc.crandn(rng, g_nreal, nf, nfeed, ntime)
    sky = gc.crandn(rng, nreal, nf, npairs, ntime)
    base = gc.crandn(rng, nreal + 2, nf, npairs, ntime)
    G, A = gc.baseline_gains_exact(g, off, mem)
    want = G * sky.astype(np.clongdouble)
    bound = gc.apply_bound(A, sky, off)
    if accumulate:   # one more rounding, of the sum with what the buffer held
        want = want + base[1:-1].astype(np.clongdouble)
        bound = bound + EPS * np.abs(want).astype(np.float64)
    buf = ctx.to_device(base)
    res = ctx.ts_gain_apply(ctx.to_device(g), off, mem, ctx.to_device(sky), out=buf[1:-1], accumulate=accumulate)
    got = ctx.to_host(buf)
    assert np.array_equal(got[0], base[0]) and np.array_equal(got[-1], base[-1])          # guard rows untouched
    err = np.abs(got[1:-1] - want).astype(np.float64)
    assert np.all(err <= bound), (nreal, g_nreal, nf, ntime, accumulate, float((err / bound).max()))
    return float((err / np.maximum(bound, 1e-300)).max()), res


@pytest.mark.parametrize("ntime", [1, 5, 17, 65])
@pytest.mark.parametrize("name", ["one", "two", "line70", "cyl12"])
def test_ts_gain_apply_against_extended_precision(name, ntime):
    """|device - clongdouble| <= 4 (n_c + 2) eps (1 / n_c) sum |g_i| |g_j| |sky| per element, plus eps |result| for the
    sum with the buffer when accumulating (the bound of the product alone cannot hold where the buffer's value dwarfs
    it).  ntime 1, 5: part of one tile of 16 samples; 17, 65: whole tiles and a part."""
    ctx = _ctx()
    nfeed, off, mem = gc.apply_tables()[name]
    if name == "line70":
        assert off[1] - off[0] == 69
    if name == "cyl12":
        assert nfeed == 12 and off.shape[0] - 1 == 28
    rng = np.random.default_rng(100 * ntime + nfeed)
    worst = 0.0
    for nf in (1, 3):
        for nreal in (1, 3, 8):
            for g_nreal in sorted({1, nreal}):
                for accumulate in (False, True):
                    worst = max(worst, _apply_case(rng, ctx, nfeed, off, mem, nreal, g_nreal, nf, ntime, accumulate)[0])
    print("ts_gain_apply %s, ntime %d: max err / bound = %.3g" % (name, ntime, worst))


@pytest.mark.parametrize("nfeed", sorted(gc.TILE_NFEED))
def test_ts_gain_apply_every_tile(nfeed):
    """More feeds, shorter tiles: 8, 4, 2 and 1 samples, the last also past 64 KiB of LDS and with all 160 KiB of it."""
    ctx = _ctx()
    assert ctx.lib.dm_ts_gain_tile(nfeed) == gc.TILE_NFEED[nfeed] and ctx.lib.dm_ts_gain_tile(12) == 16
    off, mem = gc.line_table(nfeed)
    rng = np.random.default_rng(nfeed)
    for nreal, g_nreal, accumulate in ((2, 2, False), (2, 1, True)):
        r = _apply_case(rng, ctx, nfeed, off, mem, nreal, g_nreal, 2, 19, accumulate)[0]
        print("ts_gain_apply %d feeds (tile %d): max err / bound = %.3g" % (nfeed, gc.TILE_NFEED[nfeed], r))


def test_ts_gain_apply_identities_and_batch_independence():
    ctx = _ctx()
    rng = np.random.default_rng(3)
    nfeed, off, mem = gc.apply_tables()["line70"]
    npairs, nf, ntime, nreal = off.shape[0] - 1, 3, 17, 3
    sky = gc.crandn(rng, nreal, nf, npairs, ntime)
    dsky = ctx.to_device(sky)
    n = np.diff(off)[:, None]
    # a phase common to all feeds leaves the sky as it is, a common constant multiplies it by |c|^2: the bound of the
    # product with A = 1 and A = |c|^2
    phase = np.exp(1j * rng.uniform(0, 2 * np.pi, size=(nreal, nf, 1, ntime)))
    got = ctx.to_host(ctx.ts_gain_apply(ctx.to_device(np.ascontiguousarray(np.broadcast_to(phase, (nreal, nf, nfeed, ntime)))),
                                        off, mem, dsky))
    assert np.all(np.abs(got - sky) <= 4 * (n + 2) * EPS * (1.0 + 2 * EPS) * np.abs(sky))
    c = 0.8 - 0.7j
    got = ctx.to_host(ctx.ts_gain_apply(ctx.to_device(np.full((1, nf, nfeed, ntime), c)), off, mem, dsky))
    assert np.all(np.abs(got - abs(c) ** 2 * sky) <= 4 * (n + 2) * EPS * abs(c) ** 2 * np.abs(sky))
    # a class by itself, in a call of one realisation and one frequency, has the bits it has inside the batch
    g = gc.crandn(rng, nreal, nf, nfeed, ntime)
    full = ctx.to_host(ctx.ts_gain_apply(ctx.to_device(g), off, mem, dsky))
    for cls in (0, 1, 3):
        o1, m1 = np.array([0, off[cls + 1] - off[cls]], dtype=np.int32), mem[off[cls] : off[cls + 1]]
        alone = ctx.to_host(ctx.ts_gain_apply(ctx.to_device(np.ascontiguousarray(g[1:2, 2:3])), o1, m1,
                                              ctx.to_device(np.ascontiguousarray(sky[1:2, 2:3, cls : cls + 1]))))
        assert np.array_equal(alone[0, 0, 0], full[1, 2, cls]), cls
    # frequency slices of wider arrays (what the routes pass): the same bits
    out = ctx.zeros((nreal, nf, npairs, ntime), np.complex128)
    ctx.ts_gain_apply(ctx.to_device(np.ascontiguousarray(g[:, 1:])), off, mem, dsky[:, 1:], out=out[:, 1:])
    got = ctx.to_host(out)
    assert np.array_equal(got[:, 1:], full[:, 1:]) and not got[:, 0].any()


def test_ts_gain_apply_refusals():
    """An empty class, a feed index outside g, more feeds than one sample's tile holds, mismatched arguments: an error
    and no launch — the output keeps its bits."""
    from driftscan_amd import _lib

    ctx = _ctx()
    g = ctx.to_device(np.ones((1, 1, 3, 5), dtype=np.complex128))
    sky = ctx.to_device(np.ones((1, 1, 2, 5), dtype=np.complex128))
    out = ctx.empty((1, 1, 2, 5), np.complex128)
    out.fill_(7.0)
    with pytest.raises(_lib.DriftMIError, match="class 1 is empty"):
        ctx.ts_gain_apply(g, [0, 2, 2], [[0, 1], [1, 2]], sky, out=out)
    with pytest.raises(_lib.DriftMIError, match="names feed 3 of 3"):
        ctx.ts_gain_apply(g, [0, 1, 2], [[0, 1], [3, 2]], sky, out=out)
    with pytest.raises(_lib.DriftMIError, match="names feed -1"):
        ctx.ts_gain_apply(g, [0, 1, 2], [[0, -1], [1, 2]], sky, out=out)
    with pytest.raises(_lib.DriftMIError, match="class_off"):
        ctx.ts_gain_apply(g, [1, 2, 3], [[0, 1], [1, 2], [0, 2]], sky, out=out)
    assert ctx.lib.dm_ts_gain_tile(10240) == 1 and ctx.lib.dm_ts_gain_tile(10241) == 0
    big = ctx.to_device(np.ones((1, 1, 10241, 1), dtype=np.complex128))
    one = ctx.to_device(np.ones((1, 1, 1, 1), dtype=np.complex128))
    with pytest.raises(_lib.DriftMIError, match="does not fit"):
        ctx.ts_gain_apply(big, [0, 1], [[0, 0]], one)
    wide = ctx.to_device(np.ones((1, 1, 3, 5), dtype=np.complex128))
    two = ctx.to_device(np.ones((2, 3, 2, 5), dtype=np.complex128))
    g2 = ctx.to_device(np.ones((2, 2, 3, 5), dtype=np.complex128))
    for bad in (lambda: ctx.ts_gain_apply(g, [0, 1, 2], [[0, 1]], sky),                      # members short of class_off
                lambda: ctx.ts_gain_apply(g, [0, 1], [[0, 1]], sky),                         # class_off short of npairs
                lambda: ctx.ts_gain_apply(g, [0, 1, 2], [[0, 1], [1, 2]], sky, out=sky),     # in place
                lambda: ctx.ts_gain_apply(g, [0, 1, 2], [[0, 1], [1, 2]], wide[:, :, :2], out=wide[:, :, 1:]),   # overlapping
                lambda: ctx.ts_gain_apply(g2, [0, 1, 2], [[0, 1], [1, 2]], two[:, :2], out=two[:, 1:]),       # in every row
                lambda: ctx.ts_gain_apply(g, [0, 1, 2], [[0, 1], [1, 2]], sky, accumulate=True),
                lambda: ctx.ts_gain_apply(ctx.to_device(np.ones((2, 1, 3, 5), dtype=np.complex128)), [0, 1, 2],
                                          [[0, 1], [1, 2]], sky)):                           # g_nreal neither 1 nor nreal
        with pytest.raises(ValueError):
            bad()
    assert np.array_equal(ctx.to_host(out), np.full((1, 1, 2, 5), 7.0 + 0j))
    assert np.array_equal(ctx.to_host(two), np.ones((2, 3, 2, 5))) and np.array_equal(ctx.to_host(wide), np.ones((1, 1, 3, 5)))
    # frequency slices of one buffer that share nothing, their rows interleaved: accepted
    ctx.ts_gain_apply(g2[:, :1].contiguous(), [0, 1, 2], [[0, 1], [1, 2]], two[:, :1], out=two[:, 2:])
    assert tuple(ctx.ts_gain_apply(g, [0], np.zeros((0, 2)), ctx.empty((1, 1, 0, 5), np.complex128)).shape) == (1, 1, 0, 5)


# ---- the routes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    """The products of tests/test_gpu_tsim.py: 2 cylinders, 3 feeds, 3 frequencies, polarised."""
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("gains")
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


MODEL = dict(sigma_amp=0.05, sigma_phase=0.1, corr_time=1800.0, seed=2)


def test_ensemble_with_gains_is_simulate_with_gains(prod, skyfile):
    """The bar of test_ensemble_without_noise_is_simulate, 1e-10 max |v|, between the device route and the per-m host
    route with the same gain model; and the `gain` dataset of the files against `gains_host`."""
    from driftscan_amd import skysim, storage, timestream

    pm, d = prod
    tel = pm.telescope
    first = 2
    model = skysim.GainModel(**MODEL)
    tss = timestream.simulate_ensemble(pm, str(d / "ens"), 2, maps=[skyfile], ndays=0, first=first, gains=model)
    plain = timestream.simulate(pm, str(d / "plain"), maps=[skyfile], ndays=0)
    ntime = plain.ntime
    # the host route with a sky: zero sigmas make G = n_c / n_c = 1, and the product with it changes no bit
    unit = timestream.simulate(pm, str(d / "unit"), maps=[skyfile], ndays=0, gains=dict(sigma_amp=0.0, sigma_phase=0.0))
    for fi in range(tel.nfreq):
        assert np.abs(plain.timestream_f(fi)).max() > 0 and np.array_equal(unit.timestream_f(fi), plain.timestream_f(fi))
    for i, ts in enumerate(tss):
        ref = timestream.simulate(pm, str(d / ("ens_ref%d" % i)), maps=[skyfile], ndays=0, sky_realisation=first + i, gains=model)
        want_g = skysim.gains_host(model, tel.nfeed, np.arange(tel.nfreq), ntime, 1, first=first + i)[0]
        c = {s: skysim.gain_coeff_host(model, tel.nfeed, np.arange(tel.nfreq), ntime, 1, first + i, s)[0]
             for s in (skysim.STREAM_TS_GAIN_AMP, skysim.STREAM_TS_GAIN_PHASE)}
        amp = 1.0 + np.abs(skysim.gain_series_host(c[skysim.STREAM_TS_GAIN_AMP], ntime))
        gbound = (gc.series_bound(model, c[skysim.STREAM_TS_GAIN_AMP], ntime, model.sigma_amp)
                  + gc.series_bound(model, c[skysim.STREAM_TS_GAIN_PHASE], ntime, model.sigma_phase))[..., None] * amp + 4 * EPS
        for fi in range(tel.nfreq):
            v, w, p = ts.timestream_f(fi), ref.timestream_f(fi), plain.timestream_f(fi)
            print("realisation %d, frequency %d: max |delta| / max |v| = %.3g; gains moved it by %.3g"
                  % (i, fi, np.abs(v - w).max() / np.abs(w).max(), np.abs(w - p).max() / np.abs(p).max()))
            assert np.abs(v - w).max() <= 1e-10 * np.abs(w).max(), (i, fi)
            assert np.abs(w - p).max() > 1e-3 * np.abs(p).max()
            with storage.File(ts._ffile(fi), "r") as f, storage.File(ref._ffile(fi), "r") as g:
                assert sorted(f.keys()) == sorted(g.keys()) and "gain" in f.keys()
                got_g = f["gain"][:]
            assert got_g.shape == (tel.nfeed, ntime) and np.all(np.abs(got_g - want_g[fi]) <= gbound[fi])


def test_zero_sigmas_and_common_phase_leave_the_ensemble_unchanged(prod, skyfile):
    from driftscan_amd import timestream

    pm, _ = prod
    tel = pm.telescope
    ctx = _ctx()
    kw = dict(maps=[skyfile], first=1)
    none = ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=0, **kw))
    zero = ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=0, gains=dict(sigma_amp=0.0, sigma_phase=0.0), **kw))
    assert np.abs(none).max() > 0 and np.array_equal(zero, none)
    # with noise the sky reaches the buffer in one addition instead of two, n + (a + b) instead of (n + a) + b with a, b
    # the sums over m of the two slots: the same value within 2 eps (|n| + |a| + |b|), and |a| + |b| <= sum_m |c_m|
    nz = ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=10, seed=4, **kw))
    zz = ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=10, seed=4, gains=dict(), **kw))
    noise = ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=10, seed=4, first=1))
    csum = np.stack([np.abs(ctx.to_host(ctx.mmode_transform(ctx.to_device(none[r]), tel.mmax))).sum(axis=(0, 2)) for r in range(3)])
    print("zero sigmas beside noise: identical bits: %s" % np.array_equal(zz, nz))
    assert np.all(np.abs(zz - nz) <= 2 * EPS * (np.abs(noise) + csum[..., None]))
    # an explicit phase common to all feeds, per realisation and shared: within the bound of the product with A = 1
    ntime = none.shape[-1]
    off, _ = tel.redundant_pairs()
    bound = 4 * (np.diff(off)[:, None] + 2) * EPS * (1.0 + 2 * EPS) * np.abs(none)
    rng = np.random.default_rng(8)
    for lead in ((), (3,)):
        phase = np.exp(1j * rng.uniform(0, 2 * np.pi, size=lead + (tel.nfreq, 1, ntime)))
        g = np.ascontiguousarray(np.broadcast_to(phase, lead + (tel.nfreq, tel.nfeed, ntime)))
        got = ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=0, gains=g, **kw))
        assert np.all(np.abs(got - none) <= bound)
        got = ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=0, gains=ctx.to_device(g), **kw))
        assert np.all(np.abs(got - none) <= bound)
    with pytest.raises(ValueError):
        timestream.simulate_visibilities(pm, 3, ndays=0, gains=g[:, :, :-1], **kw)
    for bad in (np.concatenate([g, g[:, :1]], axis=1), g[:, :-1]):        # a frequency too many, one too few
        with pytest.raises(ValueError, match="does not fit"):
            timestream.simulate_visibilities(pm, 3, ndays=0, gains=bad, **kw)
        with pytest.raises(ValueError, match="does not fit"):
            timestream.simulate_visibilities(pm, 3, ndays=0, gains=ctx.to_device(np.ascontiguousarray(bad)), **kw)


def test_gains_of_subsets_chunks_and_the_log(prod, skyfile):
    """A frequency subset, a realisation range and one frequency per chunk of gains reproduce the rows of the full call.
    The gains of two calls each lie within the bound of test_gain_draws_and_series_match_the_host of the host values —
    about 1e-13 here, the draw figure — so within 2e-13 of each other; G is bilinear in g and |g| < 1.5, so
    |delta G| <= 2 x 1.5 x 2e-13 < 1e-12, and the results agree within 1e-12 max |sky| (whether the bits agree is
    printed).  The noise is not touched by the gains; `sim_log` has its "gains" entry."""
    from driftscan_amd import skysim, timestream

    pm, _ = prod
    ctx = _ctx()
    model = skysim.GainModel(**MODEL)
    kw = dict(maps=[skyfile], ndays=0, gains=model)
    full = ctx.to_host(timestream.simulate_visibilities(pm, 3, **kw))
    sub = ctx.to_host(timestream.simulate_visibilities(pm, 3, freqs=[0, 2], **kw))
    part = ctx.to_host(timestream.simulate_visibilities(pm, 2, first=1, **kw))
    tiny = ctx.to_host(timestream.simulate_visibilities(pm, 3, chunk_gb=1e-9, **kw))
    scale = 1e-12 * np.abs(full).max()
    print("identical bits: frequency subset %s, realisation range %s, one frequency per chunk %s"
          % (np.array_equal(sub, full[:, [0, 2]]), np.array_equal(part, full[1:3]), np.array_equal(tiny, full)))
    assert np.abs(sub - full[:, [0, 2]]).max() <= scale and np.abs(part - full[1:3]).max() <= scale
    assert np.abs(tiny - full).max() <= scale
    assert not np.any(full[0] == full[1])
    # sky and noise: the noise of the call without gains plus the sky with gains, within one rounding of the sum
    timestream.sim_log = {}
    try:
        both = ctx.to_host(timestream.simulate_visibilities(pm, 3, **dict(kw, ndays=10, seed=5)))
        log = dict(timestream.sim_log)
    finally:
        timestream.sim_log = None
    assert log.get("gains", 0.0) > 0.0 and "synthesis" in log and "noise" in log
    n0 = ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=10, seed=5))
    assert np.all(np.abs(both - (n0 + full)) <= EPS * np.abs(both))
    # noise-only: the gains have nothing to multiply
    assert np.array_equal(ctx.to_host(timestream.simulate_visibilities(pm, 3, ndays=10, seed=5, gains=model)), n0)


def test_pipeline_manager_passes_the_gains_block(prod, skyfile, tmp_path):
    import yaml

    from driftscan_amd import pipeline, skysim, storage, timestream

    pm, d = prod
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=False, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=False),
                timestreams=[dict(name="g", directory=str(tmp_path / "ts_pipe"),
                                  simulate=dict(ndays=0, maps=[skyfile], gains=dict(MODEL)))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = pipeline.PipelineManager.from_configfile(str(cfile))
    p.simulate()
    ref = timestream.simulate(pm, str(tmp_path / "ts_ref"), maps=[skyfile], ndays=0, gains=skysim.GainModel(**MODEL))
    ts = p.timestreams["g"]
    for fi in range(pm.telescope.nfreq):
        v, w = ts.timestream_f(fi), ref.timestream_f(fi)                 # the same host route twice
        assert np.abs(v - w).max() <= 1e-12 * np.abs(w).max()
        with storage.File(ts._ffile(fi), "r") as f:
            assert f["gain"].shape == (pm.telescope.nfeed, ts.ntime)
