"""GPU: Gaussian skies from the covariance models (dm_sky_draw through driftscan_amd/skysim.py):
the unit draws, the correlated product against the longdouble oracle, the bitwise invariances of a coefficient, the roots
of the device eigensolver, the statistics of the realisations, and the way through `timestream.simulate`.

Bound of the product, per element and derived, not tuned: |a - ref| <= 4 (n + 2) eps sum_j |T_ij| |z_j| with
eps = 2^-53, the project's bound of a length-n fp64 inner product (tests/test_gpu_blockvec.py)."""
import numpy as np
import pytest

from test_host_skysim import FREQS4, LMAX, NREAL, check_statistics, models

pytestmark = pytest.mark.gpu

EPS = 2.0**-53
# |T T^T - C|_max <= ROOT_K n eps |C|_2 for the device roots: 4 x the largest ratio seen on the MI355X over the matrices of
# test_device_roots, 1.82 (signal, 4 channels; numpy's largest there is 2.46; DESIGN.md section 4.12 has all eight).  A K
# above 64 would have been a finding about herm_eig on near-singular input, not a bound.
ROOT_K = 4 * 1.82


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _draw(T, jglobal=None, nfreq=None, row0=0, nrows=None, M=None, seed=1, stream=16, first=0, nreal=1):
    """dm_sky_draw of one group into a fresh [nreal, nrows, L, M] array (numpy in, numpy out; T may be a device tensor)."""
    ctx = _ctx()
    Td = ctx.to_device(np.asarray(T, dtype=np.float64)) if isinstance(T, np.ndarray) else T
    L, n = int(Td.shape[0]), int(Td.shape[1])
    jglobal = np.arange(n) if jglobal is None else np.asarray(jglobal)
    nrows = n - row0 if nrows is None else nrows
    M = L if M is None else M
    out = ctx.empty((nreal, nrows, L, M), np.complex128)
    out.fill_(float("nan"))          # every element must be written by the call
    rowoff = np.maximum(np.arange(n) - row0, 0) * L * M
    ctx.sky_draw(Td, jglobal, rowoff, n if nfreq is None else nfreq, row0, nrows, M, seed, stream, first, nreal, out,
                 (nrows * L * M, M, 1))
    return out.cpu().numpy()


def _eye(L, n):
    return np.ascontiguousarray(np.broadcast_to(np.eye(n), (L, n, n)))


@pytest.fixture(scope="module")
def unit_draws():
    return _draw(_eye(LMAX + 1, 4), nreal=NREAL, seed=7)


def test_unit_draws(unit_draws):
    """T = identity gives the draws themselves."""
    from driftscan_amd import skysim

    z, L = unit_draws, LMAX + 1
    assert z.shape == (NREAL, 4, L, L) and np.isfinite(z.view(np.float64)).all()
    assert not z[..., 0].imag.any()                                   # m = 0 is real, exactly
    assert not z[..., np.triu(np.ones((L, L), dtype=bool), 1)].any()   # m > l is empty
    z0 = z[..., 0].real
    print("m = 0: mean(z^2) - 1 = %.4f (bound %.4f)" % (np.mean(z0**2) - 1.0, 5 * np.sqrt(2.0 / z0.size)))
    assert abs(np.mean(z0**2) - 1.0) < 5 * np.sqrt(2.0 / z0.size)
    lower = np.tril(np.ones((L, L), dtype=bool))
    lower[:, 0] = False
    zm = z[..., lower]                                                # 1 <= m <= l
    N = zm.size
    print("m > 0: mean(Re^2) - 1/2 = %.4f, mean(Im^2) - 1/2 = %.4f (bound %.4f), |mean(z z)| = %.4f (bound %.4f)"
          % (np.mean(zm.real**2) - 0.5, np.mean(zm.imag**2) - 0.5, 5 * np.sqrt(0.5 / N), abs(np.mean(zm * zm)), 5 / np.sqrt(N)))
    assert abs(np.mean(zm.real**2) - 0.5) < 5 * np.sqrt(0.5 / N)
    assert abs(np.mean(zm.imag**2) - 0.5) < 5 * np.sqrt(0.5 / N)
    assert abs(np.mean(zm * zm)) < 5 / np.sqrt(N)
    # the numpy restatement of the stream: same counters, libm against the device's log / sincos
    assert np.abs(z - skysim.draws_host(np.arange(4), L, nreal=NREAL, seed=7)).max() < 1e-13


def test_draw_selectors(unit_draws):
    z, I = unit_draws, _eye(LMAX + 1, 4)
    assert np.array_equal(_draw(I, nreal=1, seed=7), z[:1])
    for other in (dict(seed=8), dict(stream=17), dict(first=1)):
        assert not np.array_equal(_draw(I, nreal=1, **dict(dict(seed=7), **other)), z[:1]), other
    assert np.array_equal(_draw(I, nreal=3, seed=7, first=5), z[5:8])
    # a 64-bit seed uses both key words
    assert not np.array_equal(_draw(I, nreal=1, seed=7 + (1 << 32)), z[:1])


def _random_cv(rng, n, L):
    """[1, 1, L, n, n] positive definite blocks of mixed scale."""
    A = rng.standard_normal((L, n, n + 2))
    return (A @ A.transpose(0, 2, 1) / (n + 2))[None, None] * (1.0 + np.arange(L))[:, None, None]


# n = 130 and 1024 are beyond the issue's list: above n = 128 the kernel takes its narrow-chunk instantiation, and 1024 is
# the largest order (the most LDS a workgroup asks for); 1024 runs herm_eig on three matrices only (L = 3) and takes
# 0.24 s on the MI355X, as much as the n = 70 case
@pytest.mark.parametrize("n,Ls", [(1, (1, 2, 20, 70)), (3, (1, 2, 20, 70)), (16, (1, 2, 20, 70)), (17, (1, 2, 20, 70)),
                                  (70, (1, 2, 20, 70)), (130, (2, 20)), (1024, (3,))])
def test_correlate(n, Ls):
    """a = T z with the device's own roots against the longdouble sum, element by element."""
    from driftscan_amd import skysim

    rng = np.random.default_rng(100 + n)
    worst = 0.0
    for L in Ls:
        (Td,) = skysim.covariance_roots(_random_cv(rng, n, L))
        T = Td.cpu().numpy()
        z = _draw(_eye(L, n), seed=3, nreal=1)
        ref = skysim.correlate_host(T, z)
        bound = 4.0 * (n + 2) * EPS * np.einsum("lij,rjlm->rilm", np.abs(T), np.abs(z))
        for M in ([L, L - 3] if L > 3 else [L]):
            a = _draw(Td, seed=3, nreal=1, M=M)
            err = np.abs(a - ref[..., :M]).astype(np.float64)
            ok = err <= bound[..., :M]
            ratio = float((err[bound[..., :M] > 0] / bound[..., :M][bound[..., :M] > 0]).max()) if (bound[..., :M] > 0).any() else 0.0
            worst = max(worst, ratio)
            assert ok.all(), (n, L, M, ratio)
            assert not a[..., np.triu(np.ones((L, L), dtype=bool), 1)[:, :M]].any()
    print("n = %d: largest error / bound = %.3g" % (n, worst))


def test_invariance_bitwise():
    from driftscan_amd import skysim

    rng = np.random.default_rng(5)
    n, L = 17, 20
    (Td,) = skysim.covariance_roots(_random_cv(rng, n, L))
    full = _draw(Td, seed=9, nreal=2)
    assert np.array_equal(_draw(Td, seed=9, nreal=2, row0=5, nrows=7), full[:, 5:12])
    assert np.array_equal(_draw(Td, seed=9, nreal=2, M=9), full[..., :9])
    assert np.array_equal(_draw(Td, seed=9, nreal=1, first=1, row0=16, nrows=1, M=1), full[1:, 16:, :, :1])
    # a group drawn alone against the same group inside draw_alm of a polarised covariance
    cv = models(4)["foreground"]
    F = FREQS4.size
    grp, roots = skysim.groups(cv), skysim.covariance_roots(cv)
    a = skysim.draw_alm(cv, nreal=2, seed=4, stream=skysim.STREAM_SKY_FOREGROUND, roots=roots)
    assert a.shape == (2, F, 4, LMAX + 1, LMAX + 1) and a.dtype == np.complex128
    for jg, T in zip(grp, roots):
        p = int(jg[0]) // F
        alone = _draw(T, jglobal=jg, nfreq=F, seed=4, stream=17, nreal=2)
        assert np.array_equal(alone, a[:, :, p]), p
        assert (not a[:, :, p, :2].any()) == (p in (1, 2))     # E and B start at l = 2
        assert np.abs(a[:, :, p, 2:]).max() > 0
    assert not a[:, :, 3].any()                                # no V
    # the rows of some frequencies and an m cut, from the same draws
    part = skysim.draw_alm(cv, nreal=2, seed=4, stream=17, freqs=[1, 3], mmax=10, roots=roots)
    assert np.array_equal(part, a[:, [1, 3], :, :, :11])
    dev = skysim.draw_alm(cv, nreal=2, seed=4, stream=17, roots=roots, to_host=False)
    assert np.array_equal(dev.cpu().numpy(), a)


def test_joint_group():
    """A T-E cross block makes one group of npol x F components: E and B still start at l = 2, and T carries E's draws."""
    from driftscan_amd import skysim

    cv = models(4)["foreground"].copy()
    cv[0, 1] = 0.1 * cv[1, 1]
    cv[1, 0] = cv[0, 1].transpose(0, 2, 1)
    a = skysim.draw_alm(cv, nreal=1, seed=2)
    b = skysim.draw_alm(models(4)["foreground"], nreal=1, seed=2)
    assert np.isfinite(a.view(np.float64)).all()
    assert not a[:, :, 1:3, :2].any() and np.abs(a[:, :, 0, :2]).max() > 0 and not a[:, :, 3].any()
    assert not np.array_equal(a[:, :, 0, 2:], b[:, :, 0, 2:])


def test_limits():
    """A group above the supported order is refused with an error, before anything runs."""
    from driftscan_amd import _lib

    with pytest.raises(_lib.DriftMIError, match="1024"):
        _draw(_eye(1, 1025))


@pytest.mark.parametrize("nchan", [4, 16])
def test_device_roots(nchan):
    """|T T^T - C|_max <= K n eps |C|_2 for the roots of the device eigensolver on the two committed models."""
    from driftscan_amd import skysim

    eps = np.finfo(np.float64).eps
    freqs = np.linspace(400.0, 430.0, nchan)
    for name, cv in models(4, freqs=freqs).items():
        grp = skysim.groups(cv)
        dev = [T.cpu().numpy() for T in skysim.covariance_roots(cv)]
        host = skysim.covariance_roots(cv, device=False)
        worst = {"device": 0.0, "numpy": 0.0}
        for jg, Td, Th in zip(grp, dev, host):
            C = skysim.group_covariance(cv, jg)
            assert Td.shape == C.shape
            for l in range(C.shape[0]):
                scale = nchan * eps * np.linalg.norm(C[l], 2)
                worst["device"] = max(worst["device"], float(np.abs(Td[l] @ Td[l].T - C[l]).max() / scale))
                worst["numpy"] = max(worst["numpy"], float(np.abs(Th[l] @ Th[l].T - C[l]).max() / scale))
        print("%s, %d channels: |T T^T - C|_max / (n eps |C|_2) = %.3f on the device, %.3f with numpy"
              % (name, nchan, worst["device"], worst["numpy"]))
        assert worst["device"] <= ROOT_K, (name, nchan, worst)


@pytest.mark.parametrize("model", ["foreground", "signal"])
def test_statistics(model):
    """The statistic of the host test on device realisations: same shapes, same bounds, one seed."""
    from driftscan_amd import skysim

    cv = models(1)[model]
    alm = skysim.draw_alm(cv, nreal=NREAL, seed=11)
    check_statistics(alm[:, :, 0], cv[0, 0], "device " + model)


# ---- through the telescope -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    """The small polarised cylinder of tests/test_gpu_timestream.py, with one KL transform."""
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("skysim")
    conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, inverse=True, use_foregrounds=False)])
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    return pm, d


def test_visibility_covariance(prod):
    """<|v|^2> of projected foreground realisations against the diagonal of the projected covariance: the convention
    check of the draws (a factor 2 either way, as a wrong m = 0 or m > 0 normalisation would give, fails)."""
    from driftscan_amd import skysim

    pm, _ = prod
    bt, tel, kl = pm.beamtransfer, pm.telescope, pm.kltransforms["kl"]
    R = 256
    cv = kl.foreground()
    a = skysim.draw_alm(cv, nreal=R, seed=21, stream=skysim.STREAM_SKY_FOREGROUND, mmax=tel.mmax)
    for mi in (0, tel.mmax // 2):
        v2 = np.zeros((tel.nfreq, bt.ntel))
        for r in range(R):
            v2 += np.abs(bt.project_vector_sky_to_telescope(mi, np.ascontiguousarray(a[r, ..., mi]))) ** 2
        v2 /= R
        cov = bt.project_matrix_sky_to_telescope(mi, cv)
        diag = np.einsum("ftft->ft", cov).real
        keep = diag > 1e-12 * diag.max()
        ratio = v2[keep] / diag[keep]
        print("m = %d: <|v|^2> / diag in [%.3f, %.3f] over %d entries" % (mi, ratio.min(), ratio.max(), keep.sum()))
        assert keep.sum() > 0 and np.all(np.abs(ratio - 1.0) < 5 * np.sqrt(2.0 / R)), (mi, ratio.min(), ratio.max())


def test_simulate_skymodels(prod):
    from driftscan_amd import skysim, storage, timestream

    pm, d = prod
    bt, tel, kl = pm.beamtransfer, pm.telescope, pm.kltransforms["kl"]
    mmax = tel.mmax
    ts = timestream.simulate(pm, str(d / "ts_sky"), skymodels=("signal", "foreground"), sky_seed=3, ndays=0)
    ts.generate_mmodes()
    a = (skysim.draw_alm(kl.signal(), seed=3, stream=skysim.STREAM_SKY_SIGNAL)
         + skysim.draw_alm(kl.foreground(), seed=3, stream=skysim.STREAM_SKY_FOREGROUND))[0]
    assert a.shape == (tel.nfreq, tel.num_pol_sky, tel.lmax + 1, tel.lmax + 1)

    def expected(alm, mi):
        want = bt.project_vector_sky_to_telescope(mi, np.ascontiguousarray(alm[..., mi])).reshape(tel.nfreq, 2, tel.npairs)
        if mi == 0:
            want[:, 1] = 0.0
        return want

    for mi in (0, 1, mmax // 2, mmax):
        want = expected(a, mi)
        assert np.abs(want).max() > 0
        assert np.abs(ts.mmode(mi) - want).max() < 1e-10 * np.abs(want).max(), mi
    # the same seed gives the same files; another realisation differs
    again = timestream.simulate(pm, str(d / "ts_sky2"), skymodels=("signal", "foreground"), sky_seed=3, ndays=0)
    other = timestream.simulate(pm, str(d / "ts_sky3"), skymodels=("signal", "foreground"), sky_seed=3, ndays=0,
                                sky_realisation=1)
    for fi in range(tel.nfreq):
        assert np.array_equal(again.timestream_f(fi), ts.timestream_f(fi))
        assert not np.array_equal(other.timestream_f(fi), ts.timestream_f(fi))
    # with a map as well, the sky is the sum; the map comes from gaussian_sky through write_sky
    nside = 16
    maps = skysim.gaussian_sky(kl.foreground(), nside, seed=8, stream=skysim.STREAM_SKY_FOREGROUND)
    skyfile = str(d / "gsky.hdf5")
    skysim.write_sky(skyfile, maps[0])
    with storage.File(skyfile, "r") as f:
        assert f["map"].shape == (tel.nfreq, 4, 12 * nside * nside)
    only_map = timestream.simulate(pm, str(d / "ts_map"), maps=[skyfile], ndays=0)
    both = timestream.simulate(pm, str(d / "ts_both"), maps=[skyfile], skymodels=["signal"], sky_seed=3, ndays=0)
    only_sig = timestream.simulate(pm, str(d / "ts_sig"), skymodels="signal", klname="kl", sky_seed=3, ndays=0)
    assert only_map.ntime == 2 * mmax + 1
    for fi in range(tel.nfreq):
        total = only_map.timestream_f(fi) + only_sig.timestream_f(fi)
        assert np.abs(both.timestream_f(fi) - total).max() < 1e-10 * np.abs(total).max()
    with pytest.raises(ValueError):
        timestream.simulate(pm, str(d / "ts_bad"), skymodels=("galaxy",), ndays=0)


def test_gaussian_sky():
    from driftscan_amd import healpix, skysim

    nside = 16
    cv = models(4)["foreground"]
    maps = skysim.gaussian_sky(cv, nside, nreal=2, seed=6)
    assert maps.shape == (2, FREQS4.size, 4, 12 * nside * nside) and maps.dtype == np.float64
    alm = skysim.draw_alm(cv, nreal=2, seed=6)
    for r in range(2):   # gaussian_sky IS that call on the device coefficients: the same passes, the same bits
        assert np.array_equal(maps[r], healpix.sphtrans_inv_sky(alm[r], nside)), r
    assert np.abs(maps[:, :, :3]).max() > 0 and not maps[:, :, 3].any()
    # a pass per frequency (max_bytes below one frequency) gives the same maps, to the chunking invariance of the synthesis
    # (test_gpu_sht_synth.py)
    assert np.abs(skysim.gaussian_sky(cv, nside, nreal=2, seed=6, max_bytes=1) - maps).max() <= 1e-15 * np.abs(maps).max()
