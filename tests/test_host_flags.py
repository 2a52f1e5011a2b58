"""Flagged timestreams on the host: the two numpy statements of the weighted m-mode estimate
against each other, scipy and extended precision; the ridge identities and the singular-row rule; `skysim.FlagModel`; the
checker of tests/flags_cases.py rejecting doctored answers.  No GPU."""
import numpy as np
import pytest

import flags_cases as fc

EPS = fc.EPS


def _ts():
    from driftscan_amd import timestream

    return timestream


CASES = [("a", 17, 0), ("a", 65, 1), ("a", 257, 2), ("b", 65, 0), ("c", 65, 0), ("d", 17, 0), ("d", 64, 0), ("a", 1, 0),
         ("a", 2, 0), ("a", 3, 1)]


@pytest.mark.parametrize("kind,n,seed", CASES)
def test_levinson_host_within_the_bound(kind, n, seed):
    cs = fc.case(kind, n, seed)
    x, info = _ts().toeplitz_levinson_host(cs["col"], cs["B"])
    assert info == 0
    err, bound = fc.check(x, cs, what="toeplitz_levinson_host")
    print("(%s) n = %d: cond %.3g, e_ref %.3g, worst error / bound %.3g" % (kind, n, cs["cond"], cs["e_ref"].max(),
                                                                            (err / bound).max()))


def test_levinson_host_batches_and_shapes():
    a, b = fc.case("a", 17, 0), fc.case("a", 17, 1)
    cols = np.stack([a["col"], b["col"]])
    B = np.stack([a["B"][:3], b["B"][:3]])
    x, info = _ts().toeplitz_levinson_host(cols, B)
    assert x.shape == B.shape and info.shape == (2,) and not info.any()
    for i, cs in enumerate((a, b)):
        x1, i1 = _ts().toeplitz_levinson_host(cs["col"], cs["B"][:3])
        assert np.array_equal(x[i], x1) and i1 == 0
    x0, _ = _ts().toeplitz_levinson_host(a["col"], a["B"][0])
    assert x0.shape == (17,) and np.array_equal(x0, x[0, 0])


def test_levinson_host_reports_a_system_that_is_not_positive_definite():
    for n in (2, 5, 17):
        cs_col = fc.column_of("e", n)
        x, info = _ts().toeplitz_levinson_host(cs_col, np.ones((2, n)))
        assert info == 1 and not x.any()
    bad = np.array([0.0, 0.5, 0.1], dtype=np.complex128)
    x, info = _ts().toeplitz_levinson_host(bad, np.ones(3))
    assert info == 3 and not x.any()                  # c_0 <= 0: the order, which no step carries


@pytest.mark.parametrize("kind,n,seed", [("a", 17, 0), ("b", 65, 0), ("c", 65, 0)])
def test_checker_rejects_a_doctored_answer(kind, n, seed):
    cs = fc.case(kind, n, seed)
    x, _ = _ts().toeplitz_levinson_host(cs["col"], cs["B"])
    fc.check(x, cs)
    bad = x.copy()
    bad[0, n // 2] += 1e3 * cs["bound"][0] * np.linalg.norm(x[0])
    with pytest.raises(AssertionError):
        fc.check(bad, cs)
    worse = x.copy()
    worse[1, 0] = np.nan
    with pytest.raises(AssertionError):
        fc.check(worse, cs)
    just = x.copy()                                     # twice the bound in one element is caught as well
    just[2, 0] += 2.0 * cs["bound"][2] * np.linalg.norm(np.asarray(cs["Xref"][2], dtype=np.complex128))
    with pytest.raises(AssertionError):
        fc.check(just, cs)


def test_long_double_reference_solves_its_system():
    cs = fc.case("a", 65, 1)
    T = fc.toeplitz(cs["col"], np.clongdouble)
    res = np.abs(T @ cs["Xref"].T - cs["B"].T.astype(np.clongdouble)).max()
    assert float(res) < 1e3 * np.finfo(np.longdouble).eps * float(np.abs(cs["B"]).max()) * 65


@pytest.mark.parametrize("mmax,ntime,nf,npairs", [(0, 1, 1, 1), (2, 9, 2, 3), (8, 40, 3, 5), (32, 160, 2, 4)])
def test_weighted_host_against_levinson_and_scipy(mmax, ntime, nf, npairs):
    import scipy.linalg

    rng = np.random.default_rng(mmax + 7)
    N = 2 * mmax + 1
    x, a = fc.band_limited(rng, nf, npairs, mmax, ntime)
    x = x + 0.1 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))      # not band limited
    w = np.stack([fc.random_mask(ntime, 0.25, 10 * f + p) for f in range(nf) for p in range(npairs)]).reshape(nf, npairs, ntime)
    if ntime == 1:
        w[:] = 1.0
    w = w * (0.5 + rng.random(w.shape))               # real-valued weights
    host, info, bounds = fc.row_bounds(x, w, mmax)
    assert not info.any()
    got = fc.modes_unlayout(host)
    k, t = np.arange(-mmax, mmax + 1), np.arange(ntime)
    F = np.exp(2j * np.pi * ((t[:, None] * k[None, :]) % ntime) / ntime)
    for f in range(nf):
        for p in range(npairs):
            col = fc.column(w[f, p], N)
            b = F.conj().T @ (w[f, p] * x[f, p]) / ntime
            lev, li = _ts().toeplitz_levinson_host(col, b)
            assert li == 0
            assert np.linalg.norm(lev - got[f, p]) <= bounds[f, p]
            assert np.linalg.norm(scipy.linalg.solve_toeplitz(col, b) - got[f, p]) <= bounds[f, p]
    assert not host[0, :, 1].any()


def test_weighted_host_recovers_a_band_limited_signal_where_the_plain_transform_fails():
    for mmax, ntime in ((8, 40), (32, 160)):
        rng = np.random.default_rng(ntime)
        x, a = fc.band_limited(rng, 1, 2, mmax, ntime)
        w = fc.random_mask(ntime, 0.25, 3)
        host, info = _ts().mmodes_weighted_host(x * w, w, mmax)
        truth = fc.modes_layout(a, mmax)
        assert not info.any()
        assert np.abs(host - truth).max() < 1e-10 * np.abs(truth).max()
        plain, _ = _ts().mmodes_weighted_host(x * w, np.ones(ntime), mmax)        # zero-filled data, plain transform
        assert np.abs(plain - truth).max() > 0.1 * np.abs(truth).max()


def test_ridge_identities():
    rng = np.random.default_rng(5)
    mmax, ntime = 4, 12
    x = rng.standard_normal((2, 3, ntime)) + 1j * rng.standard_normal((2, 3, ntime))
    plain = np.fft.fft(x, axis=-1) / ntime
    ref = np.zeros((mmax + 1, 2, 2, 3), dtype=np.complex128)
    ref[:, :, 0] = plain[:, :, : mmax + 1].transpose(2, 0, 1)
    ref[1:, :, 1] = plain[:, :, : -mmax - 1 : -1].conj().transpose(2, 0, 1)
    for wshape in ((ntime,), (2, ntime), (2, 3, ntime)):
        m0, info = _ts().mmodes_weighted_host(x, np.ones(wshape), mmax)
        assert not info.any() and np.abs(m0 - ref).max() <= 64 * EPS * np.abs(ref).max()
        m1, _ = _ts().mmodes_weighted_host(x, np.ones(wshape), mmax, ridge=0.25)
        assert np.abs(m1 - ref / 1.25).max() <= 64 * EPS * np.abs(ref).max()
    # the eigenvalues of A lie in [rho c_0, 1 + rho c_0] for 0 <= w <= 1
    w = rng.random(ntime)
    for rho in (0.0, 0.5):
        ev = np.linalg.eigvalsh(fc.toeplitz(fc.column(w, 2 * mmax + 1, ridge=rho)))
        c0 = w.mean()
        assert ev[0] >= rho * c0 - 16 * EPS and ev[-1] <= 1.0 + rho * c0 + 16 * EPS


def test_singular_rows_are_not_solved_and_bad_input_is_refused():
    rng = np.random.default_rng(6)
    mmax, ntime = 3, 12
    N = 2 * mmax + 1
    x = rng.standard_normal((1, 3, ntime)) + 1j * rng.standard_normal((1, 3, ntime))
    w = np.ones((1, 3, ntime))
    w[0, 0] = 0.0                                    # fully flagged
    w[0, 1, N - 1 :] = 0.0                           # N - 1 samples left
    modes, info = _ts().mmodes_weighted_host(x, w, mmax)
    assert info.tolist() == [[-1, -1, 0]]
    assert not modes[:, :, :, :2].any() and modes[:, :, 0, 2].any()
    modes, info = _ts().mmodes_weighted_host(x, w, mmax, ridge=1e-3)     # a ridge makes a row with any sample solvable
    assert info.tolist() == [[-1, 0, 0]] and not modes[..., 0].any() and modes[:, :, 0, 1].any()
    for bad in (-np.ones(ntime), np.full(ntime, np.nan), np.ones(ntime + 1), np.ones((2, ntime))):
        with pytest.raises(ValueError):
            _ts().mmodes_weighted_host(x, bad, mmax)
    with pytest.raises(ValueError):
        _ts().mmodes_weighted_host(x[..., : N - 1], np.ones(N - 1), mmax)


# ---- FlagModel ----------------------------------------------------------------------------------------------------------------
def test_flag_model_is_deterministic_and_frequency_local():
    from driftscan_amd import skysim

    fm = skysim.FlagModel(fraction=0.3, burst=4, seed=11)
    full = fm.mask(200, range(6))
    assert full.shape == (6, 200) and full.dtype == np.float64 and set(np.unique(full)) <= {0.0, 1.0}
    assert np.array_equal(full, skysim.FlagModel(fraction=0.3, burst=4, seed=11).mask(200, range(6)))
    assert np.array_equal(fm.mask(200, [4, 1]), full[[4, 1]])
    assert not np.array_equal(full, skysim.FlagModel(fraction=0.3, burst=4, seed=12).mask(200, range(6)))
    assert not np.array_equal(full[0], full[1])
    assert skysim.FlagModel().mask(50, range(3)).min() == 1.0          # the defaults flag nothing
    assert skysim.STREAM_TS_FLAG == 27


def test_flag_model_from_config_and_checks():
    from driftscan_amd import skysim

    fm = skysim.FlagModel.from_config(dict(fraction=0.2, burst=3, windows=[[6, 18]], seed=5))
    assert (fm.fraction, fm.burst, fm.windows, fm.seed) == (0.2, 3, ((6.0, 18.0),), 5)
    assert np.array_equal(fm.mask(48, [0, 2]), skysim.FlagModel(0.2, 3, ((6, 18),), 5).mask(48, [0, 2]))
    with pytest.raises(ValueError):
        skysim.FlagModel.from_config(dict(fraction=0.2, bursts=3))
    for bad in (dict(fraction=-0.1), dict(fraction=1.0), dict(burst=0), dict(windows=[(1, 25)])):
        with pytest.raises(ValueError):
            skysim.FlagModel(**bad)
    w = skysim.as_weights(dict(fraction=0.2, seed=1), 2, 3, 30, [0, 1])
    assert w.shape == (2, 1, 30)
    assert skysim.as_weights(np.ones((2, 30)), 2, 3, 30, [0, 1]).shape == (2, 1, 30)
    for bad in (np.ones(29), -np.ones(30), np.full((2, 3, 30), np.inf)):
        with pytest.raises(ValueError):
            skysim.as_weights(bad, 2, 3, 30, [0, 1])


def test_flag_model_fraction_is_binomial():
    from driftscan_amd import skysim

    nf, ntime, frac = 64, 4096, 0.2
    m = skysim.FlagModel(fraction=frac, burst=1, seed=3).mask(ntime, range(nf))
    n = nf * ntime
    sigma = np.sqrt(frac * (1 - frac) / n)
    got = 1.0 - m.mean()
    print("flagged fraction %.5f, expectation %.5f, sigma %.5f" % (got, frac, sigma))
    assert abs(got - frac) <= 4 * sigma
    # with bursts the marginal probability stays `fraction` (samples are no longer independent: a wide band here)
    mb = skysim.FlagModel(fraction=frac, burst=5, seed=3).mask(ntime, range(nf))
    assert abs(1.0 - mb.mean() - frac) <= 4 * sigma * np.sqrt(2 * 5)


def test_flag_model_bursts_are_cyclic_runs():
    from driftscan_amd import skysim

    burst, ntime = 7, 64
    fm = skysim.FlagModel(fraction=0.15, burst=burst, seed=2)
    m = fm.mask(ntime, range(40))
    wrapped = 0
    for row in m:
        flagged = row == 0
        if flagged.all() or not flagged.any():
            continue
        start = int(np.flatnonzero(~flagged)[0])              # rotate so that the row starts with a kept sample
        r = np.roll(flagged, -start)
        edges = np.flatnonzero(np.diff(np.concatenate([[0], r.astype(int), [0]])))
        runs = edges[1::2] - edges[::2]
        assert runs.min() >= burst                            # every run is a union of whole bursts
        wrapped += int(flagged[0] and flagged[-1])
    assert wrapped > 0                                        # some burst runs over the end of the day


def test_flag_model_windows():
    from driftscan_amd import skysim

    m = skysim.FlagModel(windows=((6.0, 18.0),)).mask(48, [0, 5])
    assert np.array_equal(m[0], m[1])
    assert np.array_equal(np.flatnonzero(m[0] == 0), np.arange(12, 36))
    m = skysim.FlagModel(windows=((22.0, 2.0), (12.0, 12.5))).mask(48, [3])[0]
    assert np.array_equal(np.flatnonzero(m == 0), np.array([0, 1, 2, 3, 24, 44, 45, 46, 47]))


# ---- the pipeline on the host ---------------------------------------------------------------------------------------------------
def _product_dir(tmp_path):
    import yaml

    prod = tmp_path / "prod"
    prod.mkdir()
    conf = dict(config=dict(beamtransfers=False, kltransform=False, psfisher=False, output_directory=str(prod)),
                telescope=dict(type="UnpolarisedCylinder", num_freq=2, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4, tsys=1.0))
    (prod / "config.yaml").write_text(yaml.dump(conf))
    return prod


def test_pipeline_reads_the_ridge_and_hands_weights_to_simulate(tmp_path, monkeypatch):
    import yaml

    from driftscan_amd import timestream
    from driftscan_amd.pipeline import PipelineManager

    prod = _product_dir(tmp_path)
    wconf = dict(fraction=0.2, burst=3, seed=5)
    conf = dict(config=dict(product_directory=str(prod)),
                timestreams=[dict(name="a", directory=str(tmp_path / "ts_a"), mmode_ridge=1e-3,
                                  simulate=dict(ndays=0, resolution=600.0, weights=wconf)),
                             dict(name="b", directory=str(tmp_path / "ts_b"))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = PipelineManager.from_configfile(str(cfile))
    assert p.timestreams["a"].mmode_ridge == 1e-3 and p.timestreams["b"].mmode_ridge == 0.0
    seen = {}
    monkeypatch.setattr(timestream, "simulate", lambda m, outdir, **kw: seen.update(kw, outdir=outdir))
    p.simulate()
    assert seen["weights"] == wconf and seen["resolution"] == 600.0 and seen["outdir"] == str(tmp_path / "ts_a")


def _write_timestream(ts, x, w=None):
    import os

    from driftscan_amd import storage

    for fi in range(x.shape[0]):
        os.makedirs(ts._fdir(fi), exist_ok=True)
        with storage.File(ts._ffile(fi), "w") as f:
            f.create_dataset("timestream", data=np.ascontiguousarray(x[fi]))
            if w is not None:
                f.create_dataset("weight", data=np.ascontiguousarray(w[fi]))
            f.attrs["ntime"] = x.shape[-1]


def test_host_route_uses_the_weights_of_the_files(tmp_path):
    from driftscan_amd import manager, storage, timestream

    pm = manager.ProductManager.from_config(str(_product_dir(tmp_path)))
    tel = pm.telescope
    mmax, nfreq, npairs = int(tel.mmax), int(tel.nfreq), int(tel.npairs)
    N = 2 * mmax + 1
    ntime = int(np.ceil(2.5 * N))
    rng = np.random.default_rng(9)
    x, a = fc.band_limited(rng, nfreq, npairs, mmax, ntime)
    w = np.stack([fc.random_mask(ntime, 0.25, 3 * f + p) for f in range(nfreq) for p in range(npairs)]).reshape(x.shape)
    w[0, 0] = 0.0                                                # a dead baseline
    truth = fc.modes_layout(a, mmax)
    truth[:, 0, :, 0] = 0.0
    flagged = timestream.Timestream(str(tmp_path / "ts_w"), pm)
    _write_timestream(flagged, x * w, w)
    assert np.array_equal(flagged.weight_f(1), w[1])
    flagged.generate_mmodes()
    got = np.stack([flagged.mmode(mi) for mi in range(mmax + 1)])
    assert np.abs(got - truth).max() <= 1e-10 * np.abs(truth).max()
    ref, rinfo = timestream.mmodes_weighted_host(x * w, w, mmax)
    assert np.array_equal(got, ref)
    with storage.File(flagged.output_directory + "/mmodes/weights.hdf5", "r") as f:
        assert np.array_equal(f["nkept"][:], np.count_nonzero(w, axis=-1)) and np.array_equal(f["info"][:], rinfo)
        assert f["info"][:][0, 0] == -1 and np.count_nonzero(f["info"][:]) == 1
    # a ridge set on the object reaches the estimate
    ridged = timestream.Timestream(str(tmp_path / "ts_w"), pm)
    ridged.output_directory = str(tmp_path / "out_ridge")
    ridged.mmode_ridge = 0.5
    ridged.generate_mmodes()
    ref, _ = timestream.mmodes_weighted_host(x * w, w, mmax, ridge=0.5)
    assert np.array_equal(np.stack([ridged.mmode(mi) for mi in range(mmax + 1)]), ref)
    # files without `weight`: the plain transform, and no summary file
    import os

    plain = timestream.Timestream(str(tmp_path / "ts_c"), pm)
    _write_timestream(plain, x)
    assert plain.weight_f(0) is None
    plain.generate_mmodes()
    row = np.fft.fft(x, axis=-1) / ntime
    for mi in range(mmax + 1):
        v = plain.mmode(mi)
        assert np.array_equal(v[:, 0], row[:, :, mi])
        assert np.array_equal(v[:, 1], row[:, :, -mi].conj() if mi else np.zeros_like(v[:, 1]))
    assert not os.path.exists(plain.output_directory + "/mmodes/weights.hdf5")
