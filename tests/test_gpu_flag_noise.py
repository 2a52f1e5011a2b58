"""Noise of the weighted m-modes of flagged timestreams on the device: dm_toeplitz_solve_diag over
the size and batch edges of dm_toeplitz_solve (the same solutions bit for bit, the diagonal of the inverse against a dense
inverse in long double within the bound of tests/flag_noise_cases.py), its batch independence, failures and refusals;
the inflation of `Context.mmode_transform_weighted` against the host statement; the inflation files of the two pipeline
routes; and `Timestream.flag_noise_bias` — exact identities on the products of tests/test_gpu_powerspectrum.py's
configuration and a Monte-Carlo on noise-only flagged data."""
import os
import shutil

import numpy as np
import pytest

import flag_noise_cases as fn
import flags_cases as fc

pytestmark = pytest.mark.gpu

EPS = fc.EPS
GUARD = 7.25 - 3.5j
DGUARD = -123.5


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _solve_diag_guarded(ctx, col, B, b_given=True):
    """dm_toeplitz_solve_diag on buffers with guard elements around b, diag and info: (x, d, info) as numpy."""
    import torch

    batch, nrhs, n = B.shape
    g = 64
    buf = torch.full((batch * nrhs * n + 2 * g,), GUARD, dtype=torch.complex128, device="cuda")
    buf[g : g + batch * nrhs * n] = ctx.to_device(B).view(-1)
    dbuf = torch.full((batch * n + 2 * g,), DGUARD, dtype=torch.float64, device="cuda")
    ibuf = torch.full((batch + 2 * g,), -77, dtype=torch.int32, device="cuda")
    cdev = ctx.to_device(col)
    rc = ctx.lib.dm_toeplitz_solve_diag(ctx.h, n, nrhs, batch, ctx.ptr(cdev), ctx.ptr(buf[g:]) if b_given else ctx.ptr(None),
                                        ctx.ptr(dbuf[g:]), ctx.ptr(ibuf[g:]))
    ctx.check(rc, "dm_toeplitz_solve_diag")
    ctx.sync()
    hb, hd, hi = buf.cpu().numpy(), dbuf.cpu().numpy(), ibuf.cpu().numpy()
    assert np.all(hb[:g] == GUARD) and np.all(hb[-g:] == GUARD), "guard elements around b were written"
    assert np.all(hd[:g] == DGUARD) and np.all(hd[-g:] == DGUARD), "guard elements around diag were written"
    assert np.all(hi[:g] == -77) and np.all(hi[-g:] == -77), "guard elements around info were written"
    return hb[g : g + batch * nrhs * n].reshape(batch, nrhs, n), hd[g:-g].reshape(batch, n), hi[g:-g]


def _solve_plain(ctx, col, B):
    x = ctx.to_device(B).clone()
    info = ctx.zeros((B.shape[0],), np.int32)
    ctx.check(ctx.lib.dm_toeplitz_solve(ctx.h, B.shape[2], B.shape[1], B.shape[0], ctx.ptr(ctx.to_device(col)), ctx.ptr(x),
                                        ctx.ptr(info)), "dm_toeplitz_solve")
    return x.cpu().numpy(), info.cpu().numpy()


# ---- 1. sizes and batches -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 65, 128, 129, 257, 384, 385, 513])
def test_solve_diag_sizes_and_batches(n):
    ctx = _ctx()
    spool, dpool = fc.pool(n), fn.pool(n)
    worst = 0.0
    for nrhs in (0, 1, 3):
        for batch in (1, 5, 300):
            which = [(3 * s + nrhs) % len(spool) for s in range(batch)]          # mixed systems in one batch
            col = np.stack([spool[i]["col"] for i in which])
            B = np.stack([spool[i]["B"][:nrhs] for i in which]).reshape(batch, nrhs, n)
            x, d, info = _solve_diag_guarded(ctx, col, B, b_given=nrhs > 0)
            assert not info.any(), "info %s" % (info[info != 0],)
            if nrhs > 0:                                                         # the solutions of the entry without diag
                xp, ip = _solve_plain(ctx, col, B)
                assert np.array_equal(x, xp) and np.array_equal(info, ip)
            first = {}
            for s, i in enumerate(which):
                if i in first:                                                   # a repeated system repeats its bits
                    assert np.array_equal(d[s], d[first[i]])
                    continue
                first[i] = s
                worst = max(worst, fn.check(d[s], dpool[i], what="dm_toeplitz_solve_diag nrhs %d batch %d" % (nrhs, batch)))
                if dpool[i]["kind"] == "d":
                    assert np.all(d[s] == 1.0)
    print("n = %d: worst diagonal error / bound %.3g (K = %g)" % (n, worst, fn.K))


def test_inverse_diag_through_the_context_with_ridge():
    ctx = _ctx()
    cs = fn.diag_case("b", 65, 0)
    d, info = ctx.toeplitz_inverse_diag(cs["col"][None].copy())
    assert int(info.cpu()[0]) == 0 and tuple(d.shape) == (1, 65)
    fn.check(d.cpu().numpy()[0], cs, what="Context.toeplitz_inverse_diag")
    plain = fc.column(fc.gap_mask(160, 40, 16), 65)                             # system (c): the ridge added by the call
    cc, sc = fn.diag_case("c", 65, 0), fc.case("c", 65, 0)
    d, info = ctx.toeplitz_inverse_diag(plain[None], ridge=1e-6)
    assert int(info.cpu()[0]) == 0
    fn.check(d.cpu().numpy()[0], cc, what="Context.toeplitz_inverse_diag ridge")
    x, info, d2 = ctx.toeplitz_solve(plain[None], sc["B"][None].copy(), ridge=1e-6, diag=True)
    x0, i0 = ctx.toeplitz_solve(plain[None], sc["B"][None].copy(), ridge=1e-6)
    assert np.array_equal(x.cpu().numpy(), x0.cpu().numpy()) and np.array_equal(info.cpu().numpy(), i0.cpu().numpy())
    assert np.array_equal(d2.cpu().numpy(), d.cpu().numpy())                    # the same bits with and without b


# ---- 2. batch independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nrhs", [(17, 3), (513, 2)])
def test_solve_diag_batch_independence(n, nrhs):
    ctx = _ctx()
    rng = np.random.default_rng(n)
    cols = np.stack([fc.column_of("a", n, s % 3) for s in range(3)])
    B = rng.standard_normal((300, nrhs, n)) + 1j * rng.standard_normal((300, nrhs, n))
    col = cols[np.arange(300) % 3].copy()
    probe_col = fc.column_of("a", n, 1)
    probe_b = rng.standard_normal((nrhs, n)) + 1j * rng.standard_normal((nrhs, n))
    xs, info, solo = ctx.toeplitz_solve(probe_col[None], probe_b[None], diag=True)
    xs, solo = xs.cpu().numpy()[0], solo.cpu().numpy()[0]
    assert int(info.cpu()[0]) == 0
    fn.check(solo, fn.diag_case("a", n, 1))
    alone, _ = ctx.toeplitz_inverse_diag(probe_col[None])
    assert np.array_equal(alone.cpu().numpy()[0], solo)                           # without right-hand sides
    one = ctx.toeplitz_solve(probe_col[None], probe_b[None, :1], diag=True)[2]
    assert np.array_equal(one.cpu().numpy()[0], solo)                             # with another number of them
    for pos in (0, 7, 299):
        c2, b2 = col.copy(), B.copy()
        c2[pos], b2[pos] = probe_col, probe_b
        x, info, d = ctx.toeplitz_solve(c2, b2, diag=True)
        assert not info.cpu().numpy().any()
        assert np.array_equal(d.cpu().numpy()[pos], solo), "position %d of a batch of 300" % pos
        assert np.array_equal(x.cpu().numpy()[pos], xs)
        d0, _ = ctx.toeplitz_inverse_diag(c2[: pos + 1])                          # in another batch
        assert np.array_equal(d0.cpu().numpy()[pos], solo)


# ---- 3. failure and refusals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 513])
def test_solve_diag_reports_an_indefinite_system(n):
    ctx = _ctx()
    spool, dpool = fc.pool(n), fn.pool(n)
    col = np.stack([spool[s % len(spool)]["col"] for s in range(9)])
    B = np.stack([spool[s % len(spool)]["B"][:3] for s in range(9)])
    col[4] = fc.column_of("e", n)
    col[6] = 0.0
    col[6, 1] = 0.5                                                               # c_0 = 0
    x, d, info = _solve_diag_guarded(ctx, col, B)
    assert info[4] == 1 and info[6] == n and not x[4].any() and not x[6].any()
    assert np.all(d[4] == 0.0) and np.all(d[6] == 0.0)
    assert not info[[0, 1, 2, 3, 5, 7, 8]].any()
    for s in (3, 5, 7):
        sx, sd, _ = _solve_diag_guarded(ctx, col[s : s + 1], B[s : s + 1])
        assert np.array_equal(sx[0], x[s]) and np.array_equal(sd[0], d[s])
        fn.check(d[s], dpool[s % len(dpool)])
        fc.check(x[s], spool[s % len(spool)])


def test_solve_diag_arguments():
    ctx = _ctx()
    lib = ctx.lib
    col, b, info = ctx.zeros((2, 4), np.complex128), ctx.zeros((2, 1, 4), np.complex128), ctx.zeros((2,), np.int32)
    col[:, 0] = 2.0
    diag = ctx.zeros((2, 4), np.float64)
    # nrhs = 0 with a non-null b is accepted, and b is left alone
    b[:] = GUARD
    assert lib.dm_toeplitz_solve_diag(ctx.h, 4, 0, 2, ctx.ptr(col), ctx.ptr(b), ctx.ptr(diag), ctx.ptr(info)) == 0
    ctx.sync()
    assert np.all(diag.cpu().numpy() == 0.5) and not info.cpu().numpy().any() and np.all(b.cpu().numpy() == GUARD)
    for n, nrhs, batch, c, bb, dd, ii in ((4, -1, 2, col, b, diag, info), (4, 1, 2, col, b, None, info),
                                          (4, 0, 2, col, None, None, info), (0, 0, 2, col, b, diag, info),
                                          (4, 1, 2, col, None, diag, info), (4, 0, 2, None, b, diag, info),
                                          (4, 0, 2, col, b, diag, None), (4, 0, -1, col, b, diag, info),
                                          (4, lib.dm_toeplitz_max_rhs(4) + 1, 2, col, b, diag, info),
                                          (5200, 0, 1, col, b, diag, info)):
        rc = lib.dm_toeplitz_solve_diag(ctx.h, n, nrhs, batch, ctx.ptr(c), ctx.ptr(bb), ctx.ptr(dd), ctx.ptr(ii))
        assert rc == -1 and b"dm_toeplitz_solve_diag" in lib.dm_last_error(ctx.h), (n, nrhs, batch)
    # the entry without the diagonal still refuses nrhs = 0
    assert lib.dm_toeplitz_solve(ctx.h, 4, 0, 2, ctx.ptr(col), ctx.ptr(b), ctx.ptr(info)) == -1
    assert b"dm_toeplitz_solve: nrhs = 0" in lib.dm_last_error(ctx.h)
    assert lib.dm_toeplitz_solve_diag(ctx.h, 4, 0, 0, ctx.ptr(None), ctx.ptr(None), ctx.ptr(None), ctx.ptr(None)) == 0
    with pytest.raises(ValueError):
        ctx.toeplitz_inverse_diag(np.ones((2, 4)), ridge=-1.0)
    with pytest.raises(ValueError):
        ctx.toeplitz_inverse_diag(np.ones(4))


# ---- 4. the weighted transform against the host -------------------------------------------------------------------------------
@pytest.mark.parametrize("mmax,ntime,nf,npairs", [(0, 1, 1, 1), (2, 9, 2, 3), (8, 40, 3, 5), (32, 160, 2, 4)])
@pytest.mark.parametrize("wkind", ["pair", "freq", "time"])
def test_weighted_transform_inflation_against_the_host(mmax, ntime, nf, npairs, wkind):
    from driftscan_amd import timestream

    ctx = _ctx()
    N = 2 * mmax + 1
    rng = np.random.default_rng(100 * mmax + len(wkind))
    x = rng.standard_normal((nf, npairs, ntime)) + 1j * rng.standard_normal((nf, npairs, ntime))
    frac = 0.25 if ntime > 1 else 0.0
    if wkind == "pair":
        w = np.stack([fc.random_mask(ntime, frac, 10 * f + p) for f in range(nf) for p in range(npairs)])
        w = w.reshape(nf, npairs, ntime)
        if npairs >= 3:
            w[0, 1] = 1.0                                                        # complete data
            w[0, 2] = 0.25                                                       # constant weight
            w[-1, 0] = 0.0                                                       # a fully flagged baseline
            w[-1, 1] = 0.0
            w[-1, 1, : N - 1] = 1.0                                              # and one with N - 1 samples
    elif wkind == "freq":
        w = np.stack([fc.random_mask(ntime, frac, 50 + f) for f in range(nf)])
    else:
        w = fc.random_mask(ntime, frac, 77)
    X = ctx.to_device(x)
    hmodes, hinfo, hinfl = timestream.mmodes_weighted_host(x, w, mmax, inflation=True)
    out, info, infl = ctx.mmode_transform_weighted(X, w, mmax, inflation=True)
    o2, i2 = ctx.mmode_transform_weighted(X, w, mmax)
    assert np.array_equal(out.cpu().numpy(), o2.cpu().numpy()) and np.array_equal(info.cpu().numpy(), i2.cpu().numpy())
    infl, info = infl.cpu().numpy(), info.cpu().numpy()
    assert infl.shape == (mmax + 1, nf, 2, npairs) and infl.dtype == np.float64 and np.array_equal(info, hinfo)
    assert np.all(infl[0, :, 1] == 1.0)
    # per row the bound of the solver tests: K max(e_ref, EPS cond) against long double, for the device and for the host
    wb = np.broadcast_to(w[:, None, :] if w.ndim == 2 else w, x.shape)
    d_dev, d_host = fc.modes_unlayout(infl + 0j).real, fc.modes_unlayout(hinfl + 0j).real
    worst, seen = 0.0, {}
    for f in range(nf):
        for p in range(npairs):
            if info[f, p] != 0:
                assert not d_dev[f, p].any() and not d_host[f, p].any()
                continue
            key = wb[f, p].tobytes()
            if key not in seen:
                col = fc.column(wb[f, p], N)
                if wb[f, p].min() == wb[f, p].max():
                    col[1:] = 0.0
                inv = fc.dense_solve_ld(fc.toeplitz(col, np.clongdouble), np.eye(N, dtype=np.clongdouble))
                dref = inv.diagonal().real
                ev = np.linalg.eigvalsh(fc.toeplitz(col))
                dh, _ = timestream.toeplitz_inverse_diag_host(col)
                e_ref = float(np.max(np.abs(dh - dref) / dref))
                seen[key] = (dref, fn.K * max(e_ref, EPS * ev[-1] / ev[0]))
            dref, bound = seen[key]
            for got in (d_dev[f, p], d_host[f, p]):
                err = (np.abs(got - dref) / dref).astype(np.float64)
                assert np.all(err <= bound), (f, p, err.max(), bound)
            worst = max(worst, float((np.abs(d_dev[f, p] - dref) / dref).max() / bound))
    print("worst inflation error / bound: %.3g" % worst)
    if wkind == "pair" and npairs >= 3:
        assert np.all(infl[:, 0, 0, 1] == 1.0) and np.all(infl[:, 0, 1, 1] == 1.0)
        assert np.all(infl[:, 0, 0, 2] == 4.0) and np.all(infl[1:, 0, 1, 2] == 4.0)
        assert info[-1, 0] == -1 and info[-1, 1] == -1
        assert np.all(infl[:, -1, 0, :2] == 0.0) and np.all(infl[1:, -1, 1, :2] == 0.0)
    if wkind != "pair":                                                           # one system for all its baselines
        assert np.array_equal(infl, np.broadcast_to(infl[..., :1], infl.shape))
    ones = ctx.mmode_transform_weighted(X, np.ones(ntime), mmax, inflation=True)[2]
    assert bool((ones == 1.0).all())


# ---- products: the configuration of tests/test_gpu_powerspectrum.py ------------------------------------------------------------
def _conf(outdir):
    return dict(config=dict(beamtransfers=True, kltransform=True, psfisher=True, output_directory=str(outdir),
                            truncate=False),
                psfisher=[dict(type="Full", name="ps", klname="kl", threshold=0.0, bandtype="polar", num_theta=1,
                               k_bands=[dict(spacing="linear", start=0.0, stop=0.006, num=4)])],
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, use_foregrounds=False)])


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("flagnoise")
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(_conf(d / "prod")))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    return pm, d


def _ntime(tel):
    return int(np.ceil(2.5 * (2 * int(tel.mmax) + 1)))


# ---- 5. the two pipeline routes ---------------------------------------------------------------------------------------------------
def test_pipeline_routes_write_the_same_inflation(prod):
    from driftscan_amd import skysim, storage, timestream

    pm, d = prod
    tel = pm.telescope
    mmax, nfreq, npairs = int(tel.mmax), int(tel.nfreq), int(tel.npairs)
    N, ntime = 2 * mmax + 1, _ntime(tel)
    fm = skysim.FlagModel(fraction=0.2, burst=3, seed=5)
    common = dict(ndays=0, resolution=86400.0 / ntime, skymodels=("signal",), klname="kl", sky_seed=3)
    flagged = timestream.simulate_ensemble(pm, str(d / "ens_w"), 1, weights=fm, **common)[0]
    clean = timestream.simulate_ensemble(pm, str(d / "ens_c"), 1, **common)[0]
    hostdir = str(d / "ens_w_host")
    shutil.copytree(flagged.directory, hostdir)
    hostts = timestream.Timestream(hostdir, pm)
    flagged.generate_modes_batched()
    clean.generate_modes_batched()
    hostts.generate_mmodes()
    mask = fm.mask(ntime, range(nfreq))
    dev = np.stack([flagged.noise_inflation(mi) for mi in range(mmax + 1)])       # (mmax + 1, nfreq, 2, npairs)
    host = np.stack([hostts.noise_inflation(mi) for mi in range(mmax + 1)])
    assert dev.shape == (mmax + 1, nfreq, 2, npairs) and np.all(dev[0, :, 1] == 1.0) and np.all(host[0, :, 1] == 1.0)
    worst = 0.0
    for f in range(nfreq):
        col = fc.column(mask[f], N)
        dref = fc.dense_solve_ld(fc.toeplitz(col, np.clongdouble), np.eye(N, dtype=np.clongdouble)).diagonal().real
        ev = np.linalg.eigvalsh(fc.toeplitz(col))
        dh, _ = timestream.toeplitz_inverse_diag_host(col)
        bound = fn.K * max(float(np.max(np.abs(dh - dref) / dref)), EPS * ev[-1] / ev[0])
        want = fn.inflation_of(np.broadcast_to(dref.astype(np.float64), (1, npairs, N)), mmax)[:, 0]   # (mmax + 1, 2, npairs)
        for got in (dev[:, f], host[:, f]):
            assert np.all(np.abs(got - want) <= bound * want)
        worst = max(worst, float((np.abs(dev[:, f] - want) / want).max() / bound))
    print("inflation files of the device route: worst error / bound %.3g" % worst)
    for ts in (flagged, hostts):
        infl = dev if ts is flagged else host
        per_mode = np.concatenate([infl[:, :, 0], infl[1:, :, 1]], axis=0)
        with storage.File(ts.output_directory + "/mmodes/weights.hdf5", "r") as f:
            assert np.array_equal(f["inflation_mean"][:], per_mode.mean(axis=0))
            assert np.array_equal(f["inflation_max"][:], per_mode.max(axis=0))
            assert f["inflation_max"][:].min() > 1.0 and not f["info"][:].any()
    # the modes of flagged data keep their bits: the solutions of dm_toeplitz_solve_diag are those of dm_toeplitz_solve
    X = _ctx().to_device(np.stack([flagged.timestream_f(fi) for fi in range(nfreq)]))
    wts = np.broadcast_to(mask[:, None, :], (nfreq, npairs, ntime)).copy()
    plain, _ = _ctx().mmode_transform_weighted(X, wts, mmax)
    assert np.array_equal(np.stack([flagged.mmode(mi) for mi in range(mmax + 1)]), plain.cpu().numpy())
    # data without weights: no new file, ones from the reader
    for mi in range(mmax + 1):
        assert not os.path.exists(clean._mdir(mi) + "/inflation.hdf5")
    assert np.all(clean.noise_inflation(1) == 1.0) and not os.path.exists(clean.output_directory + "/mmodes/weights.hdf5")


# ---- 6. the bias, deterministic ---------------------------------------------------------------------------------------------------
def _stream(pm, path, seed):
    from driftscan_amd import timestream

    ts = timestream.Timestream(str(path), pm)
    ts.set_kltransform("kl")
    for mi in range(pm.telescope.mmax + 1):   # the m-mode directories a simulated timestream would have
        os.makedirs(ts._mdir(mi), exist_ok=True)
    np.random.seed(seed)
    ts.fake_kl_data()
    ts.set_psestimator("ps")
    return ts


def _write_inflation(ts, value):
    from driftscan_amd import storage

    tel = ts.telescope
    for mi in range(tel.mmax + 1):
        with storage.File(ts._mdir(mi) + "/inflation.hdf5", "w") as f:
            f.create_dataset("noise_inflation", data=np.full((tel.nfreq, 2, tel.npairs), float(value)))
            f.attrs["m"] = mi


def _ps_datasets(path):
    from driftscan_amd import storage

    with storage.File(path, "r") as f:
        return {k: f[k][:] for k in f.keys()}


@pytest.fixture(scope="module")
def trace(prod):
    """t_a = sum_m sum_i q_a(e_i) over the unit KL vectors (tr E_a, with q_estimator alone), the bias of fisher.hdf5 and
    the tolerance the bias tests were asked to use: 10 max(1e-12, the relative difference of the two).

    Measured: the difference is 1, because the `bias` of an exact ("Full") estimator is identically zero, here as in the
    reference — the noise bias tr E_a is not in the file.  That tolerance (10) therefore rejects nothing, and the tests
    below also assert ROUNDING: both sides are the same sum of quadratic forms of the same columns, taken through two
    projections of inner length <= nfreq * ntel and one q, so they agree to a small multiple of that length times EPS;
    1e-10 is the relative bound tests/test_gpu_powerspectrum.py uses for such sums."""
    pm, _ = prod
    ps = pm.psestimators["ps"]
    ps.genbands()
    t = np.zeros(ps.nbands)
    for mi in range(1, pm.telescope.mmax + 1):
        nkl = ps.num_evals(mi)
        if nkl:
            t += ps.q_estimator(mi, np.eye(nkl, dtype=np.complex128)).sum(axis=1)
    ps.delbands()
    _, bias = ps.fisher_bias()
    rel = float(np.abs(t - bias).max() / np.abs(t).max())
    print("tr E_a against the bias of fisher.hdf5: relative difference %.3g" % rel)
    assert np.abs(t).max() > 0
    return t, bias, 10.0 * max(1e-12, rel)


ROUNDING = 1e-10


def test_bias_is_zero_for_unit_inflation_and_off_by_default(prod):
    pm, d = prod
    ts = _stream(pm, d / "b_ones", 1)
    ref = _stream(pm, d / "b_ref", 1)                     # the same KL data, no inflation files
    _write_inflation(ts, 1.0)
    fb = ts.flag_noise_bias()
    assert fb.shape == (pm.psestimators["ps"].nbands,) and np.all(fb == 0.0)
    assert ts.flag_noise_bias_correct is False
    p, pref = ts.powerspectrum(), ref.powerspectrum()
    a, b = _ps_datasets(ts._psfile), _ps_datasets(ref._psfile)
    assert sorted(a) == sorted(b) and "flag_bias" not in a and np.array_equal(p, pref)
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k
    # switched on without inflation files: nothing to correct, the same file again
    ref2 = _stream(pm, d / "b_ref2", 1)
    ref2.flag_noise_bias_correct = True
    assert np.array_equal(ref2.powerspectrum(), pref) and "flag_bias" not in _ps_datasets(ref2._psfile)


def test_bias_of_inflation_two_is_the_trace(prod, trace):
    pm, d = prod
    t, bias, tol = trace
    ts = _stream(pm, d / "b_two", 2)
    _write_inflation(ts, 2.0)
    fb = ts.flag_noise_bias()
    err = float(np.abs(fb - t).max() / np.abs(t).max())
    print("delta b of inflation 2 against tr E_a: %.3g (tolerance %.3g)" % (err, tol))
    assert err <= tol and err <= ROUNDING
    # switched on, powerspectrum() subtracts bias + delta b and files delta b
    off = _stream(pm, d / "b_two_off", 2)
    poff = off.powerspectrum()
    ts.flag_noise_bias_correct = True
    pon = ts.powerspectrum()
    got = _ps_datasets(ts._psfile)
    assert np.array_equal(got["flag_bias"], fb)
    want = poff - np.linalg.inv(got["fisher"]) @ fb
    assert np.abs(pon - want).max() <= 1e-10 * np.abs(want).max()
    assert sorted(set(got) - {"flag_bias"}) == sorted(_ps_datasets(off._psfile))


def _columns_q(pm, mi, cols):
    """sum over the columns of q_a(P_m c): cols (nfreq * ntel, R) telescope vectors of one m."""
    ctx = _ctx()
    ps = pm.psestimators["ps"]
    bt, tel = pm.beamtransfer, pm.telescope
    vec = ctx.to_device(np.ascontiguousarray(cols).reshape(1, tel.nfreq, bt.ntel, cols.shape[1]))
    svec, off = bt.project_vectors_telescope_to_svd_device([mi], vec)
    kvec, _ = ps.kltrans.project_vectors_svd_to_kl_device([mi], svec, off=off[:1])
    return ps.q_estimator_batch([mi], [kvec], noise=False)[0].sum(axis=1)


def test_bias_trace_invariance_and_linearity(prod, trace):
    pm, d = prod
    _, _, tol = trace
    tel, bt = pm.telescope, pm.beamtransfer
    ps = pm.psestimators["ps"]
    ts = _stream(pm, d / "b_lin", 3)
    t_m = {m: ps.q_estimator(m, np.eye(ps.num_evals(m), dtype=np.complex128)).sum(axis=1) for m in (1, 2, 3)
           if ps.num_evals(m)}
    mi = max(t_m, key=lambda m: np.abs(t_m[m]).max())          # an m the bands reach
    assert np.abs(t_m[mi]).max() > 0
    n = tel.nfreq * bt.ntel
    rng = np.random.default_rng(12)
    dm = 0.5 + 2.5 * rng.random((tel.nfreq, 2, tel.npairs))
    npower = (bt._noisew() ** -2.0).ravel()
    ps.genbands()
    # (c) sum of q over the columns P D^1/2 and over P D^1/2 U, U the unitary DFT matrix
    root = np.sqrt(npower * dm.ravel())
    U = np.fft.fft(np.eye(n)) / np.sqrt(n)
    qa = _columns_q(pm, mi, np.diag(root).astype(np.complex128))
    qb = _columns_q(pm, mi, root[:, None] * U)
    q1 = _columns_q(pm, mi, np.diag(np.sqrt(npower)).astype(np.complex128))
    ps.delbands()
    err = float(np.abs(qa - qb).max() / np.abs(qa).max())
    print("trace invariance at m = %d: %.3g (tolerance %.3g)" % (mi, err, tol))
    assert err <= tol and err <= ROUNDING
    assert np.abs(q1 - t_m[mi]).max() <= ROUNDING * np.abs(q1).max()            # P N P^H = 1: nominal noise is white in KL
    ones = np.ones_like(dm)
    only = lambda arr: (lambda m: arr if m == mi else ones)   # noqa: E731
    fb = ts.flag_noise_bias(inflation=only(dm))
    assert np.abs(fb - (qa - q1)).max() <= ROUNDING * np.abs(qa).max()            # delta b = tr(P D P^H E) - tr(P N P^H E)
    # (d) linear in d - 1
    d2 = 0.5 + 2.5 * rng.random(dm.shape)
    every = lambda arr: (lambda m: arr)   # noqa: E731
    f1, f2 = ts.flag_noise_bias(inflation=every(dm)), ts.flag_noise_bias(inflation=every(d2))
    f12 = ts.flag_noise_bias(inflation=every(dm + d2 - 1.0))
    f3 = ts.flag_noise_bias(inflation=every(1.0 + 3.0 * (dm - 1.0)))
    scale = max(np.abs(f1).max(), np.abs(f2).max())
    assert np.abs(f12 - (f1 + f2)).max() <= 1e-12 * scale and np.abs(f3 - 3.0 * f1).max() <= 1e-12 * scale
    assert np.all(ts.flag_noise_bias(inflation=every(ones)) == 0.0)


# ---- 7. the bias, statistical -------------------------------------------------------------------------------------------------------
# The smallest power of two up to 256 at which the three conditions of the test hold at the committed seeds (measured at
# 8 .. 256 on an MI355X: 8 and 16 fail the third condition, z of the uncorrected bias 6.7 and 9.97; 32 .. 256 all hold).
R_STAT = 32


def bias_samples(pm, R):
    """Noise-only data of R realisations, with FlagModel(0.4, burst 3) and without flags, through the m-mode transform, the
    two batched projections and the q estimator: (q_flagged (nbands, R), q_unflagged (nbands, R), bias, delta b)."""
    from driftscan_amd import skysim, timestream

    ctx = _ctx()
    tel, bt = pm.telescope, pm.beamtransfer
    ps = pm.psestimators["ps"]
    mmax, nfreq, npairs = int(tel.mmax), int(tel.nfreq), int(tel.npairs)
    ntime = _ntime(tel)
    fm = skysim.FlagModel(fraction=0.4, burst=3, seed=8)
    mask = fm.mask(ntime, range(nfreq))
    assert np.count_nonzero(mask, axis=1).min() >= 2 * mmax + 1
    ms = list(range(1, mmax + 1))
    ps.genbands()
    out = []
    infl = None
    for weights in (fm, None):
        vis = timestream.simulate_visibilities(pm, R, resolution=86400.0 / ntime, seed=11, weights=weights)
        X = vis.permute(1, 0, 2, 3).reshape(nfreq, R * npairs, ntime).contiguous()
        if weights is None:
            modes = ctx.mmode_transform(X, mmax)
        else:
            modes, info, dinf = ctx.mmode_transform_weighted(X, mask, mmax, inflation=True)
            assert not bool(info.any())
            infl = dinf.cpu().numpy()[..., :npairs]
        del vis, X
        vec = modes.view(mmax + 1, nfreq, 2, R, npairs).permute(0, 1, 2, 4, 3).reshape(mmax + 1, nfreq, 2 * npairs, R)
        svec, off = bt.project_vectors_telescope_to_svd_device(ms, vec[1:].contiguous())
        kvec, kloff = ps.kltrans.project_vectors_svd_to_kl_device(ms, svec, off=off[:-1])
        qs = ps.q_estimator_batch(ms, [kvec[kloff[i] : kloff[i + 1]] for i in range(len(ms))], noise=False)
        out.append(np.sum(qs, axis=0))
    ts = timestream.Timestream("unused", pm)
    ts.set_psestimator("ps")
    fb = ts.flag_noise_bias(inflation=lambda m: infl[m])
    ps.delbands()
    return out[0], out[1], ps.fisher_bias()[1], fb


def bias_z(qf, qu, bias, fb, R):
    """(z unflagged, z flagged uncorrected, z flagged corrected) per band from the first R columns; `bias` is what
    nominal noise puts into sum_m q."""
    z = lambda q, b: (q[:, :R].mean(axis=1) - b) / (q[:, :R].std(axis=1, ddof=1) / np.sqrt(R))   # noqa: E731
    return z(qu, bias), z(qf, bias), z(qf, bias + fb)


def test_bias_correction_on_noise_realisations(prod, trace):
    """z = mean / (std / sqrt(R)) per band of sum_m q - b0 on unflagged and on flagged noise, and of sum_m q - b0 - delta b
    on flagged noise.  b0, the bias of nominal noise, is `bias` of fisher.hdf5 plus tr E_a: the exact estimator of this
    configuration files a zero bias (see `trace`), so the nominal term the flags' correction is relative to has to be
    supplied here; the unflagged condition checks exactly that b0.

    Measured at R = 32 (three bands): unflagged 0.22, 0.28, -0.06; flagged uncorrected 11.4, 13.2, 15.5; flagged
    corrected 0.78, 1.31, 1.64.  At R = 256: 29.4, 35.9, 44.3 uncorrected against -0.39, -1.59, 0.05 corrected."""
    pm, _ = prod
    t, _, _ = trace
    qf, qu, bias, fb = bias_samples(pm, R_STAT)
    zu, zf, zc = bias_z(qf, qu, bias + t, fb, R_STAT)
    print("R = %d\nz unflagged            %s\nz flagged, uncorrected %s\nz flagged, corrected   %s" % (R_STAT, zu, zf, zc))
    assert np.all(np.abs(zu) <= 5.0)                       # the harness is sound without the feature
    assert np.all(np.abs(zc) <= 5.0)
    assert np.max(zf) >= 10.0                              # and the flags' bias is there to be corrected
