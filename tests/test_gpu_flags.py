"""Flagged timestreams on the device: the batched Toeplitz solver (dm_toeplitz_solve) over its
size and batch edges against extended precision within the bound of tests/flags_cases.py, its batch independence and
failure reporting; `Context.mmode_transform_weighted` against `mmode_transform`, the host statement and known modes; and
the pipeline end to end on the products of the small polarised cylinder of tests/test_gpu_tsim.py."""
import os
import shutil

import numpy as np
import pytest

import flags_cases as fc

pytestmark = pytest.mark.gpu

EPS = fc.EPS
GUARD = 7.25 - 3.5j


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _solve_guarded(ctx, col, B):
    """dm_toeplitz_solve on buffers with guard elements around b and info: (x, info) as numpy, the guards checked."""
    import torch

    batch, nrhs, n = B.shape
    g = 64
    buf = torch.full((batch * nrhs * n + 2 * g,), GUARD, dtype=torch.complex128, device="cuda")
    buf[g : g + batch * nrhs * n] = ctx.to_device(B).view(-1)
    ibuf = torch.full((batch + 2 * g,), -77, dtype=torch.int32, device="cuda")
    cdev = ctx.to_device(col)
    rc = ctx.lib.dm_toeplitz_solve(ctx.h, n, nrhs, batch, ctx.ptr(cdev), ctx.ptr(buf[g:]), ctx.ptr(ibuf[g:]))
    ctx.check(rc, "dm_toeplitz_solve")
    ctx.sync()
    hb, hi = buf.cpu().numpy(), ibuf.cpu().numpy()
    assert np.all(hb[:g] == GUARD) and np.all(hb[-g:] == GUARD), "guard elements around b were written"
    assert np.all(hi[:g] == -77) and np.all(hi[-g:] == -77), "guard elements around info were written"
    return hb[g:-g].reshape(batch, nrhs, n), hi[g:-g]


# ---- 1. toeplitz_solve over the size and batch edges -----------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 17, 64, 65, 128, 129, 257, 384, 385, 513])
def test_toeplitz_solve_sizes_and_batches(n):
    ctx = _ctx()
    pool = fc.pool(n)
    worst = 0.0
    for nrhs in (1, 3, 8):
        for batch in (1, 5, 300):
            which = [(3 * s + nrhs) % len(pool) for s in range(batch)]           # mixed systems in one batch
            col = np.stack([pool[i]["col"] for i in which])
            B = np.stack([pool[i]["B"][:nrhs] for i in which])
            x, info = _solve_guarded(ctx, col, B)
            assert not info.any(), "info %s" % (info[info != 0],)
            first = {}
            for s, i in enumerate(which):
                if i in first:                                                   # a repeated system repeats its bits
                    assert np.array_equal(x[s], x[first[i]])
                    continue
                first[i] = s
                err, bound = fc.check(x[s], pool[i], what="dm_toeplitz_solve nrhs %d batch %d" % (nrhs, batch))
                worst = max(worst, float((err / bound).max()))
    print("n = %d: worst forward error / bound %.3g" % (n, worst))


def test_toeplitz_solve_through_the_context_with_ridge():
    ctx = _ctx()
    cs = fc.case("b", 65, 0)
    x, info = ctx.toeplitz_solve(cs["col"][None].copy(), cs["B"][None].copy())
    assert int(info.cpu()[0]) == 0
    fc.check(x.cpu().numpy()[0], cs, what="Context.toeplitz_solve")
    plain = fc.column(fc.gap_mask(160, 40, 16), 65)                             # system (c): the ridge added by the call
    cc = fc.case("c", 65, 0)
    x, info = ctx.toeplitz_solve(plain[None], cc["B"][None].copy(), ridge=1e-6)
    assert int(info.cpu()[0]) == 0
    fc.check(x.cpu().numpy()[0], cc, what="Context.toeplitz_solve ridge")


# ---- 2. batch independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nrhs", [(17, 3), (513, 2), (1025, 8)])
def test_toeplitz_solve_batch_independence(n, nrhs):
    ctx = _ctx()
    rng = np.random.default_rng(n)
    cols = np.stack([fc.column_of("a", n, s % 3) for s in range(3)])
    B = rng.standard_normal((300, nrhs, n)) + 1j * rng.standard_normal((300, nrhs, n))
    col = cols[np.arange(300) % 3].copy()
    probe_col = fc.column_of("a", n, 1)
    probe_b = rng.standard_normal((nrhs, n)) + 1j * rng.standard_normal((nrhs, n))
    most = ctx.toeplitz_max_rhs(n)
    if n == 1025:
        assert most < nrhs                                                        # beyond the limit by construction
        rc = ctx.lib.dm_toeplitz_solve(ctx.h, n, nrhs, 1, ctx.ptr(ctx.to_device(probe_col)),
                                       ctx.ptr(ctx.to_device(probe_b)), ctx.ptr(ctx.zeros((1,), np.int32)))
        assert rc != 0 and b"dm_toeplitz_max_rhs" in ctx.lib.dm_last_error(ctx.h)
    solo, info = ctx.toeplitz_solve(probe_col[None], probe_b[None])
    solo = solo.cpu().numpy()[0]
    assert int(info.cpu()[0]) == 0
    for r in range(nrhs):                                                         # every right-hand side in a call of its own
        one, _ = ctx.toeplitz_solve(probe_col[None], probe_b[None, r : r + 1])
        assert np.array_equal(one.cpu().numpy()[0, 0], solo[r])
    for pos in (0, 7, 299):
        c2, b2 = col.copy(), B.copy()
        c2[pos], b2[pos] = probe_col, probe_b
        x, info = ctx.toeplitz_solve(c2, b2)
        assert not info.cpu().numpy().any()
        assert np.array_equal(x.cpu().numpy()[pos], solo), "position %d of a batch of 300" % pos


def test_toeplitz_solve_refuses_bad_arguments():
    ctx = _ctx()
    col, b, info = ctx.zeros((2, 4), np.complex128), ctx.zeros((2, 1, 4), np.complex128), ctx.zeros((2,), np.int32)
    lib = ctx.lib
    for n, nrhs, batch, c, bb, ii in ((0, 1, 2, col, b, info), (4, 0, 2, col, b, info), (4, 1, -1, col, b, info),
                                      (4, 1, 2, None, b, info), (4, 1, 2, col, None, info), (4, 1, 2, col, b, None),
                                      (4, lib.dm_toeplitz_max_rhs(4) + 1, 2, col, b, info), (3411, 1, 1, col, b, info)):
        assert lib.dm_toeplitz_solve(ctx.h, n, nrhs, batch, ctx.ptr(c), ctx.ptr(bb), ctx.ptr(ii)) == -1
        assert b"dm_toeplitz_solve" in lib.dm_last_error(ctx.h)
    assert lib.dm_toeplitz_solve(ctx.h, 4, 1, 0, ctx.ptr(None), ctx.ptr(None), ctx.ptr(None)) == 0   # batch 0: a no-op
    assert lib.dm_toeplitz_max_rhs(1025) == 7 and lib.dm_toeplitz_max_rhs(2049) == 2
    assert lib.dm_toeplitz_max_rhs(3410) == 1 and lib.dm_toeplitz_max_rhs(3411) == 0 and lib.dm_toeplitz_max_rhs(0) == 0


# ---- 3. a system that is not positive definite -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [17, 513])
def test_toeplitz_solve_reports_an_indefinite_system(n):
    ctx = _ctx()
    pool = fc.pool(n)
    col = np.stack([pool[s % len(pool)]["col"] for s in range(9)])
    B = np.stack([pool[s % len(pool)]["B"][:3] for s in range(9)])
    col[4] = fc.column_of("e", n)
    col[6] = 0.0
    col[6, 1] = 0.5                                                               # c_0 = 0
    x, info = _solve_guarded(ctx, col, B)
    assert info[4] == 1 and info[6] == n and not x[4].any() and not x[6].any()
    assert not info[[0, 1, 2, 3, 5, 7, 8]].any()
    for s in (3, 5, 7):
        solo, _ = _solve_guarded(ctx, col[s : s + 1], B[s : s + 1])
        assert np.array_equal(solo[0], x[s])
        fc.check(x[s], pool[s % len(pool)])


# ---- 4. unit weights ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mmax,ntime,nf,npairs", [(0, 1, 1, 1), (8, 40, 3, 5), (32, 161, 2, 4)])
def test_weighted_transform_with_unit_weights_is_the_plain_transform(mmax, ntime, nf, npairs):
    ctx = _ctx()
    rng = np.random.default_rng(ntime)
    X = ctx.to_device(rng.standard_normal((nf, npairs, ntime)) + 1j * rng.standard_normal((nf, npairs, ntime)))
    plain = ctx.mmode_transform(X, mmax).cpu().numpy()
    for wshape in ((nf, npairs, ntime), (nf, ntime), (ntime,)):
        out, info = ctx.mmode_transform_weighted(X, np.ones(wshape), mmax)
        assert not info.cpu().numpy().any() and tuple(info.shape) == (nf, npairs)
        assert (out.cpu().numpy() == plain).all()
        rho = 0.375
        out, _ = ctx.mmode_transform_weighted(X, ctx.to_device(np.ones(wshape)), mmax, ridge=rho)
        assert np.all(np.abs(out.cpu().numpy() - plain / (1 + rho)) <= 2 * EPS * np.abs(plain / (1 + rho)))


# ---- 5. against the host statement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mmax,ntime,nf,npairs", [(0, 1, 1, 1), (2, 9, 2, 3), (8, 40, 3, 5), (32, 160, 2, 4)])
@pytest.mark.parametrize("wkind", ["pair", "freq", "time", "real"])
def test_weighted_transform_against_the_host(mmax, ntime, nf, npairs, wkind):
    ctx = _ctx()
    N = 2 * mmax + 1
    rng = np.random.default_rng(100 * mmax + len(wkind))
    x, _ = fc.band_limited(rng, nf, npairs, mmax, ntime)
    x = x + 0.1 * (rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape))
    frac = 0.25 if ntime > 1 else 0.0
    if wkind in ("pair", "real"):
        w = np.stack([fc.random_mask(ntime, frac, 10 * f + p) for f in range(nf) for p in range(npairs)])
        w = w.reshape(nf, npairs, ntime)
        if wkind == "real":
            w = w * (0.25 + rng.random(w.shape))
        elif npairs >= 3:
            w[-1, 0] = 0.0                                                       # a fully flagged baseline
            w[-1, 1] = 0.0
            w[-1, 1, : N - 1] = 1.0                                              # and one with N - 1 samples
    elif wkind == "freq":
        w = np.stack([fc.random_mask(ntime, frac, 50 + f) for f in range(nf)])
    else:
        w = fc.random_mask(ntime, frac, 77)
    host, hinfo, bounds = fc.row_bounds(x, w, mmax)
    out, info = ctx.mmode_transform_weighted(ctx.to_device(x), w, mmax)
    out, info = out.cpu().numpy(), info.cpu().numpy()
    assert np.array_equal(info, hinfo)
    if wkind == "pair" and npairs >= 3:
        assert info[-1, 0] == -1 and info[-1, 1] == -1 and np.count_nonzero(info) == 2
        assert not out[:, -1, :, :2].any()
    diff = np.linalg.norm(fc.modes_unlayout(out) - fc.modes_unlayout(host), axis=-1)
    print("worst ||device - host|| / bound: %.3g" % float((diff[bounds > 0] / bounds[bounds > 0]).max()))
    assert np.all(diff <= bounds)
    assert not out[0, :, 1].any()


# ---- 6. recovery ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mmax,ntime", [(8, 40), (32, 160)])
def test_weighted_transform_recovers_known_modes(mmax, ntime):
    ctx = _ctx()
    rng = np.random.default_rng(ntime + 1)
    nf, npairs = 2, 3
    x, a = fc.band_limited(rng, nf, npairs, mmax, ntime)
    w = np.stack([fc.random_mask(ntime, 0.25, 5 + f) for f in range(nf)])
    xz = x * w[:, None, :]
    truth = fc.modes_layout(a, mmax)
    _, _, bounds = fc.row_bounds(xz, w, mmax)
    out, info = ctx.mmode_transform_weighted(ctx.to_device(xz), w, mmax)
    assert not info.cpu().numpy().any()
    diff = np.linalg.norm(fc.modes_unlayout(out.cpu().numpy()) - a, axis=-1)
    print("weighted estimate against the known modes: worst / bound %.3g" % float((diff / bounds).max()))
    assert np.all(diff <= bounds)
    plain = ctx.mmode_transform(ctx.to_device(xz), mmax).cpu().numpy()
    off = np.abs(plain - truth).max() / np.abs(truth).max()
    print("plain transform of the zero-filled data: off by %.3g of the largest mode" % off)
    assert off > 0.1                                                             # why the feature exists


# ---- 7. refused before any launch ----------------------------------------------------------------------------------------------
def test_weighted_transform_refuses_bad_input():
    ctx = _ctx()
    X = ctx.zeros((2, 3, 20), np.complex128)
    bad = [-np.ones(20), np.full((2, 20), np.nan), np.ones(19), np.ones((3, 20)), np.ones((2, 3, 21)),
           np.full((2, 3, 20), np.inf), ctx.to_device(-np.ones(20))]
    for w in bad:
        with pytest.raises(ValueError):
            ctx.mmode_transform_weighted(X, w, 4)
    with pytest.raises(ValueError):
        ctx.mmode_transform_weighted(X, np.ones(20), 10)                         # ntime < 2 mmax + 1
    with pytest.raises(ValueError):
        ctx.mmode_transform_weighted(X, np.ones(20), 4, ridge=-1.0)


# ---- 8. the pipeline end to end -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("flags")
    conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, inverse=True, use_foregrounds=False)])
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    return pm, d


def _modes(ts, mmax):
    return np.stack([ts.mmode(mi) for mi in range(mmax + 1)])


def test_pipeline_with_flags_end_to_end(prod):
    from driftscan_amd import skysim, storage, timestream

    pm, d = prod
    tel = pm.telescope
    mmax, nfreq, npairs = int(tel.mmax), int(tel.nfreq), int(tel.npairs)
    N = 2 * mmax + 1
    ntime = int(np.ceil(2.5 * N))
    res = 86400.0 / ntime
    fm = skysim.FlagModel(fraction=0.2, burst=3, seed=5)
    common = dict(ndays=0, resolution=res, skymodels=("signal",), klname="kl", sky_seed=3)
    flagged = timestream.simulate_ensemble(pm, str(d / "ens_w"), 1, weights=fm, **common)[0]
    clean = timestream.simulate_ensemble(pm, str(d / "ens_c"), 1, **common)[0]
    assert flagged.ntime == ntime
    mask = fm.mask(ntime, range(nfreq))
    assert 0 < np.count_nonzero(mask == 0) < mask.size
    for fi in range(nfreq):
        with storage.File(flagged._ffile(fi), "r") as f:
            w, x = f["weight"][:], f["timestream"][:]
        assert w.dtype == np.float64 and np.array_equal(w, np.broadcast_to(mask[fi], (npairs, ntime)))
        assert np.all(x[w == 0] == 0) and np.all(x[w != 0] == clean.timestream_f(fi)[w != 0])
        assert clean.weight_f(fi) is None
    # simulate_visibilities zeroes the same samples, for an explicit array as for the model
    warr = np.broadcast_to(mask[:, None, :], (nfreq, npairs, ntime)).copy()
    vis = timestream.simulate_visibilities(pm, 1, weights=warr, **common).cpu().numpy()[0]
    assert np.array_equal(vis, np.stack([flagged.timestream_f(fi) for fi in range(nfreq)]))
    # `simulate` (the host route of the same sky) zeroes the same samples and writes the same weights
    hs = timestream.simulate(pm, str(d / "sim_w"), ndays=0, resolution=res, skymodels=("signal",), klname="kl", sky_seed=3,
                             sky_realisation=0, weights=dict(fraction=0.2, burst=3, seed=5))
    for fi in range(nfreq):
        x = hs.timestream_f(fi)
        assert np.array_equal(hs.weight_f(fi), np.broadcast_to(mask[fi], (npairs, ntime)))
        assert np.array_equal(x == 0, vis[fi] == 0) and np.abs(x - vis[fi]).max() <= 1e-10 * np.abs(vis).max()
    # the per-m host route on a copy of the data
    hostdir = str(d / "ens_w_host")
    shutil.copytree(flagged.directory, hostdir)
    hostts = timestream.Timestream(hostdir, pm)
    flagged.generate_modes_batched()
    clean.generate_modes_batched()
    hostts.generate_mmodes()
    vw, vc, vh = _modes(flagged, mmax), _modes(clean, mmax), _modes(hostts, mmax)          # (mmax + 1, nfreq, 2, npairs)
    xs = np.stack([flagged.timestream_f(fi) for fi in range(nfreq)])
    _, info, bounds = fc.row_bounds(xs, mask, mmax)
    assert not info.any()
    # the clean simulation is band limited, so the weighted estimate of the flagged data gives its modes back
    diff = np.linalg.norm(fc.modes_unlayout(vw) - fc.modes_unlayout(vc), axis=-1)
    print("weighted modes of flagged data against the modes of the complete data: worst / bound %.3g"
          % float((diff / bounds).max()))
    assert np.all(diff <= bounds)
    agree = np.abs(vw - vh).max() / np.abs(vw).max()
    print("device route against the per-m host route: %.3g of max |v|" % agree)
    assert agree <= 1e-10
    for ts in (flagged, hostts):
        with storage.File(ts.output_directory + "/mmodes/weights.hdf5", "r") as f:
            assert np.array_equal(f["nkept"][:], np.broadcast_to(np.count_nonzero(mask, axis=1)[:, None], (nfreq, npairs)))
            assert f["info"][:].shape == (nfreq, npairs) and not f["info"][:].any()
    assert not os.path.exists(clean.output_directory + "/mmodes/weights.hdf5")
    assert os.path.exists(flagged._svdfile(0))
