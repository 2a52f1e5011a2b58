"""Sidereal stacking on the device: `Context.sidereal_regrid` against the long-double
restatement on the cases of tests/sidereal_cases.py, its guards, determinism and refusals, and the routes
`simulate_days` -> `sidereal_stack` -> m-modes on the small polarised cylinder of tests/test_gpu_stack.py."""
import os

import numpy as np
import pytest

import sidereal_cases as sc

pytestmark = pytest.mark.gpu


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _guarded_acc(ctx, nrow, ntime, base=None):
    """(sum, wsum, sq, hits) as the inner NF frequencies of buffers with one NaN (hits: -77) guard frequency on each side."""
    bufs = []
    for i, dt in enumerate((np.complex128, np.float64, np.float64, np.int32)):
        host = np.full((sc.NF + 2, nrow, ntime), -77 if dt is np.int32 else np.nan, dtype=dt)
        host[1:-1] = 7 if base is None else base[i]
        bufs.append(ctx.to_device(host))
    return bufs


def _guards_untouched(ctx, bufs):
    for b in bufs:
        h = ctx.to_host(b)
        edge = np.stack([h[0], h[-1]])
        if not (np.all(edge == -77) if h.dtype == np.int32 else np.all(np.isnan(edge.real))):
            return False
    return True


def _run(ctx, days, ntime, a=3, min_share=1.0, base=None):
    """The days through `sidereal_regrid` into guarded accumulators (written by the first day, or added to `base`)."""
    nrow = days[0][0].shape[1]
    bufs = _guarded_acc(ctx, nrow, ntime, base)
    acc = tuple(b[1:-1] for b in bufs)
    for i, (x, w, phi0, dphi) in enumerate(days):
        xd = ctx.to_device(x)
        wd = None if w is None else ctx.to_device(w)
        if i == 0 and base is None:
            # the first call writes (accumulate = 0), through the C entry point; the later ones add through the wrapper
            rc = ctx.lib.dm_sidereal_regrid(ctx.h, sc.NF, nrow, x.shape[-1], ntime, a, phi0, dphi, min_share, ctx.ptr(xd),
                                            ctx.ptr(wd), *(ctx.ptr(t) for t in acc), 0)
            ctx.check(rc, "dm_sidereal_regrid")
        else:
            got = ctx.sidereal_regrid(xd, phi0, dphi, ntime, w=wd, a=a, min_share=min_share, acc=acc)
            assert all(g.data_ptr() == t.data_ptr() for g, t in zip(got, acc))
    ctx.sync()
    assert _guards_untouched(ctx, bufs)
    return [ctx.to_host(t) for t in acc]


def _cases(rng, nrow):
    out = []
    for ntime in (37, 64):
        for a in (1, 3, 5):
            p, d, n = sc.equal_cadence(ntime)
            out.append(("equal cadence", [(sc.crandn(rng, sc.NF, nrow, n), None, p, d)], ntime, a, 1.0))
        p, d, n = sc.on_grid(ntime)
        w = sc.run_flags(rng, (sc.NF, nrow, n), (0, n - 1), isolated=6)
        out.append(("on grid", [(sc.poison(sc.crandn(rng, sc.NF, nrow, n), w), w, p, d)], ntime, 3, 1.0))
        out.append(("on grid, no w", [(sc.crandn(rng, sc.NF, nrow, n), None, p, d)], ntime, 3, 1.0))
    for a in (3, 5):
        p, d, n = sc.downsampling(37)
        out.append(("downsampling", [(sc.crandn(rng, sc.NF, nrow, n), None, p, d)], 37, a, 1.0))
    p, d, n = sc.downsampling(150)
    w = sc.run_flags(rng, (sc.NF, nrow, n), (0, n - 1), isolated=3)
    out.append(("several tiles", [(sc.poison(sc.crandn(rng, sc.NF, nrow, n), w), w, p, d)], 150, 3, 0.8))
    p, d, n = -7.3, sc.TWO_PI / 1000, 500     # 320 taps per sample: the row tile shrinks to what LDS holds
    w = sc.run_flags(rng, (sc.NF, nrow, n), (0, n - 1), isolated=3)
    out.append(("wide taps", [(sc.poison(sc.crandn(rng, sc.NF, nrow, n), w), w, p, d)], 50, 8, 0.8))
    p, d, n = sc.partial_arc()
    out.append(("partial arc", [(sc.crandn(rng, sc.NF, nrow, n), None, p, d)], 37, 3, 1.0))
    p, d, n = sc.downsampling(37)
    for ms in (1.0, 0.8):
        w = sc.run_flags(rng, (sc.NF, nrow, n), (0, n - 1), isolated=3)
        out.append(("flags", [(sc.poison(sc.crandn(rng, sc.NF, nrow, n), w), w, p, d)], 37, 3, ms))
    out.append(("four days", sc.four_days(rng, nrow), 37, 3, 1.0))
    return out


@pytest.mark.parametrize("nrow", sc.ROWS)
def test_regrid_against_long_double(nrow):
    """Every case, element by element: the validity pattern (wsum > 0, hits) is equal, |sum - ref| <= (T + D + 8) 2^-53
    sum_d W_d sum_j |c_j / S| |x_j|, wsum and sq within (T + D + 8) 2^-53 of themselves; NaN sits in every flagged input
    and in the guard bands around every output: the guards stay and the outputs are finite."""
    ctx = _ctx()
    rng = np.random.default_rng(200 + nrow)
    for name, days, ntime, a, ms in _cases(rng, nrow):
        ref = sc.stack_exact(days, ntime, a=a, min_share=ms)
        got = _run(ctx, days, ntime, a, ms)
        assert all(np.all(np.isfinite(g)) for g in got)
        r = sc.check_stack(got, ref)
        print("%-14s ntime %3d a %d min_share %.1f rows %2d: T %2d, err / bound: sum %.2f wsum %.2f sq %.2f, valid %.2f"
              % ((name, ntime, a, ms, nrow, ref["T"]) + tuple(r) + (float((ref["hits"] > 0).mean()),)))
        if name.startswith("on grid"):     # copied: one tap of coefficient 1
            x, w = days[0][0], days[0][1]
            ok = np.ones(x.shape, dtype=bool) if w is None else w > 0
            assert np.array_equal(got[1], np.where(ok, 1.0 if w is None else w, 0.0))
            if w is None:
                assert np.array_equal(got[0], x)
        if name == "four days":
            assert ref["hits"].min() >= 1
        if name == "partial arc":
            assert 0 < (ref["hits"] > 0).mean() < 0.5


def test_optional_outputs_and_the_wrapper():
    """sq and hits are optional; acc=None allocates and writes what an explicit first call writes."""
    ctx = _ctx()
    rng = np.random.default_rng(3)
    p, d, n = sc.downsampling(37)
    w = sc.run_flags(rng, (sc.NF, 5, n), (0, n - 1), isolated=3)
    x = sc.poison(sc.crandn(rng, sc.NF, 5, n), w)
    want = _run(ctx, [(x, w, p, d)], 37)
    xd, wd = ctx.to_device(x), ctx.to_device(w)
    full = ctx.sidereal_regrid(xd, p, d, 37, w=wd)
    lean = ctx.sidereal_regrid(xd, p, d, 37, w=wd, variance=False)
    assert lean[2] is None and lean[3] is None and full[3].dtype == ctx.torch.int32
    for i in range(4):
        assert np.array_equal(ctx.to_host(full[i]), want[i])
    assert np.array_equal(ctx.to_host(lean[0]), want[0]) and np.array_equal(ctx.to_host(lean[1]), want[1])
    assert ctx.lib.dm_sidereal_max_taps() == 1024


def test_accumulate_leaves_invalid_samples_bit_identical():
    """accumulate != 0 on a partial arc and on flagged data: the samples that are not valid keep their bits (NaN, -0.0
    and denormals among them), the valid ones are within the bound of base + day."""
    ctx = _ctx()
    rng = np.random.default_rng(4)
    for geom, flags in ((sc.partial_arc(), False), (sc.downsampling(37), True)):
        p, d, n = geom
        nrow = 5
        w = sc.run_flags(rng, (sc.NF, nrow, n), (0, n - 1), isolated=3) if flags else None
        x = sc.crandn(rng, sc.NF, nrow, n)
        x = x if w is None else sc.poison(x, w)
        shape = (sc.NF, nrow, 37)
        base = [sc.crandn(rng, *shape), rng.uniform(0.5, 2, size=shape), rng.uniform(0.5, 2, size=shape),
                rng.integers(0, 5, size=shape).astype(np.int32)]
        odd = np.array([np.nan, -0.0, 5e-324, np.inf])
        ref = sc.stack_exact([(x, w, p, d)], 37)
        dead = ref["hits"] == 0
        assert dead.any() and not dead.all()
        for i in range(3):
            vals = odd[rng.integers(0, 4, size=int(dead.sum()))]
            base[i][dead] = vals
        got = _run(ctx, [(x, w, p, d)], 37, base=base)
        for i in range(4):
            assert np.array_equal(got[i][dead].view(np.uint8), base[i][dead].view(np.uint8)), i
        clean = [np.where(dead, 0, b) for b in base]
        live = sc.stack_exact([(x, w, p, d)], 37, base=clean)
        for name, i in (("sum", 0), ("wsum", 1), ("sq", 2)):
            bound = (live["T"] + live["D"] + 8) * sc.EPS * (live["scale"] if i == 0 else live[name])
            assert np.all(np.abs(got[i][~dead] - live[name][~dead]) <= bound[~dead]), name
        assert np.array_equal(got[3][~dead], live["hits"][~dead])


def test_bits_do_not_depend_on_the_batch():
    """A row alone, in a batch of 70 and at another position of the row tile gives the same bits; two frequencies
    together and apart give the same bits."""
    ctx = _ctx()
    rng = np.random.default_rng(5)
    for (p, d, n), ntime in ((sc.downsampling(37), 37), (sc.equal_cadence(64), 64), (sc.downsampling(150), 150)):
        w = sc.run_flags(rng, (sc.NF, 70, n), (0, n - 1), isolated=3)
        x = sc.poison(sc.crandn(rng, sc.NF, 70, n), w)
        for use_w in (True, False):
            xs = x if use_w else np.nan_to_num(x)

            def run(f, r):
                acc = ctx.sidereal_regrid(ctx.to_device(xs[f, r]), p, d, ntime, min_share=0.8,
                                          w=ctx.to_device(w[f, r]) if use_w else None)
                return [ctx.to_host(t) for t in acc]

            fs, rs = slice(0, sc.NF), slice(0, 70)
            full = run(fs, rs)
            for row in (0, 17, 38, 69):
                alone = run(fs, slice(row, row + 1))
                moved = run(fs, slice(row - 3 if row >= 3 else row, row + 2))      # another tile position
                k = 3 if row >= 3 else 0
                for i in range(4):
                    assert np.array_equal(alone[i][:, 0].view(np.uint8), full[i][:, row].view(np.uint8))
                    assert np.array_equal(moved[i][:, k].view(np.uint8), full[i][:, row].view(np.uint8))
            for f in range(sc.NF):
                apart = run(slice(f, f + 1), rs)
                for i in range(4):
                    assert np.array_equal(apart[i][0].view(np.uint8), full[i][f].view(np.uint8))


def test_refusals_leave_the_outputs_alone():
    """Every listed condition is refused before any launch: `dm_last_error` names it, the guards and the outputs keep
    their bits.  Zero sizes are no-ops, except that accumulate = 0 zeroes the outputs."""
    from driftscan_amd import _lib

    ctx = _ctx()
    lib, h, P = ctx.lib, ctx.h, ctx.ptr
    nrow, n, ntime = 3, 36, 37
    p, d, _ = sc.equal_cadence(ntime)
    x = ctx.to_device(np.ones((sc.NF, nrow, n), dtype=np.complex128))
    w = ctx.to_device(np.ones((sc.NF, nrow, n)))
    bufs = _guarded_acc(ctx, nrow, ntime)
    acc = tuple(b[1:-1] for b in bufs)

    def rc(nf=sc.NF, nrow_=nrow, nt_in=n, ntime_=ntime, a=3, phi0=p, dphi=d, ms=1.0, xv=x, wv=None, out=acc, accumulate=0):
        return lib.dm_sidereal_regrid(h, nf, nrow_, nt_in, ntime_, a, phi0, dphi, ms, P(xv), P(wv), P(out[0]), P(out[1]),
                                      P(out[2]), P(out[3]), accumulate)

    def last():
        return lib.dm_last_error(h).decode()

    for kw, what in ((dict(a=0), "a outside 1..8"), (dict(a=9), "a outside 1..8"),
                     (dict(dphi=0.0), "dphi"), (dict(dphi=-d), "dphi"), (dict(dphi=np.nan), "dphi"),
                     (dict(dphi=np.inf), "dphi"), (dict(phi0=np.inf), "phi0"), (dict(phi0=np.nan), "phi0"),
                     (dict(dphi=2 * np.pi / (n - 2)), "2 pi"), (dict(dphi=1.0), "2 pi"),
                     (dict(ms=0.0), "min_share"), (dict(ms=1.0000001), "min_share"), (dict(ms=np.nan), "min_share"),
                     (dict(ntime_=0), "ntime < 1"), (dict(ntime_=-3), "ntime < 1"),
                     (dict(nf=-1), "negative size"), (dict(nrow_=-1), "negative size"), (dict(nt_in=-1), "negative size"),
                     (dict(a=8, ntime_=1, dphi=2 * np.pi / 100, nt_in=36), "taps"),
                     (dict(xv=None), "null"), (dict(out=(None,) + acc[1:]), "null"),
                     (dict(out=(acc[0], None) + acc[2:]), "null"),
                     (dict(out=(x,) + acc[1:]), "shares an element"),
                     (dict(wv=w, out=(acc[0], w) + acc[2:]), "shares an element"),
                     (dict(out=(acc[0], acc[1], acc[1], acc[3])), "share an element"),
                     (dict(out=(acc[0], acc[1], acc[2], acc[2])), "share an element")):
        assert rc(**kw) != 0 and what in last(), (kw, last())
        assert rc(accumulate=1, **kw) != 0
    with pytest.raises(_lib.DriftMIError, match="a outside"):
        ctx.sidereal_regrid(x, p, d, ntime, a=11, acc=acc)
    for bad in (lambda: ctx.sidereal_regrid(x[0], p, d, ntime),
                lambda: ctx.sidereal_regrid(x, p, d, ntime, w=w[:, :, :-1]),
                lambda: ctx.sidereal_regrid(x, p, d, ntime, w=w.to(ctx.torch.float32)),
                lambda: ctx.sidereal_regrid(x, p, d, ntime, acc=acc[:3]),
                lambda: ctx.sidereal_regrid(x, p, d, ntime + 1, acc=acc),
                lambda: ctx.sidereal_regrid(x, p, d, ntime, acc=(acc[0], acc[1], acc[2], acc[2]))):
        with pytest.raises(ValueError):
            bad()
    # a tensor on the host is refused before anything is launched
    xs, ws = ctx.to_device(np.ones((2, 3, 8), dtype=np.complex128)), ctx.to_device(np.ones((2, 3, 8)))
    with pytest.raises(ValueError, match="one GPU"):
        ctx.sidereal_regrid(xs, p, d, ntime, w=ws.cpu())
    # zero sizes with accumulate != 0 touch nothing
    assert rc(nf=0, accumulate=1) == 0 and rc(nrow_=0, accumulate=1) == 0 and rc(nt_in=0, accumulate=1) == 0
    ctx.sync()
    assert _guards_untouched(ctx, bufs)
    for t in acc:
        assert np.all(ctx.to_host(t) == 7)
    assert np.all(ctx.to_host(x) == 1.0) and np.all(ctx.to_host(w) == 1.0)
    # nt_in = 0 with accumulate == 0: a day without samples zeroes the outputs
    assert rc(nt_in=0) == 0
    ctx.sync()
    assert _guards_untouched(ctx, bufs) and all(np.all(ctx.to_host(t) == 0) for t in acc)


# ---- the routes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    """The products of tests/test_gpu_stack.py: 2 cylinders, 3 feeds, 3 frequencies, polarised."""
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("sidereal")
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


def _same_files(a, b, tel):
    from driftscan_amd import storage

    for fi in range(tel.nfreq):
        with storage.File(a._ffile(fi), "r") as f, storage.File(b._ffile(fi), "r") as g:
            assert sorted(f.keys()) == sorted(g.keys())
            for name in f.keys():
                assert np.array_equal(f[name][:], g[name][:]), name
            assert int(f.attrs["ndays"]) == int(g.attrs["ndays"])


def test_stack_of_an_on_grid_directory_is_the_directory(prod, skyfile):
    """One on-grid directory through `sidereal_stack` is its `timestream` bit for bit, and so is the same directory given
    twice; the files hold weight, day_hits, ndays and (for two days) a day_variance that is zero to rounding."""
    from driftscan_amd import storage, timestream

    pm, d = prod
    tel = pm.telescope
    ntime = 2 * int(tel.mmax) + 1
    src = timestream.simulate_ensemble(pm, str(d / "grid"), 1, maps=[skyfile], ndays=0)[0]
    assert src.ntime == ntime
    once = timestream.sidereal_stack(pm, [src.directory], str(d / "grid_once"))
    twice = timestream.sidereal_stack(pm, [src.directory, src.directory], str(d / "grid_twice"))
    for fi in range(tel.nfreq):
        want = src.timestream_f(fi)
        assert np.abs(want).max() > 0
        for st, nd in ((once, 1), (twice, 2)):
            assert np.array_equal(st.timestream_f(fi), want)
            assert np.array_equal(st.weight_f(fi), np.ones(want.shape))
            with storage.File(st._ffile(fi), "r") as f:
                assert f["day_hits"].dtype == np.int32 and np.all(f["day_hits"][:] == nd)
                assert int(f.attrs["ndays"]) == nd and int(f.attrs["ntime"]) == ntime
                assert ("day_variance" in f) == (nd > 1)
                if nd > 1:
                    assert np.all(np.abs(f["day_variance"][:]) <= 16 * sc.EPS * np.abs(want) ** 2)
    # a day whose phi is not uniformly spaced is refused
    bad = timestream.simulate_ensemble(pm, str(d / "bad"), 1, maps=[skyfile], ndays=0)[0]
    with storage.File(bad._ffile(0), "r") as f:
        data, phi = f["timestream"][:], f["phi"][:]
    phi[3] += 1e-6
    timestream._write_sim_file(bad, 0, data, phi)
    with pytest.raises(ValueError, match="uniformly"):
        timestream.sidereal_stack(pm, [bad.directory], str(d / "bad_stack"))


STARTS, CADENCE = (0.3, 2.7, 5.0), 120.0   # 718 samples per turn


def _ntime(tel):
    return int(np.ceil(2.5 * (2 * int(tel.mmax) + 1)))


def test_three_noise_free_days_give_the_m_modes_of_the_direct_simulation(prod, skyfile):
    """`simulate_days` -> `sidereal_stack` (onto 2.5 (2 mmax + 1) grid samples, so that the kernel's low-pass at the grid's
    Nyquist frequency leaves the sky alone) -> `generate_modes_batched` against the m-modes of the direct
    `simulate_ensemble(ndays=0)`: the host restatement of the same three days has a distance to that ideal (the error of
    the Lanczos kernel); the device is allowed that distance plus 1e-10 of the largest mode, and its regridded data
    agree with the restatement's to 1e-10 of the largest sample."""
    from driftscan_amd import timestream

    pm, d = prod
    tel = pm.telescope
    ntime = _ntime(tel)
    per_turn = timestream.T_SIDEREAL_DAY / CADENCE
    nsamp = int(per_turn * 0.8)
    dirs = [str(d / ("day%d" % i)) for i in range(3)]
    days = timestream.simulate_days(pm, dirs, STARTS, nsamp, CADENCE, maps=[skyfile], ndays=0)
    ideal = timestream.simulate_ensemble(pm, str(d / "ideal"), 1, maps=[skyfile], ndays=0)[0]
    st = timestream.sidereal_stack(pm, dirs, str(d / "stack3"), ntime=ntime, a=5)
    dphi = 2 * np.pi * CADENCE / timestream.T_SIDEREAL_DAY
    host = timestream.Timestream(str(d / "stack3_host"), pm)
    vmax = 0.0
    for fi in range(tel.nfreq):
        s = np.zeros((tel.npairs, ntime), dtype=np.clongdouble)
        ws = np.zeros((tel.npairs, ntime), dtype=np.longdouble)
        for i, day in enumerate(days):
            assert day.ntime == nsamp
            xh, W = timestream.sidereal_regrid_host(day.timestream_f(fi), None, STARTS[i], dphi, ntime, a=5,
                                                    dtype=np.clongdouble)
            s += W * xh
            ws += W
        assert ws.min() > 0                                           # three days of 4 / 5 turn cover the circle
        mean = (s / ws).astype(np.complex128)
        got = st.timestream_f(fi)
        vmax = max(vmax, np.abs(mean).max())
        assert np.abs(got - mean).max() <= 1e-10 * np.abs(mean).max()
        assert np.abs(st.weight_f(fi) - (ws / 3).astype(np.float64)).max() <= 1e-12 * float(ws.max())
        timestream._write_sim_file(host, fi, mean, np.linspace(0, 2 * np.pi, ntime, endpoint=False),
                                   weight=(ws / 3).astype(np.float64))
    host.save()
    for ts in (st, host, ideal):
        ts.generate_modes_batched()
    mmax_abs = max(np.abs(ideal.mmode(mi)).max() for mi in range(tel.mmax + 1))
    dist_host = max(np.abs(host.mmode(mi) - ideal.mmode(mi)).max() for mi in range(tel.mmax + 1))
    dist_dev = max(np.abs(st.mmode(mi) - ideal.mmode(mi)).max() for mi in range(tel.mmax + 1))
    print("distance to the ideal m-modes / largest mode: restatement %.3g, device %.3g" % (dist_host / mmax_abs, dist_dev / mmax_abs))
    assert dist_host < 0.02 * mmax_abs                               # the days do carry the sky
    assert dist_dev <= dist_host + 1e-10 * mmax_abs
    for mi in range(tel.mmax + 1):
        assert np.abs(st.mmode(mi) - host.mmode(mi)).max() <= 1e-10 * mmax_abs, mi


def test_day_variance_measures_the_noise(prod):
    """Noise only, 16 days at one start and equal cadence, unit weights: a grid sample has 16 hits or (next to the gap of
    the day) none, and the mean of day_variance over the valid ones is sigma^2 of `simulate_days` within 5 standard
    errors.  day_variance of one sample is sigma^2 / 15 times half a chi-square of 2 * 15 degrees of freedom (complex
    data, 16 days): relative variance 1 / 15.  Neighbouring grid samples share taps: with rho_kk' the correlation of the
    regridded noise of samples k and k' (from the coefficients), the estimates are correlated by |rho|^2, so the K valid
    samples of a row count as K^2 / sum_kk' rho^2 independent terms; rows and frequencies are independent.  The count N
    is printed; the standard error of the mean ratio is 1 / sqrt(15 N)."""
    from driftscan_amd import storage, timestream

    pm, d = prod
    tel = pm.telescope
    ntime = 2 * int(tel.mmax) + 1
    nd, a = 16, 3
    cadence = timestream.T_SIDEREAL_DAY / ntime                          # equal cadence: s = 1
    dphi = 2 * np.pi * cadence / timestream.T_SIDEREAL_DAY
    dirs = [str(d / ("noise%02d" % i)) for i in range(nd)]
    timestream.simulate_days(pm, dirs, [0.4 * dphi] * nd, ntime - 1, cadence, seed=21)
    st = timestream.sidereal_stack(pm, dirs, str(d / "noise_stack"), a=a)
    sigma2 = (2 * np.pi / dphi) * np.asarray(tel.noisepower(np.arange(tel.npairs)[None, :], np.arange(tel.nfreq)[:, None],
                                                             ndays=1), dtype=np.float64).reshape(tel.nfreq, tel.npairs)
    taps = timestream.sidereal_taps_host(ntime - 1, ntime, a, 0.4 * dphi, dphi)
    valid = np.array([first >= 0 and first + len(c) <= ntime - 1 for first, c in taps])
    C = np.zeros((ntime, ntime - 1))
    for k, (first, c) in enumerate(taps):
        if valid[k]:
            C[k, first : first + len(c)] = c.astype(np.float64)
    C = C[valid]
    rho = (C @ C.T) / np.sqrt(np.outer((C * C).sum(axis=1), (C * C).sum(axis=1)))
    K = int(valid.sum())
    N = tel.nfreq * tel.npairs * K**2 / float((rho**2).sum())
    assert K >= ntime - 2 * a - 1
    ratios = []
    for fi in range(tel.nfreq):
        with storage.File(st._ffile(fi), "r") as f:
            hits, var = f["day_hits"][:], f["day_variance"][:]
        assert np.all(hits[:, valid] == nd) and np.all(hits[:, ~valid] == 0) and np.all(var[:, ~valid] == 0)
        ratios.append(var[:, valid] / sigma2[fi][:, None])
    ratios = np.stack(ratios)
    z = (ratios.mean() - 1.0) * np.sqrt(15.0 * N)
    print("mean day_variance / sigma^2 = %.4f over %d samples, N = %.0f independent terms: z = %.2f"
          % (ratios.mean(), ratios.size, N, z))
    assert abs(z) <= 5


def test_the_pipeline_entry_makes_the_files_of_the_direct_call(prod, skyfile, tmp_path):
    """`sidereal_from: {days, a, min_share}` produces the files of `sidereal_stack`, from stacked days that `stack_from`
    entries of the same file make first, and goes on to the m-modes."""
    import yaml

    from driftscan_amd import pipeline, timestream

    pm, d = prod
    tel = pm.telescope
    per_turn = timestream.T_SIDEREAL_DAY / CADENCE
    udirs = [str(tmp_path / ("u%d" % i)) for i in range(2)]
    sdirs = [str(tmp_path / ("s%d" % i)) for i in range(2)]
    timestream.simulate_days(pm, udirs, (0.2, 3.3), int(0.8 * per_turn), CADENCE, maps=[skyfile], ndays=0, unstacked=True)
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=True, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=False),
                timestreams=[dict(name="d%d" % i, directory=sdirs[i], stack_from=dict(directory=udirs[i])) for i in range(2)]
                + [dict(name="sid", directory=str(tmp_path / "sid"), sidereal_from=dict(days=sdirs, a=4, min_share=0.9))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = pipeline.PipelineManager.from_configfile(str(cfile))
    assert sorted(p.timestreams) == ["sid"] and sorted(p.days) == ["d0", "d1"]
    p.simulate()
    p.generate()
    sid = p.timestreams["sid"]
    direct = timestream.sidereal_stack(pm, sdirs, str(tmp_path / "direct"), a=4, min_share=0.9)
    _same_files(sid, direct, tel)
    assert os.path.exists(sid._mfile(0)) and np.abs(sid.timestream_f(0)).max() > 0
    # unstacked days are stacked over the days as they are, and carry their class table
    un = timestream.sidereal_stack(pm, udirs, str(tmp_path / "un"), a=4, min_share=0.9)
    assert un.is_unstacked()
    off, _ = tel.redundant_pairs()
    assert un.timestream_f(0).shape == (int(off[-1]), 2 * int(tel.mmax) + 1)
