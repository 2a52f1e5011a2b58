"""RFI flagging on the device: `Context.rfi_flag` against the long-double statement on the
decided segments, its occupancy step in integers, guards, determinism and refusals, and the routes `simulate_days(rfi=)`
-> `sidereal_stack(rfi=)` -> m-modes on the small polarised cylinder of tests/test_gpu_stack.py."""
import os

import numpy as np
import pytest

import rfi_cases as rc

pytestmark = pytest.mark.gpu


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _guarded(ctx, nrow, nt, nseg):
    """(w_out, noise, nflag, occupancy) as the inner NF frequencies of buffers with one NaN (int32: -77) guard frequency
    on each side; the inside is poisoned too."""
    bufs = []
    for shape, dt in (((nrow, nt), np.float64), ((nrow, nseg), np.float64), ((nrow,), np.int32), ((nt,), np.int32)):
        bufs.append(ctx.to_device(np.full((rc.NF + 2,) + shape, -77 if dt is np.int32 else np.nan, dtype=dt)))
    return bufs


def _guards_untouched(ctx, bufs):
    for b in bufs:
        h = ctx.to_host(b)
        edge = np.stack([h[0], h[-1]])
        if not (np.all(edge == -77) if h.dtype == np.int32 else np.all(np.isnan(edge))):
            return False
    return True


def _run(ctx, x, w, p):
    nf, nrow, nt = x.shape
    assert nf == rc.NF
    nseg = -(-nt // p["segment"])
    bufs = _guarded(ctx, nrow, nt, nseg)
    out = tuple(b[1:-1] for b in bufs)
    got = ctx.rfi_flag(ctx.to_device(x), w=None if w is None else ctx.to_device(w), out=out, **p)
    assert all(g.data_ptr() == t.data_ptr() for g, t in zip(got, out))
    ctx.sync()
    assert _guards_untouched(ctx, bufs)
    return [ctx.to_host(t) for t in out]


def _cases(rng, nrow, max_segment):
    """(name, x, w, params): the shapes at which the kernel takes another path."""
    out = []

    def data(nt, bursts=2, w=True, runs=(), frac=0.03, shared=False):
        x = rc.fringing_sky(rng, rc.NF, nrow, nt)
        rc.add_bursts(rng, x, bursts, shared=shared)
        wv = rc.input_flags(rng, x.shape, frac, runs) if w else None
        return (rc.poison(x, wv) if w else x), wv

    out.append(("nt 15 < min_good",) + data(15, 1) + (rc.params(),))
    out.append(("nt 37",) + data(37, 1) + (rc.params(),))
    for nt in (64, 65, 257):
        out.append(("nt %d" % nt,) + data(nt) + (rc.params(),))
    out.append(("short last segment",) + data(3 * 128 + 1, 4) + (rc.params(segment=128),))
    out.append(("max segment",) + data(max_segment, 12) + (rc.params(segment=max_segment),))
    out.append(("window 64 skipped",) + data(37, 1) + (rc.params(windows=(64,)),))
    out.append(("windows 1..64",) + data(257, 3) + (rc.params(windows=(1, 2, 4, 8, 16, 32, 64)),))
    out.append(("no w",) + data(257, 3, w=False) + (rc.params(),))
    x, w = data(65)
    out.append(("all input flagged", x, np.zeros_like(w), rc.params()))
    out.append(("long flag runs",) + data(257, 3, runs=((20, 18), (100, 40), (240, 17))) + (rc.params(),))
    out.append(("niter 1",) + data(257, 3) + (rc.params(niter=1),))
    out.append(("H 2",) + data(257, 3, runs=((50, 6),)) + (rc.params(kernel_sigma=0.4),))
    out.append(("H 32",) + data(257, 3, runs=((50, 70),)) + (rc.params(kernel_sigma=10.6),))
    out.append(("heavy flags",) + data(257, 3, frac=0.5) + (rc.params(),))
    return out


@pytest.mark.parametrize("nrow", rc.ROWS)
def test_flags_against_long_double(nrow):
    """Every case: the row flags are those of the long-double statement on every decided segment, at most 1 % of the
    segments are undecided, noise is within eps / sqrt(ln 2), nflag and occupancy count the new flags, kept weights are
    the input's bit for bit, NaN and Inf under the input flags reach nothing, and the guards around every output stay."""
    ctx = _ctx()
    rng = np.random.default_rng(700 + nrow)
    mx = ctx.lib.dm_rfi_max_segment()
    assert mx >= 1024
    for name, x, w, p in _cases(rng, nrow, mx):
        nt = x.shape[-1]
        ref = rc.reference(x, w, p)
        w_out, noise, nflag, occ = _run(ctx, x, w, p)
        assert np.all(np.isfinite(w_out)) and np.all(np.isfinite(noise))
        win = np.ones(x.shape) if w is None else w
        inflag = ~(win > 0)
        flags = w_out == 0
        assert np.all(flags[inflag]), name
        assert np.array_equal(w_out[~flags].view(np.int64), win[~flags].view(np.int64)), name
        bad, und = rc.check(ref, flags, noise, p, nt)
        new = flags & ~inflag
        print("%-20s nt %4d rows %2d: new flags %.3f (reference %.3f), undecided %.3f" %
              (name, nt, nrow, new.mean(), (ref["row_flags"] & ~inflag).mean(), und))
        assert not bad, (name, bad)
        assert np.array_equal(nflag, new.sum(axis=2)), name
        assert np.array_equal(occ, new.sum(axis=1)), name
        if name in ("nt 15 < min_good", "all input flagged"):
            assert flags.all() and np.all(noise == 0)
        if name == "long flag runs":   # the middle of a run of more than 2H + 1 flags has no usable sample in its window
            assert not flags.all()


@pytest.mark.parametrize("row_share", (0.5, 1.0))
def test_occupancy_in_integers(row_share):
    """The occupancy rule applied in numpy to the device's own row flags gives the device's occupancy and final w_out."""
    ctx = _ctx()
    rng = np.random.default_rng(31)
    nrow, nt = 5, 257
    x = rc.fringing_sky(rng, rc.NF, nrow, nt)
    rc.add_bursts(rng, x, 3, shared=True)
    rc.add_bursts(rng, x, 2)
    w = rc.input_flags(rng, x.shape, 0.1)
    x = rc.poison(x, w)
    rows = _run(ctx, x, w, rc.params(segment=128))
    got = _run(ctx, x, w, rc.params(segment=128, row_share=row_share))
    inflag = ~(w > 0)
    new = (rows[0] == 0) & ~inflag
    n_new, n_in = new.sum(axis=1), (~inflag).sum(axis=1)
    col = (n_in > 0) & (n_new.astype(np.float64) > np.float64(row_share) * n_in.astype(np.float64))
    want = np.where((rows[0] == 0) | col[:, None, :], 0.0, w)
    assert np.array_equal(got[3], n_new) and np.array_equal(got[2], new.sum(axis=2))
    assert np.array_equal(got[0].view(np.int64), want.view(np.int64))
    assert np.array_equal(got[1].view(np.int64), rows[1].view(np.int64))
    if row_share < 1:
        assert col.any() and not col.all() and np.any((got[0] == 0) & (rows[0] != 0))
    else:
        assert not col.any()


def test_a_row_has_the_same_bits_in_any_batch():
    """Row alone, in a batch of 70, at another position, and with or without the other frequency: w_out and noise bit
    for bit."""
    ctx = _ctx()
    rng = np.random.default_rng(5)
    nt, p = 3 * 128 + 1, rc.params(segment=128)
    x = rc.fringing_sky(rng, rc.NF, 70, nt)
    rc.add_bursts(rng, x, 4)
    w = rc.input_flags(rng, x.shape, 0.03)
    x = rc.poison(x, w)
    full = _run(ctx, x, w, p)
    assert (full[0] == 0).any()
    for r in (0, 33, 69):
        alone = _run(ctx, np.ascontiguousarray(x[:, r : r + 1]), np.ascontiguousarray(w[:, r : r + 1]), p)
        assert np.array_equal(alone[0][:, 0].view(np.int64), full[0][:, r].view(np.int64))
        assert np.array_equal(alone[1][:, 0].view(np.int64), full[1][:, r].view(np.int64))
    perm = rng.permutation(70)
    moved = _run(ctx, np.ascontiguousarray(x[:, perm]), np.ascontiguousarray(w[:, perm]), p)
    assert np.array_equal(moved[0].view(np.int64), full[0][:, perm].view(np.int64))
    assert np.array_equal(moved[1].view(np.int64), full[1][:, perm].view(np.int64))
    xd, wd = ctx.to_device(np.ascontiguousarray(x[1:])), ctx.to_device(np.ascontiguousarray(w[1:]))
    one = ctx.rfi_flag(xd, w=wd, **p)
    assert np.array_equal(ctx.to_host(one[0])[0].view(np.int64), full[0][1].view(np.int64))
    assert np.array_equal(ctx.to_host(one[1])[0].view(np.int64), full[1][1].view(np.int64))
    # in place: w_out may be w itself
    same = ctx.rfi_flag(xd, w=wd, out=(wd, one[1], one[2], one[3]), **p)
    assert same[0].data_ptr() == wd.data_ptr()
    assert np.array_equal(ctx.to_host(wd)[0].view(np.int64), full[0][1].view(np.int64))


def test_refusals_launch_nothing():
    """Every refusal of the C entry point returns nonzero with the context's error set, and the outputs keep their poison."""
    from driftscan_amd import _lib

    ctx = _ctx()
    rng = np.random.default_rng(9)
    nrow, nt = 5, 65
    xd = ctx.to_device(rc.crandn(rng, rc.NF, nrow, nt))
    wd = ctx.to_device(np.ones((rc.NF, nrow, nt)))
    mx = ctx.lib.dm_rfi_max_segment()
    good = dict(nf=rc.NF, nrow=nrow, nt=nt, segment=64, sigma=2.5, windows=(1, 2, 4), chi1=6.0, rho=1.5, niter=3, base=2.0,
                min_good=16, row_share=1.0, x=xd, w=wd)
    bads = [dict(nf=-1), dict(nt=-1), dict(segment=0), dict(segment=mx + 1), dict(sigma=0.0), dict(sigma=np.nan),
            dict(sigma=10.7), dict(windows=()), dict(windows=(1, 2, 4, 8, 16, 32, 64, 128)), dict(windows=(3,)),
            dict(windows=(2, 1)), dict(windows=(2, 2)), dict(windows=(128,)), dict(windows=(0,)), dict(chi1=0.0),
            dict(chi1=np.inf), dict(rho=0.5), dict(base=0.9), dict(niter=0), dict(niter=9), dict(min_good=0),
            dict(row_share=0.0), dict(row_share=1.5), dict(row_share=np.nan), dict(x=None), dict(out0="x"), dict(out1="w"),
            dict(out0=None), dict(out3="out2")]
    for bad in bads:
        a = dict(good, **bad)
        nseg = 2
        bufs = _guarded(ctx, nrow, nt, nseg)
        out = [b[1:-1] for b in bufs]
        ptr = {"x": ctx.ptr(xd), "w": ctx.ptr(wd), "out2": ctx.ptr(out[2]), None: None}
        op = [ctx.ptr(t) for t in out]
        for i in range(4):
            if "out%d" % i in bad:
                op[i] = ptr[bad["out%d" % i]]
        win = (_lib.c_int * max(len(a["windows"]), 1))(*a["windows"])
        rcode = ctx.lib.dm_rfi_flag(ctx.h, a["nf"], a["nrow"], a["nt"], a["segment"], a["sigma"], len(a["windows"]), win,
                                    a["chi1"], a["rho"], a["niter"], a["base"], a["min_good"], a["row_share"],
                                    None if a["x"] is None else ctx.ptr(a["x"]), ctx.ptr(a["w"]), *op)
        assert rcode != 0, bad
        with pytest.raises(_lib.DriftMIError, match="dm_rfi_flag"):
            ctx.check(rcode, "dm_rfi_flag")
        ctx.sync()
        for b in bufs:
            h = ctx.to_host(b)
            assert np.all(h == -77) if h.dtype == np.int32 else np.all(np.isnan(h)), bad
    # the wrapper's own checks
    with pytest.raises(ValueError):
        ctx.rfi_flag(xd.real.contiguous())
    with pytest.raises(ValueError):
        ctx.rfi_flag(xd, w=wd[:, :2].contiguous())
    with pytest.raises(ValueError):
        ctx.rfi_flag(xd, out=(wd, wd, wd, wd))
    # a tensor on the host is refused before anything is launched: the kernel would get its host address
    torch = ctx.torch
    xs, ws = ctx.to_device(np.ones((2, 3, 8), dtype=np.complex128)), ctx.to_device(np.ones((2, 3, 8)))
    outs = [torch.empty(s, dtype=d, device=xs.device)
            for s, d in (((2, 3, 8), torch.float64), ((2, 3, 1), torch.float64), ((2, 3), torch.int32), ((2, 8), torch.int32))]
    with pytest.raises(ValueError, match="one GPU"):
        ctx.rfi_flag(xs, w=ws.cpu())
    for i in range(4):
        with pytest.raises(ValueError, match="one GPU"):
            ctx.rfi_flag(xs, w=ws, out=tuple(o.cpu() if j == i else o for j, o in enumerate(outs)))
    with pytest.raises(ValueError, match="one GPU"):
        ctx.rfi_flag(xs.cpu(), w=ws)
    # nothing to do is not refused
    empty = ctx.rfi_flag(xd[:, :0].contiguous())
    assert tuple(empty[0].shape) == (rc.NF, 0, nt)


# ---- the routes -----------------------------------------------------------------------------------------------------------
STARTS, CADENCE = (0.3, 2.7, 5.0), 120.0   # 718 samples per turn
MODEL = dict(fraction=0.005, burst=4, amplitude=30.0, seed=11)
RFI = dict(chi1=5.5, segment=512)


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    """The products of tests/test_gpu_stack.py: 2 cylinders, 3 feeds, 3 frequencies, polarised."""
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("rfi")
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
    sky = healpix.sphtrans_inv_sky(alm, 32)
    probe = str(d / "sky_unit.hdf5")
    with storage.File(probe, "w") as f:
        f.create_dataset("map", data=sky)
    # the sky of the routes is 3 noise sigmas of one day's sample (rms over all rows): the flagger sees both, and the
    # leak of the Gaussian background on the sky's fastest fringes (18 samples) stays below the noise
    from driftscan_amd import timestream

    nsamp = int(0.8 * timestream.T_SIDEREAL_DAY / CADENCE)
    unit = timestream.simulate_days(pm, [str(d / "probe")], STARTS[:1], nsamp, CADENCE, maps=[probe], ndays=0)[0]
    rms = np.sqrt(np.mean([np.mean(np.abs(unit.timestream_f(fi)) ** 2) for fi in range(tel.nfreq)]))
    sigma = np.sqrt((timestream.T_SIDEREAL_DAY / CADENCE) * np.median(np.asarray(
        tel.noisepower(np.arange(tel.npairs)[None, :], np.arange(tel.nfreq)[:, None], ndays=1), dtype=np.float64)))
    fname = str(d / "sky.hdf5")
    with storage.File(fname, "w") as f:
        f.create_dataset("map", data=sky * (3.0 * sigma / rms))
    return fname


@pytest.fixture(scope="module")
def days(prod, skyfile):
    """Three days of 4 / 5 turn with one day's noise: without interference, and the same days with the bursts of MODEL."""
    from driftscan_amd import skysim, timestream

    pm, d = prod
    nsamp = int(0.8 * timestream.T_SIDEREAL_DAY / CADENCE)
    clean = [str(d / ("clean%d" % i)) for i in range(3)]
    dirty = [str(d / ("dirty%d" % i)) for i in range(3)]
    timestream.simulate_days(pm, clean, STARTS, nsamp, CADENCE, maps=[skyfile], seed=3)
    tss = timestream.simulate_days(pm, dirty, STARTS, nsamp, CADENCE, maps=[skyfile], seed=3, rfi=skysim.RFIModel(**MODEL))
    return clean, dirty, tss, nsamp


def _same_files(a, b, tel, attr=None):
    from driftscan_amd import storage

    for fi in range(tel.nfreq):
        with storage.File(a._ffile(fi), "r") as f, storage.File(b._ffile(fi), "r") as g:
            assert sorted(f.keys()) == sorted(g.keys())
            for name in f.keys():
                assert np.array_equal(f[name][:], g[name][:]), name
            if attr:
                assert int(f.attrs[attr]) == int(g.attrs[attr])


def test_flagged_days_through_the_stack_to_the_m_modes(prod, skyfile, days):
    """`simulate_days(rfi=RFIModel)` adds the bursts and flags nothing; `sidereal_stack(rfi=...)` equals the host route
    (`rfi_flag_host`, then `sidereal_regrid_host`) within 1e-10 of the largest sample (the bound of
    tests/test_gpu_sidereal.py) on the rows whose flags agree; and the m-modes of the flagged stack are strictly closer to
    those of the interference-free days than the m-modes of the unflagged stack.  The improvement and the detected and
    false shares against `RFIModel.mask` are printed: properties of SumThreshold, not thresholds of this test."""
    from driftscan_amd import skysim, timestream

    pm, d = prod
    tel = pm.telescope
    ctx = _ctx()
    clean, dirty, tss, nsamp = days
    ntime = int(np.ceil(2.5 * (2 * int(tel.mmax) + 1)))
    dphi = 2 * np.pi * CADENCE / timestream.T_SIDEREAL_DAY
    p = timestream.rfi_params(RFI)
    model = skysim.RFIModel(**MODEL)
    for fi in range(tel.nfreq):
        a, b = timestream.Timestream(clean[0], pm).timestream_f(fi), tss[0].timestream_f(fi)
        truth = model.mask(nsamp, [fi])[0]
        assert tss[0].weight_f(fi) is None                      # not flagged by the simulator
        assert np.array_equal(a[:, ~truth], b[:, ~truth]) and np.all(a[:, truth] != b[:, truth])
    ref = timestream.sidereal_stack(pm, clean, str(d / "st_clean"), ntime=ntime, a=3)
    raw = timestream.sidereal_stack(pm, dirty, str(d / "st_raw"), ntime=ntime, a=3)
    st = timestream.sidereal_stack(pm, dirty, str(d / "st_flagged"), ntime=ntime, a=3, rfi=RFI)
    found = false = nt = nf_ = 0
    for fi in range(tel.nfreq):
        s = np.zeros((tel.npairs, ntime), dtype=np.clongdouble)
        ws = np.zeros((tel.npairs, ntime), dtype=np.longdouble)
        agree = np.ones(tel.npairs, dtype=bool)
        for i, day in enumerate(tss):
            x = day.timestream_f(fi)
            w_h, _, _, _, det = timestream.rfi_flag_host(x[None], None, dtype=np.longdouble, details=True, **p)
            w_d = ctx.to_host(ctx.rfi_flag(ctx.to_device(x[None]), **p)[0])
            same = ((w_h == 0) == (w_d == 0)).all(axis=-1)[0]
            assert np.all(same | ~det["decided"].all(axis=-1)[0])
            agree &= same
            truth = np.broadcast_to(skysim.RFIModel(**dict(MODEL, seed=MODEL["seed"] + i)).mask(nsamp, [fi]), x.shape)
            found, nt = found + int((w_d[0] == 0)[truth].sum()), nt + int(truth.sum())
            false, nf_ = false + int((w_d[0] == 0)[~truth].sum()), nf_ + int((~truth).sum())
            xh, W = timestream.sidereal_regrid_host(x, w_h[0], STARTS[i], dphi, ntime, a=3, dtype=np.clongdouble)
            s += W * xh
            ws += W
        assert agree.mean() >= 0.99
        some = ws > 0
        mean = np.where(some, s / np.where(some, ws, 1), 0).astype(np.complex128)
        got = st.timestream_f(fi)
        assert np.abs(got - mean)[agree].max() <= 1e-10 * np.abs(mean).max()
        assert np.array_equal(st.weight_f(fi)[agree] > 0, some[agree])
    for ts in (ref, raw, st):
        ts.generate_modes_batched()
    ms = range(tel.mmax + 1)
    dist_raw = np.sqrt(sum(np.sum(np.abs(raw.mmode(mi) - ref.mmode(mi)) ** 2) for mi in ms))
    dist_st = np.sqrt(sum(np.sum(np.abs(st.mmode(mi) - ref.mmode(mi)) ** 2) for mi in ms))
    print("m-modes: distance to the interference-free days %.4g unflagged, %.4g flagged: %.1f times closer; "
          "detected %.3f of the burst samples, flagged %.4f of the others"
          % (dist_raw, dist_st, dist_raw / dist_st, found / nt, false / nf_))
    assert dist_st < dist_raw


def test_the_directory_call_and_the_pipeline_keys(prod, skyfile, days, tmp_path):
    """`timestream.rfi_flag` writes the flagger's outputs beside the data, in place or to another directory, and keeps an
    input weight as `weight_input`; `sidereal_from: {rfi}` and `stack_from: {rfi}` of the pipeline produce the files of
    the direct calls."""
    import yaml

    from driftscan_amd import pipeline, skysim, storage, timestream

    pm, d = prod
    tel = pm.telescope
    ctx = _ctx()
    clean, dirty, tss, nsamp = days
    p = timestream.rfi_params(RFI)
    out = timestream.rfi_flag(pm, dirty[0], str(tmp_path / "flagged"), **RFI)
    for fi in range(tel.nfreq):
        x = tss[0].timestream_f(fi)
        want = [ctx.to_host(t)[0] for t in ctx.rfi_flag(ctx.to_device(x[None]), **p)]
        with storage.File(out._ffile(fi), "r") as f:
            assert np.array_equal(f["timestream"][:], x) and "weight_input" not in f
            for name, wv in zip(("weight", "rfi_noise", "rfi_nflag", "rfi_occupancy"), want):
                assert np.array_equal(f[name][:], wv), name
            assert int(f.attrs["ntime"]) == nsamp
    assert any((out.weight_f(fi) == 0).any() for fi in range(tel.nfreq))
    # flagged input, in place: the second pass starts from the first one's flags and keeps them as weight_input
    first = [out.weight_f(fi) for fi in range(tel.nfreq)]
    again = timestream.rfi_flag(pm, out.directory, chi1=4.0)
    assert again.directory == out.directory
    for fi in range(tel.nfreq):
        with storage.File(out._ffile(fi), "r") as f:
            assert np.array_equal(f["weight_input"][:], first[fi]) and np.all(f["weight"][:][first[fi] == 0] == 0)
    with pytest.raises(ValueError, match="unknown key"):
        timestream.rfi_flag(pm, dirty[0], str(tmp_path / "bad"), threshold=3.0)
    # the pipeline
    nsu = int(0.8 * timestream.T_SIDEREAL_DAY / CADENCE)
    udir = str(tmp_path / "u0")
    timestream.simulate_days(pm, [udir], (0.2,), nsu, CADENCE, maps=[skyfile], seed=5, unstacked=True,
                             rfi=skysim.RFIModel(**MODEL))
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=False, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=False),
                timestreams=[dict(name="s0", directory=str(tmp_path / "s0"), stack_from=dict(directory=udir, rfi=dict(RFI))),
                             dict(name="sid", directory=str(tmp_path / "sid"),
                                  sidereal_from=dict(days=dirty, a=4, rfi=dict(RFI)))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    pl = pipeline.PipelineManager.from_configfile(str(cfile))
    pl.generate()
    direct = timestream.sidereal_stack(pm, dirty, str(tmp_path / "direct"), a=4, rfi=RFI)
    _same_files(pl.timestreams["sid"], direct, tel, "ndays")
    plain = timestream.sidereal_stack(pm, dirty, str(tmp_path / "plain"), a=4)
    assert any(not np.array_equal(plain.weight_f(fi), direct.weight_f(fi)) for fi in range(tel.nfreq))
    s0 = timestream.stack_baselines(pm, udir, str(tmp_path / "s0_direct"), rfi=RFI)
    _same_files(timestream.Timestream(str(tmp_path / "s0"), pm), s0, tel)
    assert s0.weight_f(0) is not None and (s0.weight_f(0) < 1).any()
