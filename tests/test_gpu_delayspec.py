"""Delay power spectra on the device: `Context.delay_spectrum` against the long-double statement
under the bound of tests/delayspec_cases.py, with the exact parts exact, poison around every output and guards behind the
tables; the bits of a (row, bin) in launches of other shapes; refusals; the limits; no intermediate of the size of the
data; and the routes `delay_spectrum`, `delay_normalise` on the device and the pipeline key.

What the fixed order of dm_delayspec.hip guarantees, and what is tested here: the bits of (row, bin, .) are the same in a
launch of that row alone, among other rows, with the bin alone in the table or among other bins, with h, s1, s2 and
count null, and with nd cut to a prefix (h always; q when a0 is kept)."""
import os
import shutil

import numpy as np
import pytest

import delayspec_cases as ds

pytestmark = pytest.mark.gpu

_REF = {}


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _case(name):
    if name not in _REF:
        c = ds.make(name)
        _REF[name] = (c, ds.reference(c))
    return _REF[name]


def _shapes(nrow, nbin, nd):
    return (((nrow, nbin, nd), np.float64), ((nrow, nbin, nd), np.float64), ((nrow, nbin), np.float64),
            ((nrow, nbin), np.float64), ((nrow, nbin), np.int32))


def _guarded(ctx, shapes):
    """Buffers with one NaN (int32: -77) guard plane on each side of the first axis; the inside is poisoned too."""
    return [ctx.to_device(np.full((s[0] + 2,) + tuple(s[1:]), -77 if dt is np.int32 else np.nan, dtype=dt)) for s, dt in shapes]


def _poisoned(ctx, bufs, inside=False):
    for b in bufs:
        h = ctx.to_host(b)
        h = h if inside else np.stack([h[0], h[-1]])
        if not (np.all(h == -77) if h.dtype == np.int32 else np.all(np.isnan(h))):
            return False
    return True


def _run(ctx, c, rows=None, nd=None, a0=None, bins=None, skip=()):
    """`Context.delay_spectrum` on the rows `rows` of the case into guarded buffers, the outputs named in `skip` (1 .. 4)
    null; the guards of the outputs and behind the tables are checked, and that a null output is not written.  Returns
    host arrays (q, h, s1, s2, count), None for a null output."""
    rows = np.arange(c["nrow"]) if rows is None else np.asarray(rows)
    x = np.ascontiguousarray(c["x"][:, rows])
    w = None if c["w"] is None else np.ascontiguousarray(c["w"][:, rows])
    nf, nrow, nt = x.shape
    nd = c["nd"] if nd is None else nd
    a0 = c["a0"] if a0 is None else a0
    off = c["bin_off"] if bins is None else np.asarray(bins, dtype=np.int32)
    nbin = off.size - 1
    step_d = ctx.to_device(np.concatenate([c["step"], np.full(5, np.nan)]))
    tap_d = None if c["taper"] is None else ctx.to_device(np.concatenate([c["taper"], np.full(5, np.nan)]))
    x_d, w_d = ctx.to_device(x), None if w is None else ctx.to_device(w)
    bufs = _guarded(ctx, _shapes(nrow, nbin, nd))
    out = [None if i in skip else b[1:-1] for i, b in enumerate(bufs)]
    got = ctx.delay_spectrum(x_d, w=w_d, taper=None if tap_d is None else tap_d[:nf], step=step_d[:nf], nd=nd, a0=a0,
                             weighting=c["weighting"], min_valid=c["min_valid"], bins=off, out=tuple(out))
    assert all((g is None and t is None) or g.data_ptr() == t.data_ptr() for g, t in zip(got, out))
    ctx.sync()
    assert _poisoned(ctx, bufs) and _poisoned(ctx, [bufs[i] for i in skip], inside=True)
    assert np.all(np.isnan(ctx.to_host(step_d)[nf:])) and (tap_d is None or np.all(np.isnan(ctx.to_host(tap_d)[nf:])))
    return [None if t is None else ctx.to_host(t) for t in out]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype != np.int32 else np.int32)


def _same(a, b):
    return all((u is None and v is None) or np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def test_limits():
    lib = _ctx().lib
    from ctypes import byref, c_int

    assert lib.dm_delayspec_max_nf() >= 1024 and lib.dm_delayspec_max_nd() >= 2048
    n = c_int(-1)
    assert [lib.dm_delayspec_segments(v, byref(n)) for v in (-1, 0)] == [0, 0] and n.value == 0
    for v, want in ((1, 1), (37, 1), (128, 1), (129, 2), (130, 2), (260, 3), (2049, 4), (10 ** 6, 4)):
        assert lib.dm_delayspec_segments(v, byref(n)) == want, v
        assert n.value % 64 == 0 and (want - 1) * n.value < v <= want * n.value
    # the cases cover one, two and three segments
    seen = set()
    for name in ds.CASES:
        seen |= {lib.dm_delayspec_segments(int(v), None) for v in np.diff(ds.make(name)["bin_off"])}
    assert {0, 1, 2, 3} <= seen


@pytest.mark.parametrize("name", sorted(ds.CASES))
def test_against_the_long_double_statement(name):
    """q and h within the bound of section 4.27, s1 and s2 to (nf n_t + 2) 2^-53, count and the zeros exact; NaN and Inf
    under the flags reach nothing; every element is written; the guards stay; a second call gives the same bits."""
    ctx = _ctx()
    c, ref = _case(name)
    out = _run(ctx, c)
    bad, worst = ds.check(c, out, ref)
    print("%s: worst error %.3g of its bound" % (name, worst))
    assert not bad, bad
    assert all(np.all(np.isfinite(o)) for o in out[:4]) and np.all(out[4] >= 0)
    assert _same(out, _run(ctx, c))


@pytest.mark.parametrize("name", ("edges", "seventeen"))
def test_other_weighting_and_null_inputs(name):
    """The other weighting of the case; w = None equals w = ones and taper = None equals ones, bit for bit, and with
    both weightings (omega = 1 either way)."""
    ctx = _ctx()
    base = ds.make(name)
    c = ds.make(name, weighting="weight" if base["weighting"] == "mask" else "mask")
    bad, worst = ds.check(c, _run(ctx, c), ds.reference(c))
    assert not bad, bad
    c = ds.make(name, w_none=True, taper_none=True)
    out = _run(ctx, c)
    bad, worst = ds.check(c, out, ds.reference(c))
    assert not bad, bad
    ones = dict(c, w=np.ones(c["x"].shape), taper=np.ones(c["nf"]))
    assert _same(out, _run(ctx, ones))
    assert _same(out, _run(ctx, dict(ones, weighting="weight" if c["weighting"] == "mask" else "mask")))
    assert np.array_equal(out[4], np.broadcast_to(np.diff(c["bin_off"]), out[4].shape))
    # without weights and with min_valid > nf every series is dropped: exact zeros
    out = _run(ctx, dict(c, min_valid=c["nf"] + 1))
    assert all(not o.any() for o in out)


@pytest.mark.parametrize("name", ("edges", "wide", "long"))
def test_bits_do_not_depend_on_the_launch(name):
    ctx = _ctx()
    c, _ = _case(name)
    full = _run(ctx, c)
    nbin = c["bin_off"].size - 1
    for row in (0, c["nrow"] - 1):
        one = _run(ctx, c, rows=[row])
        assert _same(one, [o[[row]] for o in full]), row
    perm = np.roll(np.arange(c["nrow"]), 2)[::-1].copy()
    assert _same(_run(ctx, c, rows=perm), [o[perm] for o in full])
    for b in range(nbin):   # a bin alone in the table
        alone = _run(ctx, c, bins=c["bin_off"][b : b + 2])
        assert _same(alone, [o[:, [b]] for o in full]), b
    for skip in ((1,), (2, 3, 4), (1, 2, 3, 4)):
        part = _run(ctx, c, skip=skip)
        assert _same(part, [None if i in skip else o for i, o in enumerate(full)]), skip
    if c["nd"] > 1:
        for cut in sorted({1, c["nd"] // 2, c["nd"] - 1} - {0}):   # h is a prefix; q too where a0 stays inside
            short = _run(ctx, c, nd=cut, a0=min(c["a0"], cut - 1))
            assert np.array_equal(_bits(short[1]), _bits(full[1][:, :, :cut])), cut
            assert _same(short[2:], full[2:])
            if c["a0"] < cut:
                assert np.array_equal(_bits(short[0]), _bits(full[0][:, :, :cut])), cut


def test_refusals_launch_nothing():
    """Every refusal of dm_delay_spectrum returns nonzero with the context's error set and leaves the poison; zero sizes
    are no-ops; the Python layer refuses what it can see."""
    from ctypes import POINTER, c_int

    from driftscan_amd import _lib

    ctx = _ctx()
    lib = ctx.lib
    nf, nrow, nt, nd, nbin = 6, 3, 9, 5, 2
    x_d, w_d = ctx.to_device(np.ones((nf, nrow, nt), dtype=np.complex128)), ctx.to_device(np.ones((nf, nrow, nt)))
    tap, step = ctx.to_device(np.ones(nf)), ctx.to_device(np.linspace(-0.4, 0.4, nf))
    good = dict(nf=nf, nrow=nrow, nt=nt, nd=nd, a0=2, weighting=0, min_valid=1, tap=tap, step=step, nbin=nbin, off=[0, 4, 9],
                x=x_d, w=w_d)
    bads = [dict(nf=-1), dict(nrow=-1), dict(nt=-1), dict(nd=-1), dict(nbin=-1), dict(nf=lib.dm_delayspec_max_nf() + 1),
            dict(nd=lib.dm_delayspec_max_nd() + 1), dict(min_valid=0), dict(min_valid=-3), dict(a0=-1), dict(a0=nd),
            dict(weighting=2), dict(weighting=-1), dict(x=None), dict(step=None), dict(off=None), dict(out0=None),
            dict(off=[0, 5, 4]), dict(off=[-1, 4, 9]), dict(off=[0, 4, 10]), dict(off=[3, 2, 9]),
            dict(out0="x"), dict(out1="w"), dict(out2="tap"), dict(out3="step"), dict(out4="x"), dict(out1="out0"),
            dict(out3="out2"), dict(out4="out2")]
    for bad in bads:
        a = dict(good, **bad)
        bufs = _guarded(ctx, _shapes(nrow, nbin, nd))
        op = [ctx.ptr(b[1:-1]) for b in bufs]
        ptr = {"x": ctx.ptr(x_d), "w": ctx.ptr(w_d), "tap": ctx.ptr(tap), "step": ctx.ptr(step), "out0": op[0], "out2": op[2],
               None: None}
        for i in range(5):
            if "out%d" % i in bad:
                op[i] = ptr[bad["out%d" % i]]
        off = None if a["off"] is None else (c_int * len(a["off"]))(*a["off"])
        rcode = lib.dm_delay_spectrum(ctx.h, a["nf"], a["nrow"], a["nt"], a["nd"], a["a0"], a["weighting"], a["min_valid"],
                                      ctx.ptr(a["tap"]), None if a["step"] is None else ctx.ptr(a["step"]), a["nbin"], off,
                                      None if a["x"] is None else ctx.ptr(a["x"]), ctx.ptr(a["w"]), *op)
        assert rcode != 0, bad
        with pytest.raises(_lib.DriftMIError, match="dm_delay_spectrum"):
            ctx.check(rcode, "dm_delay_spectrum")
        ctx.sync()
        assert _poisoned(ctx, bufs, inside=True), bad
    assert np.all(ctx.to_host(x_d) == 1) and np.all(ctx.to_host(w_d) == 1)
    for zero in ("nf", "nrow", "nt", "nd", "nbin"):   # zero sizes are no-ops, whatever else is passed
        a = dict(good, **{zero: 0})
        bufs = _guarded(ctx, _shapes(nrow, nbin, nd))
        rcode = lib.dm_delay_spectrum(ctx.h, a["nf"], a["nrow"], a["nt"], a["nd"], 0, 0, 1, None, None, a["nbin"], None, None,
                                      None, *(ctx.ptr(b[1:-1]) for b in bufs))
        assert rcode == 0, zero
        ctx.sync()
        assert _poisoned(ctx, bufs, inside=True)
    empty = ctx.delay_spectrum(x_d[:, :, :0].contiguous(), step=step, nd=nd)
    assert tuple(empty[0].shape) == (nrow, 1, nd) and tuple(empty[4].shape) == (nrow, 1)
    for kw in (dict(weighting="natural"), dict(step=None), dict(nd=None), dict(a0=nd), dict(min_valid=0), dict(bins=0),
               dict(bins=[0, 12]), dict(bins=[4, 2]), dict(bins=[0.5, 3]), dict(w=w_d[:, :2].contiguous()),
               dict(step=step[:3]), dict(taper=ctx.to_device(np.ones(nf + 1))), dict(out=(x_d,)),
               dict(out=(None, None, None, None, None))):
        with pytest.raises((ValueError, _lib.DriftMIError)):
            ctx.delay_spectrum(x_d, **dict(dict(w=w_d, step=step, nd=nd), **kw))
    with pytest.raises(ValueError):
        ctx.delay_spectrum(x_d.to(ctx.torch.complex64), step=step, nd=nd)
    for key, value in dict(w=w_d.cpu(), step=step.cpu(), taper=tap.cpu()).items():   # never reaches the kernel
        with pytest.raises(ValueError, match="one GPU"):
            ctx.delay_spectrum(x_d, **dict(dict(w=w_d, step=step, nd=nd), **{key: value}))
    # bins as an int: the last one short
    q, h, s1, s2, cnt = ctx.delay_spectrum(x_d, w=w_d, step=step, nd=nd, bins=4)
    assert tuple(q.shape) == (nrow, 3, nd) and np.array_equal(ctx.to_host(cnt), np.broadcast_to([4, 4, 1], (nrow, 3)))


def test_no_intermediate_of_the_size_of_the_data():
    """Around a call torch allocates the outputs and nothing else, and the context's workspace arena does not grow: the
    transformed cube (nd x nrow x nt complex), a weighted copy or a phase table would show in one of the two."""
    ctx = _ctx()
    torch = ctx.torch
    nf, nrow, nt, nd = 64, 8, 600, 64
    rng = np.random.default_rng(3)
    x_d = ctx.to_device(rng.standard_normal((nf, nrow, nt)) + 1j * rng.standard_normal((nf, nrow, nt)))
    w_d = ctx.to_device(np.where(rng.random((nf, nrow, nt)) < 0.3, 0.0, 1.0))
    step_d, tap_d = ctx.to_device(np.linspace(-0.5, 0.5, nf)), ctx.to_device(np.ones(nf))
    ctx.delay_spectrum(x_d, w=w_d, taper=tap_d, step=step_d, nd=nd)   # the tables are up, the arena has its size
    ctx.sync()
    arena = int(ctx.lib.dm_ctx_workspace_bytes(ctx.h))
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ctx.delay_spectrum(x_d, w=w_d, taper=tap_d, step=step_d, nd=nd, bins=64)
    ctx.sync()
    peak = torch.cuda.max_memory_allocated() - before
    nbin = out[0].shape[1]
    outputs = 8 * nrow * nbin * (2 * nd + 2) + 4 * nrow * nbin
    cube = 16 * nd * nrow * nt
    print("outputs %d bytes, torch peak %d bytes, the transformed cube would be %d bytes" % (outputs, peak, cube))
    assert peak <= outputs + 5 * 512 and outputs < cube // 4
    assert int(ctx.lib.dm_ctx_workspace_bytes(ctx.h)) == arena


# ---- the routes -----------------------------------------------------------------------------------------------------
NFREQ = 12
DELAY = dict(buffer=0.5, eigencut=1e-6, nclass=3)
SOURCE = dict(theta=np.array([1.1]), phi=np.array([2.0]), flux=np.array([10.0]), nu0=415.0, index=np.array([0.0]))


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    import yaml

    from driftscan_amd import device, manager, timestream

    device.reset_context()
    d = tmp_path_factory.mktemp("delayspec")
    conf = dict(config=dict(beamtransfers=True, kltransform=False, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="UnpolarisedCylinder", num_freq=NFREQ, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0))
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    clean = timestream.simulate(pm, str(d / "clean"), ndays=0, sources=[SOURCE])
    return pm, d, clean


def _read(path):
    from driftscan_amd import storage

    with storage.File(path, "r") as f:
        return {k: np.asarray(f[k][:]) for k in f.keys()}, dict(f.attrs)


def _with_weights(src, dst_dir, pm, w):
    """A copy of the directory of `src` with the weights w (nfreq, nrow, nt) and NaN under the flags."""
    from driftscan_amd import storage, timestream

    shutil.copytree(src.directory, dst_dir, ignore=shutil.ignore_patterns("delayspectrum_*"))
    dst = timestream.Timestream(dst_dir, pm)
    for fi in range(w.shape[0]):
        data, attrs = _read(src._ffile(fi))
        data["weight"] = w[fi]
        data["timestream"] = np.where(w[fi] > 0, data["timestream"], np.nan)
        with storage.File(dst._ffile(fi), "w") as f:
            for name, value in data.items():
                f.create_dataset(name, data=np.ascontiguousarray(value))
            for name, value in attrs.items():
                f.attrs[name] = value
    return dst


def test_route_writes_what_the_device_gives(prod):
    """`delay_spectrum` writes the file; its q, window, s1, s2 and count are those of `Context.delay_spectrum` on the
    stacked arrays, bit for bit across two values of chunk_gb, and within the bound of the long-double statement; the
    wedge is the count-weighted mean of the rows of each length bin."""
    from driftscan_amd import timestream

    pm, d, clean = prod
    ctx = _ctx()
    tel = pm.telescope
    nrow = int(tel.npairs)
    x = np.stack([clean.timestream_f(fi) for fi in range(NFREQ)])
    nt = x.shape[2]
    rng = np.random.default_rng(6)
    w = np.where(rng.random(x.shape) < 0.2, 0.0, rng.uniform(0.5, 2.0, x.shape))
    flagged = _with_weights(clean, str(d / "flagged"), pm, w)
    kw = dict(nd=17, oversample=2.0, taper="blackman", weighting="weight", min_valid=5, tbin=7, blen_bins=2)
    root = timestream.delay_spectrum(pm, flagged.directory, name="a", **kw)
    assert root == os.path.join(flagged.directory, "delayspectrum_a.hdf5")
    fa, attrs = _read(root)
    per_row = 24.0 * NFREQ * nt + 40.0 * fa["count"].shape[1] * 17 + 64.0
    fb, attrs_b = _read(timestream.delay_spectrum(pm, flagged.directory, name="b", chunk_gb=2.5 * per_row / 2.0**30, **kw))
    assert sorted(fa) == sorted(fb) == sorted(["tau", "q", "window", "spectrum", "noise", "s1", "s2", "count", "info", "bin_off",
                                               "step", "taper", "blen", "horizon", "blen_edges", "wedge", "wedge_hits"])
    assert attrs == attrs_b and attrs["nd"] == 17 and attrs["norm"] == "window" and attrs["weighting"] == "weight"
    for key in fa:
        assert fa[key].dtype == fb[key].dtype and np.array_equal(fa[key], fb[key], equal_nan=fa[key].dtype.kind == "f"), key
    with pytest.raises(ValueError, match="chunk_gb"):
        timestream.delay_spectrum(pm, flagged.directory, name="c", chunk_gb=0.5 * per_row / 2.0**30, **kw)
    tau, step, a0, dtau = timestream.delay_grid(tel, nd=17, oversample=2.0)
    tap = timestream.delay_taper(NFREQ, "blackman")
    assert np.array_equal(fa["tau"], tau) and np.array_equal(fa["step"], step) and np.array_equal(fa["taper"], tap)
    nbin = fa["bin_off"].size - 1
    assert nbin == -(-nt // 7) and fa["q"].shape == (nrow, nbin, 17)
    xn = np.where(w > 0, x, np.nan)
    got = ctx.delay_spectrum(ctx.to_device(xn), w=ctx.to_device(w), taper=tap, step=step, nd=17, a0=a0, weighting="weight",
                             min_valid=5, bins=7)
    got = [ctx.to_host(g) for g in got]
    for key, g in zip(("q", "window", "s1", "s2", "count"), got):
        assert np.array_equal(_bits(fa[key]), _bits(g)), key
    c = dict(nf=NFREQ, nrow=nrow, nt=nt, nd=17, a0=a0, step=step, taper=tap, x=xn, w=w, bin_off=fa["bin_off"], weighting="weight",
             min_valid=5)
    bad, worst = ds.check(c, got, ds.reference(c))
    print("route: worst error %.3g of its bound" % worst)
    assert not bad, bad
    blen = np.sqrt((np.asarray(tel.baselines) ** 2).sum(axis=1))
    assert np.allclose(fa["blen"], blen) and np.allclose(fa["horizon"], blen / 299.792458)
    sp, ns, info = timestream.delay_normalise(fa["q"], fa["window"], fa["s1"], norm="window")
    assert np.allclose(fa["spectrum"], sp, rtol=1e-12, equal_nan=True) and np.allclose(fa["noise"], ns, rtol=1e-12, equal_nan=True)
    assert np.array_equal(fa["info"], info) and not info.any()
    edges = fa["blen_edges"]
    assert edges.shape == (3,) and edges[0] == 0 and edges[-1] == blen.max()
    for j in range(2):
        rows = (blen >= edges[j]) & ((blen < edges[j + 1]) | (j == 1))
        cnt = fa["count"][rows].astype(np.float64)
        want = (cnt[:, :, None] * fa["spectrum"][rows]).sum(axis=0) / cnt.sum(axis=0)[:, None]
        assert np.allclose(fa["wedge"][j], want, rtol=1e-12) and np.array_equal(fa["wedge_hits"][j], cnt.sum(axis=0))


def test_point_source_peaks_at_its_geometric_delay(prod):
    """Sample by sample on an east-west row: the visibility of a source in direction cosine x east of the meridian is
    A exp(2 pi i nu u x / c) (the convention of sections 4.25 and 4.26) with A >= 0, the product of two equal beams, so
    |D_a|^2 peaks at the grid point nearest to -u x / c (the transform of a non-negative envelope is largest at 0)."""
    from driftscan_amd import timestream

    pm, d, clean = prod
    tel = pm.telescope
    bl = np.asarray(tel.baselines, dtype=np.float64)
    rows = np.nonzero((np.abs(bl[:, 1]) < 1e-9) & (np.abs(bl[:, 0]) > 1e-9))[0]
    assert rows.size
    fs, _ = _read(timestream.delay_spectrum(pm, clean.directory, name="src", nd=13, oversample=64.0, taper="hann", tbin=1))
    nt = fs["count"].shape[1]
    dtau = fs["tau"][1] - fs["tau"][0]
    ha = SOURCE["phi"][0] - 2.0 * np.pi * np.arange(nt) / nt
    xe = np.sin(SOURCE["theta"][0]) * np.sin(ha)
    near = np.nonzero((np.abs(xe) < 0.45) & (np.cos(ha) > 0))[0]
    assert near.size >= 3
    moved = 0
    for r in rows:
        want = -bl[r, 0] * xe[near] / 299.792458 / dtau          # in grid steps from a0
        peak = np.argmax(fs["q"][r, near], axis=1) - 6
        print("row %d (u = %.2f m): peaks %s, geometric delay %s steps" % (r, bl[r, 0], peak, np.round(want, 2)))
        assert np.all(np.abs(peak - want) <= 0.6)
        moved += int(np.any(np.rint(want) != 0))
    assert moved   # the delay leaves the central bin somewhere


def test_filter_takes_out_what_the_host_statement_says(prod):
    """After `delay_filter(mode="filter")` the power inside the filtered band of every row drops by the factor that
    `delay_fit_host` and `delay_spectrum_host` give on the same data: what is left is the truncation of the basis, far
    above the rounding of either route (kappa 2^-53 of the data), so the two factors agree to 1e-3."""
    from driftscan_amd import timestream

    pm, d, clean = prod
    tel = pm.telescope
    x = np.stack([clean.timestream_f(fi) for fi in range(NFREQ)])
    rng = np.random.default_rng(9)
    w = np.where(rng.random(x.shape) < 0.03, 0.0, 1.0)
    holes = _with_weights(clean, str(d / "holes"), pm, w)
    filtered = timestream.delay_filter(pm, holes.directory, str(d / "filtered"), mode="filter", **DELAY)
    kw = dict(nd=NFREQ, taper="blackman-harris", tbin=None)
    fb, _ = _read(timestream.delay_spectrum(pm, holes.directory, name="f", **kw))
    fa, _ = _read(timestream.delay_spectrum(pm, filtered.directory, name="f", **kw))
    table, rk, of, tau_row = timestream.delay_classes(tel, **DELAY)
    bases, o = [], 0
    for r in rk:
        bases.append(np.ascontiguousarray(table[o : o + NFREQ * r].reshape(r, NFREQ).T))
        o += NFREQ * r
    xh, wh, info = timestream.delay_fit_host(np.where(w > 0, x, 0.0), w, bases, of, mode="filter")
    assert not info.any()
    tau, step, a0, dtau = timestream.delay_grid(tel, nd=NFREQ)
    tap = timestream.delay_taper(NFREQ, "blackman-harris")
    hb = timestream.delay_spectrum_host(np.where(w > 0, x, 0.0), w, tap, step, NFREQ, a0, "mask", 1, [0, x.shape[2]])
    ha = timestream.delay_spectrum_host(xh, wh, tap, step, NFREQ, a0, "mask", 1, [0, x.shape[2]])
    assert np.array_equal(fa["count"], ha[4]) and np.array_equal(fb["count"], hb[4])
    for r in range(x.shape[1]):
        band = np.abs(tau) <= tau_row[r]
        assert band.any()
        dev = fa["q"][r, 0, band].sum() / fb["q"][r, 0, band].sum()
        host = ha[0][r, 0, band].sum() / hb[0][r, 0, band].sum()
        print("row %d: power in |tau| <= %.4f us drops by %.3g on the device, %.3g by the host statement" % (r, tau_row[r], dev, host))
        assert host < 1.0 and abs(dev / host - 1.0) <= 1e-3


def test_inverse_on_the_device_agrees_with_the_host(prod):
    from driftscan_amd import timestream

    pm, d, clean = prod
    ctx = _ctx()
    x = np.stack([clean.timestream_f(fi) for fi in range(NFREQ)])
    rng = np.random.default_rng(12)
    w = np.where(rng.random(x.shape) < 0.25, 0.0, 1.0)
    w[:, 1] = 0.0                                  # a row without data: info = nd, NaN
    tau, step, a0, dtau = timestream.delay_grid(pm.telescope)
    tap = timestream.delay_taper(NFREQ, "blackman")
    q, h, s1, s2, cnt = ctx.delay_spectrum(ctx.to_device(x), w=ctx.to_device(w), taper=tap, step=step, nd=NFREQ, a0=a0, bins=16)
    for norm, ridge in (("inverse", 0.0), ("inverse", 1e-3), ("window", 0.0)):
        sp, ns, info = timestream.delay_normalise(q, h, s2, norm=norm, ridge=ridge)
        hp, hn, hi = timestream.delay_normalise(ctx.to_host(q), ctx.to_host(h), ctx.to_host(s2), norm=norm, ridge=ridge)
        sp, ns, info = ctx.to_host(sp), ctx.to_host(ns), ctx.to_host(info)
        assert np.array_equal(info, hi) and np.all(info[1] == NFREQ) and not np.delete(info, 1, axis=0).any()
        assert np.all(np.isnan(sp[1])) and np.all(np.isnan(ns[1])) and np.array_equal(np.isnan(sp), np.isnan(hp))
        ok = info == 0
        peak = np.abs(hp[ok]).max(axis=1, keepdims=True)
        err = np.abs(sp[ok] - hp[ok]) / peak
        nerr = np.abs(ns[ok] - hn[ok]) / np.abs(hn[ok]).max(axis=1, keepdims=True)
        print("%s, ridge %g: device against host %.3g of the peak (noise floor %.3g)" % (norm, ridge, err.max(), nerr.max()))
        assert err.max() <= 1e-9 and nerr.max() <= 1e-9
    fi, _ = _read(timestream.delay_spectrum(pm, clean.directory, name="inv", taper="blackman", norm="inverse", tbin=16))
    assert not fi["info"].any() and np.all(np.isfinite(fi["spectrum"]))


def test_unstacked_directories_and_pipeline_key(prod, tmp_path):
    """An unstacked directory is refused; `delayspectra:` in the pipeline writes the file of the stand-alone call; an
    unknown key raises before anything runs."""
    import yaml

    from driftscan_amd import pipeline, timestream

    pm, d, clean = prod
    udir = str(tmp_path / "u")
    timestream.simulate_unstacked(pm, udir, ndays=0, sources=[SOURCE])
    with pytest.raises(ValueError, match="unstacked"):
        timestream.delay_spectrum(pm, udir)
    with pytest.raises(ValueError, match="unknown key"):
        timestream.delayspectrum_params(dict(nel=5))
    pdir = str(tmp_path / "p")
    shutil.copytree(clean.directory, pdir, ignore=shutil.ignore_patterns("delayspectrum_*"))
    entry = dict(name="w", nd=15, oversample=2.0, taper="hann", tbin=9, blen_bins=3, norm="inverse", ridge=1e-6)
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=True, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=True, nside=16, delayspectra=[entry]),
                timestreams=[dict(name="p", directory=pdir)])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    pipeline.PipelineManager.from_configfile(str(cfile)).generate()
    theirs = timestream.delay_spectrum(pm, clean.directory, **entry)
    ra, rb = _read(os.path.join(pdir, "delayspectrum_w.hdf5")), _read(theirs)
    assert sorted(ra[0]) == sorted(rb[0]) and ra[1] == rb[1] and "wedge" in ra[0]
    for key in ra[0]:
        assert np.array_equal(ra[0][key], rb[0][key], equal_nan=ra[0][key].dtype.kind == "f"), key
    conf["config"]["delayspectra"] = [dict(entry, colour="red")]
    cfile.write_text(yaml.dump(conf))
    with pytest.raises(ValueError, match="unknown key"):
        pipeline.PipelineManager.from_configfile(str(cfile))
