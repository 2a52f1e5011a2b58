"""Ring maps on the device: `Context.ringmap` against the long-double statement under the bound of
the section on the cases of tests/ringmap_cases.py, with poison around and inside every output and guards behind every
table; the bits of a (frequency, group) in launches of other shapes; refusals; and the routes `timestream.ringmap` and
the pipeline key `ringmaps`."""
import os
import shutil

import numpy as np
import pytest

import ringmap_cases as rc

pytestmark = pytest.mark.gpu

_REF = {}


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _case(name):
    if name not in _REF:
        c = rc.make(name)
        _REF[name] = (c, rc.reference(c))
    return _REF[name]


def _guarded(ctx, shape):
    """A float64 buffer with one NaN guard plane on each side of the first axis; the inside is NaN too."""
    return ctx.to_device(np.full((shape[0] + 2,) + tuple(shape[1:]), np.nan))


def _table(ctx, a, guard=5):
    """(the table with NaN behind it, its length)"""
    return ctx.to_device(np.concatenate([np.asarray(a, dtype=np.float64), np.full(guard, np.nan)])), len(a)


def _sub(c, fsel=None, gsel=None, tsel=None, esel=None):
    """The case cut down to the frequencies fsel, the groups gsel, the samples tsel (a slice) and the elevations esel."""
    fsel = list(range(c["nf"])) if fsel is None else list(fsel)
    gsel = list(range(len(c["group_off"]) - 1)) if gsel is None else list(gsel)
    tsel = slice(None) if tsel is None else tsel
    esel = np.arange(c["nel"]) if esel is None else np.asarray(esel)
    off = c["group_off"]
    pick = np.concatenate([np.arange(off[g], off[g + 1]) for g in gsel]).astype(np.int64)
    vis = np.ascontiguousarray(c["vis"][fsel][:, :, tsel])
    return dict(c, nf=len(fsel), nt=vis.shape[2], nel=len(esel), vis=vis,
                w=None if c["w"] is None else np.ascontiguousarray(c["w"][fsel][:, :, tsel]),
                group_off=np.concatenate([[0], np.cumsum([off[g + 1] - off[g] for g in gsel])]).astype(np.int32),
                members=c["members"][pick], v=c["v"][pick], taper=None if c["taper"] is None else c["taper"][pick],
                scale=c["scale"][fsel], sinza=c["sinza"][esel])


def _run(ctx, c, parts=2, norm=True, norm2=True):
    """`Context.ringmap` on the case into guarded, poisoned buffers, its tables guarded; returns host (map, D, D2)."""
    ngroup = len(c["group_off"]) - 1
    tabs = {k: _table(ctx, c[k]) for k in ("v", "scale", "sinza")}
    if c["taper"] is not None:
        tabs["taper"] = _table(ctx, c["taper"])
    bufs = [_guarded(ctx, (c["nf"], ngroup, parts, c["nel"], c["nt"])), _guarded(ctx, (c["nf"], ngroup, c["nt"])),
            _guarded(ctx, (c["nf"], ngroup, c["nt"]))]
    x_d, w_d = ctx.to_device(c["vis"]), None if c["w"] is None else ctx.to_device(c["w"])
    view = {k: t[:n] for k, (t, n) in tabs.items()}
    got = ctx.ringmap(x_d, c["group_off"], c["members"], view["v"], view["scale"], view["sinza"], w=w_d,
                      taper=view.get("taper"), parts=parts, out=bufs[0][1:-1], norm=bufs[1][1:-1] if norm else False,
                      norm2=bufs[2][1:-1] if norm2 else False)
    ctx.sync()
    assert got[0].data_ptr() == bufs[0][1:-1].data_ptr() and (got[1] is None) == (not norm) and (got[2] is None) == (not norm2)
    host = [ctx.to_host(b) for b in bufs]
    assert all(np.all(np.isnan(h[0])) and np.all(np.isnan(h[-1])) for h in host)
    assert all(np.all(np.isnan(ctx.to_host(t)[n:])) for t, n in tabs.values())
    if not norm:
        assert np.all(np.isnan(host[1]))
    if not norm2:
        assert np.all(np.isnan(host[2]))
    return host[0][1:-1], host[1][1:-1] if norm else None, host[2][1:-1] if norm2 else None


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("parts", (1, 2))
@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_against_the_long_double_statement(name, parts):
    """Every element within the bound of section 4.25, the exact zeros exact, nothing from a sample that is not kept,
    every element written, the guards untouched; a second call gives the same bits."""
    ctx = _ctx()
    c, ref = _case(name)
    got = _run(ctx, c, parts)
    bad, worst = rc.check(c, got, ref)
    print("%s parts %d: worst error %.3g of its bound" % (name, parts, worst))
    assert not bad, bad
    assert all(np.all(np.isfinite(g)) for g in got)
    again = _run(ctx, c, parts)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))


def test_without_weights_and_taper():
    """w = None equals w = ones and taper = None equals ones, bit for bit."""
    ctx = _ctx()
    c = rc.make("edges", w_none=True, taper_none=True)
    got = _run(ctx, c)
    bad, _ = rc.check(c, got, rc.reference(c))
    assert not bad, bad
    ones = _run(ctx, dict(c, w=np.ones(c["vis"].shape), taper=np.ones(c["v"].shape)))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, ones))
    assert np.array_equal(got[1], np.broadcast_to(np.diff(c["group_off"])[None, :, None].astype(float), got[1].shape))


@pytest.mark.parametrize("name", ("edges", "wide", "blocks"))
def test_bits_do_not_depend_on_the_launch(name):
    """A (frequency, group) gives the same bits among the others, alone, on a subset of samples, on a subset of
    elevations and with norm / norm2 null; plane 0 of parts = 2 is the parts = 1 result."""
    ctx = _ctx()
    c, _ = _case(name)
    full = _run(ctx, c)
    ngroup = len(c["group_off"]) - 1
    for f in range(c["nf"]):
        for g in range(ngroup):
            one = _run(ctx, _sub(c, fsel=[f], gsel=[g]))
            assert all(np.array_equal(_bits(a[0, 0]), _bits(b[f, g])) for a, b in zip(one, full)), (f, g)
    t0 = min(3, c["nt"] - 1)
    win = _run(ctx, _sub(c, tsel=slice(t0, c["nt"] - 1)))
    assert all(np.array_equal(_bits(a), _bits(b[..., t0:c["nt"] - 1])) for a, b in zip(win, full))
    esel = np.arange(1, c["nel"], 2)
    some = _run(ctx, _sub(c, esel=esel, gsel=list(range(ngroup))[::-1]))
    assert np.array_equal(_bits(some[0]), _bits(full[0][:, ::-1][:, :, :, esel]))
    assert np.array_equal(_bits(some[1]), _bits(full[1][:, ::-1])) and np.array_equal(_bits(some[2]), _bits(full[2][:, ::-1]))
    for norm, norm2 in ((False, True), (True, False), (False, False)):
        part = _run(ctx, c, norm=norm, norm2=norm2)
        assert np.array_equal(_bits(part[0]), _bits(full[0]))
        assert all(p is None or np.array_equal(_bits(p), _bits(q)) for p, q in zip(part[1:], full[1:]))
    p1 = _run(ctx, c, parts=1)
    assert np.array_equal(_bits(p1[0][:, :, 0]), _bits(full[0][:, :, 0]))
    assert np.array_equal(_bits(p1[1]), _bits(full[1])) and np.array_equal(_bits(p1[2]), _bits(full[2]))


def test_refusals_launch_nothing():
    """Every refusal of dm_ringmap returns nonzero with the context's error set and leaves the poison; zero sizes are
    no-ops; the Python layer refuses what it can see."""
    from ctypes import c_int

    from driftscan_amd import _lib

    ctx = _ctx()
    lib = ctx.lib
    nf, nrow, nt, nel = 2, 5, 9, 7
    x_d, w_d = ctx.to_device(np.ones((nf, nrow, nt), dtype=np.complex128)), ctx.to_device(np.ones((nf, nrow, nt)))
    off, mem = [0, 2, 5], [0, 1, 1, 3, 4]
    v_d, t_d = ctx.to_device(np.arange(5.0)), ctx.to_device(np.ones(5))
    sc_d, s_d = ctx.to_device(np.ones(nf)), ctx.to_device(np.linspace(-1, 1, nel))
    good = dict(nf=nf, nrow=nrow, nt=nt, ngroup=2, off=off, mem=mem, v=v_d, taper=t_d, scale=sc_d, nel=nel, sinza=s_d, parts=2,
                vis=x_d, w=w_d)

    def call(a, op):
        offp = None if a["off"] is None else (c_int * max(len(a["off"]), 1))(*a["off"])
        memp = None if a["mem"] is None else (c_int * max(len(a["mem"]), 1))(*a["mem"])
        dev = [None if a[k] is None else ctx.ptr(a[k]) for k in ("v", "taper", "scale", "sinza", "vis", "w")]
        return lib.dm_ringmap(ctx.h, a["nf"], a["nrow"], a["nt"], a["ngroup"], offp, memp, dev[0], dev[1], dev[2], a["nel"],
                              dev[3], a["parts"], dev[4], dev[5], *op)

    bads = [dict(nf=-1), dict(nrow=-1), dict(nt=-1), dict(ngroup=-1), dict(nel=-1), dict(parts=0), dict(parts=3), dict(parts=-1),
            dict(mem=[0, 1, 1, 3, 5]), dict(mem=[0, -1, 1, 3, 4]), dict(nrow=4), dict(off=[0, 3, 2]), dict(off=[2, 1, 5]),
            dict(off=[-1, 2, 5]), dict(off=None), dict(mem=None), dict(v=None), dict(scale=None), dict(sinza=None),
            dict(vis=None), dict(out0=None), dict(out0="vis"), dict(out1="w"), dict(out2="v"), dict(out1="out0"),
            dict(out2="out1"), dict(out0="sinza")]
    for bad in bads:
        a = dict(good, **{k: v for k, v in bad.items() if not k.startswith("out")})
        bufs = [_guarded(ctx, (nf, 2, 2, nel, nt)), _guarded(ctx, (nf, 2, nt)), _guarded(ctx, (nf, 2, nt))]
        op = [ctx.ptr(b[1:-1]) for b in bufs]
        ptr = {"vis": ctx.ptr(x_d), "w": ctx.ptr(w_d), "v": ctx.ptr(v_d), "sinza": ctx.ptr(s_d), "out0": op[0], "out1": op[1],
               None: None}
        for i in range(3):
            if "out%d" % i in bad:
                op[i] = ptr[bad["out%d" % i]]
        rcode = call(a, op)
        assert rcode != 0, bad
        with pytest.raises(_lib.DriftMIError, match="dm_ringmap"):
            ctx.check(rcode, "dm_ringmap")
        ctx.sync()
        assert all(np.all(np.isnan(ctx.to_host(b))) for b in bufs), bad
    assert np.all(ctx.to_host(x_d) == 1) and np.all(ctx.to_host(w_d) == 1) and np.array_equal(ctx.to_host(v_d), np.arange(5.0))
    # zero sizes are no-ops, whatever else is passed
    for zero in (dict(nf=0), dict(nt=0), dict(ngroup=0), dict(nel=0)):
        a = dict(good, **zero)
        a.update(off=None, mem=None, v=None, taper=None, scale=None, sinza=None, vis=None, w=None)
        bufs = [_guarded(ctx, (nf, 2, 2, nel, nt)), _guarded(ctx, (nf, 2, nt)), _guarded(ctx, (nf, 2, nt))]
        assert call(a, [ctx.ptr(b[1:-1]) for b in bufs]) == 0
        ctx.sync()
        assert all(np.all(np.isnan(ctx.to_host(b))) for b in bufs)
    # groups without members: zeros everywhere
    m, d, d2 = ctx.ringmap(x_d, [0, 0, 0], [], [], sc_d, s_d)
    assert tuple(m.shape) == (nf, 2, 1, nel, nt) and not ctx.to_host(m).any() and not ctx.to_host(d).any() and not ctx.to_host(d2).any()
    empty = ctx.ringmap(x_d[:, :, :0].contiguous(), off, mem, v_d, sc_d, s_d)
    assert tuple(empty[0].shape) == (nf, 2, 1, nel, 0)
    torch = ctx.torch
    base = dict(group_off=off, members=mem, v=v_d, scale=sc_d, sinza=s_d, w=w_d, taper=t_d)
    for kw in (dict(parts=3), dict(group_off=[0, 3, 2]), dict(group_off=[1, 2, 5]), dict(members=[0, 1, 1, 3, 5]),
               dict(members=[0, 1, 1, 3]), dict(v=v_d[:4]), dict(v=v_d.to(torch.float32)), dict(taper=t_d[:4]), dict(scale=sc_d[:1]),
               dict(sinza=s_d.reshape(1, -1)), dict(w=w_d[:, :2].contiguous()), dict(out=torch.empty((nf, 2, 2, nel, nt), dtype=torch.float64, device=x_d.device)),
               dict(norm=torch.empty((nf, 2), dtype=torch.float64, device=x_d.device)),
               dict(norm2=torch.empty((nf, 2, nt), dtype=torch.float32, device=x_d.device))):
        with pytest.raises(ValueError, match="ringmap"):
            ctx.ringmap(x_d, **dict(base, **kw))
    with pytest.raises(ValueError, match="ringmap"):
        ctx.ringmap(x_d.to(torch.complex64), **base)
    for key, value in dict(w=w_d.cpu(), v=v_d.cpu(), taper=t_d.cpu(), scale=sc_d.cpu(), sinza=s_d.cpu(),
                           out=torch.empty((nf, 2, 1, nel, nt), dtype=torch.float64)).items():
        with pytest.raises(ValueError, match="one GPU"):
            ctx.ringmap(x_d, **dict(base, **{key: value}))


# ---- the routes -----------------------------------------------------------------------------------------------------
NFREQ, NFEED, SPACING = 3, 16, 0.3
# one unpolarised source north of the zenith (latitude 45: theta_zenith = pi / 4), 0.35 rad from it
SOURCE = dict(theta=np.array([np.pi / 4 - 0.35]), phi=np.array([2.0]), flux=np.array([10.0]), nu0=415.0, index=np.array([0.0]))


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    import yaml

    from driftscan_amd import device, manager, timestream

    device.reset_context()
    d = tmp_path_factory.mktemp("ringmap")
    conf = dict(config=dict(beamtransfers=True, kltransform=False, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="UnpolarisedCylinder", num_freq=NFREQ, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=NFEED, feed_spacing=SPACING, tsys=1.0))
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


def _maps(ts, name, nfreq):
    return [_read(os.path.join(ts._fdir(fi), "ringmap_%s.hdf5" % name))[0] for fi in range(nfreq)]


def _peak(m, sinza, phi):
    e, t = np.unravel_index(np.argmax(m), m.shape)
    return int(e), int(t)


def test_route_writes_what_the_device_gives_and_finds_the_source(prod):
    from driftscan_amd import storage, timestream

    pm, d, clean = prod
    tel = pm.telescope
    assert SPACING < 0.5 * tel.wavelengths.min()
    ctx = _ctx()
    root = timestream.ringmap(pm, clean.directory, name="a", parts=2)
    tabs, attrs = _read(root)
    sinza, phi = tabs["sinza"], tabs["phi"]
    nel, nt = sinza.size, phi.size
    groups = timestream.ringmap_groups(tel)
    for key in ("group_off", "members", "v", "u", "pol"):
        assert np.array_equal(tabs[key], groups[key])
    assert np.array_equal(tabs["taper"], timestream.ringmap_taper(tel, groups)) and np.array_equal(sinza, timestream.ringmap_sinza(tel, groups))
    assert attrs["nel"] == nel and attrs["parts"] == 2 and attrs["weighting"] == "natural" and attrs["window"] == "none"
    files = _maps(clean, "a", NFREQ)
    ngroup = len(groups["group_off"]) - 1
    assert all(sorted(f) == ["map", "norm", "norm2"] and f["map"].shape == (ngroup, 2, nel, nt) for f in files)
    # the same data through Context.ringmap, bit for bit, and under the checker against the long-double statement
    vis = np.stack([clean.timestream_f(fi) for fi in range(NFREQ)])
    scale = 1.0 / tel.wavelengths
    got = ctx.ringmap(ctx.to_device(vis), groups["group_off"], groups["members"], groups["v"], scale, sinza, taper=tabs["taper"], parts=2)
    got = [ctx.to_host(g) for g in got]
    for name, g in zip(("map", "norm", "norm2"), got):
        assert np.array_equal(_bits(np.stack([f[name] for f in files])), _bits(g)), name
    c = dict(nf=NFREQ, nt=nt, nel=nel, vis=vis, w=None, group_off=groups["group_off"], members=groups["members"], v=groups["v"],
             taper=tabs["taper"], scale=scale, sinza=sinza)
    bad, worst = rc.check(c, got, rc.reference(c))
    print("route: worst error %.3g of its bound" % worst)
    assert not bad, bad
    # the source: two synthesised beams from the zenith at the least, found within a grid step and a sample
    s0 = np.sin(tel.zenith[0] - SOURCE["theta"][0])
    assert s0 >= 2 * tel.wavelengths.max() / (NFEED * SPACING)
    g0 = int(np.nonzero(groups["u"] == 0)[0][0])
    step, dphi = sinza[1] - sinza[0], 2 * np.pi / nt
    peaks = []
    for fi in range(NFREQ):
        e, t = _peak(files[fi]["map"][g0, 0], sinza, phi)
        print("frequency %d: peak at sinza %.4f (source %.4f, step %.4f), phi %.4f (source %.4f, step %.4f)"
              % (fi, sinza[e], s0, step, phi[t], SOURCE["phi"][0], dphi))
        assert abs(sinza[e] - s0) <= step
        assert abs((phi[t] - SOURCE["phi"][0] + np.pi) % (2 * np.pi) - np.pi) <= dphi
        peaks.append((e, t))
    # a second chunk_gb: one frequency at a time, the same bits; collapse_ew adds map_sum
    timestream.ringmap(pm, clean.directory, name="b", parts=2, chunk_gb=1e-9, collapse_ew=True)
    for fa, fb in zip(files, _maps(clean, "b", NFREQ)):
        assert sorted(fb) == ["map", "map_sum", "norm", "norm2", "norm_sum"]
        assert all(np.array_equal(_bits(fa[k]), _bits(fb[k])) for k in fa)
        want = (fb["norm"][:, None, None, :] * fb["map"]).sum(axis=0) / fb["norm"].sum(axis=0)
        assert fb["map_sum"].shape == (1, 2, nel, nt) and np.allclose(fb["map_sum"][0], want, rtol=1e-12, atol=1e-12 * np.abs(want).max())
    # flags: one baseline dropped all day and one range of samples entirely
    e0, tpk = peaks[0]
    lost = (tpk + nt // 3 + np.arange(5)) % nt
    w = np.ones((NFREQ,) + vis.shape[1:])
    w[:, int(groups["members"][groups["group_off"][g0] + 2])] = 0.0
    w[:, :, lost] = 0.0
    fdir = str(d / "flagged")
    shutil.copytree(clean.directory, fdir)
    flagged = timestream.Timestream(fdir, pm)
    for fi in range(NFREQ):
        data, at = _read(flagged._ffile(fi))
        data["weight"] = w[fi]
        data["timestream"] = np.where(w[fi] > 0, data["timestream"], np.nan)
        with storage.File(flagged._ffile(fi), "w") as f:
            for name, value in data.items():
                f.create_dataset(name, data=np.ascontiguousarray(value))
            for name, value in at.items():
                f.attrs[name] = value
    timestream.ringmap(pm, fdir, name="a", parts=2)
    for fi, fl in enumerate(_maps(flagged, "a", NFREQ)):
        assert not fl["norm"][:, lost].any() and not fl["norm2"][:, lost].any() and not fl["map"][..., lost].any()
        assert np.all(np.isfinite(fl["map"])) and np.all(np.delete(fl["norm"], lost, axis=1) > 0)
        assert np.all(np.delete(fl["norm"][g0], lost) < np.delete(files[fi]["norm"][g0], lost))
        assert _peak(fl["map"][g0, 0], sinza, phi) == peaks[fi]
    with pytest.raises(ValueError, match="parts"):
        timestream.ringmap(pm, clean.directory, parts=3)
    with pytest.raises(ValueError, match="no baseline"):
        timestream.ringmap(pm, clean.directory, ew=[77.0])


def test_unstacked_directories_are_refused(prod, tmp_path):
    from driftscan_amd import timestream

    pm, d, clean = prod
    udir = str(tmp_path / "u")
    timestream.simulate_unstacked(pm, udir, ndays=0, sources=[SOURCE])
    with pytest.raises(ValueError, match="unstacked"):
        timestream.ringmap(pm, udir)


def test_pipeline_key(prod, tmp_path):
    """`ringmaps:` in the pipeline writes the files of the stand-alone call; an unknown key raises."""
    import yaml

    from driftscan_amd import pipeline, timestream

    pm, d, clean = prod
    pdir = str(tmp_path / "p")
    shutil.copytree(clean.directory, pdir, ignore=shutil.ignore_patterns("ringmap_*"))
    entry = dict(name="w", nel=21, weighting="uniform", window="hann", intracyl=False, parts=1)
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=True, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=True, nside=32, ringmaps=[entry]),
                timestreams=[dict(name="p", directory=pdir)])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    pipeline.PipelineManager.from_configfile(str(cfile)).generate()
    timestream.ringmap(pm, clean.directory, **entry)
    ours, theirs = timestream.Timestream(pdir, pm), clean
    ra, rb = _read(os.path.join(pdir, "ringmap_w.hdf5")), _read(os.path.join(clean.directory, "ringmap_w.hdf5"))
    assert sorted(ra[0]) == sorted(rb[0]) and ra[1] == rb[1] and all(np.array_equal(ra[0][k], rb[0][k]) for k in ra[0])
    assert ra[0]["sinza"].size == 21 and np.all(ra[0]["u"] != 0) and ra[0]["taper"].max() <= 1
    for fa, fb in zip(_maps(ours, "w", NFREQ), _maps(theirs, "w", NFREQ)):
        assert sorted(fa) == ["map", "norm", "norm2"] and all(np.array_equal(_bits(fa[k]), _bits(fb[k])) for k in fa)
    conf["config"]["ringmaps"] = [dict(entry, colour="red")]
    cfile.write_text(yaml.dump(conf))
    with pytest.raises(ValueError, match="unknown key"):
        pipeline.PipelineManager.from_configfile(str(cfile))
