"""Formed beams on the device: `Context.formed_beam` against the long-double statement under the
bound of the section on the cases of tests/formedbeam_cases.py, with poison around and inside every output and guards
behind every table; the bits of a source in launches of other shapes; refusals; the ring map as the H = 0 special case;
and the routes `timestream.formed_beam` and the pipeline key `formedbeams`."""
import os
import shutil

import numpy as np
import pytest

import formedbeam_cases as fc
import ringmap_cases as rc

pytestmark = pytest.mark.gpu

_REF = {}
_TABLES = ("uvals", "vvals", "scale", "turn", "sinth", "yc0", "yc1")


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _case(name):
    if name not in _REF:
        c = fc.make(name)
        _REF[name] = (c, fc.reference(c))
    return _REF[name]


def _guarded(ctx, shape):
    """A float64 buffer with one NaN guard plane on each side of the first axis; the inside is NaN too."""
    return ctx.to_device(np.full((shape[0] + 2,) + tuple(shape[1:]), np.nan))


def _table(ctx, a, guard=5):
    """(the table with NaN behind it, its length)"""
    return ctx.to_device(np.concatenate([np.asarray(a, dtype=np.float64), np.full(guard, np.nan)])), len(a)


def _sub(c, fsel=None, gsel=None, ssel=None):
    """The case cut down to the frequencies fsel, the groups gsel and the sources ssel (in that order)."""
    fsel = list(range(c["nf"])) if fsel is None else list(fsel)
    gsel = list(range(len(c["group_off"]) - 1)) if gsel is None else list(gsel)
    ssel = np.arange(c["nsrc"]) if ssel is None else np.asarray(ssel)
    off = c["group_off"]
    pick = np.concatenate([np.arange(off[g], off[g + 1]) for g in gsel]).astype(np.int64)
    out = dict(c, nf=len(fsel), nsrc=len(ssel), vis=np.ascontiguousarray(c["vis"][fsel]),
               w=None if c["w"] is None else np.ascontiguousarray(c["w"][fsel]),
               group_off=np.concatenate([[0], np.cumsum([off[g + 1] - off[g] for g in gsel])]).astype(np.int32),
               taper=None if c["taper"] is None else c["taper"][pick], scale=c["scale"][fsel], env=c["env"][fsel])
    for k in ("members", "u", "v", "iu", "iv"):
        out[k] = c[k][pick]
    for k in ("k0", "half", "turn", "sinth", "yc0", "yc1"):
        out[k] = c[k][ssel]
    return out


def _run(ctx, c, parts=2, norm=True, norm2=True):
    """`Context.formed_beam` on the case into guarded, poisoned buffers, its tables guarded; returns host (beam, D, D2)."""
    ngroup = len(c["group_off"]) - 1
    tabs = {k: _table(ctx, c[k]) for k in _TABLES}
    if c["taper"] is not None:
        tabs["taper"] = _table(ctx, c["taper"])
    bufs = [_guarded(ctx, (c["nf"], ngroup, parts, c["nsrc"])), _guarded(ctx, (c["nf"], ngroup, c["nsrc"])),
            _guarded(ctx, (c["nf"], ngroup, c["nsrc"]))]
    x_d, w_d = ctx.to_device(c["vis"]), None if c["w"] is None else ctx.to_device(c["w"])
    view = {k: t[:n] for k, (t, n) in tabs.items()}
    got = ctx.formed_beam(x_d, c["group_off"], c["members"], c["iu"], c["iv"], view["uvals"], view["vvals"], view["scale"], c["env"],
                          c["k0"], c["half"], view["turn"], view["sinth"], view["yc0"], view["yc1"], w=w_d, taper=view.get("taper"),
                          parts=parts, out=bufs[0][1:-1], norm=bufs[1][1:-1] if norm else False,
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
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_against_the_long_double_statement(name, parts):
    """Every element within the bound of section 4.26, the exact zeros exact, nothing from a sample that is not kept,
    every element written, the guards untouched, duplicates alike; a second call gives the same bits."""
    ctx = _ctx()
    c, ref = _case(name)
    got = _run(ctx, c, parts)
    bad, worst = fc.check(c, got, ref)
    print("%s parts %d: device at %.3g of its bound" % (name, parts, worst))
    assert not bad, bad
    assert all(np.all(np.isfinite(g)) for g in got)
    if c["flagged"] is not None:
        assert all(np.array_equal(_bits(g[..., 5]), _bits(g[..., 6])) and np.array_equal(_bits(g[..., 5]), _bits(g[..., -1])) for g in got)
        assert not got[1][..., c["flagged"]].any() and not got[1][..., 7].any()
    again = _run(ctx, c, parts)
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, again))


def test_without_weights_and_taper():
    """w = None equals w = ones and taper = None equals ones, bit for bit."""
    ctx = _ctx()
    c = fc.make("five", w_none=True, taper_none=True)
    got = _run(ctx, c)
    bad, _ = fc.check(c, got, fc.reference(c))
    assert not bad, bad
    ones = _run(ctx, dict(c, w=np.ones(c["vis"].shape), taper=np.ones(c["u"].shape)))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(got, ones))
    nterms = np.diff(c["group_off"])[:, None] * (2 * c["half"] + 1)[None, :]
    assert np.array_equal(got[1][0], nterms.astype(float)) and np.array_equal(got[2][0], nterms.astype(float))   # env = 0


@pytest.mark.parametrize("name", ("main", "ragged"))
def test_bits_do_not_depend_on_the_launch(name):
    """A source gives the same bits among the others, alone, in a permuted catalogue and in a part of it; a (frequency,
    group) alone; with norm / norm2 null; plane 0 of parts = 2 is the parts = 1 result."""
    ctx = _ctx()
    c, _ = _case(name)
    full = _run(ctx, c)
    rng = np.random.default_rng(3)
    for s in (0, 2, 3, 4, 5, 9, c["nsrc"] - 1):
        one = _run(ctx, _sub(c, ssel=[s]))
        assert all(np.array_equal(_bits(a[..., 0]), _bits(b[..., s])) for a, b in zip(one, full)), s
    perm = rng.permutation(c["nsrc"])
    mixed = _run(ctx, _sub(c, ssel=perm))
    assert all(np.array_equal(_bits(a), _bits(b[..., perm])) for a, b in zip(mixed, full))
    some = np.sort(rng.permutation(c["nsrc"])[: c["nsrc"] // 3])
    part = _run(ctx, _sub(c, ssel=some))
    assert all(np.array_equal(_bits(a), _bits(b[..., some])) for a, b in zip(part, full))
    ngroup = len(c["group_off"]) - 1
    for f in range(c["nf"]):
        for g in range(ngroup):
            one = _run(ctx, _sub(c, fsel=[f], gsel=[g]))
            assert all(np.array_equal(_bits(a[0, 0]), _bits(b[f, g])) for a, b in zip(one, full)), (f, g)
    back = _run(ctx, _sub(c, gsel=list(range(ngroup))[::-1]))
    assert all(np.array_equal(_bits(a), _bits(b[:, ::-1])) for a, b in zip(back, full))
    for norm, norm2 in ((False, True), (True, False), (False, False)):
        part = _run(ctx, c, norm=norm, norm2=norm2)
        assert np.array_equal(_bits(part[0]), _bits(full[0]))
        assert all(p is None or np.array_equal(_bits(p), _bits(q)) for p, q in zip(part[1:], full[1:]))
    p1 = _run(ctx, c, parts=1)
    assert np.array_equal(_bits(p1[0][:, :, 0]), _bits(full[0][:, :, 0]))
    assert np.array_equal(_bits(p1[1]), _bits(full[1])) and np.array_equal(_bits(p1[2]), _bits(full[2]))


def test_refusals_launch_nothing():
    """Every refusal of dm_formed_beam returns nonzero with the context's error set and leaves the poison; zero sizes are
    no-ops; the Python layer refuses what it can see."""
    from ctypes import c_double, c_int

    from driftscan_amd import _lib

    ctx = _ctx()
    lib = ctx.lib
    nf, nrow, nt, nsrc = 2, 5, 9, 3
    x_d, w_d = ctx.to_device(np.ones((nf, nrow, nt), dtype=np.complex128)), ctx.to_device(np.ones((nf, nrow, nt)))
    dev = dict(uvals=ctx.to_device(np.array([0.0, 2.0])), vvals=ctx.to_device(np.arange(3.0)), taper=ctx.to_device(np.ones(5)),
               scale=ctx.to_device(np.ones(nf)), turn=ctx.to_device(np.array([0.1, 0.5, 0.9])), sinth=ctx.to_device(np.full(3, 0.6)),
               yc0=ctx.to_device(np.full(3, 0.5)), yc1=ctx.to_device(np.full(3, 0.4)), vis=x_d, w=w_d)
    good = dict(dev, nf=nf, nrow=nrow, nt=nt, ngroup=2, off=[0, 2, 5], mem=[0, 1, 1, 3, 4], iu=[0, 1, 0, 1, 1], iv=[0, 1, 2, 0, 1],
                nu=2, nv=3, env=[0.0, 1.5], nsrc=nsrc, k0=[1, 4, 8], half=[0, 4, -1], parts=2)

    def ints(v):
        return None if v is None else (c_int * max(len(v), 1))(*v)

    def call(a, op):
        envp = None if a["env"] is None else (c_double * max(len(a["env"]), 1))(*a["env"])
        d = {k: (None if a[k] is None else ctx.ptr(a[k])) for k in dev}
        return lib.dm_formed_beam(ctx.h, a["nf"], a["nrow"], a["nt"], a["ngroup"], ints(a["off"]), ints(a["mem"]), ints(a["iu"]),
                                  ints(a["iv"]), a["nu"], d["uvals"], a["nv"], d["vvals"], d["taper"], d["scale"],
                                  envp, a["nsrc"], ints(a["k0"]), ints(a["half"]),
                                  d["turn"], d["sinth"], d["yc0"], d["yc1"], a["parts"], d["vis"], d["w"], *op)

    bads = [dict(nf=-1), dict(nrow=-1), dict(nt=-1), dict(ngroup=-1), dict(nsrc=-1), dict(nu=-1), dict(nv=-1), dict(parts=0),
            dict(parts=3), dict(half=[0, 5, -1]), dict(half=[0, 4, -2]), dict(k0=[1, 9, 8]), dict(k0=[-1, 4, 8]),
            dict(mem=[0, 1, 1, 3, 5]), dict(mem=[0, -1, 1, 3, 4]), dict(nrow=4), dict(off=[0, 3, 2]), dict(off=[2, 1, 5]),
            dict(off=[-1, 2, 5]), dict(iu=[0, 2, 0, 1, 1]), dict(iv=[0, 1, 3, 0, 1]), dict(iu=[0, -1, 0, 1, 1]), dict(nu=1),
            dict(env=[0.0, -1.0]), dict(env=[np.nan, 1.0]), dict(env=[np.inf, 1.0]), dict(off=None), dict(mem=None), dict(iu=None),
            dict(iv=None), dict(uvals=None), dict(vvals=None), dict(scale=None), dict(env=None), dict(k0=None), dict(half=None),
            dict(turn=None), dict(sinth=None), dict(yc0=None), dict(yc1=None), dict(vis=None), dict(out0=None), dict(out0="vis"),
            dict(out1="w"), dict(out2="turn"), dict(out1="out0"), dict(out2="out1"), dict(out0="uvals")]
    for bad in bads:
        a = dict(good, **{k: v for k, v in bad.items() if not k.startswith("out")})
        bufs = [_guarded(ctx, (nf, 2, 2, nsrc)), _guarded(ctx, (nf, 2, nsrc)), _guarded(ctx, (nf, 2, nsrc))]
        op = [ctx.ptr(b[1:-1]) for b in bufs]
        ptr = {"vis": ctx.ptr(x_d), "w": ctx.ptr(w_d), "turn": ctx.ptr(dev["turn"]), "uvals": ctx.ptr(dev["uvals"]), "out0": op[0],
               "out1": op[1], None: None}
        for i in range(3):
            if "out%d" % i in bad:
                op[i] = ptr[bad["out%d" % i]]
        rcode = call(a, op)
        assert rcode != 0, bad
        with pytest.raises(_lib.DriftMIError, match="dm_formed_beam"):
            ctx.check(rcode, "dm_formed_beam")
        ctx.sync()
        assert all(np.all(np.isnan(ctx.to_host(b))) for b in bufs), bad
    assert np.all(ctx.to_host(x_d) == 1) and np.all(ctx.to_host(w_d) == 1) and np.array_equal(ctx.to_host(dev["turn"]), [0.1, 0.5, 0.9])
    # the good call goes through; zero sizes are no-ops, whatever else is passed
    bufs = [_guarded(ctx, (nf, 2, 2, nsrc)), _guarded(ctx, (nf, 2, nsrc)), _guarded(ctx, (nf, 2, nsrc))]
    assert call(good, [ctx.ptr(b[1:-1]) for b in bufs]) == 0
    ctx.sync()
    assert all(np.all(np.isfinite(ctx.to_host(b)[1:-1])) for b in bufs) and not ctx.to_host(bufs[1])[1:-1][..., 2].any()
    for zero in (dict(nf=0), dict(nt=0), dict(ngroup=0), dict(nsrc=0)):
        a = dict(good, **zero)
        a.update({k: None for k in ("off", "mem", "iu", "iv", "env", "k0", "half") + tuple(dev)})
        bufs = [_guarded(ctx, (nf, 2, 2, nsrc)), _guarded(ctx, (nf, 2, nsrc)), _guarded(ctx, (nf, 2, nsrc))]
        assert call(a, [ctx.ptr(b[1:-1]) for b in bufs]) == 0
        ctx.sync()
        assert all(np.all(np.isnan(ctx.to_host(b))) for b in bufs)
    # groups without members: zeros everywhere
    args = (dev["scale"], [0.0, 1.5], [1, 4, 8], [0, 4, -1], dev["turn"], dev["sinth"], dev["yc0"], dev["yc1"])
    b, d, d2 = ctx.formed_beam(x_d, [0, 0, 0], [], [], [], [], [], *args)
    assert tuple(b.shape) == (nf, 2, 1, nsrc) and not ctx.to_host(b).any() and not ctx.to_host(d).any() and not ctx.to_host(d2).any()
    torch = ctx.torch
    base = dict(group_off=good["off"], members=good["mem"], iu=good["iu"], iv=good["iv"], uvals=dev["uvals"], vvals=dev["vvals"],
                scale=dev["scale"], env=good["env"], k0=good["k0"], half=good["half"], turn=dev["turn"], sinth=dev["sinth"],
                yc0=dev["yc0"], yc1=dev["yc1"], w=w_d, taper=dev["taper"])
    for kw in (dict(parts=3), dict(group_off=[0, 3, 2]), dict(members=[0, 1, 1, 3, 5]), dict(iu=[0, 1, 0, 1]), dict(iu=[0, 2, 0, 1, 1]),
               dict(env=[0.0, -1.0]), dict(env=[0.0]), dict(k0=[1, 4, 9]), dict(half=[0, 5, -1]), dict(half=[0, 4]),
               dict(turn=dev["turn"][:2]), dict(scale=dev["scale"][:1]), dict(taper=dev["taper"][:4]), dict(w=w_d[:, :2].contiguous()),
               dict(out=torch.empty((nf, 2, 2, nsrc), dtype=torch.float64, device=x_d.device)),
               dict(norm=torch.empty((nf, 2), dtype=torch.float64, device=x_d.device))):
        with pytest.raises(ValueError, match="formed_beam"):
            ctx.formed_beam(x_d, **dict(base, **kw))
    with pytest.raises(ValueError, match="one GPU"):
        ctx.formed_beam(x_d, **dict(base, turn=dev["turn"].cpu()))


def test_ring_map_is_the_special_case():
    """H = 0, env = 0, sources exactly on samples: the formed beam of a class pair is `Context.ringmap` on sinza = [y_s] at
    sample k0, combined over the pair's east-west groups with their D, within the sum of the two checkers' bounds."""
    ctx = _ctx()
    rng = np.random.default_rng(17)
    ld = np.longdouble
    nf, nrow, nt, per_u, nsrc = 2, 40, 24, (9, 13, 11), 5
    nb = sum(per_u)
    u = np.repeat([0.0, 2.0, 4.0], per_u)
    v = np.concatenate([(np.arange(n) - n // 3) * 0.31 for n in per_u])
    members = rng.permutation(nrow)[:nb].astype(np.int32)
    taper = rng.uniform(0.5, 2.0, nb)
    vis = rng.standard_normal((nf, nrow, nt)) + 1j * rng.standard_normal((nf, nrow, nt))
    w = rng.uniform(0.5, 2.0, (nf, nrow, nt))
    w[rng.random(w.shape) < 0.2] = 0.0
    vis[~(w > 0)] = np.nan
    scale = np.array([2.1, 10.7])
    theta = fc.THETA_Z + np.array([-0.7, -0.2, 1e-3, 0.3, 0.5])
    k0 = np.array([0, 5, 11, 23, 5], dtype=np.int32)
    tabs = fc.formedbeam_tables(fc.THETA_Z, theta)
    y = tabs["yc0"] - tabs["yc1"]
    uvals, iu = np.unique(u, return_inverse=True)
    vvals, iv = np.unique(v, return_inverse=True)
    c = dict(nf=nf, nrow=nrow, nt=nt, nsrc=nsrc, group_off=np.array([0, nb], dtype=np.int32), members=members, u=u, v=v, uvals=uvals,
             vvals=vvals, iu=iu.astype(np.int32), iv=iv.astype(np.int32), taper=taper, scale=scale, env=np.zeros(nf), k0=k0,
             half=np.zeros(nsrc, dtype=np.int32), turn=k0 / nt, sinth=tabs["sinth"], yc0=tabs["yc0"], yc1=tabs["yc1"], vis=vis, w=w)
    fb = _run(ctx, c)
    fref = fc.reference(c)
    bad, _ = fc.check(c, fb, fref)
    assert not bad, bad
    fbound, _ = fc.bound(c, fref)
    roff = np.concatenate([[0], np.cumsum(per_u)]).astype(np.int32)
    for s in range(nsrc):
        r = dict(nf=nf, nt=nt, nel=1, vis=vis, w=w, group_off=roff, members=members, v=v, taper=taper, scale=scale, sinza=y[s : s + 1])
        m, d, _ = ctx.ringmap(ctx.to_device(vis), roff, members, v, scale, y[s : s + 1], w=ctx.to_device(w), taper=taper, parts=2)
        m, d = ctx.to_host(m)[..., 0, k0[s]].astype(ld), ctx.to_host(d)[..., k0[s]].astype(ld)       # (nf, 3, parts), (nf, 3)
        rbound = rc.bound(r)[0][..., k0[s]]                                                          # (nf, 3)
        dsum = d.sum(axis=1)
        comb = (d[:, :, None] * m).sum(axis=1) / dsum[:, None]
        lim = (d * rbound).sum(axis=1) / dsum + fbound[:, 0, s]
        assert np.all(dsum > 0) and np.all(np.abs(fb[0][:, 0, :, s] - comb) <= lim[:, None]), s
        assert np.all(np.abs(fb[1][:, 0, s] - dsum) <= (nb + 8) * fc.U * dsum)


# ---- the routes -----------------------------------------------------------------------------------------------------
NFREQ, NFEED, SPACING = 3, 16, 0.3
# one unpolarised source north of the zenith (latitude 45: theta_zenith = pi / 4), 0.35 rad from it
SOURCE = dict(theta=np.array([np.pi / 4 - 0.35]), phi=np.array([2.0]), flux=np.array([10.0]), nu0=415.0, index=np.array([0.0]))
HA_MAX = 0.4


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    import yaml

    from driftscan_amd import device, manager, timestream

    device.reset_context()
    d = tmp_path_factory.mktemp("formedbeam")
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


def _catalogue(tel):
    """The source, then: two synthesised east-west beams off in phi, two north-south beams off in theta (towards the
    zenith), the declination mirrored about the zenith."""
    lam = float(tel.wavelengths.max())
    th, ph = float(SOURCE["theta"][0]), float(SOURCE["phi"][0])
    tz = float(tel.zenith[0])
    dphi = 2 * lam / 2.0 / np.sin(th)                   # the east-west baseline is the 2 m between the cylinders
    s0 = np.sin(tz - th)
    th_off = tz - np.arcsin(s0 - 2 * lam / (NFEED * SPACING))
    return np.array([th, th, th_off, 2 * tz - th]), np.array([ph, ph + dphi, ph, ph])


def test_route_writes_what_the_device_gives_and_finds_the_source(prod):
    from driftscan_amd import skysim, storage, timestream

    pm, d, clean = prod
    tel = pm.telescope
    ctx = _ctx()
    theta, phi = _catalogue(tel)
    red = np.array([1420.40575 / 410.0 - 1, 1420.40575 / 415.0 - 1, 1420.40575 / 420.0 - 1, 3.0])
    kw = dict(ha_max=HA_MAX, envelope_fwhm=0.6, parts=2)
    root = timestream.formed_beam(pm, clean.directory, (theta, phi, red), name="a", **kw)
    tabs, attrs = _read(root)
    groups = timestream.formedbeam_groups(tel)
    ngroup, nsrc = len(groups["group_off"]) - 1, theta.size
    assert ngroup == 1 and tabs["beam"].shape == (nsrc, ngroup, NFREQ) and tabs["beam_imag"].shape == (nsrc, ngroup, NFREQ)
    assert attrs["parts"] == 2 and attrs["ha_max"] == HA_MAX and attrs["weighting"] == "natural" and attrs["window"] == "none"
    assert np.array_equal(tabs["theta"], theta) and np.array_equal(tabs["phi"], phi) and np.array_equal(tabs["pol"], groups["pol"])
    assert np.array_equal(tabs["freq"], tel.frequencies)
    with storage.File(clean._ffile(0), "r") as f:
        nt = int(f["timestream"].shape[1])
    win = timestream.formedbeam_windows(tel, theta, phi, nt, HA_MAX)
    assert np.array_equal(tabs["k0"], win["k0"]) and np.array_equal(tabs["half"], win["half"]) and win["half"].min() >= 2
    files = [_read(os.path.join(clean._fdir(fi), "formedbeam_a.hdf5"))[0] for fi in range(NFREQ)]
    assert all(sorted(f) == ["beam", "norm", "norm2"] and f["beam"].shape == (ngroup, 2, nsrc) for f in files)
    # the same data through Context.formed_beam, bit for bit, and under the checker against the long-double statement
    vis = np.stack([clean.timestream_f(fi) for fi in range(NFREQ)])
    stabs = timestream.formedbeam_tables(tel.zenith[0], theta)
    taper = timestream.ringmap_taper(tel, groups)
    scale, env = 1.0 / tel.wavelengths, timestream.formedbeam_env(tel.wavelengths, 0.6)
    c = dict(groups, nf=NFREQ, nrow=vis.shape[1], nt=nt, nsrc=nsrc, taper=taper, scale=scale, env=env, k0=win["k0"], half=win["half"],
             turn=win["turn"], sinth=stabs["sinth"], yc0=stabs["yc0"], yc1=stabs["yc1"], vis=vis, w=None)

    def direct(c, parts=2):
        got = ctx.formed_beam(ctx.to_device(c["vis"]), c["group_off"], c["members"], c["iu"], c["iv"], c["uvals"], c["vvals"],
                              c["scale"], c["env"], c["k0"], c["half"], c["turn"], c["sinth"], c["yc0"], c["yc1"], taper=c["taper"],
                              parts=parts)
        return [ctx.to_host(g) for g in got]

    got = direct(c)
    for name, g in zip(("beam", "norm", "norm2"), got):
        assert np.array_equal(_bits(np.stack([f[name] for f in files])), _bits(g)), name
    assert np.array_equal(_bits(tabs["beam"]), _bits(np.moveaxis(got[0][:, :, 0], 0, -1).transpose(1, 0, 2)))
    assert np.array_equal(_bits(tabs["beam_imag"]), _bits(np.moveaxis(got[0][:, :, 1], 0, -1).transpose(1, 0, 2)))
    assert np.array_equal(_bits(tabs["norm"]), _bits(np.moveaxis(got[1], 0, -1).transpose(1, 0, 2)))
    bad, worst = fc.check(c, got, fc.reference(c))
    print("route: device at %.3g of its bound" % worst)
    assert not bad, bad
    # the source: positive and the largest of the catalogue at every frequency
    beam = tabs["beam"][:, 0, :]
    print("beams (source, frequency):\n%s" % beam)
    assert np.all(beam[0] > 0) and np.all(beam[0] > 2 * np.abs(beam[1:]).max(axis=0))
    # the sign of the east-west phase: with the inter-cylinder baselines only, the hour angle mirrored (u -> -u) loses
    one = dict(c, nsrc=1, **{k: c[k][:1] for k in ("k0", "half", "turn", "sinth", "yc0", "yc1")})
    ew = timestream.formedbeam_groups(tel, intracyl=False)
    one.update(ew, taper=timestream.ringmap_taper(tel, ew))
    right = direct(one, 1)[0][:, 0, 0, 0]
    wrong = direct(dict(one, uvals=-ew["uvals"]), 1)[0][:, 0, 0, 0]
    print("inter-cylinder beams on the source: %s, hour angle mirrored: %s" % (right, wrong))
    assert np.all(right > 0) and np.all(right > 2 * np.abs(wrong))
    # a second chunk_gb: one frequency at a time, the same bits
    root_b = timestream.formed_beam(pm, clean.directory, (theta, phi, red), name="b", chunk_gb=1e-9, **kw)
    tb, ab = _read(root_b)
    assert ab == attrs and sorted(tb) == sorted(tabs) and all(np.array_equal(tabs[k], tb[k], equal_nan=True) for k in tabs)
    assert all(np.array_equal(_bits(tabs[k]), _bits(tb[k])) for k in ("beam", "beam_imag", "norm", "norm2"))
    # the stack of the file's beam
    st = skysim.stack_spectra(tabs["beam"], tabs["freq"], skysim.LINE_21CM_MHZ / (1 + red), 2, source_weight=tabs["norm"].mean(axis=(1, 2)))
    assert np.array_equal(tabs["redshift"], red)
    for key, want in (("stack", st["stack"]), ("hits", st["hits"]), ("offsets", st["offsets"]), ("stack_weight", st["weight"]),
                      ("channel", st["channel"])):
        assert np.array_equal(tabs[key], want), key
    assert tabs["channel"].tolist()[3] == -1 and tabs["hits"].max() >= 1
    # flags: one baseline dropped all day and a range of samples inside the source's window
    w = np.ones(vis.shape)
    w[:, int(groups["members"][5])] = 0.0
    lost = (win["k0"][0] + 1 + np.arange(2)) % nt
    w[:, :, lost] = 0.0
    fdir = str(d / "flagged")
    shutil.copytree(clean.directory, fdir, ignore=shutil.ignore_patterns("formedbeam_*"))
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
    tf, _ = _read(timestream.formed_beam(pm, fdir, (theta, phi), name="a", **kw))
    assert "stack" not in tf and all(np.all(np.isfinite(tf[k])) for k in ("beam", "beam_imag", "norm", "norm2"))
    assert np.all(tf["norm"][0] < tabs["norm"][0]) and np.all(tf["norm"] <= tabs["norm"]) and np.all(tf["norm"][0] > 0)
    bf = tf["beam"][:, 0, :]
    assert np.all(bf[0] > 0) and np.all(bf[0] > 2 * np.abs(bf[1:]).max(axis=0))
    with pytest.raises(ValueError, match="parts"):
        timestream.formed_beam(pm, clean.directory, (theta, phi), parts=3)
    with pytest.raises(ValueError, match="no baseline"):
        timestream.formed_beam(pm, clean.directory, (theta, phi), ew=[77.0])
    with pytest.raises(ValueError, match="unknown stack key"):
        timestream.formed_beam(pm, clean.directory, (theta, phi, red), stack=dict(width=3))
    with pytest.raises(ValueError, match="redshifts"):
        timestream.formed_beam(pm, clean.directory, (theta, phi), stack=dict(halfwidth=1))


def test_unstacked_directories_are_refused(prod, tmp_path):
    from driftscan_amd import timestream

    pm, d, clean = prod
    udir = str(tmp_path / "u")
    timestream.simulate_unstacked(pm, udir, ndays=0, sources=[SOURCE])
    with pytest.raises(ValueError, match="unstacked"):
        timestream.formed_beam(pm, udir, _catalogue(pm.telescope))


def test_pipeline_key(prod, tmp_path):
    """`formedbeams:` in the pipeline writes the files of the stand-alone call; an unknown key raises."""
    import yaml

    from driftscan_amd import pipeline, storage, timestream

    pm, d, clean = prod
    theta, phi = _catalogue(pm.telescope)
    cat = str(tmp_path / "cat.hdf5")
    with storage.File(cat, "w") as f:
        f.create_dataset("theta", data=theta)
        f.create_dataset("phi", data=phi)
        f.create_dataset("redshift", data=np.full(theta.size, 1420.40575 / 415.0 - 1))
    pdir = str(tmp_path / "p")
    shutil.copytree(clean.directory, pdir, ignore=shutil.ignore_patterns("formedbeam_*", "ringmap_*"))
    entry = dict(name="w", catalogue=cat, ha_max=0.3, envelope_fwhm=0.8, weighting="uniform", window="hann", intracyl=False, parts=1,
                 stack=dict(halfwidth=1))
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=True, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=True, nside=32, formedbeams=[entry]),
                timestreams=[dict(name="p", directory=pdir)])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    pipeline.PipelineManager.from_configfile(str(cfile)).generate()
    mine = dict(entry)
    timestream.formed_beam(pm, clean.directory, mine.pop("catalogue"), **mine)
    ra, rb = _read(os.path.join(pdir, "formedbeam_w.hdf5")), _read(os.path.join(clean.directory, "formedbeam_w.hdf5"))
    assert sorted(ra[0]) == sorted(rb[0]) and ra[1] == rb[1] and all(np.array_equal(ra[0][k], rb[0][k]) for k in ra[0])
    assert "beam_imag" not in ra[0] and ra[0]["stack"].shape == (1, 3) and ra[1]["intracyl"] == 0 and ra[1]["envelope_fwhm"] == 0.8
    ours = timestream.Timestream(pdir, pm)
    for fi in range(NFREQ):
        fa = _read(os.path.join(ours._fdir(fi), "formedbeam_w.hdf5"))[0]
        fb = _read(os.path.join(clean._fdir(fi), "formedbeam_w.hdf5"))[0]
        assert sorted(fa) == ["beam", "norm", "norm2"] and all(np.array_equal(_bits(fa[k]), _bits(fb[k])) for k in fa)
    for bad in (dict(entry, colour="red"), {k: v for k, v in entry.items() if k != "catalogue"}):
        conf["config"]["formedbeams"] = [bad]
        cfile.write_text(yaml.dump(conf))
        with pytest.raises(ValueError, match="formedbeams"):
            pipeline.PipelineManager.from_configfile(str(cfile))
