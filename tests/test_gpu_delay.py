"""The delay fit along frequency on the device: `Context.delay_fit` against the long-double
statement under the bound of the section on the cases of tests/delay_cases.py, with the exact parts bit for bit, poison
around every output and guards behind the tables; the bits of a series in launches of other shapes; refusals; and the
routes `delay_filter` -> m-modes, `stack_baselines(delay=)`, `sidereal_stack(delay=)` and the pipeline key."""
import os
import shutil

import numpy as np
import pytest

import delay_cases as dc

pytestmark = pytest.mark.gpu

_REF = {}


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _case(name):
    if name not in _REF:
        c = dc.make(name)
        _REF[name] = (c, dc.reference(c))
    return _REF[name]


def _shapes(nf, nrow, nt):
    return (((nf, nrow, nt), np.complex128), ((nf, nrow, nt), np.float64), ((nrow, nt), np.int32))


def _guarded(ctx, shapes):
    """Buffers with one NaN (int32: -77) guard plane on each side of the first axis; the inside is poisoned too."""
    return [ctx.to_device(np.full((s[0] + 2,) + tuple(s[1:]), -77 if dt is np.int32 else np.nan, dtype=dt)) for s, dt in shapes]


def _poisoned(ctx, bufs, inside=False):
    for b in bufs:
        h = ctx.to_host(b)
        h = h if inside else np.stack([h[0], h[-1]])
        if not (np.all(h == -77) if h.dtype == np.int32 else np.all(np.isnan(h.real) if np.iscomplexobj(h) else np.isnan(h))):
            return False
    return True


def _table(ctx, bases, guard=7):
    """The packed table on the device with NaN behind it, and basis_of with -77 behind it."""
    flat = np.concatenate([a.T.reshape(-1) for a in bases] + [np.full(guard, np.nan)])
    return ctx.to_device(flat)


def _run(ctx, c, mode, ridge=0.0, min_valid=None, rows=None, tsel=None, bases=None, basis_of=None, inplace=False):
    """`Context.delay_fit` on the rows `rows` and the samples `tsel` of the case, into guarded buffers (or in place);
    the guards of the outputs and behind the tables are checked.  Returns host arrays (x_out, w_out, info)."""
    rows = np.arange(c["nrow"]) if rows is None else np.asarray(rows)
    tsel = slice(None) if tsel is None else tsel
    x = np.ascontiguousarray(c["x"][:, rows][:, :, tsel])
    w = None if c["w"] is None else np.ascontiguousarray(c["w"][:, rows][:, :, tsel])
    bases = c["bases"] if bases is None else bases
    of = (c["basis_of"] if basis_of is None else np.asarray(basis_of, dtype=np.int32))[rows]
    nf, nrow, nt = x.shape
    tab = _table(ctx, bases)
    ntab = nf * sum(a.shape[1] for a in bases)
    of_d = ctx.to_device(np.concatenate([of, np.full(5, -77, dtype=np.int32)]))
    x_d, w_d = ctx.to_device(x), None if w is None else ctx.to_device(w)
    bufs = _guarded(ctx, _shapes(nf, nrow, nt))
    out = [b[1:-1] for b in bufs]
    if inplace:
        out[0] = x_d
        if w_d is not None:
            out[1] = w_d
    ranks = [int(a.shape[1]) for a in bases]
    got = ctx.delay_fit(x_d, w=w_d, basis=(tab[:ntab], ranks), basis_of=of_d[:nrow], mode=mode, ridge=ridge,
                        min_valid=min_valid, out=tuple(out))
    assert all(g.data_ptr() == t.data_ptr() for g, t in zip(got, out))
    ctx.sync()
    assert _poisoned(ctx, bufs if not inplace else bufs[2:])
    assert np.all(np.isnan(ctx.to_host(tab)[ntab:])) and np.all(ctx.to_host(of_d)[nrow:] == -77)
    return [ctx.to_host(t) for t in out]


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype != np.int32 else np.int32)


def _same(a, b):
    return all(np.array_equal(_bits(u), _bits(v)) for u, v in zip(a, b))


def test_limits_and_tiles():
    """The exported limits, and `dm_delay_tile`: a tile for every (nf, rank) within them whose nt of the cases is no
    multiple (or the tile is one series), none outside."""
    lib = _ctx().lib
    nfmax, rmax = lib.dm_delay_max_nf(), lib.dm_delay_max_rank()
    assert nfmax >= 1024 and rmax >= 64
    for nf in (1, 2, 7, 64, 65, 256, nfmax):
        for r in (1, 2, 17, 32, rmax):
            assert 1 <= lib.dm_delay_tile(nf, r) <= 8
    assert [lib.dm_delay_tile(*a) for a in ((0, 1), (nfmax + 1, 1), (64, 0), (64, rmax + 1), (-1, -1))] == [0] * 5
    assert lib.dm_delay_tile(64, 8) > 1 and lib.dm_delay_tile(nfmax, rmax) >= 1
    for name, (nf, nt, table, _) in dc.CASES.items():
        tj = lib.dm_delay_tile(nf or nfmax, max(r for _, r in table))
        assert tj == 1 or nt % tj != 0 or nt == 1, name


@pytest.mark.parametrize("mode", dc.MODES)
@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_against_the_long_double_statement(name, mode):
    """info is equal, the exact parts are bit for bit (kept samples of inpaint are x, kept weights are w, flagged samples
    of filter are 0, series that are not solved), every model value and fill weight is within the bound of section 4.23;
    NaN and Inf under the flags reach nothing; the guards stay; a second call gives the same bits."""
    ctx = _ctx()
    c, ref = _case(name)
    out = _run(ctx, c, mode)
    bad, worst = dc.check(c, ref, mode, *out)
    print("%s %s: worst error %.3g of its bound" % (name, mode, worst))
    assert not bad, bad
    assert np.all(np.isfinite(out[0].real)) and np.all(np.isfinite(out[0].imag)) and np.all(np.isfinite(out[1]))
    assert _same(out, _run(ctx, c, mode))
    if mode == "inpaint":
        kept = ref["kept"]
        assert np.array_equal(_bits(out[0][kept]), _bits(c["x"][kept])) and np.array_equal(_bits(out[1][kept]), _bits(c["w"][kept]))


@pytest.mark.parametrize("mode", dc.MODES)
def test_without_weights_and_none_flagged(mode):
    """w = None equals w = ones bit for bit and keeps every sample; weights without a flag."""
    ctx = _ctx()
    c = dc.make("nf 65", w_none=True)
    ref = dc.reference(c)
    out = _run(ctx, c, mode)
    bad, _ = dc.check(c, ref, mode, *out)
    assert not bad, bad
    ones = dict(c, w=np.ones(c["x"].shape))
    assert _same(out, _run(ctx, ones, mode))
    assert not out[2].any() and np.all(out[1] == 1)
    c = dc.make("nf 64", none_flagged=True)
    bad, _ = dc.check(c, dc.reference(c), mode, *_run(ctx, c, mode))
    assert not bad, bad


def test_rank_deficient_and_ridge():
    """The basis with one vector twice: info = 3 with ridge = 0 (the pivot is exactly 0), solved with a ridge; a ridge
    on a regular case; min_valid."""
    ctx = _ctx()
    c = dc.deficient()
    for mode in dc.MODES:
        out = _run(ctx, c, mode)
        bad, _ = dc.check(c, dc.reference(c), mode, *out)
        assert not bad, bad
        assert np.all(out[2][[0, 2]] == 3) and not out[2][1].any()
        ref = dc.reference(c, ridge=0.5)
        out = _run(ctx, c, mode, ridge=0.5)
        assert not out[2].any()
        bad, _ = dc.check(c, ref, mode, *out)
        assert not bad, bad
    c, _ = _case("nf 64")
    ref = dc.reference(c, ridge=1e-3, min_valid=40)
    assert (ref["info"] == -1).sum() > (_case("nf 64")[1]["info"] == -1).sum()
    bad, _ = dc.check(c, ref, "inpaint", *_run(ctx, c, "inpaint", ridge=1e-3, min_valid=40))
    assert not bad, bad


def test_wide_gap_scaled_bound():
    ctx = _ctx()
    c = dc.wide_gap()
    ref = dc.reference(c)
    for mode in dc.MODES:
        bad, worst = dc.check(c, ref, mode, *_run(ctx, c, mode))
        print("wide gap %s: worst error %.3g of its bound" % (mode, worst))
        assert not bad, bad


@pytest.mark.parametrize("name", ("nf 64", "nf 7", "nf 256"))
def test_bits_do_not_depend_on_the_launch(name):
    """A (row, t) gives the same bits in the full launch, in a launch of its row alone, in a launch whose t-window starts
    elsewhere, with the rows permuted, with an unused basis of the largest rank added to the table (another tile and
    another kernel instance), and in place."""
    ctx = _ctx()
    c, _ = _case(name)
    nrow, nt = c["nrow"], c["nt"]
    for mode in dc.MODES:
        full = _run(ctx, c, mode)
        for row in range(nrow):
            one = _run(ctx, c, mode, rows=[row])
            assert _same(one, [full[0][:, [row]], full[1][:, [row]], full[2][[row]]]), (mode, row)
        t0 = min(3, nt - 1)
        win = _run(ctx, c, mode, tsel=slice(t0, nt))
        assert _same(win, [full[0][:, :, t0:], full[1][:, :, t0:], full[2][:, t0:]]), mode
        perm = np.roll(np.arange(nrow), 1)[::-1].copy()
        pr = _run(ctx, c, mode, rows=perm)
        assert _same(pr, [full[0][:, perm], full[1][:, perm], full[2][perm]]), mode
        rng = np.random.default_rng(2)
        extra = c["bases"] + [dc.random_basis(rng, c["nf"], min(c["nf"], dc.limits()[1]))]
        assert _same(_run(ctx, c, mode, bases=extra), full), mode
        front = [extra[-1]] + c["bases"]
        assert _same(_run(ctx, c, mode, bases=front, basis_of=c["basis_of"] + 1), full), mode
        assert _same(_run(ctx, c, mode, inplace=True)[:2], full[:2]), mode


def test_bad_class_entries_give_minus_two():
    """A basis_of entry outside [0, nbasis) gives info = -2 for the series of its row, which are handled as not solved;
    the other rows keep their bits."""
    ctx = _ctx()
    c, _ = _case("nf 64")
    for mode in dc.MODES:
        full = _run(ctx, c, mode)
        of = c["basis_of"].copy()
        of[1], of[3] = len(c["bases"]), -1
        out = _run(ctx, c, mode, basis_of=of)
        assert np.all(out[2][[1, 3]] == -2)
        keep = [0, 2, 4]
        assert _same([o[:, keep] for o in out[:2]] + [out[2][keep]], [o[:, keep] for o in full[:2]] + [full[2][keep]])
        kept = c["w"] > 0
        for row in (1, 3):
            want = np.where(kept[:, row], c["x"][:, row], 0) if mode != "model" else np.zeros_like(c["x"][:, row])
            assert np.array_equal(_bits(out[0][:, row]), _bits(want))
            assert np.array_equal(_bits(out[1][:, row]), _bits(np.where(kept[:, row], c["w"][:, row], 0.0)))


def test_refusals_launch_nothing():
    """Every refusal of dm_delay_fit returns nonzero with the context's error set and leaves the poison; zero sizes are
    no-ops; the Python layer refuses what it can see."""
    from ctypes import c_int

    from driftscan_amd import _lib

    ctx = _ctx()
    lib = ctx.lib
    nf, nrow, nt = 6, 3, 9
    nfmax, rmax = lib.dm_delay_max_nf(), lib.dm_delay_max_rank()
    x_d, w_d = ctx.to_device(np.ones((nf, nrow, nt), dtype=np.complex128)), ctx.to_device(np.ones((nf, nrow, nt)))
    tab = ctx.to_device(np.ones(nf * 3))
    of_d = ctx.to_device(np.zeros(nrow, dtype=np.int32))
    big_x = ctx.to_device(np.ones((nfmax + 1, 1, 1), dtype=np.complex128))
    big_tab = ctx.to_device(np.ones((rmax + 1) * (rmax + 2)))
    good = dict(nf=nf, nrow=nrow, nt=nt, mode=2, ridge=0.0, min_valid=0, ranks=[2, 1], tab=tab, of=of_d, x=x_d, w=w_d)
    bads = [dict(nf=-1), dict(nrow=-1), dict(nt=-1), dict(mode=3), dict(mode=-1), dict(ridge=-1e-3), dict(ridge=np.nan),
            dict(ridge=np.inf), dict(ranks=[]), dict(ranks=[0, 1]), dict(ranks=[nf + 1]), dict(ranks=[2, -1]),
            dict(ranks=None), dict(tab=None), dict(of=None), dict(x=None), dict(out0=None), dict(out1=None), dict(out2=None),
            dict(out0="w"), dict(out1="x"), dict(out2="x"), dict(out2="w"), dict(out0="tab"), dict(out2="of"),
            dict(out1="out0"), dict(out2="out1"), dict(ranks=[1] * 257),
            dict(nf=nfmax + 1, nrow=1, nt=1, x=big_x, w=None, ranks=[1]),
            dict(nf=rmax + 2, nrow=1, nt=1, x=big_x, w=None, ranks=[rmax + 1], tab=big_tab)]
    for bad in bads:
        a = dict(good, **bad)
        bufs = _guarded(ctx, _shapes(nf, nrow, nt))
        op = [ctx.ptr(b[1:-1]) for b in bufs]
        ptr = {"x": ctx.ptr(x_d), "w": ctx.ptr(w_d), "tab": ctx.ptr(tab), "of": ctx.ptr(of_d), "out0": op[0], "out1": op[1], None: None}
        for i in range(3):
            if "out%d" % i in bad:
                op[i] = ptr[bad["out%d" % i]]
        ranks = a["ranks"]
        rk = None if ranks is None else (c_int * max(len(ranks), 1))(*ranks)
        rcode = lib.dm_delay_fit(ctx.h, a["nf"], a["nrow"], a["nt"], a["mode"], a["ridge"], a["min_valid"],
                                 0 if ranks is None else len(ranks), rk, *(None if a[k] is None else ctx.ptr(a[k])
                                                                           for k in ("tab", "of", "x", "w")), *op)
        if ranks is None:
            rcode = lib.dm_delay_fit(ctx.h, a["nf"], a["nrow"], a["nt"], a["mode"], a["ridge"], a["min_valid"], 1, None,
                                     ctx.ptr(tab), ctx.ptr(of_d), ctx.ptr(x_d), ctx.ptr(w_d), *op)
        assert rcode != 0, bad
        with pytest.raises(_lib.DriftMIError, match="dm_delay_fit"):
            ctx.check(rcode, "dm_delay_fit")
        ctx.sync()
        assert _poisoned(ctx, bufs, inside=True), bad
    assert np.all(ctx.to_host(x_d) == 1) and np.all(ctx.to_host(w_d) == 1)
    # zero sizes are no-ops, whatever else is passed
    for zero in (dict(nf=0), dict(nrow=0), dict(nt=0)):
        a = dict(good, **zero)
        bufs = _guarded(ctx, _shapes(nf, nrow, nt))
        rcode = lib.dm_delay_fit(ctx.h, a["nf"], a["nrow"], a["nt"], 2, 0.0, 0, 0, None, None, None, None, None,
                                 *(ctx.ptr(b[1:-1]) for b in bufs))
        assert rcode == 0
        ctx.sync()
        assert _poisoned(ctx, bufs, inside=True)
    empty = ctx.delay_fit(x_d[:, :, :0].contiguous(), basis=[np.ones((nf, 1))], basis_of=[0, 0, 0])
    assert tuple(empty[2].shape) == (nrow, 0)
    basis = [np.ones((nf, 1))]
    for kw in (dict(mode="fill"), dict(basis=None), dict(basis_of=None), dict(basis=[np.ones((nf + 1, 1))]),
               dict(basis_of=[0, 0]), dict(w=w_d[:, :2].contiguous()), dict(out=(x_d, w_d)),
               dict(out=(x_d, w_d, ctx.to_device(np.zeros((nrow, nt))))), dict(ridge=-1.0)):
        with pytest.raises((ValueError, _lib.DriftMIError)):
            ctx.delay_fit(x_d, **dict(dict(w=w_d, basis=basis, basis_of=[0, 0, 0]), **kw))
    with pytest.raises(ValueError):
        ctx.delay_fit(x_d.to(ctx.torch.complex64), basis=basis, basis_of=[0, 0, 0])
    # a tensor that is not on x's device never reaches the kernel
    cpu = dict(w=w_d.cpu(), basis_of=of_d.cpu(), basis=(tab[: nf].cpu(), [1]),
               out=(x_d.cpu(), w_d.cpu(), ctx.torch.empty((nrow, nt), dtype=ctx.torch.int32)))
    for key, value in cpu.items():
        with pytest.raises(ValueError, match="one GPU"):
            ctx.delay_fit(x_d, **dict(dict(w=w_d, basis=(tab[: nf], [1]), basis_of=of_d), **{key: value}))


# ---- the routes -----------------------------------------------------------------------------------------------------
NFREQ, CHAN = 12, 4
DELAY = dict(mode="inpaint", buffer=0.5, eigencut=1e-6, nclass=3)


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("delay")
    conf = dict(config=dict(beamtransfers=True, kltransform=False, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="UnpolarisedCylinder", num_freq=NFREQ, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0))
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    return pm, d


CATALOGUE = dict(theta=np.array([0.7, 1.1, 1.4, 0.9]), phi=np.array([0.3, 2.0, 4.1, 5.5]), flux=np.array([5.0, 3.0, 8.0, 2.0]),
                 nu0=415.0, index=np.array([-0.7, -0.5, -0.9, -0.6]))


def _read_all(ts, nfreq):
    from driftscan_amd import storage

    out = []
    for fi in range(nfreq):
        with storage.File(ts._ffile(fi), "r") as f:
            out.append(({k: np.asarray(f[k][:]) for k in f.keys()}, dict(f.attrs)))
    return out


def _flag_copy(src, dst_dir, pm, w, x=None):
    """A copy of the directory of `src` with the weights w (nfreq, nrow, nt) and the flagged samples at 0."""
    from driftscan_amd import storage, timestream

    shutil.copytree(src.directory, dst_dir)
    dst = timestream.Timestream(dst_dir, pm)
    for fi, (data, attrs) in enumerate(_read_all(src, w.shape[0])):
        data["weight"] = w[fi]
        data["timestream"] = np.where(w[fi] > 0, data["timestream"] if x is None else x[fi], 0.0)
        with storage.File(dst._ffile(fi), "w") as f:
            for name, value in data.items():
                f.create_dataset(name, data=np.ascontiguousarray(value))
            for name, value in attrs.items():
                f.attrs[name] = value
    return dst


def _same_files(a, b, nfreq):
    for (da, aa), (db, ab) in zip(_read_all(a, nfreq), _read_all(b, nfreq)):
        assert sorted(da) == sorted(db) and sorted(aa) == sorted(ab)
        for name in da:
            assert da[name].dtype == db[name].dtype and np.array_equal(_bits(da[name]) if da[name].dtype.kind in "fc" else da[name],
                                                                       _bits(db[name]) if db[name].dtype.kind in "fc" else db[name]), name
    from driftscan_amd import storage

    with storage.File(os.path.join(a.directory, "delay_fit.hdf5"), "r") as f, \
            storage.File(os.path.join(b.directory, "delay_fit.hdf5"), "r") as g:
        assert sorted(f.keys()) == sorted(g.keys()) == ["basis_of", "info", "rank", "tau"]
        for name in f.keys():
            assert np.array_equal(f[name][:], g[name][:]), name
        assert dict(f.attrs) == dict(g.attrs)


def test_channel_lost_all_day_is_filled_before_the_m_modes(prod):
    """A noise-free simulation of a point-source catalogue; one channel taken out for the whole day on every row plus 3 %
    random flags.  Without the step that channel's rows have info = -1 in mmodes/weights.hdf5 and modes that are exactly
    zero; after `delay_filter(mode="inpaint")` every row has info = 0, and the modes of the filled channel are those of
    the complete simulation within the error of the long-double host statement on the same data (put through the same
    m-mode route) plus the device bound carried through the weighted estimate, plus the 1e-10 of the largest mode to
    which tests/test_gpu_flags.py holds the weighted m-mode routes (the rounding of the transform itself).  The carry
    (DESIGN.md section 4.23): the estimate of a row is a = (F^H W F)^-1 F^H W x with F^H F = ntime I, so an error dx of
    the samples moves it by |da| <= |dx| sqrt(w_max) / sigma_min(W^1/2 F) <= sqrt(w_max / w_min) |dx| / sqrt(ntime), and
    |a| = |x| / sqrt(ntime) for the band-limited x of the complete simulation: relative to the modes, sqrt(w_max / w_min)
    times the error relative to the samples."""
    from driftscan_amd import storage, timestream

    pm, d = prod
    tel = pm.telescope
    nfreq, nrow, mmax = int(tel.nfreq), int(tel.npairs), int(tel.mmax)
    assert nfreq == NFREQ >= 8
    nt = int(np.ceil(2.5 * (2 * mmax + 1)))   # oversampled: the weighted m-mode estimate has samples to spare
    clean = timestream.simulate(pm, str(d / "clean"), ndays=0, resolution=86400.0 / nt, sources=[CATALOGUE])
    assert clean.ntime == nt
    xc = np.stack([clean.timestream_f(fi) for fi in range(nfreq)])
    rng = np.random.default_rng(8)
    w = np.where(rng.random(xc.shape) < 0.03, 0.0, 1.0)
    w[CHAN] = 0.0
    holes = _flag_copy(clean, str(d / "holes"), pm, w)
    before = _flag_copy(clean, str(d / "before"), pm, w)
    before.generate_mmodes()
    with storage.File(before.output_directory + "/mmodes/weights.hdf5", "r") as f:
        info = f["info"][:]
    assert np.all(info[CHAN] == -1) and not np.delete(info, CHAN, axis=0).any()
    assert all(not before.mmode(mi)[CHAN].any() for mi in range(mmax + 1))
    filled = timestream.delay_filter(pm, holes.directory, str(d / "filled"), **DELAY)
    with storage.File(os.path.join(filled.directory, "delay_fit.hdf5"), "r") as f:
        assert not f["info"][:].any() and f["info"].shape == (nrow, nt)
        basis_of, ranks = f["basis_of"][:], f["rank"][:]
    files = _read_all(filled, nfreq)
    xf, wf = np.stack([da["timestream"] for da, _ in files]), np.stack([da["weight"] for da, _ in files])
    assert np.array_equal(_bits(xf[w > 0]), _bits(xc[w > 0])) and np.all(wf[w > 0] == 1) and np.all(wf > 0)
    assert np.array_equal(np.stack([da["weight_input"] for da, _ in files]), w)
    assert np.array_equal(np.stack([da["delay_filled"] for da, _ in files]), (w == 0).sum(axis=2))
    # the long-double statement on the same data, and the device against it
    table, rk, of, _ = timestream.delay_classes(tel, **{k: DELAY[k] for k in ("buffer", "eigencut", "nclass")})
    assert np.array_equal(of, basis_of) and np.array_equal(rk, ranks) and ranks.max() < nfreq - 1
    bases, off = [], 0
    for r in rk:
        bases.append(np.ascontiguousarray(table[off : off + nfreq * r].reshape(r, nfreq).T))
        off += nfreq * r
    c = dict(nf=nfreq, nrow=nrow, nt=nt, bases=bases, ranks=[int(r) for r in rk], basis_of=of, x=np.where(w > 0, xc, 0.0), w=w)
    ref = dc.reference(c)
    bad, worst = dc.check(c, ref, "inpaint", xf, wf, np.zeros((nrow, nt), dtype=np.int32))
    assert not bad, bad
    xh, wh = dc.expected(c, ref, "inpaint")
    host = _flag_copy(clean, str(d / "hostfilled"), pm, wh.astype(np.float64), x=xh.astype(np.complex128))
    tol = (dc.C1 * nfreq + dc.C2 * np.array(c["ranks"])[of] ** 2.0)[None, :, None] * dc.U * ref["kappa"][None] \
        * ref["anorm"][:, :, None] * ref["cnorm"][None]
    fill_err = np.abs(xh[CHAN] - xc[CHAN]).astype(np.float64)
    print("kappa_2(G) up to %.3g; fill of the lost channel off by %.3g of its largest sample (long double), device within "
          "%.3g of its bound" % (ref["kappa"].max(), fill_err.max() / np.abs(xc[CHAN]).max(), worst))
    filled.generate_mmodes()
    host.generate_mmodes()
    clean.generate_mmodes()
    with storage.File(filled.output_directory + "/mmodes/weights.hdf5", "r") as f:
        assert f["info"][:].shape == (nfreq, nrow) and not f["info"][:].any()
    vd, vh, vc = (np.stack([t.mmode(mi)[CHAN] for mi in range(mmax + 1)]) for t in (filled, host, clean))
    nrm = np.linalg.norm(vc)
    rel_dev, rel_host = np.linalg.norm(vd - vc) / nrm, np.linalg.norm(vh - vc) / nrm
    carried = np.sqrt(wf[CHAN].max() / wf[CHAN].min()) * np.linalg.norm(tol[CHAN]) / np.linalg.norm(xc[CHAN])
    print("modes of the filled channel against the complete simulation: device %.3g, long-double fill %.3g, carried device "
          "bound %.3g" % (rel_dev, rel_host, carried))
    assert rel_dev <= rel_host + carried + 1e-10
    assert rel_host < 1.0
    # in place, and a second pass keeps the first input weight
    again = timestream.delay_filter(pm, filled.directory, **DELAY)
    assert again.directory == filled.directory
    f2 = _read_all(again, nfreq)
    assert all(np.array_equal(da["weight_input"], w[fi]) and not da["delay_filled"].any() for fi, (da, _) in enumerate(f2))
    # filter and model write what the device gives
    flt = timestream.delay_filter(pm, holes.directory, str(d / "filtered"), **dict(DELAY, mode="filter"))
    xo = np.stack([da["timestream"] for da, _ in _read_all(flt, nfreq)])
    assert np.all(xo[w == 0] == 0) and np.abs(xo).max() < 1e-2 * np.abs(xc).max()


def test_delay_key_of_the_routes(prod, tmp_path):
    """`stack_baselines(delay=)`, `sidereal_stack(delay=)` and `delay:` in the pipeline write what the stand-alone
    `delay_filter` writes on the output of the same call without the key; without the key no file knows of the step;
    unstacked directories and unknown keys are refused."""
    import yaml

    from driftscan_amd import pipeline, timestream

    pm, d = prod
    tel = pm.telescope
    nfreq = int(tel.nfreq)
    udir = str(tmp_path / "u0")
    wu = None
    nt = int(np.ceil(2.5 * (2 * int(tel.mmax) + 1)))
    timestream.simulate_unstacked(pm, udir, ndays=0, resolution=86400.0 / nt, sources=[CATALOGUE])
    uts = timestream.Timestream(udir, pm)
    files = _read_all(uts, nfreq)
    rng = np.random.default_rng(4)
    from driftscan_amd import storage

    for fi, (data, attrs) in enumerate(files):   # one channel lost in every pair, 3 % of the samples of a channel elsewhere
        wu = np.broadcast_to(np.where(rng.random(data["timestream"].shape[1]) < 0.03, 0.0, 1.0), data["timestream"].shape).copy()
        if fi == CHAN:
            wu[:] = 0.0
        data["weight"] = wu
        with storage.File(uts._ffile(fi), "w") as f:
            for name, value in data.items():
                f.create_dataset(name, data=np.ascontiguousarray(value))
            for name, value in attrs.items():
                f.attrs[name] = value
    with pytest.raises(ValueError, match="unstacked"):
        timestream.delay_filter(pm, udir, str(tmp_path / "no"), **DELAY)
    plain = timestream.stack_baselines(pm, udir, str(tmp_path / "s_plain"))
    assert not os.path.exists(os.path.join(plain.directory, "delay_fit.hdf5"))
    assert all("delay_filled" not in da and "weight_input" not in da for da, _ in _read_all(plain, nfreq))
    assert not plain.weight_f(CHAN).any()
    keyed = timestream.stack_baselines(pm, udir, str(tmp_path / "s_keyed"), delay=DELAY)
    after = timestream.delay_filter(pm, plain.directory, str(tmp_path / "s_after"), **DELAY)
    _same_files(keyed, after, nfreq)
    with storage.File(os.path.join(keyed.directory, "delay_fit.hdf5"), "r") as f:
        print("ranks %s, info %s" % (f["rank"][:], np.unique(f["info"][:], return_counts=True)))
    sid = dict(ntime=nt, a=3, min_share=0.5)   # oversampled, as the day: the m-mode estimate has samples to spare
    sid_plain = timestream.sidereal_stack(pm, [plain.directory], str(tmp_path / "sid_plain"), **sid)
    sid_keyed = timestream.sidereal_stack(pm, [plain.directory], str(tmp_path / "sid_keyed"), delay=DELAY, **sid)
    assert not sid_plain.weight_f(CHAN).any()
    sid_after = timestream.delay_filter(pm, sid_plain.directory, str(tmp_path / "sid_after"), **DELAY)
    _same_files(sid_keyed, sid_after, nfreq)
    with pytest.raises(ValueError, match="unknown key"):
        timestream.stack_baselines(pm, udir, str(tmp_path / "bad"), delay=dict(tau=1.0))
    with pytest.raises(ValueError, match="stacked days"):
        timestream.sidereal_stack(pm, [udir], str(tmp_path / "bad2"), delay=DELAY)
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=True, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=False),
                timestreams=[dict(name="s0", directory=str(tmp_path / "p_s0"), stack_from=dict(directory=udir, delay=dict(DELAY))),
                             dict(name="sid", directory=str(tmp_path / "p_sid"),
                                  sidereal_from=dict(days=[plain.directory], delay=dict(DELAY), **sid))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    pl = pipeline.PipelineManager.from_configfile(str(cfile))
    pl.generate()
    _same_files(timestream.Timestream(str(tmp_path / "p_s0"), pm), keyed, nfreq)
    _same_files(timestream.Timestream(str(tmp_path / "p_sid"), pm), sid_keyed, nfreq)
    for name in ("p_s0", "p_sid"):   # the data arrives at the m-modes with no unsolved row
        with storage.File(str(tmp_path / name / "mmodes" / "weights.hdf5"), "r") as f:
            print("%s: ntime %d, kept samples %d .. %d per row, info %s" % (name, int(f.attrs["ntime"]), f["nkept"][:].min(),
                                                                         f["nkept"][:].max(), np.unique(f["info"][:])))
            assert not f["info"][:].any()
