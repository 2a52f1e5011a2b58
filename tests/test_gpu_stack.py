"""Unstacked (per-feed-pair) visibilities on the device: `Context.vis_stack` and
`Context.vis_expand` against extended precision on the tables of tests/stack_cases.py, against `ts_gain_apply`, their
determinism and refusals, and the routes `simulate_ensemble(unstacked=True)` -> `stack_baselines` -> m-modes on the small
polarised cylinder of tests/test_gpu_tsim.py."""
import os

import numpy as np
import pytest

import gains_cases as gc
import stack_cases as sc

pytestmark = pytest.mark.gpu

EPS = sc.EPS


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _guarded(ctx, nreal, nf, rows, ntime, dtype, base=None):
    """A (nreal + 2, nf, rows, ntime) device buffer whose first and last realisation are NaN-poisoned guard rows."""
    host = np.full((nreal + 2, nf, rows, ntime), np.nan, dtype=dtype)
    if base is not None:
        host[1:-1] = base
    return ctx.to_device(host)


def _guards_untouched(ctx, buf):
    h = ctx.to_host(buf)
    return bool(np.all(np.isnan(h[0].real)) and np.all(np.isnan(h[-1].real)))


def _weights(rng, shape):
    """Inverse variances in (0, 1) with about a third of the samples flagged (classes of one member often wholly)."""
    return rng.uniform(size=shape) * (rng.uniform(size=shape) < 0.7)


def _stack_case(rng, ctx, nfeed, off, mem, nreal, g_nreal, w_nreal, nf, ntime, use_w, use_g, use_fw):
    """One `vis_stack` call inside guard rows, checked element by element; returns the two worst ratios."""
    npairs, nmem = off.shape[0] - 1, mem.shape[0]
    vis = gc.crandn(rng, nreal, nf, nmem, ntime)
    w = _weights(rng, (w_nreal, nf, nmem, ntime)) if use_w else None
    g = gc.crandn(rng, g_nreal, nf, nfeed, ntime) if use_g else None
    fw = None
    if use_fw:
        fw = rng.uniform(0.5, 1.5, size=nfeed)
        fw[rng.integers(0, nfeed)] = 0.0
    out, wout, scale = sc.stack_exact(vis, off, mem, w=w, g=g, feed_weight=fw)
    bo, bw = _guarded(ctx, nreal, nf, npairs, ntime, np.complex128), _guarded(ctx, nreal, nf, npairs, ntime, np.float64)
    ro, rw = ctx.vis_stack(ctx.to_device(vis), off, mem, w=None if w is None else ctx.to_device(w),
                           g=None if g is None else ctx.to_device(g), feed_weight=fw, out=bo[1:-1], wout=bw[1:-1])
    assert ro.data_ptr() == bo[1:-1].data_ptr() and rw.data_ptr() == bw[1:-1].data_ptr()
    assert _guards_untouched(ctx, bo) and _guards_untouched(ctx, bw)
    got, gotw = ctx.to_host(bo)[1:-1], ctx.to_host(bw)[1:-1]
    if not (use_w or use_g or use_fw):
        assert np.all(gotw == 1.0)
    return sc.check_stack(got, gotw, out, wout, scale, off)


VARIANTS = [(False, False, False), (True, False, False), (False, True, False), (True, True, False), (True, True, True),
            (False, False, True)]


@pytest.mark.parametrize("ntime", [1, 5, 17, 65])
@pytest.mark.parametrize("name", ["one", "two", "line70", "cyl12"])
def test_vis_stack_against_extended_precision(name, ntime):
    """|delta out| <= K (n_c + 4) eps [sum w |g_i| |g_j| |V| / D + |out|] and |delta wout| <= K (n_c + 4) eps wout per
    element against np.clongdouble, K = stack_cases.K_STACK, for every combination of weights, gains and feed weights;
    out = wout = 0 exactly where D == 0; wout == 1.0 exactly with none of them.  ntime 1, 5: part of one tile; 17, 65:
    whole tiles and a part."""
    ctx = _ctx()
    nfeed, off, mem = sc.tables()[name]
    rng = np.random.default_rng(1000 * ntime + nfeed)
    worst = (0.0, 0.0)
    for nf in (1, 3):
        for nreal in (1, 3):
            for each in sorted({1, nreal}):
                for use_w, use_g, use_fw in VARIANTS:
                    r = _stack_case(rng, ctx, nfeed, off, mem, nreal, each, 1 if each == nreal else nreal, nf, ntime,
                                    use_w, use_g, use_fw)
                    worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("vis_stack %s, ntime %d: max err / bound at K = %d: out %.3g, wout %.3g" % ((name, ntime, sc.K_STACK) + worst))


@pytest.mark.parametrize("nfeed", sorted(sc.TILE_NFEED))
def test_vis_stack_every_gain_tile(nfeed):
    """More feeds, shorter tiles of staged gains (8, 4, 2, 1 samples) on partitions of 3000 random pairs with classes of
    1 to 200 members, ntime = 5; the variants without gains run on the 16-sample tile of the same tables."""
    ctx = _ctx()
    assert ctx.lib.dm_ts_gain_tile(nfeed) == sc.TILE_NFEED[nfeed]
    _, off, mem = sc.tile_table(nfeed)
    rng = np.random.default_rng(nfeed)
    worst = (0.0, 0.0)
    for nreal, g_nreal, w_nreal, variant in ((2, 2, 1, (True, True, False)), (2, 1, 2, (True, True, True)),
                                             (1, 1, 1, (False, True, False)), (2, 1, 1, (True, False, False)),
                                             (1, 1, 1, (False, False, False))):
        r = _stack_case(rng, ctx, nfeed, off, mem, nreal, g_nreal, w_nreal, 2, 5, *variant)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
    print("vis_stack %d feeds (tile %d): max err / bound at K = %d: out %.3g, wout %.3g"
          % ((nfeed, sc.TILE_NFEED[nfeed], sc.K_STACK) + worst))


def _expand_case(rng, ctx, nfeed, off, mem, nreal, g_nreal, nf, ntime, use_g, accumulate):
    npairs, nmem = off.shape[0] - 1, mem.shape[0]
    sky = gc.crandn(rng, nreal, nf, npairs, ntime)
    g = gc.crandn(rng, g_nreal, nf, nfeed, ntime) if use_g else None
    base = gc.crandn(rng, nreal, nf, nmem, ntime) if accumulate else None
    want, bound = sc.expand_exact(sky, off, mem, g=g, base=base)
    buf = _guarded(ctx, nreal, nf, nmem, ntime, np.complex128, base=base)
    ctx.vis_expand(ctx.to_device(sky), off, mem, g=None if g is None else ctx.to_device(g), out=buf[1:-1],
                   accumulate=accumulate)
    assert _guards_untouched(ctx, buf)
    got = ctx.to_host(buf)[1:-1]
    err = np.abs(got - want).astype(np.float64)
    assert np.all(np.isfinite(got)) and np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
    return float((err / np.maximum(bound, 1e-300)).max())


@pytest.mark.parametrize("ntime", [1, 5, 17, 65])
@pytest.mark.parametrize("name", ["one", "two", "line70", "cyl12"])
def test_vis_expand_against_extended_precision(name, ntime):
    """4 eps per product (g_i conj(g_j), then times the sky: 8 eps |g_i| |g_j| |sky|), plus eps |result| when
    accumulating; without gains the class row is copied bit for bit."""
    ctx = _ctx()
    nfeed, off, mem = sc.tables()[name]
    rng = np.random.default_rng(2000 * ntime + nfeed)
    worst = 0.0
    for nf in (1, 3):
        for nreal in (1, 3):
            for g_nreal in sorted({1, nreal}):
                for use_g in (False, True):
                    for accumulate in (False, True):
                        worst = max(worst, _expand_case(rng, ctx, nfeed, off, mem, nreal, g_nreal, nf, ntime, use_g,
                                                        accumulate))
    print("vis_expand %s, ntime %d: max err / bound = %.3g" % (name, ntime, worst))


@pytest.mark.parametrize("nfeed", sorted(sc.TILE_NFEED))
def test_vis_expand_every_gain_tile(nfeed):
    ctx = _ctx()
    _, off, mem = sc.tile_table(nfeed)
    rng = np.random.default_rng(nfeed + 1)
    worst = 0.0
    for nreal, g_nreal, use_g, accumulate in ((2, 2, True, False), (2, 1, True, True), (1, 1, False, False)):
        worst = max(worst, _expand_case(rng, ctx, nfeed, off, mem, nreal, g_nreal, 2, 5, use_g, accumulate))
    print("vis_expand %d feeds (tile %d): max err / bound = %.3g" % (nfeed, sc.TILE_NFEED[nfeed], worst))


def _roundtrip_bound(g, sky, off, mem):
    """Bound on |vis_stack(vis_expand(sky, g), g=g, w) - sky| for 0/1 weights: the expansion's 8 eps |g_i| |g_j| |sky|
    per member enters the numerator times |g_i| |g_j|, so it moves the quotient by at most 8 eps |sky| (a weighted mean
    of the members' relative errors); the stack adds its own bound, whose scale sum w |g_i|^2 |g_j|^2 |sky| / D is |sky|."""
    n = sc.class_sizes(off)
    return (8 * EPS + 2 * sc.K_STACK * (n + 4) * EPS) * np.abs(sky)


def test_roundtrip_and_wholly_flagged_classes():
    """Expand with gains, stack with the same gains and random flags that keep a member of every class: the sky comes
    back.  Then with three classes flagged whole: those rows are exactly 0 with wout 0, the others keep their bits."""
    ctx = _ctx()
    rng = np.random.default_rng(21)
    for name, ntime in (("line70", 17), ("cyl12", 5)):
        nfeed, off, mem = sc.tables()[name]
        nreal, nf = 3, 2
        sky = gc.crandn(rng, nreal, nf, off.shape[0] - 1, ntime)
        g = 1.0 + 0.3 * gc.crandn(rng, nreal, nf, nfeed, ntime)
        dg = ctx.to_device(g)
        vis = ctx.vis_expand(ctx.to_device(sky), off, mem, g=dg)
        w = sc.keep_one_per_class(rng, off, (1, nf, mem.shape[0], ntime))
        out, wout = ctx.vis_stack(vis, off, mem, w=ctx.to_device(w), g=dg)
        got, gotw = ctx.to_host(out), ctx.to_host(wout)
        bound = _roundtrip_bound(g, sky, off, mem)
        print("round trip %s: max err / bound = %.3g" % (name, (np.abs(got - sky) / bound).max()))
        assert np.all(np.abs(got - sky) <= bound) and np.all(gotw > 0)
        gone = [0, 2, off.shape[0] - 2]
        w2 = w.copy()
        for c in gone:
            w2[:, :, off[c] : off[c + 1]] = 0.0
        out2, wout2 = ctx.vis_stack(vis, off, mem, w=ctx.to_device(w2), g=dg)
        got2, gotw2 = ctx.to_host(out2), ctx.to_host(wout2)
        rest = np.setdiff1d(np.arange(off.shape[0] - 1), gone)
        assert np.all(got2[:, :, gone] == 0) and np.all(gotw2[:, :, gone] == 0)
        assert np.array_equal(got2[:, :, rest], got[:, :, rest]) and np.array_equal(gotw2[:, :, rest], gotw[:, :, rest])


def test_stack_of_an_expansion_is_ts_gain_apply():
    """`vis_stack(vis_expand(sky, g))` without calibration or weights is the stacked baseline gain on the sky: within the
    sum of the bounds of the two routes of `ts_gain_apply(g, sky)`, and wout == 1.0."""
    ctx = _ctx()
    rng = np.random.default_rng(22)
    for name, ntime in (("line70", 17), ("cyl12", 65), ("two", 5)):
        nfeed, off, mem = sc.tables()[name]
        nreal, nf = 2, 3
        sky = gc.crandn(rng, nreal, nf, off.shape[0] - 1, ntime)
        g = gc.crandn(rng, nreal, nf, nfeed, ntime)
        dg, dsky = ctx.to_device(g), ctx.to_device(sky)
        out, wout = ctx.vis_stack(ctx.vis_expand(dsky, off, mem, g=dg), off, mem)
        ref = ctx.to_host(ctx.ts_gain_apply(dg, off, mem, dsky))
        _, A = gc.baseline_gains_exact(g, off, mem)
        n = sc.class_sizes(off)
        # the expansion's 8 eps per member, averaged, plus the stack's bound at scale A |sky| (and |out| <= A |sky|)
        bound = gc.apply_bound(A, sky, off) + (8 * EPS + 2 * sc.K_STACK * (n + 4) * EPS) * A * np.abs(sky)
        err = np.abs(ctx.to_host(out) - ref)
        print("stack of expansion against ts_gain_apply, %s: max err / bound = %.3g" % (name, (err / bound).max()))
        assert np.all(err <= bound) and np.all(ctx.to_host(wout) == 1.0)


def test_vis_stack_is_deterministic_across_batches():
    """A class has the same bits alone, inside the full table, at another position, and as realisation 2 of 3 against a
    call holding only that realisation — with weights and gains, on the 16-sample tile and on the 4-sample one."""
    ctx = _ctx()
    rng = np.random.default_rng(23)
    for (nfeed, off, mem), ntime in ((sc.tables()["line70"], 17), (sc.tile_table(600), 5)):
        nreal, nf, nmem = 3, 2, mem.shape[0]
        vis = gc.crandn(rng, nreal, nf, nmem, ntime)
        w = _weights(rng, (nreal, nf, nmem, ntime))
        g = gc.crandn(rng, nreal, nf, nfeed, ntime)
        full, fullw = (ctx.to_host(t) for t in ctx.vis_stack(ctx.to_device(vis), off, mem, w=ctx.to_device(w),
                                                              g=ctx.to_device(g)))
        one, onew = (ctx.to_host(t) for t in ctx.vis_stack(ctx.to_device(vis[2:3]), off, mem, w=ctx.to_device(w[2:3]),
                                                            g=ctx.to_device(g[2:3])))
        assert np.array_equal(one[0], full[2]) and np.array_equal(onew[0], fullw[2])
        plain = ctx.to_host(ctx.vis_stack(ctx.to_device(vis), off, mem)[0])
        for cls in (0, 2, 3):
            rows = slice(off[cls], off[cls + 1])
            n = off[cls + 1] - off[cls]
            sub = lambda a: ctx.to_device(np.ascontiguousarray(a[1:2, 1:2, rows]))
            alone, alonew = ctx.vis_stack(sub(vis), [0, n], mem[rows], w=sub(w), g=ctx.to_device(np.ascontiguousarray(g[1:2, 1:2])))
            assert np.array_equal(ctx.to_host(alone)[0, 0, 0], full[1, 1, cls]), cls
            assert np.array_equal(ctx.to_host(alonew)[0, 0, 0], fullw[1, 1, cls]), cls
            # at another position: behind a class of one
            off2, mem2 = np.array([0, 1, 1 + n], dtype=np.int32), np.concatenate([[[0, 0]], mem[rows]])
            pad = lambda a: ctx.to_device(np.ascontiguousarray(np.concatenate([a[1:2, 1:2, :1], a[1:2, 1:2, rows]], axis=2)))
            moved, movedw = ctx.vis_stack(pad(vis), off2, mem2, w=pad(w), g=ctx.to_device(np.ascontiguousarray(g[1:2, 1:2])))
            assert np.array_equal(ctx.to_host(moved)[0, 0, 1], full[1, 1, cls]), cls
            assert np.array_equal(ctx.to_host(movedw)[0, 0, 1], fullw[1, 1, cls]), cls
            p1 = ctx.to_host(ctx.vis_stack(sub(vis), [0, n], mem[rows])[0])
            assert np.array_equal(p1[0, 0, 0], plain[1, 1, cls]), cls
        # frequency slices of wider arrays: the same bits
        wide = ctx.zeros((nreal, nf + 1, off.shape[0] - 1, ntime), np.complex128)
        widew = ctx.zeros((nreal, nf + 1, off.shape[0] - 1, ntime), np.float64)
        ctx.vis_stack(ctx.to_device(vis), off, mem, w=ctx.to_device(w), g=ctx.to_device(g), out=wide[:, 1:], wout=widew[:, 1:])
        assert np.array_equal(ctx.to_host(wide)[:, 1:], full) and not ctx.to_host(wide)[:, 0].any()
        assert np.array_equal(ctx.to_host(widew)[:, 1:], fullw)


def test_refusals_leave_the_outputs_alone():
    """Every listed condition raises before any launch: `dm_last_error` names it and the NaN guards and the outputs keep
    their bits."""
    from driftscan_amd import _lib

    ctx = _ctx()
    vis = ctx.to_device(np.ones((1, 1, 2, 5), dtype=np.complex128))
    g = ctx.to_device(np.ones((1, 1, 3, 5), dtype=np.complex128))
    sky = ctx.to_device(np.ones((1, 1, 2, 5), dtype=np.complex128))
    bo, bw = _guarded(ctx, 1, 1, 2, 5, np.complex128), _guarded(ctx, 1, 1, 2, 5, np.float64)
    bo[1:-1] = 7.0
    bw[1:-1] = 7.0
    be = _guarded(ctx, 1, 1, 2, 5, np.complex128)
    be[1:-1] = 7.0
    kw = dict(out=bo[1:-1], wout=bw[1:-1])
    ok = [[0, 1], [1, 2]]
    with pytest.raises(_lib.DriftMIError, match="class 1 is empty"):
        ctx.vis_stack(vis, [0, 2, 2], ok, g=g, **kw)
    with pytest.raises(_lib.DriftMIError, match="class 1 is empty"):
        ctx.vis_expand(sky, [0, 2, 2], ok, g=g, out=be[1:-1])
    with pytest.raises(_lib.DriftMIError, match="class_off\\[0\\] must be 0"):
        ctx.vis_stack(ctx.to_device(np.ones((1, 1, 3, 5), dtype=np.complex128)), [1, 2, 3], [[0, 1], [1, 2], [0, 2]], g=g, **kw)
    with pytest.raises(_lib.DriftMIError, match="class_off decreases at class 1"):
        ctx.vis_stack(ctx.to_device(np.ones((1, 1, 1, 5), dtype=np.complex128)), [0, 2, 1], [[0, 1]], g=g, **kw)
    with pytest.raises(_lib.DriftMIError, match="names feed 3 of 3"):
        ctx.vis_stack(vis, [0, 1, 2], [[0, 1], [3, 2]], g=g, **kw)
    with pytest.raises(_lib.DriftMIError, match="names feed -1"):
        ctx.vis_stack(vis, [0, 1, 2], [[0, -1], [1, 2]], **kw)
    with pytest.raises(_lib.DriftMIError, match="names feed 3 of 3"):
        ctx.vis_expand(sky, [0, 1, 2], [[0, 1], [3, 2]], g=g, out=be[1:-1])
    with pytest.raises(_lib.DriftMIError, match="feed weight 1 is negative"):
        ctx.vis_stack(vis, [0, 1, 2], ok, feed_weight=[1.0, -1.0, 1.0], **kw)
    # more feeds than one sample's tile holds: refused with gains, accepted without (no LDS is used then)
    big = ctx.to_device(np.ones((1, 1, 10241, 1), dtype=np.complex128))
    one = ctx.to_device(np.ones((1, 1, 1, 1), dtype=np.complex128))
    with pytest.raises(_lib.DriftMIError, match="does not fit"):
        ctx.vis_stack(one, [0, 1], [[0, 0]], g=big)
    with pytest.raises(_lib.DriftMIError, match="does not fit"):
        ctx.vis_expand(one, [0, 1], [[0, 0]], g=big)
    o1, w1 = ctx.vis_stack(one, [0, 1], [[10240, 0]])
    assert ctx.to_host(o1)[0, 0, 0, 0] == 1.0 and ctx.to_host(w1)[0, 0, 0, 0] == 1.0
    # through the C entry point: negative sizes, null pointers with work to do, outputs sharing elements with vis
    lib, h = ctx.lib, ctx.h
    off, offp = _lib._iarr([0, 1, 2])
    mem, memp = _lib._iarr(ok)
    P = ctx.ptr

    def stack_rc(nreal=1, nf=1, nfeed=3, npairs=2, ntime=5, v=vis, o=bo[1:-1], wo=bw[1:-1]):
        return lib.dm_vis_stack(h, nreal, 1, 1, nf, nfeed, npairs, ntime, offp, memp, P(v), P(None), P(None), None, P(o),
                                P(wo), 0, 0)

    def last():
        return lib.dm_last_error(h).decode()

    assert stack_rc(ntime=-1) != 0 and "negative size" in last()
    assert stack_rc(nf=-1) != 0 and "negative size" in last()
    assert stack_rc(v=None) != 0 and "null pointer" in last()
    assert stack_rc(o=None) != 0 and "null pointer" in last()
    assert stack_rc(wo=None) != 0 and "null pointer" in last()
    assert stack_rc(o=vis) != 0 and "shares an element with vis" in last()
    both = ctx.to_device(np.ones((1, 1, 4, 5), dtype=np.complex128))
    assert stack_rc(v=both[:, :, :2], o=both[:, :, 1:3]) != 0 and "shares an element with vis" in last()
    assert stack_rc(nreal=0) == 0 and stack_rc(nf=0) == 0 and stack_rc(ntime=0) == 0          # no-ops
    rc = lib.dm_vis_expand(h, 1, 1, 1, 3, 2, 5, offp, memp, P(None), P(sky), P(None), 0, 0, 0)
    assert rc != 0 and "null pointer" in last()
    rc = lib.dm_vis_expand(h, 1, 1, 1, 3, 2, 5, offp, memp, P(None), P(sky), P(sky), 0, 0, 0)
    assert rc != 0 and "shares an element with sky" in last()
    assert lib.dm_vis_expand(h, 1, 1, 1, 3, 2, -5, offp, memp, P(None), P(sky), P(be[1:-1]), 0, 0, 0) != 0
    # the wrappers' own checks
    for bad in (lambda: ctx.vis_stack(vis, [0, 1, 2], [[0, 1]]),                               # members short of the rows
                lambda: ctx.vis_stack(vis, [0, 1, 2], ok, w=ctx.to_device(np.ones((2, 1, 2, 5)))),     # w_nreal
                lambda: ctx.vis_stack(vis, [0, 1, 2], ok, g=ctx.to_device(np.ones((2, 1, 3, 5), dtype=np.complex128))),
                lambda: ctx.vis_stack(vis, [0, 1, 2], ok, out=bo[1:-1], wout=ctx.empty((1, 1, 2, 4), np.float64)),
                lambda: ctx.vis_expand(sky, [0, 1], [[0, 1]]),                                  # class_off short of the rows
                lambda: ctx.vis_expand(sky, [0, 1, 2], ok, accumulate=True)):
        with pytest.raises(ValueError):
            bad()
    ctx.sync()
    for buf in (bo, bw, be):
        hbuf = ctx.to_host(buf)
        assert _guards_untouched(ctx, buf) and np.all(hbuf[1:-1] == 7.0)
    assert np.all(ctx.to_host(vis) == 1.0) and np.all(ctx.to_host(both) == 1.0)


# ---- the routes -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    """The products of tests/test_gpu_tsim.py: 2 cylinders, 3 feeds, 3 frequencies, polarised."""
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("stack")
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


MODEL = dict(sigma_amp=0.05, sigma_phase=0.1, corr_time=1800.0, seed=2)


def _ntime(tel):
    return int(np.ceil(2.5 * (2 * int(tel.mmax) + 1)))


def _dead_feed(tel):
    """(feed, emptied classes, thinned classes): the first feed whose removal empties a class and thins another."""
    off, mem = tel.redundant_pairs()
    n = np.diff(off)
    cls = np.repeat(np.arange(n.shape[0]), n)
    for a in range(int(tel.nfeed)):
        lost = np.bincount(cls[(mem[:, 0] == a) | (mem[:, 1] == a)], minlength=n.shape[0])
        emptied, thinned = np.nonzero(lost == n)[0], np.nonzero((lost > 0) & (lost < n))[0]
        if emptied.size and thinned.size:
            return a, emptied, thinned, (n - lost) / n
    raise AssertionError("no feed empties one class and thins another")


@pytest.fixture(scope="module")
def routes(prod, skyfile):
    """(a) unstacked with gains, stacked with the gains of the files; the stacked simulators without and with gains."""
    from driftscan_amd import skysim, timestream

    pm, d = prod
    tel = pm.telescope
    ntime = _ntime(tel)
    kw = dict(maps=[skyfile], ndays=0, resolution=86400.0 / ntime, first=1)
    model = skysim.GainModel(**MODEL)
    uns = timestream.simulate_ensemble(pm, str(d / "uns"), 1, gains=model, unstacked=True, **kw)[0]
    cal = timestream.stack_baselines(pm, uns.directory, str(d / "cal"), calibrate="file")
    ideal = timestream.simulate_ensemble(pm, str(d / "ideal"), 1, **kw)[0]
    return dict(pm=pm, d=d, tel=tel, ntime=ntime, kw=kw, model=model, uns=uns, cal=cal, ideal=ideal)


def test_calibrated_stack_of_unstacked_data_is_the_ideal_telescope(routes):
    """(a): gains applied per feed pair and undone by `stack_baselines(calibrate="file")` give the data of the
    telescope without gain errors, within the round-trip bound at max |v|; no `weight` is written and the m-modes of the
    two directories agree to 1e-10 of max |v|."""
    from driftscan_amd import storage

    tel, ntime, uns, cal, ideal = (routes[k] for k in ("tel", "ntime", "uns", "cal", "ideal"))
    off, mem = tel.redundant_pairs()
    nmem = int(off[-1])
    assert uns.ntime == ntime and uns.is_unstacked() and not cal.is_unstacked()
    with storage.File(uns._ffile(0), "r") as f:
        assert f["timestream"].shape == (nmem, ntime) and int(f.attrs["unstacked"]) == 1 and "weight" not in f
        assert np.array_equal(f["members"][:], mem) and np.array_equal(f["class_off"][:], off)
        assert f["gain"].shape == (tel.nfeed, ntime)
    nmax = int(np.diff(off).max())
    for fi in range(tel.nfreq):
        v, want = cal.timestream_f(fi), ideal.timestream_f(fi)
        scale = np.abs(want).max()
        bound = (8 * EPS + 2 * sc.K_STACK * (nmax + 4) * EPS) * scale
        print("frequency %d: max |delta| / bound = %.3g" % (fi, np.abs(v - want).max() / bound))
        assert v.shape == (tel.npairs, ntime) and scale > 0 and np.abs(v - want).max() <= bound
        with storage.File(cal._ffile(fi), "r") as f, storage.File(ideal._ffile(fi), "r") as h:
            assert "weight" not in f and sorted(f.keys()) == sorted(h.keys())
            assert sorted(f.attrs.keys()) == sorted(h.attrs.keys())
    # the same gains handed over as an array (and as a device tensor): the same bits
    from driftscan_amd import timestream

    gains = []
    for fi in range(tel.nfreq):
        with storage.File(uns._ffile(fi), "r") as f:
            gains.append(f["gain"][:])
    for k, cg in enumerate((np.stack(gains), _ctx().to_device(np.stack(gains)))):
        again = timestream.stack_baselines(routes["pm"], uns.directory, str(routes["d"] / ("cal_array%d" % k)), calibrate=cg)
        for fi in range(tel.nfreq):
            assert np.array_equal(again.timestream_f(fi), cal.timestream_f(fi))
    with pytest.raises(ValueError, match="calibrate"):
        timestream.stack_baselines(routes["pm"], uns.directory, str(routes["d"] / "cal_bad"), calibrate=np.stack(gains)[:, :-1])
    cal.generate_modes_batched()
    ideal.generate_modes_batched()
    assert not os.path.exists(cal.output_directory + "/mmodes/weights.hdf5")
    vmax = max(np.abs(ideal.timestream_f(fi)).max() for fi in range(tel.nfreq))
    for mi in range(tel.mmax + 1):
        assert np.abs(cal.mmode(mi) - ideal.mmode(mi)).max() <= 1e-10 * vmax, mi


def test_uncalibrated_stack_is_the_stacked_route_with_gains(routes):
    """(b): without calibration the stack is what the stacked simulator makes of the same gain model, within the sum of
    the two kernels' bounds; and it is not the calibrated result, by more than 1 % of max |v|."""
    from driftscan_amd import storage, timestream

    pm, d, tel, kw, model, uns, cal = (routes[k] for k in ("pm", "d", "tel", "kw", "model", "uns", "cal"))
    raw = timestream.stack_baselines(pm, uns.directory, str(d / "raw"), calibrate=None)
    ref = timestream.simulate_ensemble(pm, str(d / "gained"), 1, gains=model, **kw)[0]
    off, _ = tel.redundant_pairs()
    n = sc.class_sizes(off)
    for fi in range(tel.nfreq):
        v, want, c = raw.timestream_f(fi), ref.timestream_f(fi), cal.timestream_f(fi)
        with storage.File(uns._ffile(fi), "r") as f:
            gmax = np.abs(f["gain"][:]).max()
        # A <= max |g|^2: ts_gain_apply's 4 (n + 2) eps A |sky| plus the expansion's 8 eps and the stack's 2 K (n + 4) eps
        # at the same scale, with |sky| <= max |v| of the calibrated data (the gains move it by a few per cent)
        bound = (4 * (n + 2) + 8 + 2 * sc.K_STACK * (n + 4)) * EPS * gmax**2 * (1.01 * np.abs(c).max())
        print("frequency %d: max |delta| / bound = %.3g; calibration moves the data by %.3g of max |v|"
              % (fi, (np.abs(v - want) / bound).max(), np.abs(v - c).max() / np.abs(c).max()))
        assert np.all(np.abs(v - want) <= bound)
        assert np.abs(v - c).max() > 0.01 * np.abs(c).max()


def test_dead_feed_thins_some_classes_and_empties_others(routes):
    """(c): a dead feed of the telescope's own table: the surviving rows are the complete stack, `weight` is
    (n_c - k) / n_c exactly, the emptied rows are zero with weight 0, and `generate_modes_batched` reports info = -1 on
    exactly those rows and the modes of (a) on the others."""
    from driftscan_amd import storage, timestream

    pm, d, tel, ntime, uns, cal = (routes[k] for k in ("pm", "d", "tel", "ntime", "uns", "cal"))
    feed, emptied, thinned, frac = _dead_feed(tel)
    assert emptied.size > 0 and thinned.size > 0
    off, _ = tel.redundant_pairs()
    nmax = int(np.diff(off).max())
    dead = timestream.stack_baselines(pm, uns.directory, str(d / "dead"), calibrate="file", dead_feeds=[feed])
    left = np.setdiff1d(np.arange(tel.npairs), emptied)
    for fi in range(tel.nfreq):
        v, c, w = dead.timestream_f(fi), cal.timestream_f(fi), dead.weight_f(fi)
        bound = 2 * (8 * EPS + 2 * sc.K_STACK * (nmax + 4) * EPS) * np.abs(c).max()     # two round trips of the same sky
        assert w is not None and w.shape == (tel.npairs, ntime)
        assert np.array_equal(w, np.broadcast_to(frac[:, None], w.shape))
        assert np.all(v[emptied] == 0) and np.all(w[emptied] == 0)
        assert np.abs(v[left] - c[left]).max() <= bound
    dead.generate_modes_batched()
    with storage.File(dead.output_directory + "/mmodes/weights.hdf5", "r") as f:
        info = f["info"][:]
    want = np.zeros((tel.nfreq, tel.npairs), dtype=info.dtype)
    want[:, emptied] = -1
    assert np.array_equal(info, want)
    vmax = max(np.abs(cal.timestream_f(fi)).max() for fi in range(tel.nfreq))
    cal.generate_modes_batched()
    for mi in range(tel.mmax + 1):
        a, b = dead.mmode(mi), cal.mmode(mi)
        assert np.abs(a[:, :, left] - b[:, :, left]).max() <= 1e-10 * vmax, mi
        assert not a[:, :, emptied].any()


def test_noise_of_the_stack_has_the_level_its_weight_states(prod):
    """(d): noise only, 8 realisations, unit weights: per class z = (mean |v|^2 / (ntime noisepower) - 1) sqrt(K) within
    5 for the complete stack, and against 1 / W with the dead feed of (c) on the classes that are left."""
    from driftscan_amd import timestream

    pm, _ = prod
    tel = pm.telescope
    ctx = _ctx()
    ntime, nreal, ndays = _ntime(tel), 8, 10
    off, mem = tel.redundant_pairs()
    vis = timestream.simulate_visibilities(pm, nreal, ndays=ndays, resolution=86400.0 / ntime, seed=13, unstacked=True)
    assert tuple(vis.shape) == (nreal, tel.nfreq, int(off[-1]), ntime)
    nominal = ntime * np.asarray(tel.noisepower(np.arange(tel.npairs)[None, :], np.arange(tel.nfreq)[:, None], ndays=ndays),
                                 dtype=np.float64).reshape(tel.nfreq, tel.npairs)
    K = nreal * tel.nfreq * ntime
    out, wout = (ctx.to_host(t) for t in ctx.vis_stack(vis, off, mem))
    z = (np.mean(np.abs(out) ** 2 / nominal[None, :, :, None], axis=(0, 1, 3)) - 1) * np.sqrt(K)
    print("complete stack: max |z| = %.2f" % np.abs(z).max())
    assert np.all(wout == 1.0) and np.abs(z).max() <= 5
    feed, emptied, thinned, frac = _dead_feed(tel)
    fw = np.ones(tel.nfeed)
    fw[feed] = 0.0
    out, wout = (ctx.to_host(t) for t in ctx.vis_stack(vis, off, mem, feed_weight=fw))
    assert np.array_equal(wout, np.broadcast_to(frac[None, None, :, None], wout.shape))
    left = frac > 0
    z = (np.mean(np.abs(out) ** 2 / nominal[None, :, :, None], axis=(0, 1, 3))[left] * frac[left] - 1) * np.sqrt(K)
    print("dead feed %d: max |z| = %.2f (emptied %s, thinned %s)" % (feed, np.abs(z).max(), emptied, thinned))
    assert np.abs(z).max() <= 5 and np.all(out[:, :, ~left] == 0)


def test_unstacked_false_is_inert_and_unstacked_directories_are_refused(routes, skyfile):
    from driftscan_amd import timestream

    pm, uns, kw = routes["pm"], routes["uns"], routes["kw"]
    ctx = _ctx()
    a = ctx.to_host(timestream.simulate_visibilities(pm, 2, seed=3, **dict(kw, ndays=10), gains=routes["model"]))
    b = ctx.to_host(timestream.simulate_visibilities(pm, 2, seed=3, **dict(kw, ndays=10), gains=routes["model"], unstacked=False))
    assert np.abs(a).max() > 0 and np.array_equal(a, b)
    for call in (uns.generate_mmodes, uns.generate_modes_batched):
        with pytest.raises(ValueError, match="stack_baselines"):
            call()
    with pytest.raises(ValueError, match="unstacked"):
        timestream.stack_baselines(pm, routes["cal"].directory, str(routes["d"] / "twice"))


def test_unstacked_weights_chunks_and_the_pipeline(routes, skyfile, tmp_path):
    """Flags per feed pair zero the samples and reach the stacked `weight`; one frequency per chunk gives the rows of
    the full call (the noise bit for bit); a pipeline entry with `unstacked: true` and one with `stack_from` run."""
    import yaml

    from driftscan_amd import pipeline, storage, timestream

    pm, d, tel, ntime, kw = (routes[k] for k in ("pm", "d", "tel", "ntime", "kw"))
    ctx = _ctx()
    off, mem = tel.redundant_pairs()
    nmem = int(off[-1])
    rng = np.random.default_rng(31)
    w = (rng.uniform(size=(tel.nfreq, nmem, ntime)) < 0.8).astype(np.float64)
    full = ctx.to_host(timestream.simulate_visibilities(pm, 2, seed=3, unstacked=True, weights=w, **dict(kw, ndays=10)))
    tiny = ctx.to_host(timestream.simulate_visibilities(pm, 2, seed=3, unstacked=True, weights=w, chunk_gb=1e-9,
                                                        **dict(kw, ndays=10)))
    noise = ctx.to_host(timestream.simulate_visibilities(pm, 2, seed=3, unstacked=True, ndays=10, resolution=kw["resolution"],
                                                         first=1))
    nz = ctx.to_host(timestream.simulate_visibilities(pm, 2, seed=3, unstacked=True, ndays=10, resolution=kw["resolution"],
                                                      first=1, chunk_gb=1e-9))
    assert np.array_equal(nz, noise)
    assert np.all(full[:, w == 0] == 0) and np.all(full[:, w > 0] != 0)
    assert np.abs(tiny - full).max() <= 1e-12 * np.abs(full).max()
    # without gains every member row is its class row, bit for bit; explicit gains of one phase for all feeds leave it
    # within the bound of the two products
    cls = np.repeat(np.arange(tel.npairs), np.diff(off))
    plain = ctx.to_host(timestream.simulate_visibilities(pm, 2, **kw))[:, :, cls]
    assert np.array_equal(ctx.to_host(timestream.simulate_visibilities(pm, 2, unstacked=True, **kw)), plain)
    phase = np.exp(1j * rng.uniform(0, 2 * np.pi, size=(tel.nfreq, 1, ntime)))
    garr = np.ascontiguousarray(np.broadcast_to(phase, (tel.nfreq, tel.nfeed, ntime)))
    for gains in (garr, ctx.to_device(garr)):
        got = ctx.to_host(timestream.simulate_visibilities(pm, 2, unstacked=True, gains=gains, **kw))
        assert np.all(np.abs(got - plain) <= 8 * EPS * (1 + 4 * EPS) * np.abs(plain))
    tss = timestream.simulate_ensemble(pm, str(tmp_path / "flagged"), 1, unstacked=True, weights=w, **kw)
    st = timestream.stack_baselines(pm, tss[0].directory, str(tmp_path / "flagged_stack"))
    for fi in range(tel.nfreq):
        with storage.File(tss[0]._ffile(fi), "r") as f:
            assert np.array_equal(f["weight"][:], w[fi])
        want = np.add.reduceat(w[fi], off[:-1], axis=0) / np.diff(off)[:, None]
        assert np.array_equal(st.weight_f(fi), want)
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=True, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=False),
                timestreams=[dict(name="u", directory=str(tmp_path / "pipe_u"),
                                  simulate=dict(ndays=0, maps=[skyfile], gains=dict(MODEL), unstacked=True,
                                                resolution=kw["resolution"], sky_realisation=1)),
                             dict(name="s", directory=str(tmp_path / "pipe_s"),
                                  stack_from=dict(directory=str(tmp_path / "pipe_u"), calibrate="file"))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = pipeline.PipelineManager.from_configfile(str(cfile))
    assert sorted(p.timestreams) == ["s"] and sorted(p.unstacked) == ["u"]
    p.simulate()
    assert p.unstacked["u"].is_unstacked() and not os.path.exists(str(tmp_path / "pipe_s"))
    p.generate()
    s = p.timestreams["s"]
    for fi in range(tel.nfreq):
        v, c = s.timestream_f(fi), routes["cal"].timestream_f(fi)            # the same two calls once more
        assert np.abs(v - c).max() <= 1e-12 * np.abs(c).max()
    assert os.path.exists(s._mfile(0))


# ---- the drivers over more than one chunk of frequencies ------------------------------------------------------------------
CHUNK_RFI = dict(chi1=5.5, segment=512)
CHUNK_CADENCE = 120.0   # 718 samples per turn, as in tests/test_gpu_sidereal.py


def _same_directories(a, b, tel):
    """Every dataset and attribute of every per-frequency file of the Timestreams a and b, bit for bit."""
    from driftscan_amd import storage

    for fi in range(tel.nfreq):
        with storage.File(a._ffile(fi), "r") as f, storage.File(b._ffile(fi), "r") as g:
            assert sorted(f.keys()) == sorted(g.keys()) and sorted(f.attrs.keys()) == sorted(g.attrs.keys())
            for name in f.keys():
                x, y = f[name][:], g[name][:]
                assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (fi, name)
            for name in f.attrs.keys():
                assert np.array_equal(f.attrs[name], g.attrs[name]), (fi, name)


def _chunked_redundant(routes, name, chunk_gb):
    from driftscan_amd import timestream

    return timestream.stack_baselines(routes["pm"], routes["uns"].directory, str(routes["d"] / name), calibrate="redundant",
                                      redcal={"reference": "file"}, rfi=dict(CHUNK_RFI),
                                      dead_feeds=[_dead_feed(routes["tel"])[0]], chunk_gb=chunk_gb)


def _chunked_model(routes, name, chunk_gb):
    """The data and the model of the fixture `sky_model` of tests/test_gpu_modelcal.py: explicit gains constant over
    intervals of 16 samples, the `ideal` directory as the model."""
    from driftscan_amd import timestream

    pm, d, tel, ntime, kw, ideal = (routes[k] for k in ("pm", "d", "tel", "ntime", "kw", "ideal"))
    if "chunk_uns" not in routes:
        rng = np.random.default_rng(23)
        nint = -(-ntime // 16)
        gq = (1 + 0.05 * rng.uniform(-1, 1, (tel.nfreq, tel.nfeed, nint))) * np.exp(0.1j * rng.uniform(-1, 1, (tel.nfreq, tel.nfeed, nint)))
        gains = np.ascontiguousarray(gq[..., np.arange(ntime) // 16])
        routes["chunk_uns"] = timestream.simulate_ensemble(pm, str(d / "chunk_uns"), 1, gains=gains, unstacked=True, **kw)[0]
    return timestream.stack_baselines(pm, routes["chunk_uns"].directory, str(d / name), calibrate="model", rfi=dict(CHUNK_RFI),
                                      dead_feeds=[_dead_feed(tel)[0]],
                                      modelcal=dict(interval=16, tol=1e-12, maxiter=2000, model=ideal.directory),
                                      chunk_gb=chunk_gb)


def _chunk_days(routes):
    """Two days of 4 / 5 turn at this telescope with one day's noise and interference bursts; (directories, nsamples)."""
    from driftscan_amd import skysim, timestream

    nsamp = int(0.8 * timestream.T_SIDEREAL_DAY / CHUNK_CADENCE)
    if "chunk_days" not in routes:
        dirs = [str(routes["d"] / ("chunk_day%d" % i)) for i in range(2)]
        timestream.simulate_days(routes["pm"], dirs, (0.3, 2.7), nsamp, CHUNK_CADENCE, seed=3,
                                 rfi=skysim.RFIModel(fraction=0.005, burst=4, amplitude=30.0, seed=11))
        routes["chunk_days"] = dirs
    return routes["chunk_days"], nsamp


def _chunked_sidereal(routes, name, chunk_gb):
    from driftscan_amd import timestream

    tel, ntime = routes["tel"], routes["ntime"]
    dirs, nsamp = _chunk_days(routes)
    if chunk_gb is None:   # two frequencies fit, the third makes the second chunk: the driver's own estimate per frequency
        chunk_gb = 2.5 * int(tel.npairs) * (32.0 * nsamp + 36.0 * ntime + 16.0 * ntime) / 2.0**30
    return timestream.sidereal_stack(routes["pm"], dirs, str(routes["d"] / name), ntime=ntime, a=3, rfi=dict(CHUNK_RFI),
                                     chunk_gb=chunk_gb)


def _chunked_rfi(routes, name, chunk_gb):
    from driftscan_amd import timestream

    dirs, nsamp = _chunk_days(routes)
    if chunk_gb is None:
        chunk_gb = 2.5 * int(routes["tel"].npairs) * nsamp * 32.0 / 2.0**30
    return timestream.rfi_flag(routes["pm"], dirs[0], str(routes["d"] / name), chunk_gb=chunk_gb, **CHUNK_RFI)


@pytest.mark.parametrize("driver,small", [(_chunked_redundant, 1e-9), (_chunked_model, 1e-9), (_chunked_sidereal, None),
                                          (_chunked_rfi, None)], ids=["redundant", "model", "sidereal", "rfi"])
def test_the_chunks_of_frequencies_change_no_bit(routes, driver, small):
    """`stack_baselines` (flagged, one dead feed, calibrate="redundant" with the reference of the files, and
    calibrate="model") with all three frequencies in one chunk and with one frequency per chunk, `sidereal_stack` and
    `rfi_flag` in one chunk and in two: every dataset of every output file is bitwise equal.  Every kernel of the chain
    documents that the bits of a row, sample or interval do not depend on the batch; this holds the drivers to it."""
    from driftscan_amd import timestream

    log = {}
    timestream.sim_log = log
    try:
        one = driver(routes, driver.__name__ + "_one", 4.0)
        many = driver(routes, driver.__name__ + "_many", small)
    finally:
        timestream.sim_log = None
    assert log["read"] > 0 and log["write"] > 0
    _same_directories(one, many, routes["tel"])
