"""Sky-model gain calibration on the device: one iteration of `Context.modelcal_solve` against
extended precision on the tables of tests/redcal_cases.py, convergence on noise-free data, stationarity with noise,
determinism, refusals, and the routes `stack_baselines(calibrate="model")` and `redcal={"reference": "model"}` on the small
polarised cylinder of tests/test_gpu_stack.py."""
import logging

import numpy as np
import pytest

import gains_cases as gc
import modelcal_cases as mc
import redcal_cases as rc
import stack_cases as sc

pytestmark = pytest.mark.gpu

EPS = mc.EPS
NAMES = ("g", "iters", "step", "chi2", "gweight")


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _ts():
    from driftscan_amd import timestream

    return timestream


def _guarded_out(ctx, nreal, nf, nfeed, nint):
    """NaN-poisoned (int32: -7) buffers with a guard realisation before and after the outputs; (buffers, out=)."""
    shapes = dict(g=(nf, nfeed, nint), iters=(nf, nint), step=(nf, nint), chi2=(nf, nint), gweight=(nf, nfeed, nint))
    bufs = {}
    for k, shp in shapes.items():
        if k == "iters":
            bufs[k] = ctx.to_device(np.full((nreal + 2,) + shp, -7, dtype=np.int32))
        else:
            bufs[k] = ctx.to_device(np.full((nreal + 2,) + shp, np.nan, dtype=np.complex128 if k == "g" else np.float64))
    return bufs, {k: b[1:-1] for k, b in bufs.items()}


def _guards_untouched(ctx, bufs):
    for k, b in bufs.items():
        h = ctx.to_host(b)
        for edge in (h[0], h[-1]):
            if not (np.all(edge == -7) if k == "iters" else np.all(np.isnan(edge.real))):
                return False
    return True


def _solve(ctx, vis, model, off, mem, interval, w=None, fw=None, g0=None, active=None, **kw):
    """`modelcal_solve` inside guard rows; the five outputs on the host."""
    nreal, nf, _, ntime = vis.shape
    nfeed = g0.shape[2] if g0 is not None else (len(fw) if fw is not None else int(mem.max()) + 1)
    dev = lambda a: None if a is None else ctx.to_device(np.ascontiguousarray(a))
    bufs, out = _guarded_out(ctx, nreal, nf, nfeed, mc.nint_of(ntime, interval))
    g, info = ctx.modelcal_solve(dev(vis), dev(model), off, mem, interval, w=dev(w), feed_weight=fw, g0=dev(g0),
                                 active=dev(active), out=out, **kw)
    assert g.data_ptr() == out["g"].data_ptr() and info["gweight"].data_ptr() == out["gweight"].data_ptr()
    assert sorted(info) == sorted(NAMES[1:])
    assert _guards_untouched(ctx, bufs)
    return {k: ctx.to_host(bufs[k])[1:-1] for k in NAMES}


def _one_step(ctx, table, cases, interval):
    _, off, mem = table
    worst = 0.0
    for vis, model, w, fw, g0 in cases:
        ex = mc.step_exact(vis, model, off, mem, g0, interval, w=w, feed_weight=fw)
        got = _solve(ctx, vis, model, off, mem, interval, w=w, fw=fw, g0=g0, damping=mc.DAMPING, tol=0.0, maxiter=1)
        worst = max(worst, mc.check_step(got["g"], ex))
        assert np.all(got["iters"] == 1)
        assert np.all(np.abs(got["step"] - ex["step"]) <= 1e-12 * ex["step"].astype(np.float64) + 64 * EPS)
    return worst


@pytest.mark.parametrize("ntime,interval", mc.STEP_SHAPES)
@pytest.mark.parametrize("name", ["two", "line3", "grid43", "line70", "cyl12"])
def test_one_step_against_extended_precision(name, ntime, interval):
    """maxiter = 1, tol = 0 from a random g0 within 20 % and 0.5 rad of one: g within K (d_a L_q + 8) eps [sum omega |V|
    |z| / den + |g_a|] of `modelcal_step_host` in np.clongdouble, K = 4; gains whose denominator is 0 (a dead feed, wholly
    flagged incidences) are g0 bit for bit.  nf, nreal in {1, 3}, m_nreal and w_nreal in {1, nreal}, with and without
    weights and feed weights, one dead feed, NaN guard rows around every output; L = 1, ragged last intervals, L = 64."""
    worst = _one_step(_ctx(), mc.tables()[name], mc.step_cases(name, ntime, interval), interval)
    print("modelcal step %s, ntime %d, interval %d: max err / bound at K = %d: %.3g" % (name, ntime, interval, mc.K_MODELCAL, worst))
    assert worst < 0.5                                           # the rule of section 4.16 that fixes K


@pytest.mark.parametrize("nfeed", sorted(sc.TILE_NFEED))
def test_one_step_on_many_feeds(nfeed):
    """The random partitions of stack_cases, up to 2100 feeds (33 KiB of staged gains): ntime = 17, interval 4."""
    table = sc.tile_table(nfeed)
    worst = _one_step(_ctx(), table, mc.step_cases(table, 17, 4, (mc.STEP_BATCHES[2], mc.STEP_BATCHES[5], mc.STEP_BATCHES[0])), 4)
    print("modelcal step %d feeds: max err / bound at K = %d: %.3g" % (nfeed, mc.K_MODELCAL, worst))
    assert worst < 0.5


def test_a_single_cross_pair_is_constrained_here():
    """`two`: one class of one cross pair moves both gains, where the redundant solver leaves them at g0."""
    ctx = _ctx()
    nfeed, off, mem = mc.tables()["two"]
    vis, model, w, fw, g0 = next(iter(mc.step_cases("two", 5, 1, mc.STEP_BATCHES[:1])))
    got = _solve(ctx, vis, model, off, mem, 1, g0=g0, maxiter=1, tol=0.0)
    assert np.all(got["g"] != g0) and np.all(got["step"] > 0) and np.all(got["gweight"] > 0)
    dev = ctx.to_device
    red, _, _ = ctx.redcal_solve(dev(vis), off, mem, g0=dev(g0), maxiter=1, tol=0.0)
    assert np.array_equal(ctx.to_host(red), g0)


@pytest.mark.parametrize("name", mc.SOLVABLE)
def test_noise_free_data_converge(name):
    """V = g_true conj(g_true) M with gains constant per interval, a sixth of the samples flagged, tol = 1e-12, maxiter =
    2000: every interval converges, |iters_dev - iters_host| <= 2, after `modelcal_fix_phase(ref=g_true)` max |g - g_true|
    <= 4 max(host value, tol), and r_dev <= 4 max(r_host, tol)."""
    ctx = _ctx()
    _, off, mem = mc.tables()[name]
    c = mc.converged_case(name)
    L, tol, maxiter = (mc.CONVERGED[k] for k in ("interval", "tol", "maxiter"))
    got = _solve(ctx, c["vis"], c["model"], off, mem, L, w=c["w"], tol=tol, maxiter=maxiter)
    r = mc.residual(c["vis"], c["model"], off, mem, got["g"], L)
    dg = float(np.abs(_ts().modelcal_fix_phase(got["g"], c["comp"], ref=c["gt"]) - c["gt"]).max())
    di = np.abs(got["iters"].astype(np.int64) - c["info"]["iters"])
    print("modelcal %s: iterations %d to %d (host %d to %d, max difference %d), r = %.3g (host %.3g), max |g - g_true| = "
          "%.3g (host %.3g)" % (name, got["iters"].min(), got["iters"].max(), c["info"]["iters"].min(),
                                c["info"]["iters"].max(), di.max(), r, c["r"], dg, c["dg"]))
    assert np.all(got["step"] < tol) and np.all(got["iters"] < maxiter)
    assert di.max() <= 2
    assert dg <= 4 * max(c["dg"], tol)
    assert r <= 4 * max(c["r"], tol)


def test_stationarity_chi2_and_gweight_with_noise():
    """`grid43`, noise at 1 % of |V|, interval 8: |gh_a - g_a| / |g_a| <= tol / damping at the result; chi2 within
    K (nmem L + 8) eps sum omega |V|^2 and gweight within K (d_a L_q + 8) eps (relative) of their long-double values."""
    ctx = _ctx()
    ts = _ts()
    nfeed, off, mem = mc.tables()["grid43"]
    rng = np.random.default_rng(11)
    ntime, L = 21, 8
    vis, model, _ = mc.noise_free(rng, nfeed, off, mem, (2, 1), ntime, L)
    vis = vis + 0.01 * np.abs(vis) * gc.crandn(rng, *vis.shape) / np.sqrt(2)
    w = rc.weights(rng, (1, 1, mem.shape[0], ntime))
    got = _solve(ctx, vis, model, off, mem, L, w=w, damping=mc.DAMPING, tol=mc.TOL, maxiter=mc.MAXITER)
    assert np.all(got["step"] < mc.TOL) and np.all(got["iters"] < mc.MAXITER) and np.all(got["chi2"] > 0)
    ex = mc.step_exact(vis, model, off, mem, got["g"], L, w=w, damping=1.0)
    drift = float((np.abs(ex["g"] - got["g"]) / np.abs(got["g"])).max())
    print("stationarity: max |gh - g| / |g| = %.3g (tol / damping = %.3g)" % (drift, mc.TOL / mc.DAMPING))
    assert drift <= mc.TOL / mc.DAMPING
    exact = ts.modelcal_chi2_host(vis, model, off, mem, got["g"], L, w=w, dtype=np.clongdouble)
    err = np.abs(got["chi2"] - exact).astype(np.float64)
    bound = mc.chi2_bound(vis, off, mem, L, w=w, nfeed=nfeed)
    print("chi2: max err / bound = %.3g; gweight: max err / bound = %.3g" % ((err / bound).max(), mc.check_gweight(got["gweight"], ex)))
    assert np.all(err <= bound)


def test_an_interval_has_the_same_bits_in_any_company():
    """One interval solved alone; as interval 2 of 5; in a batch of 3 x 3; with m_nreal and w_nreal 1 and nreal; beside a
    neighbour that converges far earlier: all five outputs compared with ==.  An inactive interval returns g0, 0, 0, 0, 0
    bit for bit and its neighbours are unchanged."""
    ctx = _ctx()
    nfeed, off, mem = mc.tables()["grid43"]
    nmem = mem.shape[0]
    rng = np.random.default_rng(17)
    L, nint = 8, 5
    ntime = L * (nint - 1) + 3                                    # the last interval is ragged
    vis, model, gq = mc.noise_free(rng, nfeed, off, mem, (3, 3), ntime, L)
    vis = vis + 0.01 * np.abs(vis) * gc.crandn(rng, *vis.shape)
    w1 = rng.uniform(0.5, 1.5, size=(1, 3, nmem, ntime))
    model1 = model[:1]
    g0 = np.ones((3, 3, nfeed, nint), dtype=np.complex128)
    # the neighbour: interval 3 of (0, 0) is noise-free against model1 and starts at its solution up to 1e-9
    spread = gq[0, 0][:, np.arange(ntime) // L]
    quick = _ts().vis_expand_host(model1[0, 0], off, mem, g=spread)
    vis[0, 0, :, 3 * L : 4 * L] = quick[:, 3 * L : 4 * L]
    g0[0, 0, :, 3] = gq[0, 0, :, 3] * (1 + 1e-9)
    kw = dict(damping=mc.DAMPING, tol=mc.TOL, maxiter=mc.MAXITER)
    full = _solve(ctx, vis, model1, off, mem, L, w=w1, g0=g0, **kw)
    assert np.all(full["step"][0, 0, 2:4] < mc.TOL)
    assert full["iters"][0, 0, 2] - full["iters"][0, 0, 3] > 10, full["iters"][0, 0]

    def same(part, sel):
        for k in NAMES:
            assert np.array_equal(part[k], full[k][sel]), k

    one = (slice(0, 1), slice(0, 1))
    t2 = slice(2 * L, 3 * L)
    alone = _solve(ctx, vis[one][..., t2], model1[:, :1, :, t2], off, mem, L, w=w1[:, :1, :, t2], g0=g0[one][..., 2:3], **kw)
    for k in NAMES:
        assert np.array_equal(alone[k][..., 0], full[k][one][..., 2]), k
    same(_solve(ctx, vis[one], model1[:, :1], off, mem, L, w=w1[:, :1], g0=g0[one], **kw), one)      # interval 2 of 5
    same(_solve(ctx, vis[1:2, 2:3], model1[:, 2:3], off, mem, L, w=w1[:, 2:3], g0=g0[1:2, 2:3], **kw), (slice(1, 2), slice(2, 3)))
    each = lambda a: np.ascontiguousarray(np.broadcast_to(a, (3,) + a.shape[1:]))
    same(_solve(ctx, vis, each(model1), off, mem, L, w=each(w1), g0=g0, **kw), (slice(None), slice(None)))   # m_nreal = w_nreal = nreal
    same(_solve(ctx, vis, each(model1), off, mem, L, w=w1, g0=g0, **kw), (slice(None), slice(None)))
    # the ragged last interval alone
    t4 = slice(4 * L, ntime)
    last = _solve(ctx, vis[one][..., t4], model1[:, :1, :, t4], off, mem, L, w=w1[:, :1, :, t4], g0=g0[one][..., 4:5], **kw)
    for k in NAMES:
        assert np.array_equal(last[k][..., 0], full[k][one][..., 4]), k
    # interval 1 of frequency 2 inactive: g0, 0, 0, 0, 0 there, every other interval as before
    active = np.ones((3, nint), dtype=np.int32)
    active[2, 1] = 0
    g0r = g0 * rc.gains_near_one(rng, 3, 3, nfeed, 1)
    ref = _solve(ctx, vis, model1, off, mem, L, w=w1, g0=g0r, **kw)
    part = _solve(ctx, vis, model1, off, mem, L, w=w1, g0=g0r, active=active, **kw)
    on = np.ones((3, 3, nint), dtype=bool)
    on[:, 2, 1] = False
    assert np.array_equal(part["g"][:, 2, :, 1], g0r[:, 2, :, 1]) and np.all(part["gweight"][:, 2, :, 1] == 0)
    for k in ("iters", "step", "chi2"):
        assert np.all(part[k][~on] == 0), k
        assert np.array_equal(part[k][on], ref[k][on]), k
    for k in ("g", "gweight"):
        assert np.array_equal(np.moveaxis(part[k], 2, -1)[on], np.moveaxis(ref[k], 2, -1)[on]), k


def test_out_of_iterations_is_reported_not_refused():
    ctx = _ctx()
    _, off, mem = mc.tables()["cyl12"]
    c = mc.converged_case("cyl12")
    L = mc.CONVERGED["interval"]
    got = _solve(ctx, c["vis"], c["model"], off, mem, L, w=c["w"], tol=1e-13, maxiter=3)
    assert np.all(got["iters"] == 3) and np.all(got["step"] >= 1e-13) and np.all(np.isfinite(got["g"]))
    host, _ = _ts().modelcal_solve_host(c["vis"], c["model"], off, mem, L, w=c["w"], tol=1e-13, maxiter=3)
    assert np.abs(got["g"] - host).max() <= 1e-12
    # more iterations than one check of the host: a late and an early interval
    got = _solve(ctx, c["vis"], c["model"], off, mem, L, w=c["w"], tol=1e-6, maxiter=40)
    host, info = _ts().modelcal_solve_host(c["vis"], c["model"], off, mem, L, w=c["w"], tol=1e-6, maxiter=40)
    assert np.abs(got["iters"].astype(np.int64) - info["iters"]).max() <= 2 and np.abs(got["g"] - host).max() <= 1e-5


def test_refusals_leave_the_outputs_alone():
    """Each refusal returns non-zero with a message naming dm_modelcal_solve and writes nothing."""
    from driftscan_amd import _lib

    ctx = _ctx()
    nfeed, off, mem = mc.tables()["line3"]
    npairs, nmem = off.shape[0] - 1, mem.shape[0]
    ntime, L, nint = 5, 2, 3
    vis = ctx.to_device(np.ones((1, 1, nmem, ntime), dtype=np.complex128))
    model = ctx.to_device(np.ones((1, 1, npairs, ntime), dtype=np.complex128))
    bufs, out = _guarded_out(ctx, 1, 1, nfeed, nint)
    for k in NAMES:
        out[k].fill_(7)
    kw = dict(out=out)
    for bad, match in ((dict(damping=0.0), "damping"), (dict(damping=1.25), "damping"), (dict(damping=float("nan")), "damping"),
                       (dict(tol=-1e-3), "tol"), (dict(tol=float("inf")), "tol"), (dict(tol=float("nan")), "tol"),
                       (dict(maxiter=0), "maxiter"), (dict(feed_weight=[1.0, -1.0, 1.0]), "feed weight 1 is negative")):
        with pytest.raises(_lib.DriftMIError, match="dm_modelcal_solve.*" + match):
            ctx.modelcal_solve(vis, model, off, mem, L, **dict(kw, **bad))
    with pytest.raises(_lib.DriftMIError, match="dm_modelcal_solve.*class 1 is empty"):
        ctx.modelcal_solve(vis, model, [0, 3, 3, 6], mem, L, **kw)
    with pytest.raises(_lib.DriftMIError, match="dm_modelcal_solve.*does not fit"):      # the 64 KiB of one interval's gains
        ctx.modelcal_solve(ctx.to_device(np.ones((1, 1, 1, 1), dtype=np.complex128)),
                           ctx.to_device(np.ones((1, 1, 1, 1), dtype=np.complex128)), [0, 1], [[4096, 0]], 1)
    with pytest.raises(_lib.DriftMIError, match="dm_modelcal_solve.*does not fit"):      # what dm_vis_stack refuses with gains
        ctx.modelcal_solve(ctx.to_device(np.ones((1, 1, 1, 1), dtype=np.complex128)),
                           ctx.to_device(np.ones((1, 1, 1, 1), dtype=np.complex128)), [0, 1], [[10240, 0]], 1)
    # through the C entry point: negative sizes, null pointers with work to do, overlapping buffers, no-ops
    lib, h, P = ctx.lib, ctx.h, ctx.ptr
    offa, offp = _lib._iarr(off)
    mema, memp = _lib._iarr(mem)
    bad_mem = mem.copy()
    bad_mem[4] = (5, 0)
    bada, badp = _lib._iarr(bad_mem)

    def call(nreal=1, nf=1, nt=ntime, interval=L, v=vis, m=model, w=None, g0=None, act=None, w_nreal=1, m_nreal=1, mp=memp, **o):
        o = dict(out, **o)
        return lib.dm_modelcal_solve(h, nreal, w_nreal, m_nreal, nf, nfeed, npairs, nt, interval, offp, mp, P(v), P(m), P(w),
                                     None, P(g0), P(act), 0.5, 1e-10, 10, P(o["g"]), P(o["iters"]), P(o["step"]),
                                     P(o["chi2"]), P(o["gweight"]), 0)

    def last():
        return lib.dm_last_error(h).decode()

    assert call(mp=badp) != 0 and "dm_modelcal_solve: member 4 names feed 5 of 3" in last()
    assert call(nt=-1) != 0 and "dm_modelcal_solve: negative size" in last()
    assert call(nf=-1) != 0 and "dm_modelcal_solve: negative size" in last()
    assert call(interval=0) != 0 and "dm_modelcal_solve: interval must be at least 1" in last()
    assert call(interval=-3) != 0 and "dm_modelcal_solve: interval must be at least 1" in last()
    assert call(v=None) != 0 and "dm_modelcal_solve: null pointer" in last()
    assert call(m=None) != 0 and "dm_modelcal_solve: null pointer" in last()
    for k in NAMES:
        assert call(**{k: None}) != 0 and "dm_modelcal_solve: null pointer" in last(), k
    assert call(g=vis) != 0 and "dm_modelcal_solve: g shares an element with vis" in last()
    assert call(gweight=model) != 0 and "dm_modelcal_solve: gweight shares an element with model" in last()
    wdev = ctx.to_device(np.ones((1, 1, nmem, ntime)))
    assert call(w=wdev, w_nreal=2) != 0 and "dm_modelcal_solve: w_nreal" in last()
    assert call(m_nreal=2) != 0 and "dm_modelcal_solve: m_nreal" in last()
    assert call(w=wdev, step=wdev) != 0 and "dm_modelcal_solve: step shares an element with w" in last()
    g0 = ctx.to_device(np.ones((1, 1, nfeed, nint), dtype=np.complex128))
    assert call(g0=g0, g=g0) != 0 and "dm_modelcal_solve: g shares an element with g0" in last()
    act = ctx.to_device(np.ones((1, nint), dtype=np.int32))
    assert call(act=act, iters=act) != 0 and "dm_modelcal_solve: iters shares an element with active" in last()
    assert call(chi2=out["step"]) != 0 and "dm_modelcal_solve: chi2 shares an element with step" in last()
    assert call(gweight=out["chi2"]) != 0 and "dm_modelcal_solve: gweight shares an element with chi2" in last()
    assert call(nreal=0) == 0 and call(nf=0) == 0 and call(nt=0) == 0                             # no-ops
    # the wrapper's own checks
    for bad in (lambda: ctx.modelcal_solve(vis, model, off, mem[:-1], L),
                lambda: ctx.modelcal_solve(vis, model[:, :, :-1], off, mem, L),
                lambda: ctx.modelcal_solve(vis, model, off, mem, L, w=ctx.to_device(np.ones((2, 1, nmem, ntime)))),
                lambda: ctx.modelcal_solve(vis, model, off, mem, L, g0=ctx.to_device(np.ones((1, 1, nfeed, ntime), dtype=np.complex128))),
                lambda: ctx.modelcal_solve(vis, model, off, mem, L, active=ctx.to_device(np.ones((1, nint)))),
                lambda: ctx.modelcal_solve(vis, model, off, mem, L, out=dict(g=ctx.empty((1, 1, nfeed, nint + 1), np.complex128))),
                lambda: ctx.modelcal_solve(vis, model, off, mem, L, out=dict(y=out["g"]))):
        with pytest.raises(ValueError):
            bad()
    ctx.sync()
    assert _guards_untouched(ctx, bufs)
    for k in NAMES:
        assert np.all(ctx.to_host(bufs[k])[1:-1] == 7), k
    assert np.all(ctx.to_host(vis) == 1.0) and np.all(ctx.to_host(model) == 1.0) and np.all(ctx.to_host(wdev) == 1.0)
    assert np.all(ctx.to_host(g0) == 1.0) and np.all(ctx.to_host(act) == 1)


# ---- the routes: the fixtures of tests/test_gpu_stack.py (12 feeds, 3 frequencies, ntime = 183) ---------------------------
from test_gpu_stack import prod, routes, skyfile  # noqa: E402,F401

INTERVAL = 16
SOLVER = dict(interval=INTERVAL, tol=1e-12, maxiter=2000)
REDCAL = dict(tol=1e-10, maxiter=2000)


@pytest.fixture(scope="module")
def sky_model(routes):
    """Unstacked data with explicit gains that are constant over intervals of 16 samples (amplitudes within 5 %, phases
    within 0.1 rad, ndays = 0), (a) stacked with `calibrate="model"` against the `ideal` directory, and the host's residual
    of the same data."""
    from driftscan_amd import storage, timestream

    pm, d, tel, ntime, kw, ideal = (routes[k] for k in ("pm", "d", "tel", "ntime", "kw", "ideal"))
    rng = np.random.default_rng(23)
    nint = mc.nint_of(ntime, INTERVAL)
    gq = (1 + 0.05 * rng.uniform(-1, 1, (tel.nfreq, tel.nfeed, nint))) * np.exp(0.1j * rng.uniform(-1, 1, (tel.nfreq, tel.nfeed, nint)))
    gains = np.ascontiguousarray(gq[..., np.arange(ntime) // INTERVAL])
    uns = timestream.simulate_ensemble(pm, str(d / "mc_uns"), 1, gains=gains, unstacked=True, **kw)[0]
    a = timestream.stack_baselines(pm, uns.directory, str(d / "mc_model"), calibrate="model",
                                   modelcal=dict(SOLVER, model=ideal.directory))
    off, mem = tel.redundant_pairs()
    vis = []
    for fi in range(tel.nfreq):
        with storage.File(uns._ffile(fi), "r") as f:
            vis.append(f["timestream"][:])
    vis = np.stack(vis)
    model = np.stack([ideal.timestream_f(fi) for fi in range(tel.nfreq)])
    g, info = timestream.modelcal_solve_host(vis, model, off, mem, INTERVAL, nfeed=int(tel.nfeed), tol=SOLVER["tol"],
                                             maxiter=SOLVER["maxiter"])
    assert np.all(info["step"] < SOLVER["tol"])
    return dict(uns=uns, a=a, vis=vis, model=model, gains=gains, gq=gq, iters_host=info["iters"],
                r_host=mc.residual(vis, model, off, mem, g, INTERVAL))


def _route_bound(tel, want, r_host, tol):
    """Section 4.17's round-trip bound plus 4 max(r_host, tol) max |v|."""
    nmax = int(np.diff(tel.redundant_pairs()[0]).max())
    scale = np.abs(want).max()
    return (8 * EPS + 2 * sc.K_STACK * (nmax + 4) * EPS) * scale + 4 * max(r_host, tol) * scale


def test_calibration_against_the_model_reproduces_the_ideal_telescope(routes, sky_model):
    """(a): `calibrate="model"` with the `ideal` directory as the model gives the data of the telescope without gain
    errors within the round-trip bound of section 4.17 plus 4 max(r_host, tol) max |v|; no `weight` is written; the four
    new datasets are."""
    from driftscan_amd import storage

    tel, ntime, ideal = (routes[k] for k in ("tel", "ntime", "ideal"))
    a, nint = sky_model["a"], mc.nint_of(ntime, INTERVAL)
    for fi in range(tel.nfreq):
        v, want = a.timestream_f(fi), ideal.timestream_f(fi)
        bound = _route_bound(tel, want, sky_model["r_host"], SOLVER["tol"])
        with storage.File(a._ffile(fi), "r") as f:
            assert "weight" not in f and "redcal_iters" not in f
            gs, gq, its, valid = (f[k][:] for k in ("gain_solution", "modelcal_gain", "modelcal_iters", "modelcal_valid"))
        assert gs.shape == (tel.nfeed, ntime) and gq.shape == (tel.nfeed, nint) and its.shape == (nint,) and valid.shape == (nint,)
        assert np.all(valid == 1) and np.all(its < SOLVER["maxiter"]) and np.all(its > 0)
        assert np.array_equal(gs, gq[:, np.arange(ntime) // INTERVAL])
        assert np.abs(its.astype(np.int64) - sky_model["iters_host"][fi]).max() <= 2
        # the solved gains are the true ones up to the one phase per interval the model leaves free
        turn = (gq * sky_model["gq"][fi].conj()).sum(axis=0)
        dg = np.abs(gq * (turn.conj() / np.abs(turn)) - sky_model["gq"][fi]).max()
        print("frequency %d: max |delta| / bound = %.3g, max |g - g_true| = %.3g, iterations %d to %d, r_host = %.3g"
              % (fi, np.abs(v - want).max() / bound, dg, its.min(), its.max(), sky_model["r_host"]))
        assert np.abs(v - want).max() <= bound


def test_the_model_as_the_reference_of_the_redundant_route(routes, sky_model):
    """(b): `calibrate="redundant"` with `reference="model"` meets the bound of (a) with the redundant solver's tolerance
    and r_host the larger host residual of the two solvers that run (the redundant one's, 1e-9 at tol = 1e-10 as in section
    4.18, decides it); the same data with `reference=None` misses it by more than a factor 100, so the reference is what
    does it."""
    from driftscan_amd import storage, timestream

    pm, d, tel, ntime, ideal = (routes[k] for k in ("pm", "d", "tel", "ntime", "ideal"))
    uns = sky_model["uns"]
    b = timestream.stack_baselines(pm, uns.directory, str(d / "mc_red_model"), calibrate="redundant",
                                   redcal=dict(REDCAL, reference="model"), modelcal=dict(SOLVER, model=ideal.directory))
    ones = timestream.stack_baselines(pm, uns.directory, str(d / "mc_red_ones"), calibrate="redundant", redcal=dict(REDCAL))
    # r_host of this route: both solvers run, so the larger of the two host residuals, each at its own tolerance
    off, mem = tel.redundant_pairs()
    gh, yh, info = timestream.redcal_solve_host(sky_model["vis"], off, mem, nfeed=int(tel.nfeed), **REDCAL)
    assert np.all(info["step"] < REDCAL["tol"])
    r_host = max(sky_model["r_host"], rc.residual(sky_model["vis"], off, mem, gh, yh))
    print("r_host: model %.3g, redundant %.3g" % (sky_model["r_host"], r_host))
    for fi in range(tel.nfreq):
        want = ideal.timestream_f(fi)
        bound = _route_bound(tel, want, r_host, REDCAL["tol"])
        eb, eo = np.abs(b.timestream_f(fi) - want).max(), np.abs(ones.timestream_f(fi) - want).max()
        with storage.File(b._ffile(fi), "r") as f:
            assert "weight" not in f
            assert sorted(k for k in f.keys() if "cal" in k or "gain" in k) == ["gain_solution", "modelcal_gain", "modelcal_iters",
                                                                                "modelcal_valid", "redcal_iters"]
            assert f["gain_solution"].shape == (tel.nfeed, ntime) and np.all(f["modelcal_valid"][:] == 1)
            assert np.all(f["redcal_iters"][:] < REDCAL["maxiter"])
        print("frequency %d: reference model max |delta| / bound = %.3g, reference ones %.3g" % (fi, eb / bound, eo / bound))
        assert eb <= bound
        assert eo > 100 * bound


def test_intervals_without_model_take_the_nearest_valid_gains(routes, sky_model, caplog):
    """(c): a model that is zero outside the intervals 3 to 6 of the day, `min_model` = 0.1: only those intervals are
    solved and valid, the others carry the gains of the nearest of them, and the invalid ones are counted."""
    from driftscan_amd import storage, timestream

    pm, d, tel, ntime = (routes[k] for k in ("pm", "d", "tel", "ntime"))
    nint = mc.nint_of(ntime, INTERVAL)
    window = np.zeros(nint, dtype=bool)
    window[3:7] = True
    model = sky_model["model"] * window[np.arange(ntime) // INTERVAL]
    timestream.sim_log = {}
    try:
        with caplog.at_level(logging.WARNING, logger="driftscan_amd.timestream"):
            c = timestream.stack_baselines(pm, sky_model["uns"].directory, str(d / "mc_window"), calibrate="model",
                                           modelcal=dict(SOLVER, model=model, min_model=0.1))
        log = timestream.sim_log
    finally:
        timestream.sim_log = None
    lost = tel.nfreq * int((~window).sum())
    assert log["modelcal_invalid"] == lost and log["modelcal"] > 0
    assert any("%d of %d solution intervals" % (lost, tel.nfreq * nint) in r.getMessage() for r in caplog.records)
    src = np.array([3, 3, 3, 3, 4, 5, 6, 6, 6, 6, 6, 6])
    for fi in range(tel.nfreq):
        with storage.File(c._ffile(fi), "r") as f, storage.File(sky_model["a"]._ffile(fi), "r") as fa:
            gs, gq, its, valid = (f[k][:] for k in ("gain_solution", "modelcal_gain", "modelcal_iters", "modelcal_valid"))
            full = fa["modelcal_gain"][:]
        assert np.array_equal(valid.astype(bool), window) and np.all(its[~window] == 0) and np.all(its[window] > 0)
        assert np.array_equal(gq[:, window], full[:, window])                # an interval is a problem of its own
        assert np.array_equal(gs, gq[:, src[np.arange(ntime) // INTERVAL]])
        t = window[np.arange(ntime) // INTERVAL]
        assert np.array_equal(c.timestream_f(fi)[:, t], sky_model["a"].timestream_f(fi)[:, t])


def test_the_pipeline_entry_gives_the_same_directory(routes, sky_model, tmp_path):
    """(d): `stack_from: {calibrate: model, modelcal: {...}}` of the pipeline produces the files of (a)."""
    import yaml

    from driftscan_amd import pipeline, storage

    d, tel, ideal = (routes[k] for k in ("d", "tel", "ideal"))
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=False, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=False),
                timestreams=[dict(name="s", directory=str(tmp_path / "pipe_model"),
                                  stack_from=dict(directory=sky_model["uns"].directory, calibrate="model",
                                                  modelcal=dict(SOLVER, model=ideal.directory)))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = pipeline.PipelineManager.from_configfile(str(cfile))
    p.generate()
    s, a = p.timestreams["s"], sky_model["a"]
    for fi in range(tel.nfreq):
        assert np.array_equal(s.timestream_f(fi), a.timestream_f(fi))
        with storage.File(s._ffile(fi), "r") as f, storage.File(a._ffile(fi), "r") as h:
            assert sorted(f.keys()) == sorted(h.keys()) and "weight" not in f
            for k in ("gain_solution", "modelcal_gain", "modelcal_iters", "modelcal_valid"):
                assert np.array_equal(f[k][:], h[k][:]), k


def test_a_model_on_other_sample_positions_is_refused(routes, sky_model):
    """(e): a model directory with another `phi` raises ValueError; so do an unknown key, a missing model and a
    `modelcal` without a route that uses it."""
    from driftscan_amd import timestream

    pm, d, tel, ntime, ideal = (routes[k] for k in ("pm", "d", "tel", "ntime", "ideal"))
    uns = sky_model["uns"]
    moved = timestream.Timestream(str(d / "mc_moved"), pm)
    tphi = np.linspace(0, 2 * np.pi, ntime, endpoint=False) + 1e-3
    for fi in range(tel.nfreq):
        timestream._write_sim_file(moved, fi, ideal.timestream_f(fi), tphi)
    moved.save()
    out = str(d / "mc_bad")
    with pytest.raises(ValueError, match="phi"):
        timestream.stack_baselines(pm, uns.directory, out, calibrate="model", modelcal=dict(SOLVER, model=moved.directory))
    with pytest.raises(ValueError, match="modelcal holds"):
        timestream.stack_baselines(pm, uns.directory, out, calibrate="model", modelcal=dict(SOLVER, model=ideal.directory, floor=1))
    with pytest.raises(ValueError, match="model"):
        timestream.stack_baselines(pm, uns.directory, out, calibrate="model", modelcal=dict(SOLVER))
    with pytest.raises(ValueError, match="modelcal belongs"):
        timestream.stack_baselines(pm, uns.directory, out, calibrate="file", modelcal=dict(SOLVER, model=ideal.directory))
    with pytest.raises(ValueError, match="not \\(nfreq, npairs, ntime\\)"):
        timestream.stack_baselines(pm, uns.directory, out, calibrate="model", modelcal=dict(SOLVER, model=sky_model["model"][:, :, :-1]))
