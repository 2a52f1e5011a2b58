"""Redundant-baseline calibration on the device: one iteration of `Context.redcal_solve` against
extended precision on the tables of tests/redcal_cases.py, convergence on noise-free data, stationarity with noise,
determinism, refusals, and `stack_baselines(calibrate="redundant")` on the small polarised cylinder of
tests/test_gpu_stack.py."""
import logging

import numpy as np
import pytest

import gains_cases as gc
import redcal_cases as rc
import stack_cases as sc

pytestmark = pytest.mark.gpu

EPS = rc.EPS
NAMES = ("g", "y", "iters", "step", "chi2")


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _guarded_out(ctx, nreal, nf, nfeed, npairs, ntime):
    """NaN-poisoned (int32: -7) buffers with a guard realisation before and after the outputs; (buffers, out=)."""
    shapes = dict(g=(nf, nfeed, ntime), y=(nf, npairs, ntime), iters=(nf, ntime), step=(nf, ntime), chi2=(nf, ntime))
    bufs = {}
    for k, shp in shapes.items():
        if k == "iters":
            bufs[k] = ctx.to_device(np.full((nreal + 2,) + shp, -7, dtype=np.int32))
        else:
            bufs[k] = ctx.to_device(np.full((nreal + 2,) + shp, np.nan, dtype=np.complex128 if k in ("g", "y") else np.float64))
    return bufs, {k: b[1:-1] for k, b in bufs.items()}


def _guards_untouched(ctx, bufs):
    for k, b in bufs.items():
        h = ctx.to_host(b)
        for edge in (h[0], h[-1]):
            if not (np.all(edge == -7) if k == "iters" else np.all(np.isnan(edge.real))):
                return False
    return True


def _solve(ctx, vis, off, mem, w=None, fw=None, g0=None, **kw):
    """`redcal_solve` inside guard rows; the five outputs on the host."""
    nreal, nf, _, ntime = vis.shape
    nfeed = g0.shape[2] if g0 is not None else (len(fw) if fw is not None else int(mem.max()) + 1)
    dev = lambda a: None if a is None else ctx.to_device(a)
    bufs, out = _guarded_out(ctx, nreal, nf, nfeed, off.shape[0] - 1, ntime)
    g, y, info = ctx.redcal_solve(dev(vis), off, mem, w=dev(w), feed_weight=fw, g0=dev(g0), out=out, **kw)
    assert g.data_ptr() == out["g"].data_ptr() and info["chi2"].data_ptr() == out["chi2"].data_ptr()
    assert _guards_untouched(ctx, bufs)
    return {k: ctx.to_host(bufs[k])[1:-1] for k in NAMES}


def _one_step(ctx, table, cases):
    _, off, mem = table
    worst = (0.0, 0.0)
    for vis, w, fw, g0 in cases:
        ex = rc.step_exact(vis, off, mem, g0, w=w, feed_weight=fw)
        got = _solve(ctx, vis, off, mem, w=w, fw=fw, g0=g0, damping=rc.DAMPING, tol=0.0, maxiter=1)
        r = rc.check_step(got["g"], got["y"], ex, off)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        assert np.all(got["iters"] == 1)
        assert np.all(np.abs(got["step"] - ex["step"]) <= 1e-12 * ex["step"].astype(np.float64) + 64 * EPS)
        exact = _ts().redcal_chi2_host(vis, off, mem, got["g"], got["y"], w=w, feed_weight=fw, dtype=np.clongdouble)
        assert np.all(np.abs(got["chi2"] - exact) <= rc.chi2_bound(vis, off, mem, w=w, feed_weight=fw, nfeed=g0.shape[2]))
    return worst


def _ts():
    from driftscan_amd import timestream

    return timestream


@pytest.mark.parametrize("ntime", [1, 5, 17])
@pytest.mark.parametrize("name", ["two", "line3", "grid43", "line70", "cyl12"])
def test_one_step_against_extended_precision(name, ntime):
    """maxiter = 1 from a random g0 within 20 % and 0.5 rad of one: y within the bound of section 4.17 and g within
    K (d_a + n_max + 8) eps [sum omega |V| |z| / den + |g_a|] of `redcal_step_host` in np.clongdouble, K = 4; gains whose
    denominator is 0 (a dead feed, wholly flagged incidences) are g0 bit for bit; chi2 within its bound.  nf, nreal in
    {1, 3}, w_nreal in {1, nreal}, with and without weights and feed weights, one dead feed, NaN guard rows around every
    output."""
    worst = _one_step(_ctx(), rc.tables()[name], rc.step_cases(name, ntime))
    print("redcal step %s, ntime %d: max err / bound at K = %d: y %.3g, g %.3g" % ((name, ntime, rc.K_REDCAL) + worst))


@pytest.mark.parametrize("nfeed", sorted(sc.TILE_NFEED))
def test_one_step_on_every_gain_tile(nfeed):
    """More feeds, shorter tiles of staged gains (8, 4, 2, 1 samples): the random partitions of stack_cases, ntime = 5."""
    ctx = _ctx()
    assert ctx.lib.dm_ts_gain_tile(nfeed) == sc.TILE_NFEED[nfeed]
    table = sc.tile_table(nfeed)
    rng = np.random.default_rng(nfeed)
    nmem = table[2].shape[0]
    cases = []
    for nreal, w_nreal, use_w, use_fw in ((2, 1, True, False), (2, 2, True, True), (1, 1, False, False)):
        cases.append((gc.crandn(rng, nreal, 2, nmem, 5), rc.weights(rng, (w_nreal, 2, nmem, 5)) if use_w else None,
                      rc.feed_weights(rng, nfeed) if use_fw else None, rc.gains_near_one(rng, nreal, 2, nfeed, 5)))
    worst = _one_step(ctx, table, cases)
    print("redcal step %d feeds (tile %d): max err / bound at K = %d: y %.3g, g %.3g"
          % ((nfeed, sc.TILE_NFEED[nfeed], rc.K_REDCAL) + worst))


def test_two_feeds_constrain_nothing():
    """g = g0 = 1, y the plain stack of the non-auto members, iters = 1, step = 0, chi2 = 0."""
    ctx = _ctx()
    nfeed, off, mem = rc.tables()["two"]
    vis = gc.crandn(np.random.default_rng(3), 2, 3, mem.shape[0], 5)
    got = _solve(ctx, vis, off, mem)
    assert np.all(got["g"] == 1.0) and np.all(got["iters"] == 1) and np.all(got["step"] == 0) and np.all(got["chi2"] == 0)
    assert np.all(got["y"][:, :, 0] == 0) and np.array_equal(got["y"][:, :, 1], vis[:, :, 2])
    assert np.array_equal(got["y"][:, :, 2], vis[:, :, 3])


@pytest.mark.parametrize("name", rc.SOLVABLE)
def test_noise_free_data_converge(name):
    """V = g_true conj(g_true) y_true, tol = 1e-13, maxiter = 2000: every sample converges, r_dev <= 4 max(r_host, tol),
    |iters_dev - iters_host| <= 2 per sample, and after `fix_degeneracies(ref=g_true)` max |g - g_true| <=
    4 max(host value, tol)."""
    ctx = _ctx()
    _, off, mem = rc.tables()[name]
    c = rc.converged_case(name)
    got = _solve(ctx, c["vis"], off, mem, tol=c["tol"], maxiter=c["maxiter"])
    r = rc.residual(c["vis"], off, mem, got["g"], got["y"])
    gf, _ = _ts().fix_degeneracies(got["g"], got["y"], off, mem, ref=c["gt"])
    dg = float(np.abs(gf - c["gt"]).max())
    di = np.abs(got["iters"].astype(np.int64) - c["info"]["iters"])
    print("redcal %s: iterations %d to %d (host %d to %d, max difference %d), r = %.3g (host %.3g), max |g - g_true| = "
          "%.3g (host %.3g)" % (name, got["iters"].min(), got["iters"].max(), c["info"]["iters"].min(),
                                c["info"]["iters"].max(), di.max(), r, c["r"], dg, c["dg"]))
    assert np.all(got["step"] < c["tol"]) and np.all(got["iters"] < c["maxiter"])
    assert r <= 4 * max(c["r"], c["tol"])
    assert di.max() <= 2
    assert dg <= 4 * max(c["dg"], c["tol"])


def test_stationarity_and_chi2_with_noise():
    """Unit weights, per-member noise at 1 % of |V| on the 4 x 3 grid: at the result |gh_a - g_a| / |g_a| <= tol / damping
    for every feed, and chi2 agrees with its long-double evaluation at the returned g, y within
    K (nmem + 8) eps sum omega |V|^2."""
    ctx = _ctx()
    ts = _ts()
    nfeed, off, mem = rc.tables()["grid43"]
    rng = np.random.default_rng(11)
    vis, _, _ = rc.noise_free(rng, nfeed, off, mem, (2, 1), 5)
    vis = vis + 0.01 * np.abs(vis) * gc.crandn(rng, *vis.shape) / np.sqrt(2)
    got = _solve(ctx, vis, off, mem, damping=rc.DAMPING, tol=rc.TOL, maxiter=rc.MAXITER)
    assert np.all(got["step"] < rc.TOL) and np.all(got["iters"] < rc.MAXITER) and np.all(got["chi2"] > 0)
    gh, _, _ = ts.redcal_step_host(vis, off, mem, got["g"], damping=1.0, dtype=np.clongdouble)
    drift = float((np.abs(gh - got["g"]) / np.abs(got["g"])).max())
    print("stationarity: max |gh - g| / |g| = %.3g (tol / damping = %.3g)" % (drift, rc.TOL / rc.DAMPING))
    assert drift <= rc.TOL / rc.DAMPING
    exact = ts.redcal_chi2_host(vis, off, mem, got["g"], got["y"], dtype=np.clongdouble)
    err = np.abs(got["chi2"] - exact).astype(np.float64)
    bound = rc.chi2_bound(vis, off, mem, nfeed=nfeed)
    print("chi2: max err / bound = %.3g" % (err / bound).max())
    assert np.all(err <= bound)


def test_a_sample_has_the_same_bits_in_any_company():
    """One sample solved alone; as sample 3 of 17; in a batch of 3 x 3; with w_nreal 1 and nreal; beside a neighbour that
    converges more than 100 iterations earlier: g, y, iters, step and chi2 compared with ==."""
    ctx = _ctx()
    nfeed, off, mem = rc.tables()["grid43"]
    nmem = mem.shape[0]
    rng = np.random.default_rng(17)
    vis, _, _ = rc.noise_free(rng, nfeed, off, mem, (3, 3), 17)
    vis = vis + 0.01 * np.abs(vis) * gc.crandn(rng, *vis.shape)
    w1 = rng.uniform(0.5, 1.5, size=(1, 3, nmem, 17))           # no flags: every sample converges well inside maxiter
    # the neighbour: sample 4 of (0, 0) is noise-free and starts at its solution up to 1e-9, so it freezes early
    quick, gq, _ = rc.noise_free(rng, nfeed, off, mem, (), 1)
    vis[0, 0, :, 4] = quick[:, 0]
    g0 = np.ones((3, 3, nfeed, 17), dtype=np.complex128)
    g0[0, 0, :, 4] = gq[:, 0] * (1 + 1e-9)
    kw = dict(damping=rc.DAMPING, tol=rc.TOL, maxiter=rc.MAXITER)
    full = _solve(ctx, vis, off, mem, w=w1, g0=g0, **kw)
    assert np.all(full["step"][0, 0, 3:5] < rc.TOL)             # (a few slow samples of the batch may run out of iterations:
    assert full["iters"][0, 0, 3] - full["iters"][0, 0, 4] > 100, full["iters"][0, 0]    # their bits are compared all the same)

    def same(part, sel):
        for k in NAMES:
            assert np.array_equal(part[k], full[k][sel]), k

    one = (slice(0, 1), slice(0, 1))
    alone = _solve(ctx, vis[one][..., 3:4], off, mem, w=w1[:, :1, :, 3:4], g0=g0[one][..., 3:4], **kw)
    for k in NAMES:
        assert np.array_equal(alone[k][..., 0], full[k][one][..., 3]), k
    same(_solve(ctx, vis[one], off, mem, w=w1[:, :1], g0=g0[one], **kw), one)                      # sample 3 of 17
    same(_solve(ctx, vis[1:2, 2:3], off, mem, w=w1[:, 2:3], g0=g0[1:2, 2:3], **kw), (slice(1, 2), slice(2, 3)))
    each = np.ascontiguousarray(np.broadcast_to(w1, (3,) + w1.shape[1:]))
    same(_solve(ctx, vis, off, mem, w=each, g0=g0, **kw), (slice(None), slice(None)))               # w_nreal = nreal
    # without weights and from ones: the default arguments, alone and in the batch
    plain = _solve(ctx, vis, off, mem, **kw)
    p1 = _solve(ctx, vis[2:3, 1:2, :, 16:17], off, mem, **kw)
    for k in NAMES:
        assert np.array_equal(p1[k][..., 0], plain[k][2:3, 1:2][..., 16]), k


def test_out_of_iterations_is_reported_not_refused():
    ctx = _ctx()
    nfeed, off, mem = rc.tables()["cyl12"]
    c = rc.converged_case("cyl12")
    got = _solve(ctx, c["vis"], off, mem, tol=1e-13, maxiter=3)
    assert np.all(got["iters"] == 3) and np.all(got["step"] >= 1e-13) and np.all(np.isfinite(got["g"]))
    host = _ts().redcal_solve_host(c["vis"], off, mem, tol=1e-13, maxiter=3)
    assert np.abs(got["g"] - host[0]).max() <= 1e-12 and np.abs(got["y"] - host[1]).max() <= 1e-12 * np.abs(host[1]).max()


def test_refusals_leave_the_outputs_alone():
    """Each refusal returns non-zero with a message naming dm_redcal_solve and writes nothing."""
    from driftscan_amd import _lib

    ctx = _ctx()
    nfeed, off, mem = rc.tables()["line3"]
    npairs, nmem = off.shape[0] - 1, mem.shape[0]
    vis = ctx.to_device(np.ones((1, 1, nmem, 5), dtype=np.complex128))
    bufs, out = _guarded_out(ctx, 1, 1, nfeed, npairs, 5)
    for k in NAMES:
        out[k].fill_(7)
    kw = dict(out=out)
    for bad, match in ((dict(damping=0.0), "damping"), (dict(damping=1.25), "damping"), (dict(damping=float("nan")), "damping"),
                       (dict(tol=-1e-3), "tol"), (dict(tol=float("inf")), "tol"), (dict(tol=float("nan")), "tol"),
                       (dict(maxiter=0), "maxiter"), (dict(feed_weight=[1.0, -1.0, 1.0]), "feed weight 1 is negative")):
        with pytest.raises(_lib.DriftMIError, match="dm_redcal_solve.*" + match):
            ctx.redcal_solve(vis, off, mem, **dict(kw, **bad))
    with pytest.raises(_lib.DriftMIError, match="dm_redcal_solve.*class 1 is empty"):
        ctx.redcal_solve(vis, [0, 3, 3, 6], mem, **kw)
    with pytest.raises(_lib.DriftMIError, match="dm_redcal_solve.*class_off\\[0\\] must be 0"):
        ctx.redcal_solve(ctx.to_device(np.ones((1, 1, nmem + 1, 5), dtype=np.complex128)), [1, 3, 5, 7], np.vstack([mem, [[0, 1]]]),
                         **kw)
    with pytest.raises(_lib.DriftMIError, match="dm_redcal_solve.*does not fit"):
        ctx.redcal_solve(ctx.to_device(np.ones((1, 1, 1, 1), dtype=np.complex128)), [0, 1], [[10240, 0]])
    # through the C entry point: negative sizes, null pointers with work to do, overlapping buffers, no-ops
    lib, h, P = ctx.lib, ctx.h, ctx.ptr
    offa, offp = _lib._iarr(off)
    mema, memp = _lib._iarr(mem)

    bad_mem = mem.copy()
    bad_mem[4] = (5, 0)
    bada, badp = _lib._iarr(bad_mem)

    def call(nreal=1, nf=1, ntime=5, v=vis, w=None, g0=None, w_nreal=1, mp=memp, **o):
        o = dict(out, **o)
        return lib.dm_redcal_solve(h, nreal, w_nreal, nf, nfeed, npairs, ntime, offp, mp, P(v), P(w), None, P(g0), 0.4, 1e-10,
                                   10, P(o["g"]), P(o["y"]), P(o["iters"]), P(o["step"]), P(o["chi2"]), 0)

    def last():
        return lib.dm_last_error(h).decode()

    assert call(mp=badp) != 0 and "dm_redcal_solve: member 4 names feed 5 of 3" in last()
    assert call(ntime=-1) != 0 and "dm_redcal_solve: negative size" in last()
    assert call(nf=-1) != 0 and "dm_redcal_solve: negative size" in last()
    assert call(v=None) != 0 and "dm_redcal_solve: null pointer" in last()
    for k in NAMES:
        assert call(**{k: None}) != 0 and "dm_redcal_solve: null pointer" in last(), k
    assert call(y=vis) != 0 and "dm_redcal_solve: y shares an element with vis" in last()
    assert call(g=vis) != 0 and "dm_redcal_solve: g shares an element with vis" in last()
    wdev = ctx.to_device(np.ones((1, 1, nmem, 5)))
    assert call(w=wdev, w_nreal=2) != 0 and "dm_redcal_solve: w_nreal" in last()
    assert call(w=wdev, step=wdev) != 0 and "dm_redcal_solve: step shares an element with w" in last()
    g0 = ctx.to_device(np.ones((1, 1, nfeed, 5), dtype=np.complex128))
    assert call(g0=g0, g=g0) != 0 and "dm_redcal_solve: g shares an element with g0" in last()
    assert call(chi2=out["step"]) != 0 and "dm_redcal_solve: chi2 shares an element with step" in last()
    assert call(nreal=0) == 0 and call(nf=0) == 0 and call(ntime=0) == 0                          # no-ops
    # the wrapper's own checks
    for bad in (lambda: ctx.redcal_solve(vis, off, mem[:-1]),
                lambda: ctx.redcal_solve(vis, off, mem, w=ctx.to_device(np.ones((2, 1, nmem, 5)))),
                lambda: ctx.redcal_solve(vis, off, mem, g0=ctx.to_device(np.ones((1, 1, 2, 5), dtype=np.complex128))),
                lambda: ctx.redcal_solve(vis, off, mem, out=dict(g=ctx.empty((1, 1, nfeed, 4), np.complex128))),
                lambda: ctx.redcal_solve(vis, off, mem, out=dict(gains=out["g"]))):
        with pytest.raises(ValueError):
            bad()
    ctx.sync()
    assert _guards_untouched(ctx, bufs)
    for k in NAMES:
        assert np.all(ctx.to_host(bufs[k])[1:-1] == 7), k
    assert np.all(ctx.to_host(vis) == 1.0) and np.all(ctx.to_host(wdev) == 1.0) and np.all(ctx.to_host(g0) == 1.0)


# ---- the routes: the fixtures of tests/test_gpu_stack.py (12 feeds, ntime = 183) ------------------------------------------
from test_gpu_stack import MODEL, _dead_feed, prod, routes, skyfile  # noqa: E402,F401

SOLVER = dict(tol=1e-10, maxiter=2000)


@pytest.fixture(scope="module")
def redundant(routes):
    """(a) and (b): the unstacked data with a GainModel, solved with the file's gains and with ones as the reference;
    the host's residual of the same data."""
    from driftscan_amd import storage, timestream

    pm, d, tel, uns = (routes[k] for k in ("pm", "d", "tel", "uns"))
    a = timestream.stack_baselines(pm, uns.directory, str(d / "red_file"), calibrate="redundant",
                                   redcal=dict(SOLVER, reference="file"))
    b = timestream.stack_baselines(pm, uns.directory, str(d / "red_ones"), calibrate="redundant", redcal=dict(SOLVER))
    off, mem = tel.redundant_pairs()
    vis, gains = [], []
    for fi in range(tel.nfreq):
        with storage.File(uns._ffile(fi), "r") as f:
            vis.append(f["timestream"][:])
            gains.append(f["gain"][:])
    vis, gains = np.stack(vis), np.stack(gains)
    g, y, info = timestream.redcal_solve_host(vis, off, mem, nfeed=int(tel.nfeed), **SOLVER)
    assert np.all(info["step"] < SOLVER["tol"])
    return dict(a=a, b=b, vis=vis, gains=gains, r_host=rc.residual(vis, off, mem, g, y), iters_host=info["iters"])


def test_redundant_calibration_with_the_files_reference_is_the_calibrated_stack(routes, redundant):
    """(a): `calibrate="redundant"` with `reference="file"` reproduces the stack of `calibrate="file"` within the round-trip
    bound of section 4.17 plus 4 max(r_host, tol) max |v|; no `weight` is written; `gain_solution` and `redcal_iters` are."""
    from driftscan_amd import storage

    tel, ntime, cal = (routes[k] for k in ("tel", "ntime", "cal"))
    a = redundant["a"]
    off, _ = tel.redundant_pairs()
    nmax = int(np.diff(off).max())
    for fi in range(tel.nfreq):
        v, want = a.timestream_f(fi), cal.timestream_f(fi)
        scale = np.abs(want).max()
        bound = (8 * EPS + 2 * sc.K_STACK * (nmax + 4) * EPS) * scale + 4 * max(redundant["r_host"], SOLVER["tol"]) * scale
        with storage.File(a._ffile(fi), "r") as f:
            assert "weight" not in f
            gs, its = f["gain_solution"][:], f["redcal_iters"][:]
        assert gs.shape == (tel.nfeed, ntime) and its.shape == (ntime,) and np.all(its < SOLVER["maxiter"])
        assert np.abs(its.astype(np.int64) - redundant["iters_host"][fi]).max() <= 2
        print("frequency %d: max |delta| / bound = %.3g, max |g - g_file| = %.3g, iterations %d to %d, r_host = %.3g"
              % (fi, np.abs(v - want).max() / bound, np.abs(gs - redundant["gains"][fi]).max(), its.min(), its.max(),
                 redundant["r_host"]))
        assert np.abs(v - want).max() <= bound


def test_redundant_calibration_from_ones_leaves_the_degenerate_part(routes, redundant):
    """(b): with `reference=None` the result differs from (a) by no more than the projection of the true ln g on the
    degeneracy bases predicts (factor 2), and it is closer to (a) than the uncalibrated stack is, in the root mean square
    over the whole directory: the uncalibrated stack keeps all 24 real parameters of the gain errors (averaged over the
    members of a class), the redundant one only the 6 of the degenerate subspace.  (Of a single frequency, in the maximum
    norm, that need not hold: the figures are printed, and in DESIGN.md section 4.18.)"""
    from driftscan_amd import timestream

    pm, d, tel, uns = (routes[k] for k in ("pm", "d", "tel", "uns"))
    off, mem = tel.redundant_pairs()
    n = np.diff(off)
    d_amp, d_ph = timestream.redcal_degeneracies(off, mem, int(tel.nfeed))
    lg = np.log(redundant["gains"])
    h = np.exp(np.einsum("ab,cb,fct->fat", d_amp, d_amp, lg.real) + 1j * np.einsum("ab,cb,fct->fat", d_ph, d_ph, lg.imag))
    # with g_b = g_true / h member (i, j) enters the stack as y h_i conj(h_j): what is left in the data, per member
    move = np.abs(h[:, mem[:, 0]] * h[:, mem[:, 1]].conj() - 1)
    move = np.maximum.reduceat(move, off[:-1], axis=1)
    raw = timestream.stack_baselines(pm, uns.directory, str(d / "red_raw"), calibrate=None)
    sq_b = sq_r = 0.0
    for fi in range(tel.nfreq):
        va, vb, vr = redundant["a"].timestream_f(fi), redundant["b"].timestream_f(fi), raw.timestream_f(fi)
        slack = 1e-8 * np.abs(va).max()
        print("frequency %d: max |b - a| = %.3g of max |v| (predicted at most %.3g), uncalibrated %.3g"
              % (fi, np.abs(vb - va).max() / np.abs(va).max(), (move[fi] * np.abs(va)).max() / np.abs(va).max(),
                 np.abs(vr - va).max() / np.abs(va).max()))
        assert np.all(np.abs(vb - va) <= 2 * move[fi] * np.abs(va) + slack)
        assert np.abs(vb - va).max() > slack
        sq_b, sq_r = sq_b + (np.abs(vb - va) ** 2).sum(), sq_r + (np.abs(vr - va) ** 2).sum()
    print("rms |b - a| / rms |uncalibrated - a| = %.3g" % np.sqrt(sq_b / sq_r))
    assert sq_b < sq_r


def test_redundant_calibration_with_a_dead_feed(routes, redundant):
    """(c): the classes the dead feed empties come out with weight 0 and info = -1 downstream, as today; the rest converge,
    carry the weight (n_c - k) / n_c and are the calibrated stack within 2e3 tol max |v|: a stacked value moves by the sum
    of the relative errors of two gains, each within the 1e3 tol the residual is held to on the CPU."""
    from driftscan_amd import storage, timestream

    pm, d, tel, ntime, uns, cal = (routes[k] for k in ("pm", "d", "tel", "ntime", "uns", "cal"))
    feed, emptied, thinned, frac = _dead_feed(tel)
    dead = timestream.stack_baselines(pm, uns.directory, str(d / "red_dead"), calibrate="redundant", dead_feeds=[feed],
                                      redcal=dict(SOLVER, reference="file"))
    left = np.setdiff1d(np.arange(tel.npairs), emptied)
    for fi in range(tel.nfreq):
        v, c, w = dead.timestream_f(fi), cal.timestream_f(fi), dead.weight_f(fi)
        with storage.File(dead._ffile(fi), "r") as f:
            assert np.all(f["redcal_iters"][:] < SOLVER["maxiter"])
        assert np.array_equal(w, np.broadcast_to(frac[:, None], w.shape))
        assert np.all(v[emptied] == 0) and np.all(w[emptied] == 0)
        assert np.abs(v[left] - c[left]).max() <= 2e3 * SOLVER["tol"] * np.abs(c).max()
    dead.generate_modes_batched()
    with storage.File(dead.output_directory + "/mmodes/weights.hdf5", "r") as f:
        info = f["info"][:]
    want = np.zeros((tel.nfreq, tel.npairs), dtype=info.dtype)
    want[:, emptied] = -1
    assert np.array_equal(info, want)


def test_out_of_iterations_gets_weight_zero_and_is_counted(routes, caplog):
    """(d): maxiter = 3: every sample is reported as not converged, the stacked `weight` is 0 there, the log counts them."""
    from driftscan_amd import storage, timestream

    pm, d, tel, ntime, uns = (routes[k] for k in ("pm", "d", "tel", "ntime", "uns"))
    timestream.sim_log = {}
    try:
        with caplog.at_level(logging.WARNING, logger="driftscan_amd.timestream"):
            short = timestream.stack_baselines(pm, uns.directory, str(d / "red_short"), calibrate="redundant",
                                               redcal=dict(maxiter=3))
        log = timestream.sim_log
    finally:
        timestream.sim_log = None
    assert log["redcal_not_converged"] == tel.nfreq * ntime and log["redcal"] > 0
    assert any("%d of %d samples did not converge" % (tel.nfreq * ntime, tel.nfreq * ntime) in r.getMessage()
               for r in caplog.records)
    for fi in range(tel.nfreq):
        w = short.weight_f(fi)
        assert w is not None and w.shape == (tel.npairs, ntime) and np.all(w == 0)
        with storage.File(short._ffile(fi), "r") as f:
            assert np.all(f["redcal_iters"][:] == 3)
    with pytest.raises(ValueError, match="redcal"):
        timestream.stack_baselines(pm, uns.directory, str(d / "red_bad"), calibrate="file", redcal=dict(maxiter=3))
    with pytest.raises(ValueError, match="redcal holds"):
        timestream.stack_baselines(pm, uns.directory, str(d / "red_bad"), calibrate="redundant", redcal=dict(iterations=3))


def test_the_pipeline_entry_gives_the_same_directory(routes, redundant, tmp_path):
    """(e): `stack_from: {calibrate: redundant, redcal: {...}}` of the pipeline produces the files of (b)."""
    import yaml

    from driftscan_amd import pipeline, storage

    d, tel, uns = (routes[k] for k in ("d", "tel", "uns"))
    conf = dict(config=dict(product_directory=str(d / "params.yaml"), generate_modes=False, generate_klmodes=False,
                            generate_powerspectra=False, generate_maps=False),
                timestreams=[dict(name="s", directory=str(tmp_path / "pipe_red"),
                                  stack_from=dict(directory=uns.directory, calibrate="redundant", redcal=dict(SOLVER)))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = pipeline.PipelineManager.from_configfile(str(cfile))
    p.generate()
    s, b = p.timestreams["s"], redundant["b"]
    for fi in range(tel.nfreq):
        assert np.array_equal(s.timestream_f(fi), b.timestream_f(fi))
        with storage.File(s._ffile(fi), "r") as f, storage.File(b._ffile(fi), "r") as h:
            assert sorted(f.keys()) == sorted(h.keys()) and "weight" not in f
            assert np.array_equal(f["gain_solution"][:], h["gain_solution"][:])
            assert np.array_equal(f["redcal_iters"][:], h["redcal_iters"][:])
