"""The numpy statements of the redundant-calibration solver without a GPU: the complex128
iteration inside the bounds the device is held to, convergence on noise-free data, stationarity with noise, the
degeneracy bases and `fix_degeneracies`."""
import numpy as np
import pytest

import gains_cases as gc
import redcal_cases as rc
import stack_cases as sc


def _ts():
    from driftscan_amd import timestream

    return timestream


@pytest.mark.parametrize("ntime", [1, 5, 17])
@pytest.mark.parametrize("name", ["two", "line3", "grid43", "line70", "cyl12"])
def test_complex128_step_stays_inside_the_device_bounds(name, ntime):
    """One iteration in complex128 against np.clongdouble on every shape of the GPU test: y within the bound of section
    4.17, g within K (d_a + n_max + 8) eps [sum omega |V| |z| / den + |g_a|], K = 4."""
    ts = _ts()
    _, off, mem = rc.tables()[name]
    worst = (0.0, 0.0)
    for vis, w, fw, g0 in rc.step_cases(name, ntime):
        ex = rc.step_exact(vis, off, mem, g0, w=w, feed_weight=fw)
        g, y, step = ts.redcal_step_host(vis, off, mem, g0, w=w, feed_weight=fw, damping=rc.DAMPING)
        r = rc.check_step(g, y, ex, off, K=4)
        worst = (max(worst[0], r[0]), max(worst[1], r[1]))
        # (a class left with one weighted member fits exactly: its feeds move by rounding only, hence the absolute term)
        assert np.all(np.abs(step - ex["step"]) <= 1e-12 * ex["step"].astype(np.float64) + 64 * rc.EPS)
    print("redcal step %s, ntime %d, complex128: max err / bound at K = 4: y %.3g, g %.3g" % ((name, ntime) + worst))


@pytest.mark.parametrize("nfeed", sorted(sc.TILE_NFEED))
def test_complex128_step_on_the_tile_tables(nfeed):
    ts = _ts()
    table = sc.tile_table(nfeed)
    _, off, mem = table
    rng = np.random.default_rng(nfeed)
    vis = gc.crandn(rng, 2, 2, mem.shape[0], 5)
    w = rc.weights(rng, (1, 2, mem.shape[0], 5))
    g0 = rc.gains_near_one(rng, 2, 2, nfeed, 5)
    ex = rc.step_exact(vis, off, mem, g0, w=w)
    g, y, _ = ts.redcal_step_host(vis, off, mem, g0, w=w, damping=rc.DAMPING)
    print("redcal step %d feeds, complex128: max err / bound at K = 4: y %.3g, g %.3g" % ((nfeed,) + rc.check_step(g, y, ex, off, K=4)))


def test_checker_rejects_an_element_moved_by_twice_its_bound():
    ts = _ts()
    _, off, mem = rc.tables()["grid43"]
    vis, w, fw, g0 = next(iter(rc.step_cases("grid43", 5)))
    ex = rc.step_exact(vis, off, mem, g0)
    g, y, _ = ts.redcal_step_host(vis, off, mem, g0)
    rc.check_step(g, y, ex, off)
    bad = g.copy()
    bad[0, 0, 3, 2] = np.complex128(ex["g"][0, 0, 3, 2]) + 2 * rc.gain_bound(ex)[0, 0, 3, 2]
    with pytest.raises(AssertionError, match="g misses"):
        rc.check_step(bad, y, ex, off)
    by, _ = sc.stack_bounds(ex["yout"], ex["ywout"], ex["yscale"], off, rc.K_REDCAL)
    bad = y.copy()
    bad[0, 0, 2, 1] = np.complex128(ex["yout"][0, 0, 2, 1]) + 2j * by[0, 0, 2, 1]
    with pytest.raises(AssertionError, match="y misses"):
        rc.check_step(g, bad, ex, off)


def test_two_feeds_constrain_nothing():
    """No class has two members between different feeds: g = g0, y the plain stack of the non-auto members, iters = 1,
    step = 0, chi2 = 0."""
    ts = _ts()
    nfeed, off, mem = rc.tables()["two"]
    rng = np.random.default_rng(3)
    vis = gc.crandn(rng, 2, 3, mem.shape[0], 5)
    g, y, info = ts.redcal_solve_host(vis, off, mem)
    assert np.all(g == 1.0) and np.all(info["iters"] == 1) and np.all(info["step"] == 0) and np.all(info["chi2"] == 0)
    want, _ = ts.vis_stack_host(vis, off, mem, feed_weight=None, w=(mem[:, 0] != mem[:, 1]).astype(float)[:, None])
    assert np.array_equal(y, want) and np.all(y[:, :, 0] == 0) and np.array_equal(y[:, :, 1], vis[:, :, 2])
    yfac, gfac = ts.redcal_weights(off, mem, nfeed)
    assert np.array_equal(yfac, [0, 0, 1, 1]) and not gfac.any()


@pytest.mark.parametrize("name", rc.SOLVABLE)
def test_noise_free_data_converge_to_the_model(name):
    """V = g_true conj(g_true) y_true, tol = 1e-13, maxiter = 2000: every sample converges, the model reproduces V on the
    weighted members to 1e3 tol of max |V|, and `fix_degeneracies(ref=g_true)` gives the true gains back."""
    c = rc.converged_case(name)
    info = c["info"]
    print("redcal %s, complex128: iterations %d to %d, r = %.3g, max |g - g_true| = %.3g"
          % (name, info["iters"].min(), info["iters"].max(), c["r"], c["dg"]))
    assert np.all(info["step"] < c["tol"]) and np.all(info["iters"] < c["maxiter"]) and np.all(info["iters"] > 1)
    assert c["r"] <= 1e3 * c["tol"]
    assert c["dg"] <= 1e4 * c["tol"]
    assert np.all(info["chi2"] <= (1e3 * c["tol"]) ** 2 * (np.abs(c["vis"]) ** 2).sum(axis=-2))


def test_damping_one_stalls_on_the_three_feed_line():
    """Why damping is a parameter: at damping = 1 samples of the 3-feed line have not converged after 500 iterations and
    are reported so (iters = maxiter, step >= tol), where 0.4 converges in under 100."""
    ts = _ts()
    nfeed, off, mem = rc.tables()["line3"]
    vis, _, _ = rc.noise_free(np.random.default_rng(5), nfeed, off, mem, (), 4)
    _, _, slow = ts.redcal_solve_host(vis, off, mem, damping=1.0, tol=1e-10, maxiter=500)
    _, _, fast = ts.redcal_solve_host(vis, off, mem, damping=0.4, tol=1e-10, maxiter=500)
    assert np.all(fast["iters"] < 100) and np.all(fast["step"] < 1e-10)
    stalled = slow["iters"] == 500
    assert stalled.any() and np.all(slow["step"][stalled] >= 1e-10) and np.all(slow["step"][~stalled] < 1e-10)


def test_stationarity_and_chi2_with_noise():
    """Unit weights, per-member noise at 1 % of |V|: at the result |gh_a - g_a| / |g_a| <= tol / damping for every feed
    (the freeze rule), and chi2 agrees with its evaluation in np.clongdouble within K (nmem + 8) eps sum omega |V|^2."""
    ts = _ts()
    nfeed, off, mem = rc.tables()["grid43"]
    rng = np.random.default_rng(11)
    vis, _, _ = rc.noise_free(rng, nfeed, off, mem, (2,), 5)
    vis = vis + 0.01 * np.abs(vis) * gc.crandn(rng, *vis.shape) / np.sqrt(2)
    g, y, info = ts.redcal_solve_host(vis, off, mem, damping=rc.DAMPING, tol=rc.TOL, maxiter=rc.MAXITER)
    assert np.all(info["step"] < rc.TOL) and np.all(info["chi2"] > 0)
    gh, _, _ = ts.redcal_step_host(vis, off, mem, g, damping=1.0, dtype=np.clongdouble)
    drift = (np.abs(gh - g) / np.abs(g)).max()
    print("stationarity: max |gh - g| / |g| = %.3g (tol / damping = %.3g)" % (drift, rc.TOL / rc.DAMPING))
    assert drift <= rc.TOL / rc.DAMPING
    exact = ts.redcal_chi2_host(vis, off, mem, g, y, dtype=np.clongdouble)
    assert np.all(np.abs(info["chi2"] - exact) <= rc.chi2_bound(vis, off, mem, nfeed=nfeed))


@pytest.mark.parametrize("table,dims", [((3, 1), (2, 2)), ((4, 3), (1, 3)), ((16, 1), (1, 2))])
def test_degeneracy_bases(table, dims):
    """Dimensions (amplitude, phase), orthonormality, and chi^2's blindness: moving g along any basis vector with the
    matching change of y leaves every model visibility unchanged to 1e-13."""
    ts = _ts()
    nfeed, off, mem = rc.grid_table(*table)
    d_amp, d_ph = ts.redcal_degeneracies(off, mem, nfeed)
    assert (d_amp.shape[1], d_ph.shape[1]) == dims
    for d in (d_amp, d_ph):
        assert np.abs(d.T @ d - np.eye(d.shape[1])).max() <= 1e-13
    rng = np.random.default_rng(2)
    g = rc.gains_near_one(rng, nfeed, 3)
    y = gc.crandn(rng, off.shape[0] - 1, 3)
    model = ts.vis_expand_host(y, off, mem, g=g)
    n = np.diff(off)
    first = off[:-1]                                                # a member of every class (class 0: the autos)
    for d, unit in ((d_amp, 1.0), (d_ph, 1j)):
        for k in range(d.shape[1]):
            h = np.exp(0.3 * unit * d[:, k])[:, None]
            fac = h[mem[first, 0]] * h[mem[first, 1]].conj()
            moved = ts.vis_expand_host(y / fac, off, mem, g=h * g)
            keep = np.repeat(np.arange(n.shape[0]) > 0, n)          # the autocorrelations are not in chi^2
            assert np.abs(moved - model)[keep].max() <= 1e-13 * np.abs(model).max()
    # fix_degeneracies removes exactly such a move
    h = np.exp(0.3 * d_amp[:, 0] + 0.2j * d_ph[:, -1])[:, None]
    fac = h[mem[first, 0]] * h[mem[first, 1]].conj()
    g2, y2 = ts.fix_degeneracies(h * g, y / fac, off, mem, ref=g)
    assert np.abs(g2 - g).max() <= 1e-13
    assert np.abs(ts.vis_expand_host(y2, off, mem, g=g2) - model)[np.repeat(np.arange(n.shape[0]) > 0, n)].max() <= 1e-13 * np.abs(model).max()


def test_host_refusals():
    ts = _ts()
    nfeed, off, mem = rc.tables()["line3"]
    vis = np.ones((mem.shape[0], 2), dtype=np.complex128)
    for kw in (dict(damping=0.0), dict(damping=1.5), dict(tol=-1.0), dict(tol=np.inf), dict(maxiter=0)):
        with pytest.raises(ValueError):
            ts.redcal_solve_host(vis, off, mem, **kw)
    with pytest.raises(ValueError):
        ts.redcal_weights(off, mem, nfeed, feed_weight=[1.0, -1.0, 1.0])
    with pytest.raises(ValueError):
        ts.redcal_weights([0, 2, 2], [[0, 1], [1, 2]], 3)
