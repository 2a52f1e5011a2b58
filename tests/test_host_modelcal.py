"""Sky-model gain calibration on the host: the complex128 statement `modelcal_step_host` against
its long-double evaluation inside the bound the device is held to, the checker's teeth, convergence and the reason for the
damping parameter, the connected components, the phase convention and the spreading of interval gains over samples."""
import numpy as np
import pytest

import modelcal_cases as mc
import redcal_cases as rc


def _ts():
    from driftscan_amd import timestream

    return timestream


@pytest.mark.parametrize("ntime,interval", mc.STEP_SHAPES)
@pytest.mark.parametrize("name", ["two", "line3", "grid43", "line70", "cyl12"])
def test_the_complex128_statement_stays_inside_the_device_bound(name, ntime, interval):
    ts = _ts()
    _, off, mem = mc.tables()[name]
    worst = 0.0
    for vis, model, w, fw, g0 in mc.step_cases(name, ntime, interval, mc.STEP_BATCHES[:5]):
        ex = mc.step_exact(vis, model, off, mem, g0, interval, w=w, feed_weight=fw)
        gn, step, den = ts.modelcal_step_host(vis, model, off, mem, g0, interval, w=w, feed_weight=fw, damping=mc.DAMPING)
        worst = max(worst, mc.check_step(gn, ex))
        mc.check_gweight(den, ex)
        assert gn.shape == g0.shape and step.shape == g0.shape[:2] + g0.shape[3:]
        assert np.all(np.abs(step - ex["step"]) <= 1e-12 * ex["step"].astype(np.float64) + 64 * mc.EPS)
    print("modelcal host step %s (%d, %d): max err / bound at K = %d: %.3g" % (name, ntime, interval, mc.K_MODELCAL, worst))
    assert worst < 0.5


def test_the_checker_rejects_one_element_moved_by_twice_its_bound():
    _, off, mem = mc.tables()["grid43"]
    vis, model, w, fw, g0 = next(iter(mc.step_cases("grid43", 17, 4, mc.STEP_BATCHES[4:5])))
    ex = mc.step_exact(vis, model, off, mem, g0, 4, w=w, feed_weight=fw)
    good = np.asarray(ex["g"], dtype=np.complex128)
    mc.check_step(good, ex)
    live = np.argwhere(np.asarray(ex["den"] > 0))
    at = tuple(live[len(live) // 2])
    bad = good.copy()
    bad[at] += 2 * mc.gain_bound(ex)[at]
    with pytest.raises(AssertionError, match="misses its bound"):
        mc.check_step(bad, ex)
    dead = np.argwhere(np.asarray(ex["den"] == 0))                          # the dead feed: g0 bit for bit
    assert len(dead)
    bad = good.copy()
    bad[tuple(dead[0])] *= 1 + 2.0**-52
    with pytest.raises(AssertionError):
        mc.check_step(bad, ex)
    den = ex["den"].astype(np.float64)
    mc.check_gweight(den, ex)
    den[at] *= 1 + 2 * mc.gain_factor(ex)[at[2:]]
    with pytest.raises(AssertionError):
        mc.check_gweight(den, ex)


def test_a_single_cross_pair_is_constrained_here():
    """`two`: one class of one cross pair.  The redundant solver leaves its gains alone; against a model both move."""
    ts = _ts()
    nfeed, off, mem = mc.tables()["two"]
    vis, model, w, fw, g0 = next(iter(mc.step_cases("two", 5, 1, mc.STEP_BATCHES[:1])))
    gn, step, den = ts.modelcal_step_host(vis, model, off, mem, g0, 1)
    assert np.all(den > 0) and np.all(gn != g0) and np.all(step > 0)
    assert np.all(ts.redcal_weights(off, mem, nfeed)[1] == 0) and np.any(ts.modelcal_weights(off, mem, nfeed) > 0)


@pytest.mark.parametrize("name", mc.SOLVABLE)
def test_noise_free_data_converge_to_the_true_gains(name):
    c = mc.converged_case(name)
    tol = mc.CONVERGED["tol"]
    it = c["info"]["iters"]
    print("modelcal host %s: iterations %d to %d, r = %.3g, max |g - g_true| = %.3g" % (name, it.min(), it.max(), c["r"], c["dg"]))
    assert np.all(c["info"]["step"] < tol) and np.all(it < mc.CONVERGED["maxiter"])
    assert np.all(c["info"]["gweight"] > 0)
    assert c["r"] <= 1e3 * tol and c["dg"] <= 1e3 * tol


def test_without_damping_the_fixed_point_does_not_converge():
    """The reason damping is a parameter: delta = 1 on `line3` still steps after 500 iterations where 0.5 converges."""
    ts = _ts()
    _, off, mem = mc.tables()["line3"]
    c = mc.converged_case("line3")
    kw = dict(w=c["w"], tol=mc.CONVERGED["tol"], maxiter=500)
    _, info = ts.modelcal_solve_host(c["vis"], c["model"], off, mem, mc.CONVERGED["interval"], damping=1.0, **kw)
    print("delta = 1: steps after 500 iterations %.3g to %.3g" % (info["step"].min(), info["step"].max()))
    assert np.all(info["iters"] == 500) and np.all(info["step"] >= mc.CONVERGED["tol"])
    _, info = ts.modelcal_solve_host(c["vis"], c["model"], off, mem, mc.CONVERGED["interval"], damping=0.5, **kw)
    assert np.all(info["iters"] < 500) and np.all(info["step"] < mc.CONVERGED["tol"])


def test_an_inactive_interval_keeps_its_start():
    ts = _ts()
    nfeed, off, mem = mc.tables()["grid43"]
    c = mc.converged_case("grid43")
    L = mc.CONVERGED["interval"]
    g0 = rc.gains_near_one(np.random.default_rng(5), 2, 1, nfeed, 3)
    active = np.array([[1, 0, 1]], dtype=np.int32)
    g, info = ts.modelcal_solve_host(c["vis"], c["model"], off, mem, L, w=c["w"], g0=g0, active=active, maxiter=50)
    assert np.array_equal(g[..., 1], g0[..., 1]) and np.all(g[..., 0] != g0[..., 0])
    for k in ("iters", "step", "chi2"):
        assert np.all(info[k][..., 1] == 0) and np.all(info[k][..., 0] > 0), k
    assert np.all(info["gweight"][..., 1] == 0) and np.all(info["gweight"][..., 0] > 0)
    full, finfo = ts.modelcal_solve_host(c["vis"], c["model"], off, mem, L, w=c["w"], g0=g0, maxiter=50)
    assert np.array_equal(full[..., 0], g[..., 0]) and np.array_equal(finfo["chi2"][..., 2], info["chi2"][..., 2])


def test_components_of_a_model_without_cross_polarisation():
    """An unpolarised source on the polarised cylinder: with the XY classes zeroed the X and the Y feeds are two
    components; the full model joins them; a dead feed is a component of its own."""
    ts = _ts()
    nfeed, off, mem = mc.tables()["cyl12"]
    n = np.diff(off)
    cls = np.repeat(np.arange(n.shape[0]), n)
    full = ts.modelcal_components(off, mem, nfeed, np.ones(n.shape[0]))
    assert np.all(full == 0)
    # polarisation of a feed: the two components of the table with only the classes that join like feeds
    power = np.ones(n.shape[0])
    first = ts.modelcal_components(off, mem, nfeed, power)
    # find a bipartition: the classes whose members all join feeds of the same half (feeds come as X block, Y block)
    half = np.arange(nfeed) >= nfeed // 2
    cross = np.zeros(n.shape[0], dtype=bool)
    np.logical_or.at(cross, cls, half[mem[:, 0]] != half[mem[:, 1]])
    assert cross.any() and not cross.all()
    power[cross] = 0.0
    comp = ts.modelcal_components(off, mem, nfeed, power)
    assert np.array_equal(comp, half.astype(np.int64)) and np.all(first == 0)
    weak = np.where(cross, 1e-9, 1.0)                                        # under the floor: the same two
    assert np.array_equal(ts.modelcal_components(off, mem, nfeed, weak), comp)
    assert np.all(ts.modelcal_components(off, mem, nfeed, weak, edge_floor=1e-12) == 0)
    fw = np.ones(nfeed)
    fw[2] = 0.0
    dead = ts.modelcal_components(off, mem, nfeed, power, feed_weight=fw)
    assert len(np.unique(dead)) == 3 and np.sum(dead == dead[2]) == 1


def test_fix_phase_leaves_every_product_inside_a_component():
    ts = _ts()
    rng = np.random.default_rng(9)
    nfeed, nint = 12, 4
    comp = (np.arange(nfeed) >= 6).astype(np.int64)
    g = rc.gains_near_one(rng, 2, 3, nfeed, nint) * np.exp(2j * np.pi * rng.uniform(size=(2, 3, 1, nint)))
    ref = rc.gains_near_one(rng, 2, 3, nfeed, nint)
    fw = rng.uniform(0.5, 1.5, size=nfeed)
    out = ts.modelcal_fix_phase(g, comp, ref=ref, feed_weight=fw)
    for sel in (comp == 0, comp == 1):
        a, b = g[..., sel, :], out[..., sel, :]
        pa, pb = a[..., :, None, :] * a[..., None, :, :].conj(), b[..., :, None, :] * b[..., None, :, :].conj()
        assert np.abs(pa - pb).max() <= 16 * mc.EPS * np.abs(pa).max()
        s = (fw[sel, None] * b * ref[..., sel, :].conj()).sum(axis=-2)
        assert np.all(s.real > 0) and np.abs(s.imag).max() <= 64 * mc.EPS * np.abs(s).max()
    # rotating one component by a phase of its own is undone; the default reference is ones
    turned = g * np.where(comp == 1, np.exp(1.3j), np.exp(-0.4j))[:, None]
    assert np.abs(ts.modelcal_fix_phase(turned, comp, ref=ref, feed_weight=fw) - out).max() <= 64 * mc.EPS
    s = ts.modelcal_fix_phase(g, comp)[..., comp == 0, :].sum(axis=-2)
    assert np.all(s.real > 0) and np.abs(s.imag).max() <= 64 * mc.EPS * np.abs(s).max()
    # labels that differ between intervals
    per = np.broadcast_to(comp[:, None], (nfeed, nint)).copy()
    per[:, 0] = 0
    mixed = ts.modelcal_fix_phase(g, per, ref=ref, feed_weight=fw)
    assert np.array_equal(mixed[..., 1:], out[..., 1:])
    s = (fw[:, None] * mixed * ref.conj()).sum(axis=-2)[..., 0]
    assert np.all(s.real > 0) and np.abs(s.imag).max() <= 64 * mc.EPS * np.abs(s).max()


def test_spread_takes_the_nearest_valid_interval():
    ts = _ts()
    g = (np.arange(1, 7)[None, :] * np.array([[1.0], [1j]])).astype(np.complex128)     # (2 feeds, 6 intervals)
    ntime, L = 22, 4                                                                   # the last interval holds 2 samples
    full, found = ts.modelcal_spread(g, np.ones(6, dtype=bool), L, ntime)
    assert found and full.shape == (2, ntime) and np.array_equal(full[0], (np.arange(ntime) // L + 1).astype(np.complex128))
    # invalid at both ends, and interval 3 between the valid 2 and 4: a tie, the earlier wins
    got, found = ts.modelcal_spread(g, np.array([0, 0, 1, 0, 1, 0], dtype=bool), L, ntime)
    want = np.array([3, 3, 3, 3, 5, 5])[np.arange(ntime) // L]
    assert found and np.array_equal(got[0], want.astype(np.complex128)) and np.array_equal(got[1], 1j * want)
    none, found = ts.modelcal_spread(g, np.zeros(6, dtype=bool), L, ntime)
    assert not found and np.all(none == 1.0) and none.shape == (2, ntime)
    with pytest.raises(ValueError):
        ts.modelcal_spread(g, np.ones(5, dtype=bool), L, ntime)
    with pytest.raises(ValueError):
        ts.modelcal_spread(g, np.ones(6, dtype=bool), 0, ntime)
