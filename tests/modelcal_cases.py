"""Shared cases of the sky-model calibration tests: inputs on the class tables of
tests/redcal_cases.py, the bounds of one iteration against extended precision and the checkers the CPU and GPU tests
use.  No telescope products are needed."""
import functools

import numpy as np

import gains_cases as gc
import redcal_cases as rc

EPS = gc.EPS
# The constant of the bounds, by the rule of section 4.16: start at 4 and take the next power of two that brings the worst
# measured ratio of device error to bound under 0.5; the worst ratios per table are in DESIGN.md section 4.21.
K_MODELCAL = 4
DAMPING, TOL, MAXITER = 0.5, 1e-10, 500
# (ntime, interval): one sample; L = 1; a ragged last interval (17 = 4 x 4 + 1); L = 64, the last of 150 - 128 = 22
STEP_SHAPES = ((1, 1), (5, 1), (17, 4), (150, 64))
# (nf, nreal, m_nreal, w_nreal, weights, feed weights with one dead feed)
STEP_BATCHES = ((1, 1, 1, 1, False, False), (3, 1, 1, 1, True, False), (1, 3, 1, 1, True, True), (1, 3, 3, 3, False, True),
                (3, 3, 3, 3, True, True), (3, 3, 1, 3, True, False), (3, 3, 3, 1, True, False))

tables = rc.tables
SOLVABLE = rc.SOLVABLE


def nint_of(ntime, interval):
    return -(-ntime // interval)


def lengths(ntime, interval):
    """The samples L_q of every interval."""
    return np.diff(np.append(np.arange(0, ntime, interval), ntime))


def step_cases(table, ntime, interval, batches=STEP_BATCHES):
    """Yields (vis, model, w, fw, g0) on the host for every batch shape: random V and M, g0 within 20 % and 0.5 rad of
    one, weights with about a sixth of the samples flagged."""
    nfeed, off, mem = tables()[table] if isinstance(table, str) else table
    rng = np.random.default_rng(1000 * ntime + 10 * interval + nfeed)
    nmem, npairs, nint = mem.shape[0], off.shape[0] - 1, nint_of(ntime, interval)
    for nf, nreal, m_nreal, w_nreal, use_w, use_fw in batches:
        vis = gc.crandn(rng, nreal, nf, nmem, ntime)
        model = gc.crandn(rng, m_nreal, nf, npairs, ntime)
        w = rc.weights(rng, (w_nreal, nf, nmem, ntime)) if use_w else None
        fw = rc.feed_weights(rng, nfeed) if use_fw else None
        yield vis, model, w, fw, rc.gains_near_one(rng, nreal, nf, nfeed, nint)


def step_exact(vis, model, off, mem, g, interval, w=None, feed_weight=None, damping=DAMPING):
    """One iteration in np.clongdouble with what its bound needs: dict(g, step, den, gscale, d, lq, g0).
    gscale[..., a, q] = sum omega |V| |z| / den over the incidences of feed a and the samples of interval q (0 where
    den == 0), d[a] the incidences of feed a, lq[q] the samples of interval q."""
    from driftscan_amd import timestream

    nfeed, ntime = g.shape[-2], vis.shape[-1]
    gn, step, den = timestream.modelcal_step_host(vis, model, off, mem, g, interval, w=w, feed_weight=feed_weight,
                                                  damping=damping, dtype=np.clongdouble)
    fac = timestream.modelcal_weights(off, mem, nfeed, feed_weight)
    n = np.diff(off)
    cls = np.repeat(np.arange(n.shape[0]), n)
    use = np.nonzero(fac > 0)[0]
    i, j = mem[use, 0], mem[use, 1]
    va = np.abs(vis)[..., use, :].astype(np.longdouble)
    om = np.broadcast_to(fac[use, None] if w is None else (w * fac[:, None])[..., use, :], va.shape)
    gb = np.broadcast_to(g, vis.shape[:-2] + g.shape[-2:])
    ga = np.abs(gb).astype(np.longdouble)[..., np.arange(ntime) // interval]
    ma = np.broadcast_to(np.abs(model).astype(np.longdouble), vis.shape[:-2] + model.shape[-2:])[..., cls[use], :]
    mag = np.zeros((nfeed,) + gb.shape[:-2] + gb.shape[-1:], dtype=np.longdouble)
    starts = np.arange(0, ntime, interval)
    first = lambda x: np.moveaxis(np.add.reduceat(x, starts, axis=-1), -2, 0)
    if use.size:
        np.add.at(mag, i, first(om * va * ga[..., j, :] * ma))
        np.add.at(mag, j, first(om * va * ga[..., i, :] * ma))
    mag = np.moveaxis(mag, 0, -2)
    gscale = np.where(den > 0, mag / np.where(den > 0, den, 1), 0).astype(np.float64)
    d = np.bincount(np.concatenate([i, j]), minlength=nfeed)
    return dict(g=gn, step=step, den=den, gscale=gscale, d=d, lq=lengths(ntime, interval), g0=gb)


def gain_factor(ex, K=K_MODELCAL):
    """K (d_a L_q + 8) eps, (nfeed, nint): numerator and denominator are sums of d_a L_q products, and the quotient, the
    damped sum and the products add a fixed few roundings."""
    return K * (ex["d"][:, None] * ex["lq"][None, :] + 8) * EPS


def gain_bound(ex, K=K_MODELCAL):
    """K (d_a L_q + 8) eps [sum omega |V| |z| / den + |g_a|] per element of the new gains."""
    return gain_factor(ex, K) * (ex["gscale"] + np.abs(ex["g0"]).astype(np.float64))


def check_step(got_g, ex, K=K_MODELCAL):
    """The worst ratio of |got - exact| to `gain_bound`; a gain whose denominator is 0 must be g0 bit for bit.  Raises
    AssertionError when the bound is missed."""
    bg = gain_bound(ex, K)
    eg = np.abs(got_g - ex["g"]).astype(np.float64)
    assert got_g.shape == ex["g"].shape and np.all(np.isfinite(got_g))
    ratio = float((eg / np.maximum(bg, 1e-300)).max()) if eg.size else 0.0
    assert np.all(eg <= bg), "g misses its bound by %.3g" % ratio
    kept = np.asarray(ex["den"] == 0)
    assert np.array_equal(np.asarray(got_g)[kept], np.asarray(ex["g0"], dtype=np.complex128)[kept])
    return ratio


def check_gweight(got, ex, K=K_MODELCAL):
    """gweight against the long-double denominator: within K (d_a L_q + 8) eps of it, relatively (a sum of positive
    terms); exactly 0 where it is 0."""
    den = ex["den"].astype(np.float64)
    err = np.abs(got - ex["den"]).astype(np.float64)
    assert np.all(err <= gain_factor(ex, K) * den)
    return float((err / np.maximum(gain_factor(ex, K) * den, 1e-300)).max()) if err.size else 0.0


def chi2_bound(vis, off, mem, interval, w=None, feed_weight=None, nfeed=None, K=K_MODELCAL):
    """K (nmem L + 8) eps sum omega |V|^2 per interval."""
    from driftscan_amd import timestream

    fac = timestream.modelcal_weights(off, mem, nfeed, feed_weight)
    om = fac[:, None] if w is None else w * fac[:, None]
    per = (om * np.abs(vis) ** 2).sum(axis=-2)
    return K * (mem.shape[0] * interval + 8) * EPS * np.add.reduceat(per, np.arange(0, vis.shape[-1], interval), axis=-1)


def piecewise_gains(rng, shape, nfeed, ntime, interval):
    """Gains (shape, nfeed, nint) within 20 % and 0.5 rad of one and their spread over the samples (shape, nfeed, ntime)."""
    gq = rc.gains_near_one(rng, *(shape + (nfeed, nint_of(ntime, interval))))
    return gq, gq[..., np.arange(ntime) // interval]


def noise_free(rng, nfeed, off, mem, shape, ntime, interval):
    """(V, M, g_true (.., nfeed, nint)): V = g_i conj(g_j) M_c with a random complex model and piecewise constant gains."""
    from driftscan_amd import timestream

    gq, gt = piecewise_gains(rng, shape, nfeed, ntime, interval)
    model = gc.crandn(rng, *(shape + (off.shape[0] - 1, ntime)))
    return np.asarray(timestream.vis_expand_host(model, off, mem, g=gt), dtype=np.complex128), model, gq


def residual(vis, model, off, mem, g, interval, feed_weight=None):
    """r = max over the weighted members of |g_i conj(g_j) M_c - V_m| / max |V| (section 4.18's, with the model for y)."""
    from driftscan_amd import timestream

    fac = timestream.modelcal_weights(off, mem, g.shape[-2], feed_weight)
    gs = np.asarray(g)[..., np.arange(vis.shape[-1]) // interval]
    fit = timestream.vis_expand_host(model, off, mem, g=gs, dtype=np.clongdouble)
    return float(np.abs(fit - vis)[..., fac > 0, :].max() / np.abs(vis).max())


CONVERGED = dict(ntime=21, interval=8, tol=1e-12, maxiter=2000)


@functools.lru_cache(maxsize=None)
def converged_case(name):
    """Noise-free data of a solvable table (21 samples in intervals of 8, 8 and 5, a sixth of them flagged) and its
    solution by the complex128 statement, computed once: dict(vis, model, w, gt, g, info, r, dg) with r the residual and
    dg = max |g - g_true| after `modelcal_fix_phase(ref=g_true)`."""
    from driftscan_amd import timestream

    nfeed, off, mem = tables()[name]
    ntime, interval, tol, maxiter = (CONVERGED[k] for k in ("ntime", "interval", "tol", "maxiter"))
    rng = np.random.default_rng(21 + nfeed)
    vis, model, gt = noise_free(rng, nfeed, off, mem, (2, 1), ntime, interval)
    w = rc.weights(rng, (1, 1, mem.shape[0], ntime))
    g, info = timestream.modelcal_solve_host(vis, model, off, mem, interval, w=w, tol=tol, maxiter=maxiter)
    comp = timestream.modelcal_components(off, mem, nfeed, np.ones(off.shape[0] - 1))
    gf = timestream.modelcal_fix_phase(g, comp, ref=gt)
    return dict(vis=vis, model=model, w=w, gt=gt, g=g, info=info, comp=comp,
                r=residual(vis, model, off, mem, g, interval), dg=float(np.abs(gf - gt).max()))
