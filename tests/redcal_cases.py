"""Shared cases of the redundant-calibration tests: class tables, inputs, the bounds of one
iteration against extended precision and the checkers the CPU and GPU tests use.  No telescope products are needed."""
import functools

import numpy as np

import gains_cases as gc
import stack_cases as sc

EPS = gc.EPS
# The constant of the bounds: 4 as in sections 4.15 to 4.17, by the rule of section 4.16 (the next power of two that
# brings the worst measured ratio of device error to bound under 0.5); the worst ratios are in DESIGN.md section 4.18.
K_REDCAL = 4
DAMPING, TOL, MAXITER = 0.4, 1e-10, 500


def grid_table(nx, ny=1):
    """(nfeed, class_off, members) of a regular nx x ny grid of feeds: the autocorrelations as one class, then one class
    per displacement with its pairs (i, j), i > j, in feed order."""
    pos = [(x, y) for y in range(ny) for x in range(nx)]
    cl = {}
    for i in range(len(pos)):
        for j in range(i):
            cl.setdefault((pos[i][1] - pos[j][1], pos[i][0] - pos[j][0]), []).append((i, j))
    return (len(pos),) + gc.table([[(i, i) for i in range(len(pos))]] + [cl[k] for k in sorted(cl)])


@functools.lru_cache(maxsize=None)
def tables():
    """name -> (nfeed, class_off, members).  `two`: nothing is constrained.  `line3`, `grid43`, `line70` (the regular
    line of 70 feeds with all its baselines: 16-sample tile, classes of 69 down to 1 members; the nearest-neighbour table
    of gains_cases has two constrained classes only and does not converge in 2000 iterations) and `cyl12` (the polarised
    2 x 3 cylinder of stack_cases) are solvable."""
    t = sc.tables()
    return dict(two=t["two"], line3=grid_table(3), grid43=grid_table(4, 3), line70=grid_table(70), cyl12=t["cyl12"])


SOLVABLE = ("line3", "grid43", "line70", "cyl12")


def gains_near_one(rng, *shape):
    """Gains within 20 % in amplitude and 0.5 rad in phase of one."""
    return (1 + 0.2 * rng.uniform(-1, 1, shape)) * np.exp(0.5j * rng.uniform(-1, 1, shape))


def weights(rng, shape):
    """Inverse variances in (0, 1) with about a sixth of the samples flagged."""
    return rng.uniform(0.1, 1.0, size=shape) * (rng.uniform(size=shape) < 0.85)


def feed_weights(rng, nfeed, dead=True):
    fw = rng.uniform(0.5, 1.5, size=nfeed)
    if dead:
        fw[rng.integers(0, nfeed)] = 0.0
    return fw


def noise_free(rng, nfeed, off, mem, shape, ntime):
    """(V, g_true, y_true): V = g_i conj(g_j) y_c exactly representable up to the rounding of the products."""
    from driftscan_amd import timestream

    gt = gains_near_one(rng, *(shape + (nfeed, ntime)))
    yt = gc.crandn(rng, *(shape + (off.shape[0] - 1, ntime)))
    return np.asarray(timestream.vis_expand_host(yt, off, mem, g=gt), dtype=np.complex128), gt, yt


def step_exact(vis, off, mem, g, w=None, feed_weight=None, damping=DAMPING):
    """One iteration in np.clongdouble with what its bounds need: dict(g, y, step, yout, ywout, yscale, gscale, d, nmax).
    gscale[..., a, t] = sum omega |V| |z| / den over the incidences of feed a (0 where den == 0), d[a] the number of
    incidences of feed a, nmax[a] the largest class it touches."""
    from driftscan_amd import timestream

    nfeed = g.shape[-2]
    gn, y, step = timestream.redcal_step_host(vis, off, mem, g, w=w, feed_weight=feed_weight, damping=damping,
                                              dtype=np.clongdouble)
    yfac, gfac = timestream.redcal_weights(off, mem, nfeed, feed_weight)
    wy = yfac[:, None] if w is None else w * yfac[:, None]
    gb = np.broadcast_to(g, vis.shape[:-2] + g.shape[-2:])
    yout, ywout, yscale = sc.stack_exact(vis, off, mem, w=np.broadcast_to(wy, vis.shape), g=gb)
    n = np.diff(off)
    cls = np.repeat(np.arange(n.shape[0]), n)
    use = np.nonzero(gfac > 0)[0]
    i, j = mem[use, 0], mem[use, 1]
    om = np.broadcast_to(gfac[use, None] if w is None else (w * gfac[:, None])[..., use, :], vis[..., use, :].shape)
    ga, ya, va = np.abs(gb).astype(np.longdouble), np.abs(y)[..., cls[use], :], np.abs(vis)[..., use, :].astype(np.longdouble)
    mag = np.zeros((nfeed,) + vis.shape[:-2] + vis.shape[-1:], dtype=np.longdouble)
    den = np.zeros(mag.shape, dtype=np.longdouble)
    first = lambda x: np.moveaxis(x, -2, 0)
    np.add.at(mag, i, first(om * va * ga[..., j, :] * ya))
    np.add.at(mag, j, first(om * va * ga[..., i, :] * ya))
    np.add.at(den, i, first(om * (ga[..., j, :] * ya) ** 2))
    np.add.at(den, j, first(om * (ga[..., i, :] * ya) ** 2))
    mag, den = np.moveaxis(mag, 0, -2), np.moveaxis(den, 0, -2)
    gscale = np.where(den > 0, mag / np.where(den > 0, den, 1), 0).astype(np.float64)
    d = np.bincount(np.concatenate([i, j]), minlength=nfeed)
    nmax = np.zeros(nfeed, dtype=np.int64)
    np.maximum.at(nmax, i, n[cls[use]])
    np.maximum.at(nmax, j, n[cls[use]])
    return dict(g=gn, y=y, step=step, yout=yout, ywout=ywout, yscale=yscale, gscale=gscale, d=d, nmax=nmax, g0=gb)


def gain_bound(ex, K=K_REDCAL):
    """K (d_a + n_max + 8) eps [sum omega |V| |z| / den + |g_a|] per element of the new gains: numerator and denominator
    are sums of d_a products, each with a y_c that carries the (n_c + 4) eps of its own sums, and the quotient, the
    damped sum and the products add a fixed few roundings."""
    f = K * (ex["d"] + ex["nmax"] + 8)[:, None] * EPS
    return f * (ex["gscale"] + np.abs(ex["g0"]).astype(np.float64))


def check_step(got_g, got_y, ex, off, K=K_REDCAL):
    """Worst ratios (error of y / bound of section 4.17, error of g / gain_bound) of an answer against the exact
    iteration; a gain whose denominator is 0 must be g0 bit for bit.  Raises AssertionError when a bound is missed."""
    by, _ = sc.stack_bounds(ex["yout"], ex["ywout"], ex["yscale"], off, K)
    ey = np.abs(got_y - ex["yout"]).astype(np.float64)
    bg = gain_bound(ex, K)
    eg = np.abs(got_g - ex["g"]).astype(np.float64)
    assert got_g.shape == ex["g"].shape and got_y.shape == ex["yout"].shape
    assert np.all(np.isfinite(got_g)) and np.all(np.isfinite(got_y))
    ry = float((ey / np.maximum(by, 1e-300)).max()) if ey.size else 0.0
    rg = float((eg / np.maximum(bg, 1e-300)).max()) if eg.size else 0.0
    assert np.all(ey <= by), "y misses its bound by %.3g" % ry
    assert np.all(eg <= bg), "g misses its bound by %.3g" % rg
    kept = ex["gscale"] == 0
    assert np.array_equal(got_g[kept], np.asarray(ex["g0"], dtype=np.complex128)[kept])
    return ry, rg


def step_cases(name, ntime):
    """The shapes of the single-step tests on one table: nf, nreal in {1, 3}, w_nreal in {1, nreal}, with and without
    weights and feed weights (one dead feed).  Yields (vis, w, fw, g0) float64 / complex128 on the host."""
    nfeed, off, mem = tables()[name] if isinstance(name, str) else name
    rng = np.random.default_rng(100 * ntime + nfeed)
    for nf, nreal in ((1, 1), (3, 1), (1, 3), (3, 3)):
        for w_nreal in sorted({1, nreal}):
            for use_w, use_fw in ((False, False), (True, False), (True, True)):
                if w_nreal != 1 and not use_w:
                    continue
                vis = gc.crandn(rng, nreal, nf, mem.shape[0], ntime)
                w = weights(rng, (w_nreal, nf, mem.shape[0], ntime)) if use_w else None
                fw = feed_weights(rng, nfeed) if use_fw else None
                yield vis, w, fw, gains_near_one(rng, nreal, nf, nfeed, ntime)


def residual(vis, off, mem, g, y, feed_weight=None):
    """r = max over the weighted members of |g_i conj(g_j) y_c - V_m| / max |V|."""
    from driftscan_amd import timestream

    _, gfac = timestream.redcal_weights(off, mem, g.shape[-2], feed_weight)
    model = timestream.vis_expand_host(y, off, mem, g=g, dtype=np.clongdouble)
    return float(np.abs(model - vis)[..., gfac > 0, :].max() / np.abs(vis).max())


@functools.lru_cache(maxsize=None)
def converged_case(name, ntime=5, tol=1e-13, maxiter=2000):
    """Noise-free data of a solvable table and its solution by the complex128 statement, computed once: dict(vis, gt, yt,
    g, y, info, r, dg) with r the residual and dg = max |g - g_true| after `fix_degeneracies(ref=g_true)`."""
    from driftscan_amd import timestream

    nfeed, off, mem = tables()[name]
    rng = np.random.default_rng(7 + nfeed)
    vis, gt, yt = noise_free(rng, nfeed, off, mem, (2, 1), ntime)
    g, y, info = timestream.redcal_solve_host(vis, off, mem, tol=tol, maxiter=maxiter)
    gf, _ = timestream.fix_degeneracies(g, y, off, mem, ref=gt)
    return dict(vis=vis, gt=gt, yt=yt, g=g, y=y, info=info, r=residual(vis, off, mem, g, y),
                dg=float(np.abs(gf - gt).max()), tol=tol, maxiter=maxiter)


def chi2_bound(vis, off, mem, w=None, feed_weight=None, nfeed=None, K=K_REDCAL):
    """K (nmem + 8) eps sum omega |V|^2 per sample."""
    from driftscan_amd import timestream

    _, gfac = timestream.redcal_weights(off, mem, nfeed, feed_weight)
    om = gfac[:, None] if w is None else w * gfac[:, None]
    return K * (mem.shape[0] + 8) * EPS * (om * np.abs(vis) ** 2).sum(axis=-2)
