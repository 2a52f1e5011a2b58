"""Shared cases of the unstacked-visibility tests: class tables, the extended-precision
statements of `Context.vis_stack` / `Context.vis_expand` with their rounding bounds, and the checker the GPU tests use.
No telescope products are needed."""
import numpy as np

import gains_cases as gc

EPS = gc.EPS
# The constant of the stack bounds: section 4.15 and 4.16 start from 4; the rule of section 4.16 (the next power of two that
# brings the worst measured ratio of device error to bound under 0.5) keeps it there — worst ratio at K = 4: see
# DESIGN.md section 4.17.
K_STACK = 4


def random_partition(nfeed, nmem, seed):
    """(class_off, members) of `nmem` random feed pairs of `nfeed` feeds cut into classes of uneven lengths: one of 200
    members (more than three times a wave's lanes), one of 65, singletons, and random lengths up to 40 for the rest.  The
    first and the last feed are named, so every row of a gain tile is read."""
    rng = np.random.default_rng(seed)
    lens = [200, 1, 65, 1, 1]
    while sum(lens) < nmem:
        lens.append(int(min(rng.integers(1, 41), nmem - sum(lens))))
    mem = rng.integers(0, nfeed, size=(sum(lens), 2))
    mem[0], mem[-1] = (0, nfeed - 1), (nfeed - 1, 0)
    return gc.table([[tuple(p) for p in mem[a:b]] for a, b in zip(np.cumsum([0] + lens[:-1]), np.cumsum(lens))])


def tables():
    """name -> (nfeed, class_off, members): {(0, 0)}, two feeds, the 70-feed line (a class of 69 beside classes of one),
    the 12-feed polarised 2 x 3 cylinder — all on the 16-sample gain tile."""
    return dict(gc.apply_tables())


# nfeed -> gain tile (8, 4, 2, 1): synthetic partitions of a few thousand pairs, so a case stays at a few MB at ntime = 5
TILE_NFEED = {300: 8, 600: 4, 1100: 2, 2100: 1}


def tile_table(nfeed):
    return (nfeed,) + random_partition(nfeed, 3000, nfeed)


def class_sizes(class_off):
    return np.diff(class_off)[:, None]


def stack_exact(vis, off, mem, w=None, g=None, feed_weight=None):
    """(out, wout, scale) of the statement in np.clongdouble / np.longdouble (`timestream.vis_stack_host`) and
    scale = sum_m w_m |g_i| |g_j| |V_m| / D (float64, 0 where D == 0), the first term of the bound on out."""
    from driftscan_amd import timestream

    out, wout = timestream.vis_stack_host(vis, off, mem, w=w, g=g, feed_weight=feed_weight, dtype=np.clongdouble)
    i, j = mem[:, 0], mem[:, 1]
    mag = np.abs(vis).astype(np.longdouble)
    den = np.ones(vis.shape, dtype=np.longdouble)
    if g is not None:
        ga = np.abs(g.astype(np.clongdouble))
        mag = ga[..., i, :] * ga[..., j, :] * mag
        den = den * (ga[..., i, :] * ga[..., j, :]) ** 2
    if w is not None:
        mag, den = w * mag, w * den
    if feed_weight is not None:
        fac = (np.asarray(feed_weight)[i] * np.asarray(feed_weight)[j])[:, None]
        mag, den = fac * mag, fac * den
    M = np.add.reduceat(mag, off[:-1], axis=-2)
    D = np.add.reduceat(den, off[:-1], axis=-2)
    scale = np.where(D > 0, M / np.where(D > 0, D, 1), 0).astype(np.float64)
    return out, wout, scale


def stack_bounds(out, wout, scale, off, K=K_STACK):
    """(bound on |delta out|, bound on |delta wout|) per element:
    K (n_c + 4) eps [sum_m w_m |g_i| |g_j| |V_m| / D + |out|] and K (n_c + 4) eps wout.  Numerator and denominator are
    sums of n_c products (n_c products and n_c - 1 additions each, every term below the sum of magnitudes), the weight,
    the gain products and the quotient add a fixed few roundings: hence n_c + 4."""
    n = class_sizes(off)
    f = K * (n + 4) * EPS
    return f * (scale + np.abs(out).astype(np.float64)), f * wout.astype(np.float64)


def check_stack(got_out, got_w, out, wout, scale, off, K=K_STACK):
    """Worst ratios (error of out / bound, error of wout / bound) of a device answer against the exact one; where the
    bound is 0 (a class with D == 0) the answer must be exactly 0.  Raises AssertionError when a bound is missed."""
    b_out, b_w = stack_bounds(out, wout, scale, off, K)
    e_out = np.abs(got_out - out).astype(np.float64)
    e_w = np.abs(got_w - wout).astype(np.float64)
    assert got_out.shape == out.shape and got_w.shape == wout.shape
    assert np.all(np.isfinite(got_out)) and np.all(np.isfinite(got_w))
    assert np.all(e_out <= b_out), "out misses its bound by %.3g" % float((e_out / np.maximum(b_out, 1e-300)).max())
    assert np.all(e_w <= b_w), "wout misses its bound by %.3g" % float((e_w / np.maximum(b_w, 1e-300)).max())
    r_out = float((e_out / np.maximum(b_out, 1e-300)).max()) if e_out.size else 0.0
    r_w = float((e_w / np.maximum(b_w, 1e-300)).max()) if e_w.size else 0.0
    return r_out, r_w


def expand_exact(sky, off, mem, g=None, base=None):
    """(want, bound) of `Context.vis_expand`: the statement in np.clongdouble, and 4 eps per product — g_i conj(g_j)
    and its product with the sky, so 8 eps |g_i| |g_j| |sky| with gains and nothing without — plus eps |result| for the
    sum with what the buffer held when accumulating."""
    from driftscan_amd import timestream

    want = timestream.vis_expand_host(sky, off, mem, g=g, dtype=np.clongdouble)
    if g is None:
        bound = np.zeros(want.shape)
    else:
        ga = np.abs(g)
        cls = np.repeat(np.arange(off.shape[0] - 1), np.diff(off))
        bound = 8 * EPS * ga[..., mem[:, 0], :] * ga[..., mem[:, 1], :] * np.abs(sky)[..., cls, :]
    if base is not None:
        want = want + base.astype(np.clongdouble)
        bound = bound + EPS * np.abs(want).astype(np.float64)
    return want, bound


def keep_one_per_class(rng, off, shape):
    """Random 0/1 weights of `shape` [..., nmem, ntime] with at least one kept member per class and sample."""
    w = (rng.uniform(size=shape) < 0.6).astype(np.float64)
    for c in range(off.shape[0] - 1):
        keep = rng.integers(off[c], off[c + 1], size=shape[:-2] + shape[-1:])
        np.put_along_axis(w, keep[..., None, :], 1.0, axis=-2)
    return w
