"""Shared cases of the per-feed gain tests: hand-made pair tables, the extended-precision
statement of the stacked baseline gain and the bounds of the device kernels.  No telescope products are needed."""
import numpy as np

EPS = np.finfo(np.float64).eps


def table(classes):
    """(class_off, members) int32 of a list of classes, each a list of (i, j)."""
    off = np.concatenate([[0], np.cumsum([len(c) for c in classes])]).astype(np.int32)
    mem = np.array([p for c in classes for p in c], dtype=np.int32).reshape(-1, 2)
    return off, mem


def line_table(nfeed):
    """A line of nfeed feeds: the nearest neighbours (nfeed - 1 members, more than a wave has lanes from nfeed = 66 on),
    then classes of one (the longest baseline, an auto-correlation), then the half-length baselines."""
    half = nfeed // 2
    return table([[(i + 1, i) for i in range(nfeed - 1)], [(nfeed - 1, 0)], [(0, 0)],
                  [(i + half, i) for i in range(nfeed - half)], [(nfeed - 1, nfeed - 1)]])


def cylinder_telescope(**over):
    """The polarised 2 x 3 cylinder of the tsim tests: 12 feeds."""
    from driftscan_amd import cylinder

    conf = dict(num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge", num_cylinders=2, cylinder_width=2.0,
                num_feeds=3, feed_spacing=0.4, tsys=1.0)
    conf.update(over)
    return cylinder.PolarisedCylinderTelescope.from_config(conf)


def apply_tables():
    """name -> (nfeed, class_off, members): the tables of the ts_gain_apply tests (all of them use the 16-sample tile)."""
    return {
        "one": (1,) + table([[(0, 0)]]),
        "two": (2,) + table([[(0, 0), (1, 1)], [(1, 0)], [(0, 1)]]),
        "line70": (70,) + line_table(70),
        "cyl12": (12,) + tuple(cylinder_telescope().redundant_pairs()),
    }


# nfeed at which dm_ts_gain_apply takes each of its other tiles: 8, 4, 2, 1, 1 with more than 64 KiB of LDS, and 1 with
# all 160 KiB of it, the most feeds it accepts
TILE_NFEED = {300: 8, 600: 4, 1100: 2, 2100: 1, 4200: 1, 10240: 1}


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def baseline_gains_exact(g, class_off, members):
    """(G, A): G[..., c, t] of `skysim.baseline_gains_host` summed in np.clongdouble, and
    A[..., c, t] = (1 / n_c) sum |g_i| |g_j| (float64), the scale of its rounding bound."""
    gl = g.astype(np.clongdouble)
    ga = np.abs(g)
    n = np.diff(class_off)
    i, j = members[:, 0], members[:, 1]
    prod = gl[..., i, :] * gl[..., j, :].conj()
    mag = ga[..., i, :] * ga[..., j, :]
    G = np.add.reduceat(prod, class_off[:-1], axis=-2) / n[:, None].astype(np.longdouble)
    A = np.add.reduceat(mag, class_off[:-1], axis=-2) / n[:, None]
    return G, A


def apply_bound(A, sky, class_off):
    """4 (n_c + 2) eps (1 / n_c) sum |g_i| |g_j| |sky| per element: n_c products and n_c - 1 additions of the class sum,
    the division and the product with the sky, each within eps / 2, with the project's factor 4 of slack on the count."""
    n = np.diff(class_off)
    return 4 * (n[:, None] + 2) * EPS * A * np.abs(sky)


def series_bound(model, coeff, ntime, sigma):
    """Bound on |x_device - x_host| of one component, [...] over the rows of coeff [..., K + 1]: the draw figure of
    DESIGN.md sections 4.12 / 4.13, 1e-13 of the scale sigma sum_k c_k of the coefficients, plus the synthesis bound of
    section 4.13 for a sum of K + 1 terms, 4 (2 K + 3) eps sum_k |coeff_k|."""
    ck = model.weights(ntime)
    K = ck.shape[0] - 1
    return 1e-13 * sigma * ck.sum() + 4 * (2 * K + 3) * EPS * np.abs(coeff).sum(axis=-1)
