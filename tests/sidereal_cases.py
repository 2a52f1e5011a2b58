"""Shared cases of the sidereal-stacking tests: the geometries and flags of the issue's table,
the long-double reference of a stack of days, and the element-wise comparison both test files use.  All cases have two
frequencies; rows in {1, 5, 70} are a partial row tile, one tile and several."""
import numpy as np

EPS = 2.0**-53
NF = 2
ROWS = (1, 5, 70)
TWO_PI = 2 * np.pi
# input samples per turn of the downsampling cases: s = 93 / 37 = 2.5135, 161 / 64 = 2.5156, 377 / 150 = 2.5133
PER_TURN = {37: 93, 64: 161, 150: 377}
FOUR_DAYS = ((0.3, 92), (4.0, 92), (2.2, 60), (5.9, 40))   # (start, nt_in) at 93 samples per turn, in call order
# flagged runs (first sample, last sample of the window the run may lie in) of the four days: placed so that every
# grid sample keeps a day whose taps are all there (asserted on the host in tests/test_host_sidereal.py)
FOUR_DAYS_RUNS = ((14, 30), (9, 19), (5, 50), (3, 35))


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def equal_cadence(ntime, offset=0.37):
    """nt_in = ntime - 1 samples at the grid's own spacing, shifted by a fraction of a sample: (phi0, dphi, nt_in)."""
    d = TWO_PI / ntime
    return offset * d, d, ntime - 1


def on_grid(ntime):
    """The grid itself, as np.linspace writes it."""
    phi = np.linspace(0, TWO_PI, ntime, endpoint=False)
    return float(phi[0]), float((phi[-1] - phi[0]) / (ntime - 1)), ntime


def downsampling(ntime, start=0.3):
    n = PER_TURN[ntime]
    return start, TWO_PI / n, n - 1


def partial_arc():
    """40 samples from phi = 5.9 at 93 per turn: the day wraps through 2 pi and most of the grid gets nothing."""
    return 5.9, TWO_PI / 93, 40


def run_flags(rng, shape, window, length=(3, 7), isolated=0, weights=(0.5, 2.0)):
    """Weights in `weights` with one contiguous flagged run per row inside `window` (inclusive sample indices) and
    `isolated` single flags per row anywhere; the flag values are 0, negative and NaN in turn."""
    w = rng.uniform(weights[0], weights[1], size=shape)
    flat = w.reshape(-1, shape[-1])
    bad = (0.0, -1.0, np.nan)
    for i in range(flat.shape[0]):
        n = int(rng.integers(length[0], length[1] + 1))
        j0 = int(rng.integers(window[0], max(window[0], window[1] - n + 1) + 1))
        flat[i, j0 : j0 + n] = bad[i % 3]
        for j in rng.integers(0, shape[-1], size=isolated):
            flat[i, j] = bad[(i + 1) % 3]
    return w


def poison(x, w):
    """NaN planted in the data of every flagged sample."""
    x = x.copy()
    x[~(w > 0)] = np.nan + 1j * np.nan
    return x


def four_days(rng, nrow):
    """[(x, w, phi0, dphi)] of FOUR_DAYS with runs of flags, NaN in the flagged data."""
    days = []
    for (start, n), win in zip(FOUR_DAYS, FOUR_DAYS_RUNS):
        w = run_flags(rng, (NF, nrow, n), win)
        days.append((poison(crandn(rng, NF, nrow, n), w), w, start, TWO_PI / 93))
    return days


def stack_exact(days, ntime, a=3, min_share=1.0, base=None):
    """The accumulators of `days` = [(x, w or None, phi0, dphi)] in np.longdouble, in call order, on top of `base`
    (sum, wsum, sq, hits) when given: returns dict(sum, wsum, sq, hits, scale, T, D) with scale = sum_d W_d sum_j
    |c_j / S| |x_j|, T the largest tap count and D the number of days."""
    from driftscan_amd import timestream

    acc, T = None, 0
    for x, w, phi0, dphi in days:
        xh, W, det = timestream.sidereal_regrid_host(x, w, phi0, dphi, ntime, a=a, min_share=min_share,
                                                     dtype=np.clongdouble, details=True)
        T = max(T, int(det["ntaps"].max()))
        if acc is None:
            zero = np.zeros(xh.shape, dtype=np.longdouble)
            acc = dict(sum=zero.astype(np.clongdouble), wsum=zero.copy(), sq=zero.copy(),
                       hits=np.zeros(xh.shape, dtype=np.int64), scale=zero.copy())
            if base is not None:
                acc["sum"] += base[0]
                acc["wsum"] += base[1]
                acc["sq"] += base[2]
                acc["hits"] += base[3]
                acc["scale"] += np.abs(base[0])
        acc["sum"] += W * xh
        acc["wsum"] += W
        acc["sq"] += W * np.abs(xh) ** 2
        acc["hits"] += W > 0
        acc["scale"] += W * det["bound"]
    acc["T"], acc["D"] = T, len(days) + (0 if base is None else 1)
    return acc


def check_stack(got, ref, tol=None):
    """got = (sum, wsum, sq, hits) as numpy arrays against `stack_exact`: the validity pattern is equal and every element
    is within (T + D + 8) 2^-53 of its scale.  Returns the three worst ratios to the bound."""
    s_, ws_, sq_, h_ = got
    k = (ref["T"] + ref["D"] + 8) * EPS if tol is None else tol
    assert np.all(np.isfinite(s_)) and np.all(np.isfinite(ws_))
    assert np.array_equal(ws_ > 0, ref["wsum"] > 0), "validity pattern"
    ratios = []
    for name, g, bound in (("sum", s_, k * ref["scale"]), ("wsum", ws_, k * ref["wsum"])) + \
            ((("sq", sq_, k * ref["sq"]),) if sq_ is not None else ()):
        err = np.abs(g - ref[name]).astype(np.float64)
        b = bound.astype(np.float64)
        r = float((err / np.maximum(b, 1e-300)).max()) if err.size else 0.0
        assert np.all(err <= b), "%s: max err / bound = %.3g" % (name, r)
        ratios.append(r)
    if h_ is not None:
        assert np.array_equal(h_, ref["hits"]), "hits"
    return ratios
