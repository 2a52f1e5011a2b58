"""The host statements of the unstacked-visibility model, on the CPU: identities of
`timestream.vis_stack_host` / `vis_expand_host` in extended precision, the checker of the GPU tests, the table checks
the kernels share with their callers, and the noise statement by Monte-Carlo."""
import numpy as np
import pytest

import gains_cases as gc
import stack_cases as sc

EPS = sc.EPS


def _ts():
    from driftscan_amd import timestream

    return timestream


@pytest.fixture(scope="module")
def case():
    """The 70-feed line at (nreal, nf, ntime) = (2, 2, 5): sky, gains, expansion in clongdouble."""
    rng = np.random.default_rng(1)
    nfeed, off, mem = sc.tables()["line70"]
    sky = gc.crandn(rng, 2, 2, off.shape[0] - 1, 5)
    g = 1.0 + 0.3 * gc.crandn(rng, 2, 2, nfeed, 5)
    vis = _ts().vis_expand_host(sky, off, mem, g=g, dtype=np.clongdouble)
    return rng, nfeed, off, mem, sky, g, vis


def test_expand_then_stack_with_the_same_gains_returns_the_sky(case):
    rng, nfeed, off, mem, sky, g, vis = case
    w = rng.uniform(size=vis.shape) * (rng.uniform(size=vis.shape) < 0.7)
    w[:, :, off[3] : off[4], 2] = 0.0                      # class 3 wholly flagged at one sample
    out, wout = _ts().vis_stack_host(vis, off, mem, w=w, g=g, dtype=np.clongdouble)
    some = wout > 0
    assert some.any() and not some[:, :, 3, 2].any()
    err = np.abs(out - sky)[some].astype(np.float64)
    print("round trip in clongdouble: max |delta| = %.3g" % err.max())
    assert err.max() <= 1e-16 * np.abs(sky).max()
    assert np.all(out[~some] == 0) and np.all(wout[~some] == 0)


def test_uncalibrated_stack_is_the_baseline_gain_times_the_sky(case):
    from driftscan_amd import skysim

    rng, nfeed, off, mem, sky, g, vis = case
    out, wout = _ts().vis_stack_host(vis, off, mem, dtype=np.clongdouble)
    G = skysim.baseline_gains_host(g.astype(np.clongdouble), off, mem)
    assert np.abs(out - G * sky).max() <= 1e-16 * np.abs(sky).max()
    assert np.all(wout == 1.0)
    # float64 too: complete classes, unit weights, no gains -> exactly 1.0
    out64, wout64 = _ts().vis_stack_host(vis.astype(np.complex128), off, mem)
    assert wout64.dtype == np.float64 and np.all(wout64 == 1.0)
    ones = np.ones(vis.shape)
    assert np.all(_ts().vis_stack_host(vis.astype(np.complex128), off, mem, w=ones, feed_weight=np.ones(nfeed))[1] == 1.0)


def test_a_wholly_flagged_class_gives_exact_zeros(case):
    rng, nfeed, off, mem, sky, g, vis = case
    w = np.ones(vis.shape)
    w[:, :, off[0] : off[1]] = 0.0
    out, wout = _ts().vis_stack_host(vis, off, mem, w=w, g=g, dtype=np.clongdouble)
    assert np.all(out[:, :, 0] == 0) and np.all(wout[:, :, 0] == 0) and np.all(wout[:, :, 1:] > 0)
    # a dead feed: the classes (69, 0) and (0, 0) lose their only member, the nearest neighbours one of 69
    fw = np.ones(nfeed)
    fw[0] = 0.0
    out, wout = _ts().vis_stack_host(vis.astype(np.complex128), off, mem, feed_weight=fw)
    assert np.all(out[:, :, 1:3] == 0) and np.all(wout[:, :, 1:3] == 0)
    assert np.all(wout[:, :, 0] == 68.0 / 69.0)


def test_expand_without_gains_copies_and_accumulates(case):
    rng, nfeed, off, mem, sky, g, vis = case
    plain = _ts().vis_expand_host(sky, off, mem)
    cls = np.repeat(np.arange(off.shape[0] - 1), np.diff(off))
    assert plain.dtype == np.complex128 and np.array_equal(plain, sky[:, :, cls])
    base = gc.crandn(rng, *plain.shape)
    assert np.array_equal(_ts().vis_expand_host(sky, off, mem, out=base, accumulate=True), base + plain)
    with pytest.raises(ValueError):
        _ts().vis_expand_host(sky, [0, 2, 2], [[0, 1], [1, 0]])
    with pytest.raises(ValueError):
        _ts().vis_stack_host(vis, [1, 2], [[0, 1], [1, 0]])


def test_the_checker_rejects_twice_the_bound(case):
    rng, nfeed, off, mem, sky, g, vis = case
    v64 = vis.astype(np.complex128)
    w = sc.keep_one_per_class(rng, off, v64.shape)
    out, wout, scale = sc.stack_exact(v64, off, mem, w=w, g=g)
    got, gotw = _ts().vis_stack_host(v64, off, mem, w=w, g=g)
    r = sc.check_stack(got, gotw, out, wout, scale, off)
    print("numpy in float64 against clongdouble: out %.3g, wout %.3g of the bound" % r)
    b_out, b_w = sc.stack_bounds(out, wout, scale, off)
    assert np.all(b_out > 0) and np.all(b_w > 0)
    exact, exactw = out.astype(np.complex128), wout.astype(np.float64)
    sc.check_stack(exact, exactw, out, wout, scale, off)
    for idx in ((0, 0, 0, 0), (1, 1, 3, 4), (1, 0, off.shape[0] - 2, 2)):
        bad = exact.copy()
        bad[idx] += 2 * b_out[idx]
        with pytest.raises(AssertionError, match="out misses"):
            sc.check_stack(bad, exactw, out, wout, scale, off)
        badw = exactw.copy()
        badw[idx] *= 1 + 2 * sc.K_STACK * (sc.class_sizes(off)[idx[2], 0] + 4) * EPS
        with pytest.raises(AssertionError, match="wout misses"):
            sc.check_stack(exact, badw, out, wout, scale, off)


def test_tables_reach_every_gain_tile():
    for nfeed, tile in sc.TILE_NFEED.items():
        _, off, mem = sc.tile_table(nfeed)
        n = np.diff(off)
        assert off[-1] == mem.shape[0] and 3000 <= off[-1] < 3100 and n.min() == 1 and n.max() == 200
        assert mem.min() == 0 and mem.max() == nfeed - 1
        # the rule of dm_gain_tile: the largest power of two <= 16 with nfeed x tile x 16 B <= 64 KiB
        assert tile == max(t for t in (1, 2, 4, 8, 16) if nfeed * t * 16 <= 65536)


def test_monte_carlo_of_the_noise_statement():
    """One class of 6 pairs on 7 feeds, two of them removed by dead feeds: the per-member noise has variance n_c times
    the nominal, so the stack of the 4 that are left has 6 / 4 = 1 / W of it — not the nominal level."""
    rng = np.random.default_rng(5)
    off, mem = gc.table([[(k + 1, k) for k in range(6)]])
    R, nominal = 20000, 1.0
    vis = np.sqrt(6 * nominal / 2) * gc.crandn(rng, 6, R)
    fw = np.ones(7)
    fw[[0, 6]] = 0.0
    out, wout = _ts().vis_stack_host(vis, off, mem, feed_weight=fw)
    assert np.all(wout == 4.0 / 6.0)
    var = np.mean(np.abs(out[0]) ** 2)
    print("variance of the stack: %.4f, nominal / W = %.4f" % (var, nominal / wout[0, 0]))
    assert abs(var / (nominal / wout[0, 0]) - 1) <= 5 / np.sqrt(R)
    assert abs(var / nominal - 1) > 0.2
    full, wfull = _ts().vis_stack_host(vis, off, mem)
    assert np.all(wfull == 1.0) and abs(np.mean(np.abs(full[0]) ** 2) / nominal - 1) <= 5 / np.sqrt(R)


def test_the_noise_statistic_of_the_gpu_test_holds_on_the_host():
    """The statistic of the noise-only end-to-end test at its sizes (the 12-feed cylinder's table, nreal = 8, 3
    frequencies, ntime = 183 = ceil(2.5 x 73)), on numpy draws: per class z = (mean |v|^2 / nominal - 1) sqrt(K) within 5,
    complete and with a dead feed against 1 / W."""
    rng = np.random.default_rng(9)
    nfeed, off, mem = sc.tables()["cyl12"]
    n = np.diff(off)
    nreal, nf, ntime = 8, 3, 183
    sigma = np.repeat(np.sqrt(n / 2.0), n)[:, None]
    vis = sigma * gc.crandn(rng, nreal, nf, off[-1], ntime)
    K = nreal * nf * ntime
    out, wout = _ts().vis_stack_host(vis, off, mem)
    z = (np.mean(np.abs(out) ** 2, axis=(0, 1, 3)) - 1) * np.sqrt(K)
    print("complete: max |z| = %.2f" % np.abs(z).max())
    assert np.all(wout == 1.0) and np.abs(z).max() <= 5
    fw = np.ones(nfeed)
    fw[0] = 0.0
    out, wout = _ts().vis_stack_host(vis, off, mem, feed_weight=fw)
    W = wout[0, 0, :, 0]
    left = W > 0
    assert left.any() and (~left).any() and np.any((W > 0) & (W < 1))
    z = (np.mean(np.abs(out) ** 2, axis=(0, 1, 3))[left] * W[left] - 1) * np.sqrt(K)
    print("dead feed: max |z| = %.2f" % np.abs(z).max())
    assert np.abs(z).max() <= 5
