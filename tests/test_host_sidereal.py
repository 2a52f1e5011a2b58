"""Sidereal stacking on the host: `timestream.sidereal_regrid_host` in double against itself in
long double within the bounds the device is held to, planted errors that must not pass, the identities of the method,
and the method itself on a band-limited signal.  No GPU."""
import numpy as np
import pytest

import sidereal_cases as sc
from driftscan_amd import timestream


def _stack_double(days, ntime, a=3, min_share=1.0, regrid=None):
    """The accumulators of `days` with the restatement in double, as (sum, wsum, sq, hits)."""
    regrid = regrid or timestream.sidereal_regrid_host
    acc = None
    for x, w, phi0, dphi in days:
        xh, W = regrid(x, w, phi0, dphi, ntime, a=a, min_share=min_share)
        part = [W * xh, W, W * np.abs(xh) ** 2, (W > 0).astype(np.int64)]
        acc = part if acc is None else [u + v for u, v in zip(acc, part)]
    return acc


def _cases(rng, nrow):
    """(name, days, ntime, a, min_share) of the issue's table for one row count."""
    out = []
    for ntime in (37, 64):
        for a in (1, 3, 5):
            p, d, n = sc.equal_cadence(ntime)
            out.append(("equal cadence", [(sc.crandn(rng, sc.NF, nrow, n), None, p, d)], ntime, a, 1.0))
        p, d, n = sc.on_grid(ntime)
        w = sc.run_flags(rng, (sc.NF, nrow, n), (0, n - 1), isolated=6)
        out.append(("on grid", [(sc.poison(sc.crandn(rng, sc.NF, nrow, n), w), w, p, d)], ntime, 3, 1.0))
    for a in (3, 5):
        p, d, n = sc.downsampling(37)
        out.append(("downsampling", [(sc.crandn(rng, sc.NF, nrow, n), None, p, d)], 37, a, 1.0))
    p, d, n = sc.downsampling(150)
    out.append(("several tiles", [(sc.crandn(rng, sc.NF, nrow, n), None, p, d)], 150, 3, 1.0))
    p, d, n = -7.3, sc.TWO_PI / 1000, 500     # 320 taps per sample: the row tile shrinks to what LDS holds
    w = sc.run_flags(rng, (sc.NF, nrow, n), (0, n - 1), isolated=3)
    out.append(("wide taps", [(sc.poison(sc.crandn(rng, sc.NF, nrow, n), w), w, p, d)], 50, 8, 0.8))
    p, d, n = sc.partial_arc()
    out.append(("partial arc", [(sc.crandn(rng, sc.NF, nrow, n), None, p, d)], 37, 3, 1.0))
    p, d, n = sc.downsampling(37)
    for ms in (1.0, 0.8):
        w = sc.run_flags(rng, (sc.NF, nrow, n), (0, n - 1), isolated=3)
        out.append(("flags", [(sc.poison(sc.crandn(rng, sc.NF, nrow, n), w), w, p, d)], 37, 3, ms))
    out.append(("four days", sc.four_days(rng, nrow), 37, 3, 1.0))
    return out


@pytest.mark.parametrize("nrow", sc.ROWS)
def test_double_against_long_double(nrow):
    """Every case of the table: the validity pattern and the hits are equal and sum, wsum and sq are within
    (T + D + 8) 2^-53 of their scales — what tests/test_gpu_sidereal.py asks of the device."""
    rng = np.random.default_rng(100 + nrow)
    for name, days, ntime, a, ms in _cases(rng, nrow):
        ref = sc.stack_exact(days, ntime, a=a, min_share=ms)
        r = sc.check_stack(_stack_double(days, ntime, a, ms), ref)
        print("%-14s ntime %3d a %d min_share %.1f: T %2d, err / bound: sum %.2f wsum %.2f sq %.2f, valid %.2f"
              % ((name, ntime, a, ms, ref["T"]) + tuple(r) + (float((ref["hits"] > 0).mean()),)))
        if name == "flags":
            assert 0 < (ref["hits"] > 0).mean() < 1
    # min_share 0.8 keeps samples that 1.0 loses, and never the other way round
    days = _cases(np.random.default_rng(5), 5)[-2][1]
    strict = sc.stack_exact(days, 37, min_share=1.0)["hits"]
    loose = sc.stack_exact(days, 37, min_share=0.8)["hits"]
    assert np.all(loose >= strict) and loose.sum() > strict.sum()


def test_four_days_leave_no_grid_sample_uncovered():
    """The flags of the four-day case are runs placed so that the long-double restatement alone covers every grid
    sample of every row with min_share = 1; single days do not."""
    for nrow in sc.ROWS:
        days = sc.four_days(np.random.default_rng(nrow), nrow)
        ref = sc.stack_exact(days, 37)
        assert ref["hits"].min() >= 1 and ref["hits"].max() >= 3
        for day in days:
            assert sc.stack_exact([day], 37)["hits"].min() == 0


def test_planted_errors_do_not_pass(monkeypatch):
    """A wrong s, a missing division by S, a flagged tap let through and a hit counted for an invalid sample all fail the
    comparison that the correct restatement passes."""
    rng = np.random.default_rng(7)
    p, d, n = sc.downsampling(37)
    w = sc.run_flags(rng, (sc.NF, 5, n), (0, n - 1), isolated=2)
    x = sc.poison(sc.crandn(rng, sc.NF, 5, n), w)
    days = [(x, w, p, d)]
    ref = sc.stack_exact(days, 37, min_share=0.8)
    sc.check_stack(_stack_double(days, 37, 3, 0.8), ref)

    def acc_of(xh, W):
        return [W * xh, W, W * np.abs(xh) ** 2, (W > 0).astype(np.int64)]

    xh, W = timestream.sidereal_regrid_host(x, w, p, d, 37, min_share=0.8)
    # no division by S: xh S instead of xh, with S of the long-double statement
    taps = timestream.sidereal_taps_host(n, 37, 3, p, d)
    S = np.zeros(xh.shape)
    for k, (first, c) in enumerate(taps):
        j = first + np.arange(len(c))
        ins = (j >= 0) & (j < n)
        S[..., k] = (np.where(w[..., j[ins]] > 0, c[ins].astype(np.float64), 0)).sum(axis=-1)
    assert np.abs(S[W > 0] - 1).max() > 0.1
    with pytest.raises(AssertionError):
        sc.check_stack(acc_of(xh * S, W), ref)
    # a flagged tap let through (its data made finite so that only the rule is at fault)
    w_open = np.where(w > 0, w, 1.0)
    x_fin = np.where(w > 0, x, 1.0 + 0j)
    with pytest.raises(AssertionError):
        sc.check_stack(acc_of(*timestream.sidereal_regrid_host(x_fin, w_open, p, d, 37, min_share=0.8)), ref)
    # a hit counted for an invalid sample
    bad = acc_of(xh, W)
    f, r, k = (int(v[0]) for v in np.nonzero(W == 0))
    bad[3][f, r, k] += 1
    with pytest.raises(AssertionError, match="hits"):
        sc.check_stack(bad, ref)
    # a wrong s: the kernel not stretched to the coarser spacing
    monkeypatch.setattr(timestream, "_sidereal_stretch", lambda step: np.longdouble(1))
    with pytest.raises(AssertionError):
        sc.check_stack(_stack_double(days, 37, 3, 0.8), ref)


def test_identities():
    rng = np.random.default_rng(11)
    # on-grid input is copied exactly with W = w, even with every neighbour flagged
    for ntime in (37, 64):
        p, d, n = sc.on_grid(ntime)
        x = sc.crandn(rng, 3, n)
        w = rng.uniform(0.5, 2.0, size=(3, n))
        w[:, ::2] = 0.0                               # every neighbour of an odd sample is flagged
        xh, W = timestream.sidereal_regrid_host(sc.poison(x, w), w, p, d, ntime)
        assert np.array_equal(W, w) and np.array_equal(xh[w > 0], x[w > 0]) and np.all(xh[w == 0] == 0)
        assert all(len(c) == 1 and c[0] == 1 for _, c in timestream.sidereal_taps_host(n, ntime, 3, p, d))
        # the same day with its start given one turn on
        xh2, _ = timestream.sidereal_regrid_host(x, None, p + 2 * np.pi, d, ntime)
        assert np.array_equal(xh2, x)
    # with min_share = 1 a tap beyond the end of the day invalidates the sample
    p, d, n = sc.downsampling(37)
    taps = timestream.sidereal_taps_host(n, 37, 3, p, d)
    beyond = np.array([first < 0 or first + len(c) > n for first, c in taps])
    _, W = timestream.sidereal_regrid_host(np.ones((1, n), dtype=np.complex128), None, p, d, 37)
    assert beyond.any() and not beyond.all() and np.array_equal(W[0] == 0, beyond)
    _, W8 = timestream.sidereal_regrid_host(np.ones((1, n), dtype=np.complex128), None, p, d, 37, min_share=0.8)
    assert (W8[0] > 0).sum() > (W[0] > 0).sum()
    # constant data come out as 1 to rounding for any flags that leave the sample valid
    w = sc.run_flags(rng, (40, n), (0, n - 1), isolated=4)
    for ms in (1.0, 0.6):
        xh, W = timestream.sidereal_regrid_host(sc.poison(np.ones((40, n), dtype=np.complex128), w), w, p, d, 37,
                                                min_share=ms)
        assert (W > 0).any() and np.abs(xh[W > 0] - 1).max() <= 32 * sc.EPS
    # unit weights and every tap there: W = S^2 / sum c^2, more than one sample's weight when downsampling
    _, W1 = timestream.sidereal_regrid_host(np.ones((1, n), dtype=np.complex128), None, p, d, 37)
    assert W1[W1 > 0].min() > 1.5
    for bad in (dict(a=0), dict(a=9), dict(min_share=0.0), dict(min_share=1.5)):
        with pytest.raises(ValueError):
            timestream.sidereal_regrid_host(np.ones((1, n), dtype=np.complex128), None, p, d, 37, **bad)
    with pytest.raises(ValueError):
        timestream.sidereal_regrid_host(np.ones((1, n), dtype=np.complex128), None, p, -d, 37)
    with pytest.raises(ValueError):
        timestream.sidereal_regrid_host(np.ones((1, 95), dtype=np.complex128), None, p, d, 37)    # a turn and more


# (ntime, input samples per turn, a, the issue's bound: twice the long-double figure of the formula)
METHOD = ((37, 37, 3, 2e-2), (37, 93, 5, 3e-3), (64, 161, 3, 3e-3))


@pytest.mark.parametrize("ntime,per_turn,a,bound", METHOD)
def test_method_on_a_band_limited_signal(ntime, per_turn, a, bound):
    """mmax = 8, random coefficients: the regridded value against the exact one, worst over 11 sample offsets and over
    the valid grid samples, relative to the largest |signal|.  The bounds catch a wrong formula; they do not grade
    Lanczos.  Measured in long double: 1.06e-2, 1.35e-3 and 1.22e-3."""
    ld = np.longdouble
    rng = np.random.default_rng(3)
    mm = np.arange(-8, 9)
    coef = sc.crandn(rng, 17)
    twopi = 2 * timestream._ld_pi()
    dphi = float(twopi / per_turn)
    n = per_turn - 1

    def signal(phi):
        return (coef[None, :] * np.exp(1j * mm[None, :].astype(ld) * np.asarray(phi, dtype=ld)[:, None])).sum(axis=-1)

    grid = twopi * np.arange(ntime) / ntime
    worst = 0.0
    for i in range(11):
        phi0 = float((i / 11.0) * dphi + 0.3)
        x = signal(ld(phi0) + ld(dphi) * np.arange(n))
        xh, W = timestream.sidereal_regrid_host(x[None], None, phi0, dphi, ntime, a=a, dtype=np.clongdouble)
        ok = W[0] > 0
        assert ok.sum() >= ntime - 2 * a - 2
        worst = max(worst, float(np.abs(xh[0][ok] - signal(grid)[ok]).max() / np.abs(signal(grid)).max()))
    print("ntime %d from %d per turn, a = %d: worst relative error %.3g (bound %.0e)" % (ntime, per_turn, a, worst, bound))
    assert bound / 20 < worst <= bound
