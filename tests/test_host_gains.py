"""CPU-only: the host side of the per-feed gain errors — the pair table of
`TransitTelescope.redundant_pairs`, the counter layout and the statistics of the numpy restatement (`skysim.gains_host`,
the oracle of the device route), the identities of `skysim.baseline_gains_host` and the per-m `simulate` with gains."""
import os
import types

import numpy as np
import pytest

import gains_cases as gc
import telescope_cases as tc

EPS = gc.EPS


# ---- the pair table -------------------------------------------------------------------------------------------------------
def _check_pairs(tel):
    off, mem = tel.redundant_pairs()
    assert off.dtype == np.int32 and mem.dtype == np.int32
    assert off.shape == (tel.npairs + 1,) and off[0] == 0 and mem.shape == (off[-1], 2)
    assert np.array_equal(np.diff(off), tel.redundancy)
    fmap, mask, conj = np.asarray(tel.feedmap), np.asarray(tel.feedmask), np.asarray(tel.feedconj)
    listed = set()
    for c in range(tel.npairs):
        m = mem[off[c] : off[c + 1]]
        assert np.all(fmap[m[:, 0], m[:, 1]] == c) and np.all(mask[m[:, 0], m[:, 1]])
        assert not np.any(conj[m[:, 0], m[:, 1]])                       # no conjugate-marked pair
        flat = m[:, 0].astype(np.int64) * tel.nfeed + m[:, 1]
        assert np.all(np.diff(flat) > 0)                                # row-major (i, j) order
        assert tuple(tel.uniquepairs[c]) in {tuple(p) for p in m.tolist()}
        assert tuple(tel.uniquepairs[c]) == tuple(m[0])
        listed.update(tuple(p) for p in m.tolist())
    assert len(listed) == mem.shape[0]
    # every unordered masked pair exactly once: as itself or, when it is marked conjugate, as its transpose
    want = {}
    for i, j in zip(*np.nonzero(mask)):
        key = (min(i, j), max(i, j))
        want[key] = want.get(key, 0) + 1
    got = {}
    for i, j in mem.tolist():
        key = (min(i, j), max(i, j))
        got[key] = got.get(key, 0) + 1
    assert set(got) == set(want) and all(v == 1 for v in got.values())
    assert tel.redundant_pairs()[1] is mem                              # cached with the pairs
    return off, mem


@pytest.mark.parametrize("name", ["gmrt", "restricted_box", "restricted_pol_gauss", "restricted_extra", "random", "gradient",
                                  "extra", "perturbed", "dish_pol"])
def test_redundant_pairs_of_the_telescope_classes(golden_dir, name):
    gold = np.load(os.path.join(golden_dir, "telescopes.npz"))
    _check_pairs(tc.build(gold, name))


@pytest.mark.parametrize("over", [dict(), dict(auto_correlations=True), dict(minlength=0.5), dict(maxlength=1.0),
                                  dict(minlength=0.5, maxlength=2.1, auto_correlations=True), dict(num_feeds=5, num_cylinders=3)])
def test_redundant_pairs_of_polarised_cylinders(over):
    tel = gc.cylinder_telescope(**over)
    off, mem = _check_pairs(tel)
    if over.get("auto_correlations") and "minlength" not in over:
        assert np.any(mem[:, 0] == mem[:, 1])
    tel._finalise_config()                                              # the cache goes with the pairs
    assert tel._pairs is None and np.array_equal(tel.redundant_pairs()[1], mem)


# ---- the draws ------------------------------------------------------------------------------------------------------------
def test_gain_model_arguments():
    from driftscan_amd import skysim

    m = skysim.GainModel.from_config(dict(sigma_amp=0.01, sigma_phase=0.02, corr_time=600.0, freq_corr="full", seed=5))
    assert (m.sigma_amp, m.sigma_phase, m.corr_time, m.freq_corr, m.seed) == (0.01, 0.02, 600.0, "full", 5)
    d = skysim.GainModel()
    assert (d.sigma_amp, d.sigma_phase, d.corr_time, d.freq_corr, d.seed) == (0.0, 0.0, 0.0, "none", 0)
    for bad in (dict(sigma_amp=-1.0), dict(freq_corr="some"), dict(corr_time=-1.0)):
        with pytest.raises(ValueError):
            skysim.GainModel(**bad)
    with pytest.raises(ValueError):
        skysim.GainModel.from_config(dict(sigma=0.1))
    assert isinstance(skysim.as_gains(dict(sigma_amp=0.1)), skysim.GainModel) and skysim.as_gains(None) is None
    with pytest.raises(ValueError):
        skysim.as_gains(np.ones((3, 4)))
    # K and the weights: (ntime - 1) // 2, capped where exp(-(2 pi k tau / T)^2 / 2) < 2^-53
    assert [d.kmax(n) for n in (1, 2, 5, 17, 64)] == [0, 0, 2, 8, 31]
    tau = 3600.0
    m = skysim.GainModel(corr_time=tau)
    K = m.kmax(100001)
    s = lambda k: np.exp(-0.5 * (2 * np.pi * k * tau / skysim.T_SIDEREAL) ** 2)
    assert K < 50000 and s(K) >= 2.0**-53 > s(K + 1)
    for mod, n in ((d, 17), (m, 17), (m, 1025), (d, 64)):
        c = mod.weights(n)
        assert c.shape == (mod.kmax(n) + 1,) and abs(np.sum(c**2) - 1.0) <= 4 * EPS
        assert abs(mod.correlation(n, 0) - 1.0) <= 4 * EPS
    assert np.all(d.weights(17) == d.weights(17)[0])                    # corr_time = 0: equal weights
    # ... which for odd ntime is white but for the k = 0 term, whose single coefficient A_0 carries the weight that two
    # (A_k, B_k) share elsewhere: sum_{k <= K} cos(2 pi k D / ntime) = 1 / 2, so every lag D != 0 correlates by
    # 1 / (2 (K + 1)) = 1 / (ntime + 1) exactly (a common offset of variance sigma^2 / (ntime + 1)), and by nothing more
    assert max(abs(d.correlation(17, lag) - 1.0 / 18.0) for lag in range(1, 17)) <= 16 * EPS


def test_gain_stream_depends_on_its_six_numbers_only():
    """(seed, feed, global frequency or the broadband marker, k, realisation, component) fix a coefficient."""
    from driftscan_amd import skysim

    m = skysim.GainModel(0.1, 0.2, corr_time=1800.0, seed=3)
    fg = np.array([0, 1, 2, 5])
    A, P = skysim.STREAM_TS_GAIN_AMP, skysim.STREAM_TS_GAIN_PHASE
    assert (A, P) == (25, 26)
    full = skysim.gain_coeff_host(m, 5, fg, 17, 4, stream=A)
    assert full.shape == (4, 4, 5, 9) and full.dtype == np.complex128
    # rows of a frequency subset, a realisation range, fewer feeds, fewer k (a shorter day has the first coefficients'
    # draws: compare the unit draws, the weights differ)
    assert np.array_equal(skysim.gain_coeff_host(m, 5, fg[[1, 3]], 17, 4, stream=A), full[:, [1, 3]])
    assert np.array_equal(skysim.gain_coeff_host(m, 5, fg, 17, 2, first=2, stream=A), full[2:4])
    assert np.array_equal(skysim.gain_coeff_host(m, 3, fg, 17, 4, stream=A), full[:, :, :3])
    white = skysim.GainModel(0.1, 0.2, seed=3)
    w17, w9 = skysim.gain_coeff_host(white, 5, fg, 17, 4, stream=A), skysim.gain_coeff_host(white, 5, fg, 9, 4, stream=A)
    assert np.all(np.abs(w9 / white.weights(9)[0] - w17[..., :5] / white.weights(17)[0]) <= 8 * EPS * np.abs(w9 / white.weights(9)[0]))
    # it scales with sigma, and the other sigma does not enter
    twice = skysim.gain_coeff_host(skysim.GainModel(0.2, 0.7, corr_time=1800.0, seed=3), 5, fg, 17, 4, stream=A)
    assert np.all(np.abs(twice - 2.0 * full) <= 4 * EPS * np.abs(twice))
    # realisations, seeds, frequencies, feeds and components are different draws
    other = skysim.gain_coeff_host(m, 5, fg, 17, 4, stream=P) / 2.0
    seed4 = skysim.gain_coeff_host(skysim.GainModel(0.1, 0.2, corr_time=1800.0, seed=4), 5, fg, 17, 4, stream=A)
    assert not np.any(full[0] == full[1]) and not np.any(full == seed4) and not np.any(full == other)
    assert not np.any(full[:, 0] == full[:, 1]) and not np.any(full[:, :, 0] == full[:, :, 1])
    assert not np.any(full[..., 0] / m.weights(17)[0] == full[..., 1] / m.weights(17)[1])
    # apart from the noise and the sky streams at the same counters
    n = skysim.noise_host(np.ones((4, 5)), fg, 9, 4, seed=3)            # counter (pair, f, t, r): the same four numbers
    assert not np.any(n.conj() * (0.1 * m.weights(17) * 2**0.5) == full)
    # broadband: every frequency row the same, and none of them a channel's
    bb = skysim.gain_coeff_host(skysim.GainModel(0.1, 0.2, corr_time=1800.0, freq_corr="full", seed=3), 5, fg, 17, 4, stream=A)
    assert np.array_equal(bb, np.broadcast_to(bb[:, :1], bb.shape)) and not np.any(bb == full)
    with pytest.raises(ValueError):
        skysim.gain_coeff_host(m, 5, fg, 17, 2, first=(1 << 24) - 1)
    with pytest.raises(ValueError):
        skysim.gain_coeff_host(m, 5, fg, 17, 2, stream=skysim.STREAM_TS_NOISE)
    # gains_host: the rows of subsets again, through the series and the exponential
    g = skysim.gains_host(m, 5, fg, 17, 4)
    assert g.shape == (4, 4, 5, 17) and g.dtype == np.complex128
    assert np.array_equal(skysim.gains_host(m, 5, fg[[0, 2]], 17, 2, first=1), g[1:3][:, [0, 2]])
    one = skysim.gains_host(skysim.GainModel(seed=9), 5, fg, 17, 4)
    assert np.array_equal(one, np.ones_like(one))                       # zero sigmas: exactly 1


# ---- statistics -----------------------------------------------------------------------------------------------------------
def gain_statistics(model, g, lags):
    """[(max |d|, rms d)] of the normalised deviations over the (frequency, feed) cells and the two components of gains g
    (nreal, nf, nfeed, ntime): the mean, the variance and the cyclic lag products at `lags`.  With
    x = sigma sum_k c_k (A_k cos + B_k sin) and k <= K < ntime / 2 the time averages of one realisation are
        mean_t x = sigma c_0 A_0,   mean_t x(t) x(t + D) = sigma^2 (c_0^2 A_0^2 + sum_{k>=1} c_k^2 (A_k^2 + B_k^2) / 2 cos(2 pi k D / ntime))
    exactly, so E = sigma^2 sum_k c_k^2 cos(2 pi k D / ntime) — the model correlation — and
    Var = sigma^4 (2 c_0^4 + sum_{k>=1} c_k^4 cos^2(2 pi k D / ntime)); D = 0 is the variance."""
    nreal, ntime = g.shape[0], g.shape[-1]
    c = model.weights(ntime)
    k = np.arange(c.shape[0])
    comps = [(np.abs(g) - 1.0, model.sigma_amp), (np.angle(g), model.sigma_phase)]
    out = []
    mean = np.concatenate([(x.mean(axis=(0, 3)) / (s * c[0] / np.sqrt(nreal))).ravel() for x, s in comps])
    out.append(mean)
    for lag in (0,) + tuple(lags):
        cs = np.cos(2 * np.pi * k * lag / ntime)
        expect = np.sum(c**2 * cs)
        assert abs(expect - model.correlation(ntime, lag)) <= 4 * EPS
        sd = np.sqrt((2 * c[0] ** 4 * cs[0] ** 2 + np.sum(c[1:] ** 4 * cs[1:] ** 2)) / nreal)
        out.append(np.concatenate([(((x * np.roll(x, -lag, axis=-1)).mean(axis=(0, 3)) / s**2 - expect) / sd).ravel()
                                   for x, s in comps]))
    return [(float(np.abs(d).max()), float(np.sqrt((d**2).mean()))) for d in out]


GAIN_STATS = {
    0.0: [(2.55, 0.93), (2.54, 1.05), (2.91, 1.05), (3.27, 1.09), (2.49, 1.02)],
    3600.0: [(2.55, 0.93), (2.93, 0.93), (2.93, 0.93), (2.93, 0.93), (2.89, 0.94)],
}


@pytest.mark.parametrize("corr_time", [0.0, 3600.0])
def test_gain_statistics(corr_time):
    """Mean, variance and lag products (lags 1, 2 and 7 samples) of x_amp and x_phase over 64 realisations of 257 samples
    against the exact model values; 64 cells x 2 components = 128 normalised deviations each: the project's band of
    DESIGN.md section 4.12 is max |d| < 5 and 0.6 < rms < 1.4."""
    from driftscan_amd import skysim

    model = skysim.GainModel(0.05, 0.03, corr_time=corr_time, seed=11)
    g = skysim.gains_host(model, 16, np.arange(4), 257, 64)
    stats = gain_statistics(model, g, (1, 2, 7))
    print("gains_host statistics, corr_time = %g (max |d|, rms):" % corr_time, stats)
    for dmax, rms in stats:
        assert dmax < 5.0 and 0.6 < rms < 1.4, stats
    # the figures this counter layout and seed give (recorded in DESIGN.md section 4.15)
    assert [(round(a, 2), round(b, 2)) for a, b in stats] == GAIN_STATS[corr_time]


# ---- the stacked baseline gain --------------------------------------------------------------------------------------------
def test_baseline_gains_identities():
    from driftscan_amd import skysim

    rng = np.random.default_rng(6)
    tel = gc.cylinder_telescope()
    off, mem = tel.redundant_pairs()
    nfeed, ntime = tel.nfeed, 17
    # a phase common to all feeds drops out
    phi = rng.uniform(0.0, 2 * np.pi, size=(2, 3, 1, ntime))
    G = skysim.baseline_gains_host(np.broadcast_to(np.exp(1j * phi), (2, 3, nfeed, ntime)), off, mem)
    assert G.shape == (2, 3, tel.npairs, ntime)
    print("common phase: max |G - 1| / eps = %.3g" % (np.abs(G - 1.0).max() / EPS))
    assert np.abs(G - 1.0).max() <= 4 * EPS
    # a common constant gives |c|^2
    c = 0.8 - 0.7j
    G = skysim.baseline_gains_host(np.full((3, nfeed, ntime), c), off, mem)
    assert np.abs(G - abs(c) ** 2).max() <= 4 * EPS * abs(c) ** 2
    # against the definition, member by member, in extended precision
    g = gc.crandn(rng, 2, 3, nfeed, ntime)
    G = skysim.baseline_gains_host(g, off, mem)
    want, A = gc.baseline_gains_exact(g, off, mem)
    assert np.all(np.abs(G - want) <= 4 * (np.diff(off)[:, None] + 2) * EPS * A)
    # orientation: swapping the two entries of a member conjugates its term — a doctored table gives the doctored answer
    for cls in (0, 9):
        k = off[cls]
        swapped = mem.copy()
        swapped[k] = swapped[k, ::-1]
        i, j = mem[k]
        term = g[..., i, :] * g[..., j, :].conj()
        delta = skysim.baseline_gains_host(g, off, swapped) - G
        expect = np.zeros_like(G)
        expect[..., cls, :] = (term.conj() - term) / (off[cls + 1] - off[cls])
        assert np.abs(expect).max() > 0.1 and np.all(np.abs(delta - expect) <= 16 * EPS * A.max())
    # a whole class the other way round is the conjugate
    one_off, one = gc.table([[(3, 1), (4, 2)]])
    fwd, rev = skysim.baseline_gains_host(g, one_off, one), skysim.baseline_gains_host(g, one_off, one[:, ::-1])
    assert np.abs(fwd.imag).max() > 0.1 and np.all(np.abs(rev - fwd.conj()) <= 4 * (2 + 2) * EPS * gc.baseline_gains_exact(g, one_off, one)[1])
    for bad_off, bad_mem in ((np.array([0, 0, 1]), [[0, 1]]), (np.array([0, 1]), [[0, nfeed]]), (np.array([1, 2]), [[0, 1], [1, 2]])):
        with pytest.raises(ValueError):
            skysim.baseline_gains_host(g, bad_off, np.array(bad_mem))


# ---- simulate -------------------------------------------------------------------------------------------------------------
def test_simulate_with_gains_on_the_host(tmp_path):
    """Noise-only `simulate` needs no device: zero sigmas leave every bit as `simulate()` without gains writes it, real
    gains leave the noise alone too (they multiply the sky part, which is empty here), and the `gain` dataset holds what
    `gains_host` gives for the realisation."""
    from driftscan_amd import skysim, storage, timestream

    tel = gc.cylinder_telescope()
    pm = types.SimpleNamespace(beamtransfer=types.SimpleNamespace(telescope=tel, directory=str(tmp_path / "bt")),
                               directory=str(tmp_path / "prod"))
    kw = dict(ndays=10, seed=5)
    ref = timestream.simulate(pm, str(tmp_path / "ref"), **kw)
    zero = timestream.simulate(pm, str(tmp_path / "zero"), gains=dict(sigma_amp=0.0, sigma_phase=0.0), **kw)
    model = skysim.GainModel(0.05, 0.1, corr_time=900.0, seed=2)
    real = timestream.simulate(pm, str(tmp_path / "real"), gains=model, sky_realisation=3, **kw)
    ntime = ref.ntime
    want = skysim.gains_host(model, tel.nfeed, np.arange(tel.nfreq), ntime, 1, first=3)[0]
    for fi in range(tel.nfreq):
        v = ref.timestream_f(fi)
        assert np.abs(v).max() > 0
        assert np.array_equal(zero.timestream_f(fi), v) and np.array_equal(real.timestream_f(fi), v)
        with storage.File(ref._ffile(fi), "r") as f, storage.File(zero._ffile(fi), "r") as z, storage.File(real._ffile(fi), "r") as r:
            assert "gain" not in f.keys() and sorted(set(z.keys()) - set(f.keys())) == ["gain"]
            assert np.array_equal(z["gain"][:], np.ones((tel.nfeed, ntime)))
            assert np.array_equal(r["gain"][:], want[fi])
    # an explicit array, and one of the wrong shape
    ex = timestream.simulate(pm, str(tmp_path / "ex"), gains=want, **kw)
    assert np.array_equal(ex.timestream_f(1), ref.timestream_f(1))
    with pytest.raises(ValueError):
        timestream.simulate(pm, str(tmp_path / "bad"), gains=want[:, :-1], **kw)
    for bad in (np.concatenate([want, want[:1]]), want[:-1]):              # a frequency too many, one too few
        with pytest.raises(ValueError, match="does not fit"):
            timestream.simulate(pm, str(tmp_path / "bad"), gains=bad, **kw)
