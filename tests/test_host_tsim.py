"""CPU-only: the host side of the timestream ensembles.

The problem table of the batched sky -> telescope projection is executed by a small numpy interpreter standing in for
`dm_blockvec_grouped` and compared with `beam @ alm` per (m, frequency); the numpy restatement of the noise stream
(`skysim.noise_host`, the oracle of `Context.ts_noise`) is checked for its statistics and for the independence of a draw
from everything but (seed, pair, global frequency, time sample, realisation)."""
import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided


def run_table(A, x, y, tab, R):
    """y_p = op(A_p) x_p for every row of a problem table on flat complex128 numpy buffers."""
    for p in tab:
        M, K = int(p["M"]), int(p["K"])
        if M == 0 or K == 0:
            continue
        Am = as_strided(A[int(p["a0"]):], (M, K), (16 * int(p["rsA"]), 16 * int(p["csA"])))
        xm = as_strided(x[int(p["x0"]):], (K, R), (16 * int(p["rsB"]), 16 * int(p["csB"])))
        ym = as_strided(y[int(p["y0"]):], (M, R), (16 * int(p["ldc"]), 16))
        ym[...] = (Am.conj() if p["conjA"] else Am) @ (xm.conj() if p["conjB"] else xm)


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- the problem table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [1, 3, 8])
@pytest.mark.parametrize("nf", [1, 3])
@pytest.mark.parametrize("nb", [1, 3])
def test_sky_to_telescope_table_matches_per_block_products(nb, nf, R):
    from driftscan_amd import beamtransfer as btmod

    rng = np.random.default_rng(100 * nb + 10 * nf + R)
    ntel, nsky = 6, 10
    beam = _crandn(rng, nb, nf, ntel, nsky)
    alm = _crandn(rng, nb, nf, nsky, R)
    tab = btmod.sky_to_telescope_table(nb, nf, ntel, nsky, R)
    assert len(tab) == nb * nf and np.all(tab["M"] == ntel) and np.all(tab["K"] == nsky)
    out = np.full((nb * nf * ntel * R,), 7.0 + 7.0j)
    run_table(beam.reshape(-1), alm.reshape(-1), out, tab, R)
    out = out.reshape(nb, nf, ntel, R)
    for i in range(nb):
        for f in range(nf):
            want = beam[i, f] @ alm[i, f]
            # O(1) values, sums of nsky = 10 products: two orders of summation
            assert np.all(np.abs(out[i, f] - want) <= 1e-13 * (1.0 + np.abs(want))), (i, f)


def test_sky_to_telescope_table_frequency_subset_and_empty():
    """A `freqs` subset is the same table on the beam blocks and a_lm of those frequencies alone; no frequency, no
    problem."""
    from driftscan_amd import beamtransfer as btmod

    rng = np.random.default_rng(5)
    nb, nfreq, ntel, nsky, R = 3, 4, 6, 10, 3
    freqs = [0, 2, 3]
    beam = _crandn(rng, nb, nfreq, ntel, nsky)
    alm = _crandn(rng, nb, nfreq, nsky, R)
    tab = btmod.sky_to_telescope_table(nb, len(freqs), ntel, nsky, R)
    out = np.full((nb * len(freqs) * ntel * R,), 7.0 + 7.0j)
    run_table(np.ascontiguousarray(beam[:, freqs]).reshape(-1), np.ascontiguousarray(alm[:, freqs]).reshape(-1), out, tab, R)
    out = out.reshape(nb, len(freqs), ntel, R)
    for i in range(nb):
        for k, f in enumerate(freqs):
            want = beam[i, f] @ alm[i, f]
            assert np.all(np.abs(out[i, k] - want) <= 1e-13 * (1.0 + np.abs(want))), (i, f)
    empty = btmod.sky_to_telescope_table(nb, 0, ntel, nsky, R)
    assert empty.shape == (0,) and empty.dtype == tab.dtype


# ---- the noise stream -----------------------------------------------------------------------------------------------------
def noise_statistics(z):
    """[(max |d|, rms d)] of the normalised deviations over the (f, pair) cells of unit noise z (nreal, nf, npairs, ntime):
    the sample variance, the lag-1 product (real and imaginary parts) and the mean (real and imaginary parts)."""
    nreal, ntime = z.shape[0], z.shape[-1]
    N, N1 = nreal * ntime, nreal * (ntime - 1)
    var = ((np.abs(z) ** 2).mean(axis=(0, 3)) - 1.0) * np.sqrt(N)
    lag = (z[..., :-1] * z[..., 1:].conj()).sum(axis=(0, 3)) * np.sqrt(2.0 / N1)
    mean = z.sum(axis=(0, 3)) * np.sqrt(2.0 / N)
    out = []
    for d in (var.ravel(), np.concatenate([lag.real.ravel(), lag.imag.ravel()]),
              np.concatenate([mean.real.ravel(), mean.imag.ravel()])):
        out.append((float(np.abs(d).max()), float(np.sqrt((d ** 2).mean()))))
    return out


def test_noise_stream_statistics():
    """Unit variance, no correlation between neighbouring time samples, zero mean: every normalised deviation is a
    unit normal if the stream is sound, so over 64 (or 128) of them the project's acceptance band (DESIGN.md section
    4.12) is max |d| < 5 and 0.6 < rms < 1.4."""
    from driftscan_amd import skysim

    z = skysim.noise_host(np.ones((4, 16)), np.arange(4), 257, 4, seed=11)
    assert z.shape == (4, 4, 16, 257) and z.dtype == np.complex128
    stats = noise_statistics(z)
    print("noise_host statistics (max |d|, rms):", stats)
    for dmax, rms in stats:
        assert dmax < 5.0 and 0.6 < rms < 1.4, stats
    # the figures this counter layout and seed give (recorded in DESIGN.md section 4.13)
    assert [(round(a, 2), round(b, 2)) for a, b in stats] == [(2.33, 1.16), (2.91, 0.95), (2.94, 0.92)]


def test_noise_stream_depends_on_its_five_numbers_only():
    from driftscan_amd import skysim

    rng = np.random.default_rng(2)
    sigma = rng.uniform(0.5, 2.0, size=(4, 5))
    fg = np.array([0, 1, 2, 5])
    full = skysim.noise_host(sigma, fg, 17, 4, seed=3)
    # rows of a frequency subset, and a realisation range
    sub = skysim.noise_host(sigma[[1, 3]], fg[[1, 3]], 17, 4, seed=3)
    assert np.array_equal(sub, full[:, [1, 3]])
    part = skysim.noise_host(sigma, fg, 17, 2, seed=3, first=2)
    assert np.array_equal(part, full[2:4])
    # it scales with sigma (sigma multiplies the radius before the cosine and sine: two roundings apart per part)
    unit = skysim.noise_host(np.ones((4, 5)), fg, 17, 4, seed=3) * sigma[None, :, :, None]
    assert np.all(np.abs(full - unit) <= 4 * np.finfo(float).eps * np.abs(unit))
    # realisations, seeds, frequencies and streams are different draws
    assert not np.any(full[0] == full[1])
    assert not np.any(full == skysim.noise_host(sigma, fg, 17, 4, seed=4))
    assert not np.any(full[:, 0] / sigma[0, :, None] == full[:, 1] / sigma[1, :, None])
    other = skysim.noise_host(sigma, fg, 17, 4, seed=3, stream=skysim.STREAM_SKY_SIGNAL)
    assert skysim.STREAM_TS_NOISE == 24 and not np.any(full == other)
    with pytest.raises(ValueError):
        skysim.noise_host(sigma, fg, 17, 2, seed=3, first=(1 << 24) - 1)


def test_m_batches_is_the_timestream_rule():
    from driftscan_amd import timestream

    gb = float(1 << 30)
    assert timestream.m_batches(list(range(5)), lambda mi: 0.4 * gb, 1.0) == [[0, 1], [2, 3], [4]]
    assert timestream.m_batches([3, 4], lambda mi: 2.0 * gb, 1.0) == [[3], [4]]
    assert timestream.m_batches([], lambda mi: 1.0, 1.0) == []
