"""CPU: the definition of the Gaussian sky draws (driftscan_amd/skysim.py) in its numpy
restatement: the grouping of the components, the symmetric roots of the covariances, and the statistics of
``correlate_host`` on ``draws_host``.  The GPU tests share the shapes, the statistic and its bounds."""
import numpy as np
import pytest

EPS = np.finfo(np.float64).eps
FREQS4 = np.linspace(400.0, 430.0, 4)
LMAX = 24
NREAL = 16


def models(npol, freqs=FREQS4, lmax=LMAX):
    from driftscan_amd import skymodel

    return {"foreground": skymodel.foreground_model(lmax, freqs, npol), "signal": skymodel.im21cm_model(lmax, freqs, npol)}


def clhat_deviations(alm, cl):
    """Normalised deviations of the estimated spectra of unpolarised realisations alm [R, F, L, M = L] from cl (L, F, F):
    C^_l = [a_l0 a'_l0 + 2 sum_{m > 0} Re a_lm conj(a'_lm)] / ((2 l + 1) R) summed over realisations, against
    Var = (C_ff C_f'f' + C_ff'^2) / ((2 l + 1) R)."""
    R, F, L, M = alm.shape
    assert M == L
    ell = np.arange(L)
    prod = np.einsum("rflm,rglm->lfgm", alm, alm.conj()).real
    clhat = (prod[..., 0] + 2.0 * prod[..., 1:].sum(axis=-1)) / ((2.0 * ell + 1.0) * R)[:, None, None]
    diag = np.einsum("lff->lf", cl)
    var = (diag[:, :, None] * diag[:, None, :] + cl**2) / ((2.0 * ell + 1.0) * R)[:, None, None]
    return (clhat - cl) / np.sqrt(var)


def check_statistics(alm, cl, what):
    d = clhat_deviations(alm, cl)
    dmax, rms = float(np.abs(d).max()), float(np.sqrt(np.mean(d**2)))
    print("%s: max |d| = %.3f, rms(d) = %.3f over %d spectra entries" % (what, dmax, rms, d.size))
    assert dmax < 5.0, (what, dmax)
    assert 0.6 < rms < 1.4, (what, rms)


def test_grouping():
    from driftscan_amd import skysim

    F = FREQS4.size
    fg, sg = models(4)["foreground"], models(4)["signal"]
    g = skysim.groups(fg)
    assert [x.tolist() for x in g] == [list(range(p * F, (p + 1) * F)) for p in (0, 1, 2)]   # T, E, B; no V
    assert [x.tolist() for x in skysim.groups(sg)] == [list(range(F))]
    assert [x.tolist() for x in skysim.groups(models(1)["foreground"])] == [list(range(F))]
    cross = fg.copy()
    cross[0, 1] = 0.1 * fg[1, 1]
    cross[1, 0] = cross[0, 1].transpose(0, 2, 1)
    g = skysim.groups(cross)
    assert len(g) == 1 and g[0].tolist() == list(range(4 * F))
    C = skysim.group_covariance(cross, g[0])
    assert C.shape == (LMAX + 1, 4 * F, 4 * F)
    assert np.array_equal(C[:, :F, F : 2 * F], cross[0, 1]) and np.array_equal(C[:, 2 * F : 3 * F, 2 * F : 3 * F], fg[2, 2])
    assert np.array_equal(C[:, F : 2 * F, :F], cross[1, 0]) and not C[:, 3 * F :].any()
    assert skysim.STREAM_SKY_SIGNAL == 16 and skysim.STREAM_SKY_FOREGROUND == 17
    with pytest.raises(ValueError):
        skysim.groups(np.zeros((1, 1, 65537, 1, 1)))


@pytest.mark.parametrize("model", ["foreground", "signal"])
def test_host_roots(model):
    """T symmetric and |T T^T - C|_max <= 16 n eps |C|_max (numpy.linalg.eigh gives 9e-16 relative on these)."""
    from driftscan_amd import skysim

    cv = models(4)[model]
    grp = skysim.groups(cv)
    roots = skysim.covariance_roots(cv, device=False)
    assert len(roots) == len(grp)
    n = FREQS4.size
    for jg, T in zip(grp, roots):
        C = skysim.group_covariance(cv, jg)
        assert T.shape == C.shape == (LMAX + 1, n, n) and T.dtype == np.float64
        assert np.array_equal(T, T.transpose(0, 2, 1))
        for l in range(LMAX + 1):
            err = np.abs(T[l] @ T[l].T - C[l]).max()
            assert err <= 16 * n * EPS * np.abs(C[l]).max(), (l, err / np.abs(C[l]).max())


def test_host_draws():
    """draws_host: real at m = 0, empty for m > l, unit variance, a fixed function of its counters."""
    from driftscan_amd import skysim

    z = skysim.draws_host(np.arange(4), LMAX + 1, nreal=NREAL, seed=7)
    L = LMAX + 1
    assert z.shape == (NREAL, 4, L, L) and z.dtype == np.complex128
    assert not z[..., 0].imag.any()
    upper = np.triu(np.ones((L, L), dtype=bool), 1)
    assert not z[..., upper].any()
    z0 = z[..., 0]
    assert abs(np.mean(z0.real**2) - 1.0) < 5 * np.sqrt(2.0 / z0.size)
    lower = np.tril(np.ones((L, L), dtype=bool))
    lower[:, 0] = False
    zm = z[..., lower]                                       # 1 <= m <= l
    assert abs(np.mean(zm.real**2) - 0.5) < 5 * np.sqrt(0.5 / zm.size) and abs(np.mean(zm.imag**2) - 0.5) < 5 * np.sqrt(0.5 / zm.size)
    assert abs(np.mean(zm * zm)) < 5 / np.sqrt(zm.size)
    # rows, the m cut and the realisation range select from the same draws
    assert np.array_equal(skysim.draws_host([2, 3], L, M=9, nreal=3, seed=7, first=5), z[5:8, 2:4, :, :9])
    assert not np.array_equal(skysim.draws_host(np.arange(4), L, nreal=1, seed=8), z[:1])
    assert not np.array_equal(skysim.draws_host(np.arange(4), L, nreal=1, seed=7, stream=skysim.STREAM_SKY_FOREGROUND), z[:1])


@pytest.mark.parametrize("model", ["foreground", "signal"])
def test_host_statistics(model):
    from driftscan_amd import skysim

    cv = models(1)[model]
    (jg,), (T,) = skysim.groups(cv), skysim.covariance_roots(cv, device=False)
    z = skysim.draws_host(jg, LMAX + 1, nreal=NREAL, seed=11)
    alm = skysim.correlate_host(T, z).astype(np.complex128)
    check_statistics(alm, cv[0, 0], "host " + model)
