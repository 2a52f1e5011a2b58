"""CPU: the host statement of the delay spectrum in float64 against long double under the bound
of tests/delayspec_cases.py on every case; the checker rejects planted errors; the Toeplitz identity of the window
matrix; `delay_normalise` on a grid tone behind flags; `delay_grid`, `delay_taper` and `delayspectrum_params`."""
import numpy as np
import pytest

import delayspec_cases as ds
from driftscan_amd import timestream

_REF = {}


def _case(name):
    if name not in _REF:
        c = ds.make(name)
        _REF[name] = (c, ds.reference(c))
    return _REF[name]


@pytest.mark.parametrize("name", sorted(ds.CASES))
def test_float64_statement_under_the_bound(name):
    c, ref = _case(name)
    got = ds.reference(c, dtype=np.float64)
    bad, worst = ds.check(c, got, ref)
    print("%s: worst error %.3g of its bound" % (name, worst))
    assert not bad, bad
    assert all(np.all(np.isfinite(np.asarray(g, dtype=np.float64))) for g in got)


def test_cases_hold_what_they_promise():
    """Empty bins, bins whose series are all dropped, samples outside every bin, every a0, both weightings, and no shape
    that is a multiple of the kernel's tile."""
    a0s, weightings = set(), set()
    for name in ds.CASES:
        c, ref = _case(name)
        a0s.add("lo" if c["a0"] == 0 else "hi" if c["a0"] == c["nd"] - 1 else "mid")
        weightings.add(c["weighting"])
        for v, tile in ((c["nf"], 16), (c["nd"], 128), (c["nt"], 64)):
            assert v == 1 or v % tile != 0, name
        if c["nt"] > 1:
            assert np.isnan(c["w"]).any() and (c["w"] < 0).any() and (c["w"] == 0).any()
            assert np.isnan(c["x"]).any() and np.isinf(c["x"]).any() and np.all(~np.isfinite(c["x"][~(c["w"] > 0)]))
    assert a0s == {"lo", "mid", "hi"} and weightings == {"mask", "weight"}
    c, ref = _case("edges")
    assert np.array_equal(np.diff(c["bin_off"]) == 0, [False, True, False, False, False])
    assert not ref[4][:, 1].any() and not ref[4][:, 3].any() and ref[4][:, [0, 2, 4]].all()
    assert c["bin_off"][0] > 0 and c["bin_off"][-1] < c["nt"]
    assert not ref[0][:, [1, 3]].any() and not ref[1][:, [1, 3]].any()
    c, ref = _case("seventeen")
    assert not ref[4][:, [0, 2]].any() and np.all(ref[4][:, 1] < 48) and ref[4][:, 1].all()


def test_checker_rejects_planted_errors():
    c, ref = _case("seventeen")
    good = [np.asarray(g, dtype=np.float64) if i < 4 else g.copy() for i, g in enumerate(ds.reference(c, dtype=np.float64))]
    assert not ds.check(c, good, ref)[0]
    bq, bh, _ = ds.bound(c)
    q = good[0].copy()
    q[2, 1, 7] += 4.0 * float(bq[2, 1])
    assert any(m.startswith("q:") for m in ds.check(c, [q] + good[1:], ref)[0])
    h = good[1].copy()
    h[0, 3, 0] -= 4.0 * float(bh[0, 3])
    assert any(m.startswith("h:") for m in ds.check(c, [good[0], h] + good[2:], ref)[0])
    cnt = good[4].copy()
    cnt[1, 2] += 1                                        # a dropped series counted
    assert "count differs" in ds.check(c, good[:4] + [cnt], ref)[0]
    # a dropped series let into the sums
    let_in = ds.reference(dict(c, min_valid=1), dtype=np.float64)
    msgs = ds.check(c, let_in, ref)[0]
    assert any("without a used series" in m for m in msgs) and "count differs" in msgs
    q = good[0].copy()
    q[4, 3, 5] = np.nan                                   # a flagged NaN let in
    assert any(m.startswith("q:") for m in ds.check(c, [q] + good[1:], ref)[0])
    s1 = good[2].copy()
    s1[0, 1] *= 1.0 + 1e-12
    assert any(m.startswith("s1") for m in ds.check(c, good[:2] + [s1] + good[3:], ref)[0])
    # the optional outputs may be missing
    assert not ds.check(c, [good[0], None, None, None, None], ref)[0]


def _dense_fisher(c, row, b):
    """F_ab = sum_t | sum_f y_f exp(2 pi i step_f (a - b)) |^2 from its definition, in long double."""
    ld = np.longdouble
    nf, nd = c["nf"], c["nd"]
    kept = c["w"] > 0
    T = c["taper"].astype(ld)
    om = kept.astype(ld) if c["weighting"] == "mask" else np.where(kept, c["w"], 0.0).astype(ld)
    used = kept.sum(axis=0) >= c["min_valid"]
    ts = np.arange(c["bin_off"][b], c["bin_off"][b + 1])
    ts = ts[used[row, ts]]
    y = T[:, None] * om[:, row, ts]
    pi = timestream._ld_pi()
    F = np.zeros((nd, nd), dtype=ld)
    for a in range(nd):
        for bb in range(nd):
            phi = c["step"].astype(ld) * ld(a - bb)
            ang = pi * (2 * (phi - np.rint(phi)))
            F[a, bb] = (((np.cos(ang)[:, None] * y).sum(axis=0)) ** 2 + ((np.sin(ang)[:, None] * y).sum(axis=0)) ** 2).sum()
    return F


@pytest.mark.parametrize("name,b", [("edges", 2), ("four", 1), ("seventeen", 3)])
def test_window_matrix_is_the_toeplitz_matrix_of_h(name, b):
    c, ref = _case(name)
    nd = c["nd"]
    idx = np.abs(np.arange(nd)[:, None] - np.arange(nd)[None, :])
    for row in (0, 3):
        F = _dense_fisher(c, row, b)
        Th = ref[1][row, b][idx]
        assert np.max(np.abs(F - Th)) <= 1e-15 * np.max(np.abs(Th))
        assert np.array_equal(F, F.T)


def _tone(nf=48, nd=48, nt=6, k=7, flagged=0.25, taper="blackman", seed=5):
    """A delay tone on the grid, x_f = exp(-2 pi i step_f k), behind a fixed set of flagged channels."""
    rng = np.random.default_rng(seed)
    nu = 400.0 + 0.5 * np.arange(nf)
    tau, step, a0, dtau = timestream.delay_grid(nu, nd=nd)
    x = np.exp(-2j * np.pi * step * k)[:, None, None] * np.ones((1, 1, nt))
    w = np.ones((nf, 1, nt))
    w[rng.permutation(nf)[: int(flagged * nf)]] = 0.0
    tap = timestream.delay_taper(nf, taper)
    q, h, s1, s2, cnt = timestream.delay_spectrum_host(x, w, tap, step, nd, a0, "mask", 1, [0, nt])
    return q, h, s2, a0 + k   # D_a peaks where a - a0 = k


def test_normalise_inverse_recovers_a_grid_tone_behind_flags():
    q, h, s, peak = _tone()
    lam = np.linalg.eigvalsh(h[0, 0][np.abs(np.arange(48)[:, None] - np.arange(48)[None, :])])
    print("lambda_min / lambda_max of the window matrix: %.3g" % (lam[0] / lam[-1]))
    p, n, info = timestream.delay_normalise(q, h, s, norm="inverse")
    assert not info.any() and p.shape == q.shape and n.shape == q.shape and info.shape == s.shape
    others = np.delete(p[0, 0], peak)
    assert np.argmax(p[0, 0]) == peak and np.max(np.abs(others)) <= 1e-10 * p[0, 0, peak]
    pw, nw, iw = timestream.delay_normalise(q, h, s, norm="window")
    leak = np.max(np.abs(np.delete(pw[0, 0], peak))) / pw[0, 0, peak]
    print("window normalisation leaves %.3g of the peak in the wrong bins" % leak)
    assert not iw.any() and np.argmax(pw[0, 0]) == peak and leak > 0.05
    rows = np.array([sum(h[0, 0, abs(a - b)] for b in range(48)) for a in range(48)])
    assert np.allclose(pw[0, 0], q[0, 0] / rows, rtol=1e-14) and np.allclose(nw[0, 0], s[0, 0] / rows, rtol=1e-14)


def test_normalise_singular_window_and_ridge():
    """All but one channel flagged: H_d = H_0 for every lag, the window matrix has rank one."""
    nf, nd, nt = 8, 8, 3
    tau, step, a0, dtau = timestream.delay_grid(400.0 + np.arange(nf), nd=nd)
    w = np.zeros((nf, 2, nt))
    w[3, 0] = 1.0        # row 0: one channel; row 1: nothing at all
    x = np.ones((nf, 2, nt), dtype=np.complex128)
    q, h, s1, s2, cnt = timestream.delay_spectrum_host(x, w, None, step, nd, a0, "mask", 1, [0, nt])
    assert cnt[0, 0] == nt and cnt[1, 0] == 0 and np.all(h[0, 0] == h[0, 0, 0])
    p, n, info = timestream.delay_normalise(q, h, s2, norm="inverse")
    assert info[0, 0] != 0 and info[1, 0] == nd and np.all(np.isnan(p)) and np.all(np.isnan(n))
    p, n, info = timestream.delay_normalise(q, h, s2, norm="inverse", ridge=1e-3)
    assert info[0, 0] == 0 and np.all(np.isfinite(p[0])) and info[1, 0] == nd and np.all(np.isnan(p[1]))
    p, n, info = timestream.delay_normalise(q, h, s2, norm="window")
    assert info[0, 0] == 0 and info[1, 0] == nd and np.all(np.isfinite(p[0])) and np.all(np.isnan(p[1]))
    for kw in (dict(norm="fft"), dict(ridge=-1.0), dict(ridge=np.nan)):
        with pytest.raises(ValueError):
            timestream.delay_normalise(q, h, s2, **kw)
    with pytest.raises(ValueError):
        timestream.delay_normalise(q, h[:, :, :4], s2)


def test_grid_taper_and_params():
    nu = 400.0 + 0.25 * np.arange(32)
    tau, step, a0, dtau = timestream.delay_grid(nu)
    assert tau.shape == (32,) and a0 == 16 and tau[a0] == 0 and np.isclose(dtau, 1.0 / (32 * 0.25))
    assert np.allclose(step, (nu - 0.5 * (nu[0] + nu[-1])) * dtau) and np.allclose(np.diff(tau), dtau)
    tau, step, a0, dtau2 = timestream.delay_grid(nu, oversample=2.0, tau_max=1.0)
    assert np.isclose(dtau2, dtau / 2) and tau.size % 2 == 1 and tau[-1] >= 1.0 > tau[-2] and tau[0] == -tau[-1]

    class Tel(object):
        frequencies = nu[::-1]

    assert np.allclose(timestream.delay_grid(Tel(), nd=5)[1], step[::-1] * (dtau / dtau2))
    for bad in (dict(tel=nu[:1]), dict(tel=np.array([400.0, np.nan])), dict(tel=nu, oversample=0.0), dict(tel=nu, nd=0),
                dict(tel=nu, oversample=np.inf), dict(tel=nu, tau_max=-1.0), dict(tel=nu, tau_max=np.nan),
                dict(tel=np.array([400.0, 400.0]))):
        with pytest.raises(ValueError):
            timestream.delay_grid(**bad)
    for kind in (None, "hann", "blackman", "blackman-harris"):
        t = timestream.delay_taper(33, kind)
        assert t.shape == (33,) and np.all(t > 0) and np.allclose(t, t[::-1]) and np.isclose(t.max(), 1.0, atol=2e-3)
    assert np.all(timestream.delay_taper(4) == 1)
    for bad in ((0, None), (8, "kaiser")):
        with pytest.raises(ValueError):
            timestream.delay_taper(*bad)
    p = timestream.delayspectrum_params(dict(name="a", tbin=16, taper="none"))
    assert p["name"] == "a" and p["tbin"] == 16 and p["taper"] is None and p["norm"] == "window"
    assert timestream.delayspectrum_params()["taper"] == "blackman-harris"
    with pytest.raises(ValueError, match="unknown key"):
        timestream.delayspectrum_params(dict(nel=3))
    for bad in (dict(taper="kaiser"), dict(weighting="natural"), dict(norm="fft"), dict(ridge=-1.0), dict(oversample=0.0),
                dict(nd=0), dict(tbin=0), dict(min_valid=0), dict(tau_max=-2.0)):
        with pytest.raises(ValueError):
            timestream.delayspectrum_params(bad)


def test_pipeline_refuses_an_unknown_key_before_anything_runs(tmp_path):
    import yaml

    from driftscan_amd import pipeline

    conf = dict(config=dict(product_directory=str(tmp_path / "nowhere"), delayspectra=[dict(name="a", nel=3)]))
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    with pytest.raises(ValueError, match="delayspectra: unknown key"):
        pipeline.PipelineManager.from_configfile(str(cfile))


def test_host_statement_refusals():
    c, _ = _case("edges")
    args = dict(x=c["x"], w=c["w"], taper=c["taper"], step=c["step"], nd=c["nd"], a0=c["a0"], weighting="mask", min_valid=1,
                bin_off=c["bin_off"])
    for bad in (dict(dtype=np.float32), dict(weighting="natural"), dict(w=c["w"][:, :2]), dict(step=c["step"][:2]),
                dict(a0=c["nd"]), dict(a0=-1), dict(min_valid=0), dict(bin_off=[5, 3]), dict(bin_off=[0, c["nt"] + 1]),
                dict(bin_off=[-1, 3]), dict(taper=np.ones(c["nf"] + 1)), dict(x=c["x"].real)):
        with pytest.raises(ValueError):
            timestream.delay_spectrum_host(**dict(args, **bad))
