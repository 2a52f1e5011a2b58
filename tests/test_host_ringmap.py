"""CPU: the host statement of the ring map in float64 against long double under the checker of
tests/ringmap_cases.py, the checker against planted errors, the sign convention on an analytic source, the group, taper
and grid helpers on four telescopes, and every ValueError of the host functions."""
import numpy as np
import pytest

import ringmap_cases as rc
from driftscan_amd import cylinder, telescope, timestream

_REF = {}


def _case(name):
    if name not in _REF:
        c = rc.make(name)
        _REF[name] = (c, rc.reference(c))
    return _REF[name]


def _host(c, parts=2, **over):
    a = dict(c, **over)
    return timestream.ringmap_host(a["vis"], a["w"], a["group_off"], a["members"], a["v"], a["scale"], a["sinza"],
                                   taper=a["taper"], parts=parts, dtype=np.float64)


@pytest.mark.parametrize("name", sorted(rc.CASES))
def test_float64_meets_the_checker(name):
    c, ref = _case(name)
    for parts in (1, 2):
        got = _host(c, parts)
        assert got[0].dtype == np.float64 and got[0].shape == (c["nf"], len(c["group_off"]) - 1, parts, c["nel"], c["nt"])
        bad, worst = rc.check(c, got, ref)
        print("%s parts %d: worst error %.3g of its bound" % (name, parts, worst))
        assert not bad, bad
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[1])) and np.all(np.isfinite(got[2]))
    if c["nt"] > 1:
        assert not ref[1][:, :, 0].any() and (ref[1] == 0).sum() >= 2 * c["nf"] and (ref[1] != 0).any()


def test_without_weights_and_taper():
    c = rc.make("edges", w_none=True, taper_none=True)
    ref = rc.reference(c)
    got = _host(c)
    bad, _ = rc.check(c, got, ref)
    assert not bad, bad
    ones = _host(c, w=np.ones(c["vis"].shape), taper=np.ones(c["v"].shape))
    assert all(np.array_equal(a, b) for a, b in zip(got, ones))
    assert np.array_equal(got[1], np.broadcast_to(np.diff(c["group_off"])[None, :, None].astype(float), got[1].shape))


def test_checker_rejects_planted_errors():
    c, ref = _case("edges")
    good = _host(c)
    assert not rc.check(c, good, ref)[0]
    # the phase sign flipped
    assert rc.check(c, _host(c, v=-c["v"]), ref)[0]
    # the taper left out
    assert rc.check(c, _host(c, taper=None), ref)[0]
    # one member dropped from the largest group
    off, mem = c["group_off"].copy(), c["members"]
    off[-1] -= 1
    assert rc.check(c, _host(c, group_off=off, members=mem[:-1], v=c["v"][:-1], taper=c["taper"][:-1]), ref)[0]
    # a sample that is not kept let in
    f, row = 0, int(c["members"][c["group_off"][4] + 2])
    t = int(np.nonzero(~(c["w"][f, row] > 0))[0][-1])
    w, vis = c["w"].copy(), c["vis"].copy()
    w[f, row, t], vis[f, row, t] = 1.0, 1.0 + 1.0j
    assert rc.check(c, _host(c, w=w, vis=vis), ref)[0]
    # an error of 100 x the bound on one element
    bnd, _ = rc.bound(c)
    i = np.unravel_index(np.argmax(bnd), bnd.shape)
    m = good[0].copy()
    m[i[0], i[1], 1, 3, i[2]] += float(100 * bnd[i])
    assert rc.check(c, (m, good[1], good[2]), ref)[0]
    m = good[0].copy()
    m[i[0], i[1], 0, 0, i[2]] = np.nan
    assert rc.check(c, (m, good[1], good[2]), ref)[0]
    # the normalisation by D2
    with np.errstate(invalid="ignore", divide="ignore"):
        m = np.where(good[2][:, :, None, None, :] != 0, good[0] * (good[1] / good[2])[:, :, None, None, :], 0.0)
    assert rc.check(c, (m, good[1], good[2]), ref)[0]
    # D and D2 themselves, and a value where D = 0
    assert rc.check(c, (good[0], good[1] * (1 + 1e-13), good[2]), ref)[0]
    assert rc.check(c, (good[0], good[1], good[2] * (1 - 1e-13)), ref)[0]
    m = good[0].copy()
    m[0, 0, 0, 0, 0] = 1e-300
    assert rc.check(c, (m, good[1], good[2]), ref)[0]


def test_point_source_on_the_meridian_pins_the_sign():
    """V_b = exp(2 pi i scale v_b s0), the fringe of oracle/btgen.py with v pointing north: the map is the Dirichlet-type
    sum sum_b cos(2 pi scale v_b (s0 - s)) / nb at every s, and 1 at s0."""
    nb, scale, s0 = 12, 2.4, 0.33
    v = (np.arange(nb) + 1) * 0.3
    sinza = np.concatenate([np.linspace(-1, 1, 41), [s0]])
    vis = np.exp(2j * np.pi * scale * v * s0)[None, :, None] * np.ones((1, nb, 3))
    m, d, d2 = timestream.ringmap_host(vis, None, [0, nb], np.arange(nb), v, [scale], sinza, parts=2)
    want = np.cos(2 * np.pi * scale * v[:, None] * (s0 - sinza[None, :])).mean(axis=0)
    assert np.abs(m[0, 0, 0] - want[:, None]).max() < 1e-13
    assert np.abs(m[0, 0, 0, -1] - 1).max() < 1e-14 and np.abs(m[0, 0, 1, -1]).max() < 1e-14
    assert np.argmax(m[0, 0, 0, :, 0]) == sinza.size - 1
    assert np.all(d == nb) and np.all(d2 == nb)
    assert m[0, 0, 0, np.argmin(np.abs(sinza[:-1] + s0)), 0] < 0.9   # not at -s0


def _telescopes():
    cyl = cylinder.UnpolarisedCylinderTelescope.from_config(dict(num_freq=3, freq_start=400.0, freq_end=430.0, num_cylinders=3,
                                                                  cylinder_width=2.0, num_feeds=5, feed_spacing=0.3))
    pol = cylinder.PolarisedCylinderTelescope.from_config(dict(num_freq=2, freq_start=400.0, freq_end=430.0, num_cylinders=2,
                                                               cylinder_width=2.0, num_feeds=4, feed_spacing=0.3))
    ncm = cylinder.UnpolarisedCylinderTelescope.from_config(dict(num_freq=2, freq_start=400.0, freq_end=430.0, num_cylinders=2,
                                                                  cylinder_width=2.0, num_feeds=5, feed_spacing=0.3,
                                                                  non_commensurate=True))

    class Dishes(telescope.SimpleUnpolarisedTelescope):
        u_width = v_width = 1.0

        @property
        def _single_feedpositions(self):
            return np.array([[0.0, 0.0], [1.3, 0.2], [2.1, -1.7], [0.4, 3.3], [5.2, 0.9]])

    dish = Dishes.from_config(dict(num_freq=2, freq_start=400.0, freq_end=430.0))
    return dict(cyl=cyl, pol=pol, ncm=ncm, dish=dish)


@pytest.mark.parametrize("which", ("cyl", "pol", "ncm", "dish"))
def test_groups(which):
    tel = _telescopes()[which]
    g = timestream.ringmap_groups(tel)
    off, mem, v = g["group_off"], g["members"], g["v"]
    npairs = int(tel.npairs)
    assert off.dtype == np.int32 and mem.dtype == np.int32 and off[0] == 0 and off[-1] == mem.size == v.size
    assert sorted(mem.tolist()) == list(range(npairs))           # every unique baseline in exactly one group
    assert g["u"].shape == (off.size - 1,) and g["pol"].shape == (off.size - 1, 2) and np.all(np.diff(off) > 0)
    bl, cls, pairs = tel.baselines, np.asarray(tel.beamclass), tel.uniquepairs
    keys = []
    for k in range(off.size - 1):
        rows = mem[off[k]:off[k + 1]]
        assert np.all(np.around(bl[rows, 0], 6) == g["u"][k])
        assert np.all(cls[pairs[rows, 0]] == g["pol"][k, 0]) and np.all(cls[pairs[rows, 1]] == g["pol"][k, 1])
        assert np.array_equal(v[off[k]:off[k + 1]], bl[rows, 1])
        order = np.lexsort((rows, bl[rows, 1]))
        assert np.array_equal(order, np.arange(rows.size))       # by v, then index
        keys.append((int(g["pol"][k, 0]), int(g["pol"][k, 1]), float(g["u"][k])))
    assert keys == sorted(keys) and len(set(keys)) == len(keys)
    want = {(int(cls[i]), int(cls[j]), float(np.around(b[0], 6) + 0.0)) for (i, j), b in zip(pairs, bl)}
    assert set(keys) == want
    us = np.unique(g["u"])
    if which == "cyl":
        assert len(keys) == 3 and us.tolist() == [0.0, 2.0, 4.0]
        assert np.diff(off).tolist() == [4, 9, 9]                # v > 0 within a cylinder, every v between two
    if which == "pol":
        assert np.unique(g["pol"], axis=0).tolist() == [[0, 0], [0, 1], [1, 0], [1, 1]]
    if which == "ncm":
        assert len(np.unique(np.around(np.abs(np.diff(np.unique(v))), 9))) > 2    # unequal spacing
    if which == "dish":
        assert np.all(np.diff(off) == 1) and off.size - 1 == npairs
    # intracyl and ew take effect
    no0 = timestream.ringmap_groups(tel, intracyl=False)
    assert np.all(no0["u"] != 0) and sorted(no0["members"].tolist()) == sorted(np.nonzero(np.around(bl[:, 0], 6) != 0)[0].tolist())
    pick = timestream.ringmap_groups(tel, ew=[float(us[-1])])
    assert np.all(pick["u"] == us[-1]) and sorted(pick["members"].tolist()) == sorted(np.nonzero(np.around(bl[:, 0], 6) == us[-1])[0].tolist())
    assert timestream.ringmap_groups(tel, ew=[123.0])["members"].size == 0
    if us[0] == 0:
        both = timestream.ringmap_groups(tel, ew=[0.0, float(us[-1])], intracyl=False)
        assert np.all(both["u"] == us[-1])


def test_taper_and_sinza():
    tel = _telescopes()["cyl"]
    g = timestream.ringmap_groups(tel)
    nat = timestream.ringmap_taper(tel, g)
    assert np.array_equal(nat, tel.redundancy[g["members"]].astype(float)) and nat.max() > 1
    uni = timestream.ringmap_taper(tel, g, weighting="uniform")
    assert np.all(uni == 1)
    edge = np.abs(g["v"]).max() + np.abs(g["v"])[np.abs(g["v"]) > 0].min()
    x = g["v"] / edge
    hann = timestream.ringmap_taper(tel, g, weighting="uniform", window="hann")
    assert np.allclose(hann, np.cos(np.pi * x / 2) ** 2, rtol=1e-14, atol=0) and hann.min() > 0 and np.all(hann[g["v"] == 0] == 1)
    bman = timestream.ringmap_taper(tel, g, weighting="natural", window="blackman")
    assert np.allclose(bman, nat * (0.42 + 0.5 * np.cos(np.pi * x) + 0.08 * np.cos(2 * np.pi * x)), rtol=1e-14, atol=0)
    assert bman.min() > 0
    s = timestream.ringmap_sinza(tel, g)
    assert s.size % 2 == 1 and s[0] == -1 and s[-1] == 1 and s[s.size // 2] == 0 and np.allclose(np.diff(s), 2.0 / (s.size - 1))
    period = 1.0 / (np.abs(g["v"]).max() / tel.wavelengths.min())
    assert s[1] - s[0] <= period / 2 and 2.0 / (s.size - 3) > period / 2       # the smallest odd count
    assert timestream.ringmap_sinza(tel, g, nel=8).size == 8 and timestream.ringmap_sinza(tel, g, nel=1).tolist() == [0.0]
    for bad in (dict(weighting="robust"), dict(window="boxcar")):
        with pytest.raises(ValueError):
            timestream.ringmap_taper(tel, g, **bad)
    with pytest.raises(ValueError):
        timestream.ringmap_sinza(tel, g, nel=0)


def test_value_errors_of_the_host_statement():
    c = rc.make("sixteen")
    good = dict(vis=c["vis"], w=c["w"], group_off=c["group_off"], members=c["members"], v=c["v"], scale=c["scale"],
                sinza=c["sinza"], taper=c["taper"], parts=1, dtype=np.float64)
    timestream.ringmap_host(**good)
    dec = c["group_off"].copy()
    dec[1], dec[2] = dec[2], dec[1]
    out = c["members"].copy()
    out[3] = c["nrow"]
    neg = c["members"].copy()
    neg[0] = -1
    for bad in (dict(dtype=np.float32), dict(parts=3), dict(parts=0), dict(vis=c["vis"][0]), dict(vis=c["vis"].real),
                dict(w=c["w"][:, :-1]), dict(group_off=dec), dict(group_off=c["group_off"] + 1), dict(group_off=c["group_off"][:-1]),
                dict(members=out), dict(members=neg), dict(members=c["members"][:-1]), dict(v=c["v"][:-1]),
                dict(scale=c["scale"][:-1]), dict(sinza=c["sinza"][None]), dict(taper=c["taper"][:-1])):
        with pytest.raises(ValueError, match="ringmap_host"):
            timestream.ringmap_host(**dict(good, **bad))
    for bad in (dict(colour="red"), dict(weighting="robust"), dict(window="boxcar"), dict(parts=3)):
        with pytest.raises(ValueError, match="ringmaps"):
            timestream.ringmap_params(bad)
    assert timestream.ringmap_params(dict(name="a", nel=9))["nel"] == 9
