"""CPU: the host statement of the formed beam in float64 against long double under the checker of
tests/formedbeam_cases.py, the checker against planted errors, the windows, the groups against `ringmap_groups`, the
parameters, and the ring map as the H = 0, x = 0 special case."""
import numpy as np
import pytest

import formedbeam_cases as fc
from driftscan_amd import cylinder, telescope, timestream

_REF = {}


def _case(name):
    if name not in _REF:
        c = fc.make(name)
        _REF[name] = (c, fc.reference(c))
    return _REF[name]


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_float64_meets_the_checker(name):
    c, ref = _case(name)
    ngroup = len(c["group_off"]) - 1
    for parts in (1, 2):
        got = fc.host(c, parts)
        assert got[0].dtype == np.float64 and got[0].shape == (c["nf"], ngroup, parts, c["nsrc"])
        bad, worst = fc.check(c, got, ref)
        print("%s parts %d: float64 statement at %.3g of its bound" % (name, parts, worst))
        assert not bad, bad
        assert all(np.all(np.isfinite(g)) for g in got)
    if c["flagged"] is not None:
        s = c["flagged"]
        assert not ref[1][:, :, s].any() and not ref[0][:, :, :, s].any()      # every sample flagged: exact zeros
        drop = int(np.nonzero(c["half"] < 0)[0][0])
        assert not ref[1][:, :, drop].any() and ref[1][:, :, drop - 1].any() and ref[1][:, :, drop + 1].any()
        assert np.array_equal(got[0][..., 5], got[0][..., 6]) and np.array_equal(got[0][..., 5], got[0][..., -1])   # duplicates


def test_without_weights_and_taper():
    c = fc.make("single", w_none=True, taper_none=True)
    ref = fc.reference(c)
    got = fc.host(c)
    bad, _ = fc.check(c, got, ref)
    assert not bad, bad
    ones = fc.host(c, w=np.ones(c["vis"].shape), taper=np.ones(c["u"].shape))
    assert all(np.array_equal(a, b) for a, b in zip(got, ones))
    nterms = np.diff(c["group_off"])[:, None] * (2 * c["half"] + 1)[None, :]
    assert np.array_equal(got[1][0], nterms.astype(float))                      # env = 0 at frequency 0: D counts the terms


def test_checker_rejects_planted_errors():
    c, ref = _case("main")
    good = fc.host(c)
    assert not fc.check(c, good, ref)[0]
    # the sign of the u phase flipped
    assert fc.check(c, fc.host(c, u=-c["u"]), ref)[0]
    # one end sample of a window dropped: nothing kept at the last sample of source 1 (H = 1)
    w = c["w"].copy()
    w[:, :, (c["k0"][1] + c["half"][1]) % c["nt"]] = 0.0
    assert c["half"][1] == 1 and fc.check(c, fc.host(c, w=w), ref)[0]
    # the window shifted by one sample
    assert fc.check(c, fc.host(c, k0=(c["k0"] + 1) % c["nt"]), ref)[0]
    # the envelope left out
    assert c["env"].max() > 0 and fc.check(c, fc.host(c, env=np.zeros_like(c["env"])), ref)[0]
    # one member's taper left out
    taper = c["taper"].copy()
    taper[c["group_off"][3] + 7] = 1.0
    assert fc.check(c, fc.host(c, taper=taper), ref)[0]
    # a flagged sample let in: its NaN replaced by a value, its weight by a number; everything stays finite
    f, row = 0, int(c["members"][c["group_off"][4] + 2])
    for s in range(13, c["nsrc"]):
        ks = (c["k0"][s] + np.arange(-c["half"][s], c["half"][s] + 1)) % c["nt"]
        lost = np.nonzero(~(c["w"][f, row, ks] > 0))[0]
        if lost.size:
            break
    t = int(ks[lost[0]])
    w, vis = c["w"].copy(), c["vis"].copy()
    w[f, row, t], vis[f, row, t] = 1.0, 1.0 + 1.0j
    let_in = fc.host(c, w=w, vis=vis)
    assert all(np.all(np.isfinite(g)) for g in let_in) and fc.check(c, let_in, ref)[0]
    # an error of 100 x the bound on one element, a NaN, D and D2 themselves, a value where D = 0
    bnd, _ = fc.bound(c, ref)
    i = np.unravel_index(np.argmax(bnd), bnd.shape)
    b = good[0].copy()
    b[i[0], i[1], 1, i[2]] += float(100 * bnd[i])
    assert fc.check(c, (b, good[1], good[2]), ref)[0]
    b = good[0].copy()
    b[0, 0, 0, 0] = np.nan
    assert fc.check(c, (b, good[1], good[2]), ref)[0]
    assert fc.check(c, (good[0], good[1] * (1 + 1e-12), good[2]), ref)[0]
    assert fc.check(c, (good[0], good[1], good[2] * (1 - 1e-12)), ref)[0]
    b = good[0].copy()
    b[0, 0, 0, 7] = 1e-300                                                       # the dropped source
    assert fc.check(c, (b, good[1], good[2]), ref)[0]


def _cyl(**kw):
    conf = dict(num_freq=3, freq_start=400.0, freq_end=430.0, num_cylinders=3, cylinder_width=2.0, num_feeds=5, feed_spacing=0.3)
    conf.update(kw)
    return cylinder.UnpolarisedCylinderTelescope.from_config(conf)


def test_windows():
    tel = _cyl()
    tz = tel.zenith[0]
    rng = np.random.default_rng(5)
    nt = 200
    theta = np.concatenate([tz + rng.uniform(-1.2, 1.2, 40), [tz, np.pi - 0.01, 0.3 * tz]])
    theta = np.clip(theta, 1e-3, np.pi - 1e-3)
    phi = np.concatenate([rng.uniform(-7.0, 7.0, 40), [0.0, 1.0, 2 * np.pi - 1e-12]])
    for scale_dec in (True, False):
        win = timestream.formedbeam_windows(tel, theta, phi, nt, 0.3, zmin=0.05, scale_dec=scale_dec)
        turn, k0, half = win["turn"], win["k0"], win["half"]
        assert k0.dtype == np.int32 and half.dtype == np.int32 and turn.dtype == np.float64
        assert np.all((turn >= 0) & (turn < 1)) and np.all((k0 >= 0) & (k0 < nt)) and np.all(half >= -1) and np.all(2 * half + 1 <= nt)
        d = (turn - phi / (2 * np.pi) + 0.5) % 1.0 - 0.5
        assert np.abs(d).max() < 1e-15
        assert np.all(np.abs(((k0 - turn * nt + nt / 2) % nt) - nt / 2) <= 0.5 + 1e-9)
        h0 = int(np.floor(0.3 / (2 * np.pi / nt)))
        if not scale_dec:
            assert half.max() == h0
        else:
            assert half.max() > h0 and half.max() <= nt // 4
        # z >= zmin at both ends against a long-double evaluation of the geometry itself; one step more would not do
        ld = np.longdouble
        pi = np.longdouble("3.14159265358979323846264338327950288")

        def z(k):
            delta = 2 * pi * (turn.astype(ld) - k.astype(ld) / nt)
            return np.cos(ld(tz)) * np.cos(theta.astype(ld)) + np.sin(ld(tz)) * np.sin(theta.astype(ld)) * np.cos(delta)

        live = half >= 0
        assert live.any() and (~live).any()
        for sign in (-1, 1):
            assert np.all(z(k0 + sign * half)[live] >= 0.05 - 1e-15)
        assert np.all(z(k0)[~live] < 0.05 + 1e-15)
        ha = np.minimum(0.3 / np.sin(theta), 7.0) if scale_dec else np.full(theta.shape, 0.3)
        full = np.minimum(np.floor(ha / (2 * np.pi / nt)).astype(int), nt // 4 if scale_dec else (nt - 1) // 2)
        cut = live & (half < full)
        assert np.all(half[live] <= full[live])
        assert np.all(np.minimum(z(k0 - half - 1), z(k0 + half + 1))[cut] < 0.05 + 1e-15)
    # a source that never rises: theta beyond the horizon of the transit
    never = timestream.formedbeam_windows(tel, [min(tz + np.pi / 2 + 0.1, np.pi - 1e-3)], [1.0], nt, 0.3)
    assert never["half"].tolist() == [-1]
    whole = timestream.formedbeam_windows(tel, [tz], [0.0], 9, 10.0, scale_dec=False, zmin=-2.0)
    assert whole["half"].tolist() == [4]
    with pytest.raises(ValueError, match="formedbeam_windows"):
        timestream.formedbeam_windows(tel, [1.0, 2.0], [1.0], nt, 0.3)


def _telescopes():
    pol = cylinder.PolarisedCylinderTelescope.from_config(dict(num_freq=2, freq_start=400.0, freq_end=430.0, num_cylinders=2,
                                                               cylinder_width=2.0, num_feeds=4, feed_spacing=0.3))

    class Dishes(telescope.SimpleUnpolarisedTelescope):
        u_width = v_width = 1.0

        @property
        def _single_feedpositions(self):
            return np.array([[0.0, 0.0], [1.3, 0.2], [2.1, -1.7], [0.4, 3.3], [5.2, 0.9]])

    dish = Dishes.from_config(dict(num_freq=2, freq_start=400.0, freq_end=430.0))
    return dict(cyl=_cyl(), pol=pol, ncm=_cyl(num_freq=2, num_cylinders=2, non_commensurate=True), dish=dish)


@pytest.mark.parametrize("which", ("cyl", "pol", "ncm", "dish"))
def test_groups_against_ringmap_groups(which):
    tel = _telescopes()[which]
    for kw in (dict(), dict(intracyl=False), dict(ew=[float(np.around(np.abs(tel.baselines[:, 0]).max(), 6))])):
        g, rg = timestream.formedbeam_groups(tel, **kw), timestream.ringmap_groups(tel, **kw)
        off, mem = g["group_off"], g["members"]
        assert off.dtype == np.int32 and mem.dtype == np.int32 and g["iu"].dtype == np.int32 and g["iv"].dtype == np.int32
        assert off[0] == 0 and off[-1] == mem.size == g["u"].size == g["v"].size and np.all(np.diff(off) > 0)
        assert np.array_equal(g["uvals"][g["iu"]], g["u"]) and np.array_equal(g["vvals"][g["iv"]], g["v"])
        assert np.all(np.diff(g["uvals"]) > 0) and np.all(np.diff(g["vvals"]) > 0)
        assert np.array_equal(g["u"], np.around(tel.baselines[mem, 0], 6) + 0.0)
        assert np.abs(g["v"] - tel.baselines[mem, 1]).max() <= 5.1e-7
        pols = [tuple(p) for p in g["pol"]]
        assert pols == sorted(set(pols)) == sorted({tuple(p) for p in rg["pol"]})
        for k, pp in enumerate(pols):                   # the same members per class pair
            want = np.concatenate([rg["members"][rg["group_off"][j]:rg["group_off"][j + 1]]
                                   for j in range(len(rg["u"])) if tuple(rg["pol"][j]) == pp])
            mine = mem[off[k]:off[k + 1]]
            assert sorted(mine.tolist()) == sorted(want.tolist())
            key = list(zip(g["v"][off[k]:off[k + 1]], g["u"][off[k]:off[k + 1]], mine))
            assert key == sorted(key)
    g = timestream.formedbeam_groups(tel)
    if which == "cyl":
        assert len(g["pol"]) == 1 and g["uvals"].tolist() == [0.0, 2.0, 4.0] and g["vvals"].size == 9
    if which == "dish":
        assert g["uvals"].size + g["vvals"].size == 2 * g["members"].size      # no structure: the direct path
    assert timestream.formedbeam_groups(tel, ew=[123.0])["members"].size == 0
    t = timestream.ringmap_taper(tel, g, weighting="natural", window="hann")
    assert t.shape == g["members"].shape and t.min() > 0


def test_params_and_env():
    p = timestream.formedbeam_params(dict(name="a", catalogue="c.hdf5", ha_max=0.1, stack=dict(halfwidth=3)))
    assert p["name"] == "a" and p["parts"] == 1 and p["weighting"] == "natural" and p["envelope_fwhm"] is None and p["intracyl"] is True
    assert sorted(p) == sorted(["name", "catalogue", "ha_max", "envelope_fwhm", "weighting", "window", "ew", "intracyl", "parts", "stack"])
    for bad in (dict(colour="red"), dict(weighting="robust"), dict(window="boxcar"), dict(parts=3), dict(stack=dict(width=2)),
                dict(ha_max=-1.0), dict(envelope_fwhm=0.0)):
        with pytest.raises(ValueError, match="formedbeams"):
            timestream.formedbeam_params(bad)
    lam = np.array([0.75, 0.5])
    assert not timestream.formedbeam_env(lam, None).any()
    env = timestream.formedbeam_env(lam, 0.4)
    assert np.allclose(np.exp(-env * (0.5 * 0.4 * lam) ** 2), 0.5, rtol=1e-14)    # half the maximum at half the full width
    with pytest.raises(ValueError):
        timestream.formedbeam_env(lam, -1.0)


def test_value_errors_of_the_host_statement():
    c = fc.make("single")
    fc.host(c, 1)
    dec = c["group_off"].copy()
    dec[1], dec[2] = dec[2], dec[1]
    out = c["members"].copy()
    out[3] = c["nrow"]
    for bad in (dict(dtype=np.float32), dict(parts=3), dict(vis=c["vis"][0]), dict(vis=c["vis"].real), dict(w=c["w"][:, :-1]),
                dict(group_off=dec), dict(group_off=c["group_off"][:-1]), dict(members=out), dict(u=c["u"][:-1]), dict(v=c["v"][:-1]),
                dict(scale=c["scale"][:-1]), dict(env=c["env"][:-1]), dict(env=-np.ones(c["nf"])), dict(env=np.full(c["nf"], np.inf)),
                dict(taper=c["taper"][:-1]), dict(k0=[c["nt"]]), dict(k0=[-1]), dict(half=[-2]), dict(half=[c["nt"] // 2]),
                dict(turn=[0.1, 0.2]), dict(sinth=[]), dict(yc0=[0.1, 0.2]), dict(yc1=[])):
        a = dict(c, parts=1, dtype=np.float64)
        a.update(bad)
        with pytest.raises(ValueError, match="formed_beam_host"):
            timestream.formed_beam_host(a["vis"], a["w"], a["group_off"], a["members"], a["u"], a["v"], a["scale"], a["env"], a["k0"],
                                        a["half"], a["turn"], a["sinth"], a["yc0"], a["yc1"], taper=a["taper"], parts=a["parts"],
                                        dtype=a["dtype"])


def test_ring_map_is_the_special_case():
    """H = 0 on a source exactly on a sample (x = 0), env = 0: the formed beam is the ring map at sinza = y of that
    sample, to a few ulp of sum x_b |V_b| / D."""
    rng = np.random.default_rng(11)
    nf, nrow, nt, nb = 2, 9, 12, 9
    vis = rng.standard_normal((nf, nrow, nt)) + 1j * rng.standard_normal((nf, nrow, nt))
    w = rng.uniform(0.5, 2.0, (nf, nrow, nt))
    w[:, 2, :] = 0.0
    v, taper = (np.arange(nb) - 3) * 0.31, rng.uniform(0.5, 2.0, nb)
    u = np.repeat([0.0, 2.0, 4.0], 3)
    scale = np.array([2.1, 6.3])
    theta = np.array([0.4, 1.1, 0.885])
    k0 = np.array([3, 0, 11], dtype=np.int32)
    tabs = timestream.formedbeam_tables(0.885, theta)
    y = tabs["yc0"] - tabs["yc1"]                                                # D = 0 exactly
    fb = timestream.formed_beam_host(vis, w, [0, nb], np.arange(nb), u, v, scale, np.zeros(nf), k0, np.zeros(3, dtype=np.int32),
                                     k0 / nt, tabs["sinth"], tabs["yc0"], tabs["yc1"], taper=taper, parts=2)
    rm = timestream.ringmap_host(vis, w, [0, nb], np.arange(nb), v, scale, y, taper=taper, parts=2)
    mag = timestream.ringmap_host(np.abs(vis).astype(complex), w, [0, nb], np.arange(nb), 0 * v, scale, y, taper=taper)[0]
    for s in range(3):
        assert np.all(np.abs(fb[1][:, 0, s] - rm[1][:, 0, k0[s]]) <= 2 * nb * fc.U * rm[1][:, 0, k0[s]])   # two orders of nb terms
        # two sums of 2 nb products in two orders, the products and the division: (2 nb + 8) u
        assert np.all(np.abs(fb[0][:, 0, :, s] - rm[0][:, 0, :, s, k0[s]]) <= (2 * nb + 8) * fc.U * mag[:, 0, :, s, k0[s]])
