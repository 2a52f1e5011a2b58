"""CPU: the Monte-Carlo estimators exist with the reference's names, properties and defaults (drift/core/psmc.py,
crosspower.py), the product manager resolves them, and numpy restatements — of the Philox4x32-10 sample stream, of
the Box-Muller / Rademacher mapping and of both estimators — agree with the unmodified reference
(tests/golden/psmc.npz, from tests/gen_golden_psmc.py).  The GPU tests use the restatements as well."""
import inspect
import logging
import os

import numpy as np
import pytest

from test_host_qestimator import _as, q_estimate, sky_to_svd, svd_to_sky

M32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al. 2011) on uint32 arrays: ctr (4, ...) and key (2,) -> (4, ...)."""
    c = [np.asarray(ctr[i], dtype=np.uint64) & M32 for i in range(4)]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & M32
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
    return [x.astype(np.uint32) for x in c]


def u53(a, b):
    k = (a.astype(np.uint64) >> np.uint64(5)) << np.uint64(26) | (b.astype(np.uint64) >> np.uint64(6))
    return (k + np.uint64(1)).astype(np.float64) * 2.0**-53


def draws(seed, m, nmodes, nsamples, stream, kind=0, power=0, evals=None, start=0):
    """The (nmodes, nsamples) draws of dm_psmc_draw: kind 0 complex normal (Box-Muller), 1 Rademacher; scaled by
    (evals + 1)^(power / 2)."""
    i, s = np.meshgrid(np.arange(nmodes), np.arange(start, start + nsamples), indexing="ij")
    ctr = [i, s, np.full_like(i, m), np.full_like(i, stream)]
    w = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32))
    if kind == 1:
        z = np.where(w[0] >> np.uint32(31), -1.0, 1.0).astype(np.complex128)
    else:
        rad = np.sqrt(-np.log(u53(w[0], w[1])))
        th = 6.283185307179586 * u53(w[2], w[3])
        z = rad * np.cos(th) + 1j * (rad * np.sin(th))
    if power:
        sc = np.sqrt(np.asarray(evals) + 1.0)
        sc = sc if power > 0 else 1.0 / sc
        z = z * sc[:, np.newaxis]
    return z


def alt_vecs(evals, evecs, beam_svd, svnum, clarray, signs, dtype=np.complex128):
    """v_a = cf E B C_a B^H E^H cf xv (psmc.py:111-161), clarray (nbands, L, F, F).  `dtype`: the complex type of the
    arithmetic (np.clongdouble for an extended-precision reference)."""
    evecs, beam_svd, signs, evals, clarray = _as(dtype, (evecs, beam_svd, signs), (evals, clarray))
    cf = (evals + 1.0) ** -0.5
    x3 = svd_to_sky(beam_svd, svnum, evecs.conj().T @ (cf[:, np.newaxis] * signs), dtype=dtype)   # (F, L, ns)
    out = []
    for a in range(clarray.shape[0]):
        x4 = np.einsum("lfg,gls->fls", clarray[a], x3)
        x5 = sky_to_svd(beam_svd, svnum, x4[:, np.newaxis], dtype=dtype)
        out.append(cf[:, np.newaxis] * (evecs @ x5))
    return out


def alt_fisher(vecs, ns, dtype=np.complex128):
    nb = len(vecs)
    vecs = _as(dtype, vecs)
    f = np.zeros((nb, nb), dtype=dtype)
    for a in range(nb):
        for b in range(a + 1):
            f[a, b] = np.sum(vecs[a] * vecs[b].conj()) / ns
            f[b, a] = np.conj(f[a, b])
    return f


def golden_products(q, mi):
    """(evals, evecs, beam_svd (F, nsv, 1, L), svnum) of the reference at m = mi."""
    return q["m%d_evals" % mi], q["m%d_evecs" % mi], q["m%d_beam_svd" % mi][:, :, np.newaxis], q["m%d_svnum" % mi]


# ---- the API ---------------------------------------------------------------------------------------------------------
def test_classes_and_defaults():
    from driftscan_amd import psestimation, psmc

    assert issubclass(psmc.PSMonteCarlo, psestimation.PSEstimation)
    assert issubclass(psmc.PSMonteCarloAlt, psestimation.PSEstimation)
    assert issubclass(psmc.CrossPower, psmc.PSMonteCarlo)
    assert psmc.CrossPower.crosspower and not psmc.PSMonteCarlo.crosspower
    props = {c: c._properties() for c in (psmc.PSMonteCarlo, psmc.PSMonteCarloAlt, psmc.CrossPower)}
    for c, p in props.items():
        assert p["nsamples"].default == 500 and p["seed"].default == 0, c
    assert props[psmc.PSMonteCarloAlt]["nswitch"].default == 0
    assert list(inspect.signature(psmc.PSMonteCarlo.gen_sample).parameters)[:4] == ["self", "mi", "nsamples", "noiseonly"]
    assert list(inspect.signature(psmc.PSMonteCarloAlt.gen_vecs).parameters) == ["self", "mi"]
    for c in (psmc.PSMonteCarlo, psmc.PSMonteCarloAlt, psmc.CrossPower):
        assert list(inspect.signature(c._work_fisher_bias_m).parameters) == ["self", "mi"]
        assert list(inspect.signature(c.fisher_bias_batch).parameters) == ["self", "ms"]


def _manager(tmp_path, psentry):
    import yaml

    from driftscan_amd import manager

    conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=True, output_directory=str(tmp_path / "out")),
                telescope=dict(type="UnpolarisedCylinder", num_freq=2, freq_start=400.0, freq_end=420.0,
                               num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4),
                kltransform=[dict(type="KLTransform", name="kl")],
                psfisher=[dict(psentry, name="ps", klname="kl")])
    cfile = tmp_path / "params.yaml"
    cfile.write_text(yaml.dump(conf))
    return manager.ProductManager.from_config(str(cfile)).psestimators["ps"]


@pytest.mark.parametrize("entry, cls, warns", [
    (dict(type="MonteCarlo"), "PSExact", True),
    (dict(type="MonteCarloAlt"), "PSExact", True),
    (dict(type="MonteCarlo", exact=True), "PSExact", True),
    (dict(type="MonteCarlo", exact=False, nsamples=64, seed=3), "PSMonteCarlo", False),
    (dict(type="MonteCarloAlt", exact=False, nswitch=7), "PSMonteCarloAlt", False),
    (dict(type="Cross"), "CrossPower", False),
    (dict(type=dict(module="driftscan_amd.psmc", **{"class": "PSMonteCarlo"})), "PSMonteCarlo", False),
    (dict(type=dict(module="driftscan_amd.psmc", **{"class": "CrossPower"})), "CrossPower", False),
])
def test_manager_resolution(tmp_path, caplog, entry, cls, warns):
    with caplog.at_level(logging.WARNING, logger="driftscan_amd.manager"):
        ps = _manager(tmp_path, entry)
    assert type(ps).__name__ == cls
    assert any("exact Fisher matrix instead of a Monte-Carlo" in r.getMessage() for r in caplog.records) == warns
    if "nsamples" in entry:
        assert ps.nsamples == 64 and ps.seed == 3
    if "nswitch" in entry:
        assert ps.nswitch == 7


def test_unknown_type_still_raises(tmp_path):
    with pytest.raises(Exception, match="Unsupported PS estimator"):
        _manager(tmp_path, dict(type="Nope"))


# ---- the sample stream -----------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """The Random123 known-answer vectors of Philox4x32-10."""
    cases = [
        ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
        ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
        ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
         (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
    ]
    for ctr, key, want in cases:
        got = philox4x32_10([np.array([c], dtype=np.uint64) for c in ctr], key)
        assert tuple(int(g[0]) for g in got) == want


def test_draw_mapping():
    u = u53(np.array([0, 0xFFFFFFFF], dtype=np.uint32), np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert u[0] == 2.0**-53 and u[1] == 1.0
    z = draws(5, 3, 400, 500, 0)
    assert z.shape == (400, 500)
    assert abs(np.mean(np.abs(z) ** 2) - 1.0) < 5 * 1.0 / np.sqrt(z.size)
    assert abs(np.mean(z)) < 5 / np.sqrt(z.size)
    # the first k of n columns are a k-column draw; streams, m and seeds are independent
    assert np.array_equal(draws(5, 3, 7, 4, 0), z[:7, :4])
    assert np.array_equal(draws(5, 3, 7, 4, 0, start=10), z[:7, 10:14])
    for other in (draws(5, 3, 7, 4, 1), draws(5, 4, 7, 4, 0), draws(6, 3, 7, 4, 0)):
        assert not np.any(other == z[:7, :4])
    r = draws(5, 3, 400, 500, 2, kind=1)
    assert set(np.unique(r.real)) == {-1.0, 1.0} and not r.imag.any()
    assert abs(r.real.mean()) < 5 / np.sqrt(r.size)
    ev = np.linspace(0.0, 3.0, 7)
    assert np.array_equal(draws(5, 3, 7, 4, 2, kind=1, power=-1, evals=ev),
                          draws(5, 3, 7, 4, 2, kind=1)[:7] / np.sqrt(ev + 1.0)[:, np.newaxis])


def test_split_m_matches_caput():
    from driftscan_amd.psmc import split_m

    num, s, e = split_m(10, 3)
    assert list(num) == [4, 3, 3] and list(s) == [0, 4, 7] and list(e) == [4, 7, 10]


# ---- the estimators against the reference ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "psmc.npz")), np.load(os.path.join(golden_dir, "psfisher.npz"))["clarray"]


def test_montecarlo_restatement(gold):
    q, cl = gold
    ns = int(q["nsamples"])
    for mi in q["mlist"]:
        if int(q["m%d_nmodes" % mi]) == 0:
            continue
        ev, E, bs, sv = golden_products(q, mi)
        qa = q_estimate(ev, E, bs, sv, cl, q["m%d_x" % mi])
        assert qa.shape == (cl.shape[0], ns)
        f, b = q["m%d_mc_fisher" % mi], q["m%d_mc_bias" % mi]
        assert np.abs(np.cov(qa) - f).max() <= 1e-12 * np.abs(f).max(), mi
        assert np.abs(qa.mean(axis=1) - b).max() <= 1e-12 * np.abs(b).max(), mi


def test_alt_restatement(gold):
    q, cl = gold
    ns = int(q["nsamples"])
    for mi in q["mlist"]:
        if int(q["m%d_nmodes" % mi]) == 0:
            continue
        ev, E, bs, sv = golden_products(q, mi)
        f = alt_fisher(alt_vecs(ev, E, bs, sv, cl, q["m%d_signs" % mi]), ns)
        ref = q["m%d_alt_fisher" % mi]
        assert np.abs(f - ref).max() <= 1e-12 * np.abs(ref).max(), mi
        assert not q["m%d_alt_bias" % mi].any()
