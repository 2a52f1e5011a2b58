"""GPU: the Monte-Carlo Fisher estimators (dm_psmc_draw, dm_psmc_moments, dm_psmc_alt): the device draws against the
numpy restatement of the Philox stream, both estimators against the unmodified reference with its recorded draws
(tests/golden/psmc.npz), the moments kernel against numpy, convergence to the exact Fisher matrix, determinism over
runs, batches, sample chunks and ranks, and ProductManager / Timestream end to end.  Every draw is a fixed function
of the seed, so each statistical bound either always holds or never does."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_pipeline as tp
from test_host_psmc import alt_fisher, alt_vecs, draws
from test_host_qestimator import q_estimate

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def setup(golden_dir, tmp_path_factory):
    from driftscan_amd import beamtransfer, device, kltransform, psestimation, psmc, storage

    device.reset_context()
    g = np.load(os.path.join(golden_dir, "svdkl_unpol.npz"))
    p = np.load(os.path.join(golden_dir, "psfisher.npz"))
    gold = np.load(os.path.join(golden_dir, "psmc.npz"))
    tel = tp.FakeTelescope(g)
    bt = beamtransfer.BeamTransfer(str(tmp_path_factory.mktemp("psmc")), telescope=tel)
    bt.polsvcut, bt.svcut = float(g["polsvcut"]), float(g["svcut"])
    bt._generate_dirs()
    mlist = [int(m) for m in g["mlist"]]
    for mi in mlist:
        with storage.File(bt._mfile(mi), "w") as f:
            f.create_dataset("beam_m", data=g["m%d_beam_m" % mi][..., mi:])
    bt._my_ms = lambda mlist_=None: mlist
    bt._generate_svdfiles(regen=True)
    kl = kltransform.KLTransform.from_config(dict(threshold=float(g["threshold"])), bt, subdir="kl")
    kl._cvsg, kl._cvfg = g["cv_sg"], g["cv_fg"]
    for mi in mlist:
        kl.transform_save(mi)

    def make(cls, name, **cfg):
        ps = cls.from_config(dict(cfg), kl, subdir=name)
        ps.clarray = p["clarray"]
        ps.k_center = np.arange(p["clarray"].shape[0], dtype=np.float64)
        return ps

    exact = make(psestimation.PSExact, "exact")
    return dict(gold=gold, bt=bt, kl=kl, mlist=mlist, make=make, exact=exact)


def host_products(s, mi):
    ev, E = s["kl"].modes_m(mi)
    return ev, E, np.asarray(s["bt"].beam_svd(mi)), np.asarray(s["bt"]._svd_num(mi)[0])


# ---- 1. draws --------------------------------------------------------------------------------------------------------
def test_draws_match_restatement():
    from driftscan_amd import device

    ctx = device.get_context()
    rng = np.random.default_rng(3)
    nm = [37, 0, 300]
    ms = [4, 9, 130]
    ev = [rng.random(n) * 5.0 for n in nm]
    evd = ctx.to_device(np.concatenate(ev))
    eoff = np.concatenate([[0], np.cumsum(nm)[:-1]])
    seed = 0x123456789AB
    for kind, power, stream in ((0, 1, 0), (0, 0, 1), (1, -1, 2), (1, 0, 2)):
        R = 33
        got = ctx.psmc_draw(ms, nm, R, seed, stream=stream, kind=kind, power=power, s0=5, evals=evd,
                            evals_off=eoff).cpu().numpy()
        o = 0
        for m, n, e in zip(ms, nm, ev):
            ref = draws(seed, m, n, R, stream, kind=kind, power=power, evals=e, start=5)
            blk = got[o : o + n * R].reshape(n, R)
            o += n * R
            if kind == 1:
                assert np.array_equal(blk, ref), (kind, power)
            elif n:
                assert np.abs(blk - ref).max() <= 1e-14 * np.abs(ref).max(), (kind, power)
        # the first k of n columns are a k-column draw, bit for bit
        few = ctx.psmc_draw(ms, nm, 7, seed, stream=stream, kind=kind, power=power, s0=5, evals=evd,
                            evals_off=eoff).cpu().numpy()
        o, of = 0, 0
        for n in nm:
            assert np.array_equal(few[of : of + n * 7].reshape(n, 7), got[o : o + n * R].reshape(n, R)[:, :7])
            o, of = o + n * R, of + n * 7


def test_draw_moments():
    from driftscan_amd import device

    ctx = device.get_context()
    n, R = 1000, 1000
    ev = np.linspace(0.0, 9.0, n)
    x = ctx.psmc_draw([17], [n], R, 11, power=1, evals=ctx.to_device(ev), evals_off=[0]).cpu().numpy().reshape(n, R)
    w = np.abs(x) ** 2 / (ev + 1.0)[:, np.newaxis]   # Exp(1): mean 1, sd 1
    assert abs(w.mean() - 1.0) <= 5.0 / np.sqrt(w.size)
    z = x / np.sqrt(ev + 1.0)[:, np.newaxis]
    assert abs(z.real.mean()) <= 5.0 * np.sqrt(0.5 / z.size) and abs(z.imag.mean()) <= 5.0 * np.sqrt(0.5 / z.size)
    assert abs(np.mean(z.real**2) - 0.5) <= 5.0 * np.sqrt(0.5 / z.size)
    assert abs(np.mean(z.real * z.imag)) <= 5.0 * 0.5 / np.sqrt(z.size)
    per_mode = np.mean(np.abs(x) ** 2, axis=1) / (ev + 1.0)   # each mode's variance is lambda + 1
    assert np.all(np.abs(per_mode - 1.0) <= 5.0 / np.sqrt(R))
    r = ctx.psmc_draw([17], [n], R, 11, stream=2, kind=1).cpu().numpy()
    assert abs(r.real.mean()) <= 5.0 / np.sqrt(r.size)


# ---- 2. the reference with its recorded draws ------------------------------------------------------------------------
def _phase_map(s, mi):
    """U: the reference's KL coordinates -> these.  The two SVD bases span the same rows of each frequency's beam, so
    S_f = B_own,f pinv(B_ref,f) maps the reference's SVD coordinates to these; a mode of each side then agrees up to a
    phase, E_own S = diag(phi) E_ref, and U = diag(phi)."""
    gold = s["gold"]
    ev, E, bs, sv = host_products(s, mi)
    rb, rsv, Er = gold["m%d_beam_svd" % mi], gold["m%d_svnum" % mi], gold["m%d_evecs" % mi]
    assert np.array_equal(sv, rsv)
    bounds = np.concatenate([[0], np.cumsum(sv)])
    S = np.zeros((bounds[-1], bounds[-1]), dtype=np.complex128)
    for f in range(len(sv)):
        S[bounds[f] : bounds[f + 1], bounds[f] : bounds[f + 1]] = bs[f, : sv[f], 0, :] @ np.linalg.pinv(rb[f, : sv[f]])
    W = E @ S
    phi = np.sum(W * Er.conj(), axis=1) / np.sum(np.abs(Er) ** 2, axis=1)
    assert np.abs(np.abs(phi) - 1.0).max() < 1e-8
    assert np.abs(W - phi[:, np.newaxis] * Er).max() < 1e-8 * np.abs(Er).max()
    return np.diag(phi)


def test_against_reference(setup):
    from driftscan_amd import psmc

    s = setup
    gold = s["gold"]
    ns = int(gold["nsamples"])

    class Injected(psmc.PSMonteCarlo):
        def gen_sample(self, mi, nsamples=None, noiseonly=False):
            return _phase_map(s, mi) @ gold["m%d_x" % mi][:, :nsamples]

    class InjectedAlt(psmc.PSMonteCarloAlt):
        def gen_signs(self, mi, nsamples=None, start=0):
            return _phase_map(s, mi) @ gold["m%d_signs" % mi]

    mc = s["make"](Injected, "gold_mc", nsamples=ns)
    alt = s["make"](InjectedAlt, "gold_alt", nsamples=ns)
    # The reference's modes and these come from different eigensolvers and agree (after the phase map) to ~1e-11, which
    # carries into the estimates: the reference is pinned to GOLD_TOL (the exact Fisher pin allows 1e-8 for the same
    # reason); the device kernels are pinned to 1e-12 by the restatement on this side's own modes.
    GOLD_TOL = 1e-10
    for mi in s["mlist"]:
        if int(gold["m%d_nmodes" % mi]) == 0:
            continue
        ev, E, bs, sv = host_products(s, mi)
        x = _phase_map(s, mi) @ gold["m%d_x" % mi]
        f, b = mc.fisher_bias_m(mi)
        rf, rb = gold["m%d_mc_fisher" % mi], gold["m%d_mc_bias" % mi]
        assert f.shape == rf.shape and b.shape == rb.shape
        assert np.abs(f - rf).max() <= GOLD_TOL * np.abs(rf).max(), mi
        assert np.abs(b - rb).max() <= GOLD_TOL * np.abs(rb).max(), mi
        qa = q_estimate(ev, E, bs, sv, mc.clarray, x)
        assert np.abs(f - np.cov(qa)).max() <= 1e-12 * np.abs(rf).max(), mi
        assert np.abs(b - qa.mean(axis=1)).max() <= 1e-12 * np.abs(rb).max(), mi
        f, b = alt.fisher_bias_m(mi)
        rf = gold["m%d_alt_fisher" % mi]
        assert np.abs(f - rf).max() <= GOLD_TOL * np.abs(rf).max(), mi
        assert not np.any(b)
        alt.gen_vecs(mi)
        ref = alt_vecs(ev, E, bs, sv, alt.clarray, _phase_map(s, mi) @ gold["m%d_signs" % mi])
        assert len(alt.vec_cache) == alt.nbands
        for a in range(alt.nbands):
            assert np.abs(alt.vec_cache[a] - ref[a]).max() <= 1e-12 * max(np.abs(r).max() for r in ref)
        assert np.abs(alt_fisher(ref, ns) - f).max() <= 1e-12 * np.abs(rf).max()


# ---- 3. moments ------------------------------------------------------------------------------------------------------
def test_moments_kernel(setup):
    from driftscan_amd import device

    s = setup
    from driftscan_amd import psmc

    ctx = device.get_context()
    ps = s["make"](psmc.PSMonteCarlo, "mom", nsamples=300, seed=4)
    qs = []
    for mi in s["mlist"]:
        x = ps.gen_sample(mi)
        qs.append(ps.q_estimator(mi, x, noise=True))
    q = np.stack(qs)
    mean, cov = ctx.psmc_moments(ctx.to_device(q))
    mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
    for k in range(len(qs)):
        rc = np.cov(q[k])
        assert np.abs(cov[k] - rc).max() <= 1e-13 * np.abs(rc).max()
        assert np.abs(mean[k] - q[k].mean(axis=1)).max() <= 1e-13 * np.abs(q[k]).max()
        assert np.array_equal(cov[k], cov[k].T)


# ---- 4. convergence --------------------------------------------------------------------------------------------------
def _exact_bias(s, ps, mi):
    """tr(C^-1 Q_a) in the KL basis of the device's modes, C = diag(lambda + 1)."""
    ev, E, bs, sv = host_products(s, mi)
    F, L = bs.shape[0], bs.shape[-1]
    bounds = np.concatenate([[0], np.cumsum(sv)])
    M = np.zeros((bounds[-1], F * L), dtype=np.complex128)
    for f in range(F):
        M[bounds[f] : bounds[f + 1], f * L : (f + 1) * L] = bs[f, : sv[f], 0, :]
    out = np.zeros(ps.nbands)
    for a in range(ps.nbands):
        C = np.zeros((F * L, F * L))
        for l in range(mi, L):
            C[l::L, l::L] = ps.clarray[a, l]
        Q = E @ (M @ C @ M.conj().T) @ E.conj().T
        out[a] = (np.diag(Q).real / (ev + 1.0)).sum()
    return out


@pytest.mark.parametrize("kind", ["mc", "alt", "cross"])
def test_convergence(setup, kind):
    from driftscan_amd import psmc

    s = setup
    cls = dict(mc=psmc.PSMonteCarlo, alt=psmc.PSMonteCarloAlt, cross=psmc.CrossPower)[kind]
    factor = 0.5 if kind == "cross" else 1.0   # the cross q's y side is projected from x2
    nseeds, ns = 8, 2000
    runs = [s["make"](cls, "conv_%s_%d" % (kind, k), nsamples=ns, seed=100 + k).fisher_bias_batch(s["mlist"])
            for k in range(nseeds)]
    for j, mi in enumerate(s["mlist"]):
        fe = factor * s["exact"].fisher_bias_m(mi)[0].real
        fs = np.array([r[j][0].real for r in runs])
        mean, se = fs.mean(axis=0), fs.std(axis=0, ddof=1) / np.sqrt(nseeds)
        scale = np.abs(fe).max()
        assert np.all(np.abs(mean - fe) <= 5.0 * se + 1e-10 * scale), (kind, mi)
        # a few per cent: the seed mean's relative standard error is ~ sqrt(2 / (nseeds ns)) = 1.1 % per element, and a
        # handful of modes carry each m's Fisher matrix
        assert np.linalg.norm(mean - fe) <= 0.05 * np.linalg.norm(fe), (kind, mi)
        if kind == "mc":
            be = _exact_bias(s, s["exact"], mi)
            bs_ = np.array([r[j][1] for r in runs])
            bm, bse = bs_.mean(axis=0), bs_.std(axis=0, ddof=1) / np.sqrt(nseeds)
            assert np.all(np.abs(bm - be) <= 5.0 * bse + 1e-10 * np.abs(be).max()), mi
            assert np.linalg.norm(bm - be) <= 0.05 * np.linalg.norm(be), mi


# ---- 5. determinism --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["mc", "alt", "cross"])
def test_batching_and_chunks_bit_identical(setup, kind):
    from driftscan_amd import psmc

    s = setup
    cls = dict(mc=psmc.PSMonteCarlo, alt=psmc.PSMonteCarloAlt, cross=psmc.CrossPower)[kind]
    ps = s["make"](cls, "det_" + kind, nsamples=200, seed=9)
    one = ps.fisher_bias_batch(s["mlist"])
    again = ps.fisher_bias_batch(s["mlist"])
    # a budget that holds one m at the full width but not two
    need = max(ps._mc_need(mi, ps.nsamples) for mi in s["mlist"])
    ps.ps_chunk_gb = 1.01 * need / (1 << 30)
    assert all(len(b) == 1 for b in ps._mc_plan(s["mlist"])[1]) and ps._mc_plan(s["mlist"])[0] == ps.nsamples
    per_m = ps.fisher_bias_batch(s["mlist"])
    # and one that splits the samples into chunks
    fixed = max(ps._mc_need(mi, 0) for mi in s["mlist"])
    ps.ps_chunk_gb = (fixed + 0.3 * (need - fixed)) / (1 << 30)
    R = ps._mc_plan(s["mlist"])[0]
    assert R < ps.nsamples
    chunked = ps.fisher_bias_batch(s["mlist"])
    for a, b, c, d in zip(one, again, per_m, chunked):
        for k in range(2):
            assert np.array_equal(a[k], b[k]) and np.array_equal(a[k], c[k])
            if kind == "alt" and k == 0:   # the chunks' Fisher sums are added: a different summation order
                assert np.abs(a[k] - d[k]).max() <= 1e-13 * np.abs(a[k]).max()
            else:
                assert np.array_equal(a[k], d[k])


def _conf(outdir, psentry):
    return dict(config=dict(beamtransfers=True, kltransform=True, psfisher=True, output_directory=str(outdir),
                            truncate=False),
                psfisher=[dict(psentry, name="ps", klname="kl", threshold=0.0, bandtype="polar", num_theta=1,
                               k_bands=[dict(spacing="linear", start=0.0, stop=0.006, num=4)])],
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, use_foregrounds=False)])


def _generate(d, psentry):
    import yaml

    from driftscan_amd import manager

    os.makedirs(str(d), exist_ok=True)
    cfile = os.path.join(str(d), "params.yaml")
    open(cfile, "w").write(yaml.dump(_conf(os.path.join(str(d), "prod"), psentry)))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    return pm, cfile


ENTRIES = dict(mc=dict(type="MonteCarlo", exact=False, nsamples=256, seed=5), cross=dict(type="Cross", nsamples=256, seed=6),
               alt=dict(type="MonteCarloAlt", exact=False, nsamples=256, seed=7))


@pytest.fixture(scope="module")
def prods(tmp_path_factory):
    from driftscan_amd import device

    device.reset_context()
    d = tmp_path_factory.mktemp("psmc_e2e")
    return {k: (d / k,) + _generate(d / k, e) for k, e in ENTRIES.items()}


def _fisher_file(pm):
    from driftscan_amd import storage

    with storage.File(pm.psestimators["ps"].psdir + "/fisher.hdf5", "r") as f:
        return {k: f[k][:] for k in ("fisher", "bias", "covariance")}


@pytest.mark.parametrize("kind", ["mc", "cross", "alt"])
def test_generate_twice_bit_identical(prods, tmp_path, kind):
    from driftscan_amd import psmc

    d, pm, _ = prods[kind]
    ps = pm.psestimators["ps"]
    assert type(ps) is dict(mc=psmc.PSMonteCarlo, cross=psmc.CrossPower, alt=psmc.PSMonteCarloAlt)[kind]
    a = _fisher_file(pm)
    assert np.abs(a["fisher"]).max() > 0 and np.all(np.diag(a["fisher"]) > 0)
    pm2, _ = _generate(tmp_path / "again", ENTRIES[kind])
    b = _fisher_file(pm2)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


_RANK_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group(backend="gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
from driftscan_amd import manager
pm = manager.ProductManager.from_config(%(cfile)r)
ps = pm.psestimators["ps"]
ps.psdir = %(psdir)r
ps.generate(regen=True)
dist.barrier()
dist.destroy_process_group()
'''


def test_two_ranks_match_one(prods, tmp_path):
    from driftscan_amd import storage

    d, pm, cfile = prods["mc"]
    one = _fisher_file(pm)
    psdir = str(tmp_path / "ps2")
    os.makedirs(psdir)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % dict(root=ROOT, port=port, cfile=cfile, psdir=psdir))
    env = dict(os.environ, DRIFTMI_DEVICE="0", DRIFTMI_WORKSPACE_GB="2")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    with storage.File(psdir + "/fisher.hdf5", "r") as f:
        for k in ("fisher", "bias"):
            a, b = one[k], f[k][:]
            assert np.abs(a - b).max() <= 1e-13 * np.abs(a).max(), k


# ---- 6. power spectra against the sampled estimators -----------------------------------------------------------------
def _stream(pm, path, seed):
    from driftscan_amd import timestream

    ts = timestream.Timestream(str(path), pm)
    ts.set_kltransform("kl")
    for mi in range(pm.telescope.mmax + 1):
        os.makedirs(ts._mdir(mi), exist_ok=True)
    np.random.seed(seed)
    ts.fake_kl_data()
    ts.set_psestimator("ps")
    return ts


@pytest.mark.parametrize("kind", ["mc", "cross"])
def test_powerspectra(prods, kind):
    from driftscan_amd import timestream

    d, pm, _ = prods[kind]
    ps = pm.psestimators["ps"]
    mlist = list(range(1, pm.telescope.mmax + 1))
    ts = _stream(pm, d / "ts0", 1)
    p = ts.powerspectrum()
    ps.genbands()
    fisher, bias = ps.fisher_bias()
    qsum = sum(ps.q_estimator(mi, ts.mmode_kl(mi)) for mi in mlist)
    ref = np.linalg.inv(fisher) @ (qsum - bias)
    assert np.all(np.isfinite(p)) and np.abs(p - ref).max() <= 1e-10 * np.abs(ref).max()
    streams = [ts, _stream(pm, d / "ts1", 2)]
    cp = timestream.cross_powerspectrum(streams, "ps", str(d / "cross.hdf5"))
    ps.genbands()
    qp = sum(ps.q_estimator(mi, streams[0].mmode_kl(mi), streams[1].mmode_kl(mi)) for mi in mlist)
    ref = np.linalg.inv(fisher) @ (qp - bias)
    assert np.abs(cp[0, 1] - ref).max() <= 1e-10 * np.abs(ref).max()
    ps.delbands()
