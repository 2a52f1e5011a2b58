"""GPU: the quadratic estimator (dm_qestimate) against the unmodified reference's q_estimator
(tests/golden/qestimator.npz), the Fisher identity sum_r q_a(V_b e_r) = F_ab, the cross path, batching, the
many-column path and run-to-run determinism."""
import os

import numpy as np
import pytest

import test_gpu_pipeline as tp
from test_host_qestimator import q_estimate, sky_to_svd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def setup(golden_dir, tmp_path_factory):
    from driftscan_amd import beamtransfer, device, kltransform, psestimation, storage

    device.reset_context()
    g = np.load(os.path.join(golden_dir, "svdkl_unpol.npz"))
    p = np.load(os.path.join(golden_dir, "psfisher.npz"))
    q = np.load(os.path.join(golden_dir, "qestimator.npz"))
    tel = tp.FakeTelescope(g)
    bt = beamtransfer.BeamTransfer(str(tmp_path_factory.mktemp("qest")), telescope=tel)
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
    ps = psestimation.PSExact.from_config(dict(threshold=float(p["ps_threshold"])), kl, subdir="ps")
    ps.clarray = p["clarray"]
    ps.k_center = np.arange(p["clarray"].shape[0], dtype=np.float64)
    return q, bt, kl, ps, mlist


def host_products(bt, kl, mi):
    ev, E = kl.modes_m(mi)
    return ev, E, np.asarray(bt.beam_svd(mi)), np.asarray(bt._svd_num(mi)[0])


def kl_data(bt, kl, mi, a):
    ev, E, bs, sv = host_products(bt, kl, mi)
    return E @ sky_to_svd(bs, sv, a)


def test_against_reference(setup):
    q, bt, kl, ps, mlist = setup
    for mi in mlist:
        assert kl.modes_m(mi)[0].size == int(q["m%d_nmodes" % mi])
        v = kl_data(bt, kl, mi, q["m%d_a" % mi])
        scale = np.abs(q["m%d_q" % mi]).max()
        got = ps.q_estimator(mi, v)
        assert got.shape == q["m%d_q" % mi].shape
        assert np.abs(got - q["m%d_q" % mi]).max() <= 1e-12 * scale, mi
        got1 = ps.q_estimator(mi, v[:, 0])
        assert got1.shape == (ps.nbands,)
        assert np.abs(got1 - q["m%d_q1" % mi]).max() <= 1e-12 * scale, mi
        try:
            for cp in (0, 1):
                for zm in (0, 1):
                    ps.crosspower, ps.zero_mean = bool(cp), bool(zm)
                    ref = q["m%d_qn_%d%d" % (mi, cp, zm)]
                    got = ps.q_estimator(mi, v, noise=True)
                    assert got.shape == (ps.nbands + 1, 3)
                    assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max(), (mi, cp, zm)
        finally:
            ps.crosspower, ps.zero_mean = False, True


def test_fisher_identity(setup):
    """With V_b V_b^H = C_b (band b in the KL basis of the device's own modes), sum_r q_a(V_b e_r) = Re F_ab."""
    q, bt, kl, ps, mlist = setup
    cl = ps.clarray
    for mi in mlist:
        ev, E, bs, sv = host_products(bt, kl, mi)
        F, L = bs.shape[0], bs.shape[-1]
        bounds = np.concatenate([[0], np.cumsum(sv)])
        M = np.zeros((bounds[-1], F * L), dtype=np.complex128)   # SVD basis <- (f, l) sky, temperature
        for f in range(F):
            M[bounds[f] : bounds[f + 1], f * L : (f + 1) * L] = bs[f, : sv[f], 0, :]
        fisher, _ = ps.fisher_bias_m(mi)
        nb = cl.shape[0]
        lhs = np.zeros((nb, nb))
        for b in range(nb):
            C = np.zeros((F * L, F * L))
            for l in range(L):
                C[l::L, l::L] = cl[b, l]
            Ckl = E @ (M @ C @ M.conj().T) @ E.conj().T
            w, U = np.linalg.eigh(0.5 * (Ckl + Ckl.conj().T))
            V = U * np.sqrt(np.clip(w, 0.0, None))
            lhs[:, b] = ps.q_estimator(mi, V).sum(axis=1)
        assert np.abs(lhs - fisher.real).max() <= 1e-11 * np.abs(fisher).max(), mi


def test_cross_path(setup):
    q, bt, kl, ps, mlist = setup
    rng = np.random.default_rng(7)
    for mi in mlist:
        ev, E, bs, sv = host_products(bt, kl, mi)
        x = kl_data(bt, kl, mi, q["m%d_a" % mi])
        y = kl_data(bt, kl, mi, q["m%d_a" % mi][..., ::-1] + 0.3 * rng.standard_normal(q["m%d_a" % mi].shape))
        qxy = ps.q_estimator(mi, x, y)
        qxx, qyy = ps.q_estimator(mi, x), ps.q_estimator(mi, y)
        ref = q_estimate(ev, E, bs, sv, ps.clarray, x, y)
        tol = 1e-12 * np.sqrt(np.abs(qxx) * np.abs(qyy)).max()
        assert np.abs(qxy - ref).max() <= tol, mi
        assert np.abs(ps.q_estimator(mi, y, x) - qxy).max() <= tol
        assert np.abs(ps.q_estimator(mi, x, x) - qxx).max() <= 1e-13 * np.abs(qxx).max()
        qn = ps.q_estimator(mi, x, y, noise=True)
        refn = q_estimate(ev, E, bs, sv, ps.clarray, x, y, noise=True, crosspower=False, zero_mean=True)
        assert np.abs(qn - refn).max() <= 1e-12 * np.abs(refn).max()


def test_batch_equals_per_m_and_empty_block(setup):
    q, bt, kl, ps, mlist = setup
    vs = [kl_data(bt, kl, mi, q["m%d_a" % mi]) for mi in mlist]
    batch = ps.q_estimator_batch(mlist, vs, noise=True)
    for mi, v, qb in zip(mlist, vs, batch):
        one = ps.q_estimator(mi, v, noise=True)
        assert np.abs(qb - one).max() <= 1e-13 * np.abs(one).max()
    orig = kl.modes_m
    kl.modes_m = lambda mi, threshold=None, device=False: (None, None) if mi == 99 else orig(mi, threshold, device=device)
    try:
        out = ps.q_estimator_batch([mlist[0], 99], [vs[0], np.zeros(0, dtype=np.complex128)])
    finally:
        kl.modes_m = orig
    assert out[1].shape == (ps.nbands,) and not out[1].any()
    assert np.abs(out[0] - batch[0][: ps.nbands]).max() <= 1e-13 * np.abs(batch[0]).max()


def test_many_columns(setup):
    """R = 256 columns per block (N = 768 over the batch): the wide MFMA path against the restatement."""
    q, bt, kl, ps, mlist = setup
    rng = np.random.default_rng(11)
    vs = []
    for mi in mlist:
        n = kl.modes_m(mi)[0].size
        vs.append(rng.standard_normal((n, 256)) + 1j * rng.standard_normal((n, 256)))
    got = ps.q_estimator_batch(mlist, vs)
    for mi, v, g in zip(mlist, vs, got):
        ev, E, bs, sv = host_products(bt, kl, mi)
        ref = q_estimate(ev, E, bs, sv, ps.clarray, v)
        assert g.shape == (ps.nbands, 256)
        assert np.abs(g - ref).max() <= 1e-12 * np.abs(ref).max(), mi


def test_bit_identical_calls(setup):
    q, bt, kl, ps, mlist = setup
    rng = np.random.default_rng(12)
    vs = [rng.standard_normal((kl.modes_m(mi)[0].size, 64)) + 0j for mi in mlist]
    a = ps.q_estimator_batch(mlist, vs, noise=True)
    b = ps.q_estimator_batch(mlist, vs, noise=True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
