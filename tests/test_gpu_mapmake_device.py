"""The map-makers of Timestream (mapmake_kl with the Wiener filter, mapmake_svd) write the synthesis of their per-m
a_lm: checked against the host loop healpix.sphtrans_inv_sky_host on a small polarised cylinder."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ts(tmp_path_factory):
    import yaml

    from driftscan_amd import device, healpix, manager, storage, timestream

    device.reset_context()
    d = tmp_path_factory.mktemp("mapmake")
    conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="PolarisedCylinder", num_freq=2, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, inverse=True, use_foregrounds=False)])
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    tel = pm.telescope
    rng = np.random.default_rng(21)
    lmax = tel.lmax
    alm = np.zeros((tel.nfreq, 4, lmax + 1, lmax + 1), dtype=np.complex128)
    for m in range(lmax + 1):
        alm[:, :, m:, m] = rng.standard_normal((tel.nfreq, 4, lmax + 1 - m)) + (
            1j * rng.standard_normal((tel.nfreq, 4, lmax + 1 - m)) if m else 0)
    alm[:, 1:3, :2] = 0.0
    skyfile = str(d / "sky.hdf5")
    with storage.File(skyfile, "w") as f:
        f.create_dataset("map", data=healpix.sphtrans_inv_sky_host(alm, 32))
    t = timestream.simulate(pm, str(d / "ts"), maps=[skyfile], ndays=0)
    t.generate_mmodes()
    t.generate_mmodes_svd()
    t.set_kltransform("kl")
    t.generate_mmodes_kl()
    return pm, t


def _read_map(t, name):
    from driftscan_amd import storage

    with storage.File(t.output_directory + "/" + name, "r") as f:
        return f["map"][:]


def _alm_of(pm, make_alm, mlist):
    tel = pm.telescope
    alm = np.zeros((tel.nfreq, tel.num_pol_sky, tel.lmax + 1, tel.lmax + 1), dtype=np.complex128)
    for mi in mlist:
        alm[..., mi] = make_alm(mi)
    return alm


def test_mapmake_kl_wiener(ts):
    from driftscan_amd import healpix

    pm, t = ts
    nside = 16
    t.mapmake_kl(nside, "map_kl_wiener.hdf5", wiener=True)
    kl, bt = pm.kltransforms["kl"], pm.beamtransfer

    def make_alm(mi):
        klmode = t.mmode_kl(mi)
        if klmode.size == 0:
            return 0.0
        evals = kl.evals_m(mi, t.klthreshold)
        if evals is not None:
            klmode = klmode * (evals / (1.0 + evals))
        return bt.project_vector_svd_to_sky(mi, kl.project_vector_kl_to_svd(mi, klmode, threshold=t.klthreshold))

    alm = _alm_of(pm, make_alm, range(1 if t.no_m_zero else 0, pm.telescope.mmax + 1))
    mp = _read_map(t, "map_kl_wiener.hdf5")
    want = healpix.sphtrans_inv_sky_host(alm, nside)
    assert np.abs(alm).max() > 0
    assert np.abs(mp - want).max() <= 1e-10 * np.abs(alm).max()


def test_mapmake_svd(ts):
    from driftscan_amd import healpix

    pm, t = ts
    nside = 16
    t.mapmake_svd(nside, "map_svd_dev.hdf5")
    bt = pm.beamtransfer
    alm = _alm_of(pm, lambda mi: bt.project_vector_svd_to_sky(mi, t.mmode_svd(mi)), range(pm.telescope.mmax + 1))
    mp = _read_map(t, "map_svd_dev.hdf5")
    want = healpix.sphtrans_inv_sky_host(alm, nside)
    assert np.abs(alm).max() > 0
    assert np.abs(mp - want).max() <= 1e-10 * np.abs(alm).max()
