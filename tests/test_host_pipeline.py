"""CPU-only: `PipelineManager` configuration handling, and the problem tables of the batched vector projections.

The tables (where every (m, frequency[, polarisation]) block of a batch lies in the stacked products and in the packed
vectors) are plain numpy, so they are executed here by a small numpy interpreter standing in for `dm_blockvec_grouped`
and compared with the per-(m, frequency) loops of `project_vector_telescope_to_svd`, `project_vector_svd_to_sky`,
`project_vector_svd_to_kl` and `project_vector_kl_to_svd`, restated below."""
import numpy as np
import pytest
import yaml
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


def _close(a, b):
    """Same shape and equal up to the rounding of two orders of summation (values are O(1), sums of < 20 terms)."""
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= 1e-13 * (1.0 + np.abs(b))))


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@pytest.mark.parametrize("R", [1, 3])
def test_svd_tables_match_per_block_loops(R):
    from driftscan_amd import beamtransfer as btmod

    rng = np.random.default_rng(11)
    nb, F, svd_len, ntel, P, L = 4, 5, 7, 6, 3, 9
    svnum = rng.integers(0, svd_len + 1, size=(nb, F))
    svnum[1] = 0            # an m without any mode
    svnum[0, 2] = 0         # frequencies without modes inside an m that has some
    svnum[3, 0] = 0
    beam_ut = _crandn(rng, nb, F, svd_len, ntel)
    invbeam = _crandn(rng, nb, F, P, L, svd_len)
    vec = _crandn(rng, nb, F, ntel, R)

    tab, off = btmod.svd_forward_table(svnum, svd_len, ntel, R)
    assert len(tab) == int((svnum > 0).sum()) and off[-1] == svnum.sum() and off[2] == off[1]
    sentinel = 7.0 + 7.0j
    out = np.full((int(off[-1]) * R,), sentinel)
    run_table(beam_ut.reshape(-1), vec.reshape(-1), out, tab, R)
    out = out.reshape(-1, R)
    packed = []
    for i in range(nb):     # BeamTransfer.project_vector_telescope_to_svd, restated
        bounds = np.concatenate([[0], np.cumsum(svnum[i])])
        vecf = np.zeros((bounds[-1], R), dtype=np.complex128)
        for fi in range(F):
            if svnum[i, fi] > 0:
                vecf[bounds[fi] : bounds[fi + 1]] = beam_ut[i, fi, : svnum[i, fi], :] @ vec[i, fi]
        assert _close(out[off[i] : off[i + 1]], vecf), i
        packed.append(vecf)
    assert not (out == sentinel).any()     # the packed layout has no gaps

    # back to the sky: packed vectors with one spare row between the m (offsets need not be back to back)
    offs = np.array([int(off[i]) + i for i in range(nb + 1)])
    svec = np.zeros((int(offs[-1]), R), dtype=np.complex128)
    for i in range(nb):
        svec[offs[i] : offs[i] + packed[i].shape[0]] = packed[i]
    tab2 = btmod.svd_to_sky_table(svnum, offs, svd_len, P, L, R)
    assert len(tab2) == P * int((svnum > 0).sum())
    alm = np.zeros((nb * F * P * L * R,), dtype=np.complex128)
    run_table(invbeam.reshape(-1), svec.reshape(-1), alm, tab2, R)
    alm = alm.reshape(nb, F, P, L, R)
    for i in range(nb):     # BeamTransfer.project_vector_svd_to_sky, restated
        bounds = np.concatenate([[0], np.cumsum(svnum[i])])
        vecf = np.zeros((F, P, L, R), dtype=np.complex128)
        for pi in range(P):
            for fi in range(F):
                if svnum[i, fi] > 0:
                    vecf[fi, pi] += invbeam[i, fi, pi, :, : svnum[i, fi]] @ packed[i][bounds[fi] : bounds[fi + 1]]
        assert _close(alm[i], vecf), i
    assert not alm[1].any()


@pytest.mark.parametrize("R", [1, 2])
def test_kl_tables_match_per_m_products(R):
    from driftscan_amd import kltransform as klmod

    rng = np.random.default_rng(12)
    ndofs = np.array([6, 0, 9, 4, 5])
    nmodes = np.array([3, 0, 0, 4, 1])     # an m without degrees of freedom, one whose modes all fall below the threshold
    evecs = [_crandn(rng, n, d) for n, d in zip(nmodes, ndofs)]
    evinv = [_crandn(rng, n, d) for n, d in zip(nmodes, ndofs)]          # rows of `evinv` as the files hold them
    off = np.concatenate([[0], np.cumsum(ndofs + 1)])[:-1]               # a spare row behind every m
    svec = _crandn(rng, int((ndofs + 1).sum()), R)
    tab, kloff = klmod.kl_forward_table(nmodes, ndofs, off, R)
    assert len(tab) == 3 and list(kloff) == [0, 3, 3, 3, 7, 8]
    E = np.concatenate([e.reshape(-1) for e in evecs])
    out = np.full((int(kloff[-1]) * R,), 5.0 + 0j)
    run_table(E, svec.reshape(-1), out, tab, R)
    out = out.reshape(-1, R)
    for i in range(len(ndofs)):            # KLTransform.project_vector_svd_to_kl: evecs @ vec
        assert _close(out[kloff[i] : kloff[i + 1]], evecs[i] @ svec[off[i] : off[i] + ndofs[i]]), i

    soff = np.concatenate([[0], np.cumsum(ndofs)])
    tab2 = klmod.kl_backward_table(nmodes, ndofs, kloff, soff, R)
    assert len(tab2) == 3 and np.all(tab2["rsA"] == 1) and list(tab2["csA"]) == [6, 4, 5]
    back = np.zeros((int(soff[-1]) * R,), dtype=np.complex128)
    run_table(np.concatenate([e.reshape(-1) for e in evinv]), out.reshape(-1), back, tab2, R)
    back = back.reshape(-1, R)
    for i in range(len(ndofs)):            # KLTransform.project_vector_kl_to_svd: invmodes_m = evinv.T
        want = evinv[i].T @ out[kloff[i] : kloff[i + 1]] if nmodes[i] else np.zeros((ndofs[i], R))
        assert _close(back[soff[i] : soff[i + 1]], want), i


def test_blockvec_table_broadcasts_and_defaults():
    from driftscan_amd import _lib

    tab = _lib.blockvec_table(a0=np.arange(3) * 10, x0=0, y0=np.arange(3), M=[1, 2, 3], K=4, rsA=4, csA=1, rsB=1, csB=1, ldc=1)
    assert tab.shape == (3,) and tab.dtype.names == _lib.BLOCKVEC_FIELDS
    assert list(tab["a0"]) == [0, 10, 20] and list(tab["K"]) == [4, 4, 4] and not tab["conjA"].any() and not tab["conjB"].any()
    assert _lib.blockvec_table(a0=[], x0=[], y0=[], M=[], K=[], rsA=1, csA=1, rsB=1, csB=1, ldc=1).shape == (0,)


def test_blockvec_route_follows_the_measured_rule():
    from driftscan_amd import _lib

    short = _lib.blockvec_table(a0=0, x0=0, y0=0, M=[200, 100], K=[216, 92], rsA=1, csA=1, rsB=1, csB=1, ldc=1)
    long_ = _lib.blockvec_table(a0=0, x0=0, y0=0, M=[1472, 10], K=[1472, 92], rsA=1, csA=1, rsB=1, csB=1, ldc=1)
    for R in (1, 2, 4, 6):
        assert _lib.blockvec_route(short, R) == _lib.blockvec_route(long_, R) == "blockvec"
    for R in (7, 8):
        assert _lib.blockvec_route(short, R) == "zgemm" and _lib.blockvec_route(long_, R) == "blockvec"
    assert _lib.blockvec_route(long_, 9) == "zgemm"


# ---- PipelineManager ---------------------------------------------------------------------------------------------------
def test_pipeline_defaults():
    from driftscan_amd.pipeline import PipelineManager

    p = PipelineManager()
    assert p.product_directory == ""
    assert p.generate_modes is True and p.generate_klmodes is True
    assert p.generate_powerspectra is True and p.generate_maps is True
    assert p.no_m_zero is True
    assert p.klmodes == [] and p.powerspectra == [] and p.klmaps == [] and p.crosspower == []
    assert p.nside == 128 and p.wiener is False and p.collect_klmodes is True
    assert p.batched is True
    assert p.timestreams == {} and p.simulations == {}
    assert PipelineManager.run is PipelineManager.generate


def test_pipeline_missing_sections(tmp_path):
    from driftscan_amd.pipeline import PipelineManager

    f1 = tmp_path / "noconfig.yaml"
    f1.write_text(yaml.dump(dict(timestreams=[])))
    with pytest.raises(Exception, match="'config' section"):
        PipelineManager.from_configfile(str(f1))
    f2 = tmp_path / "nots.yaml"
    f2.write_text(yaml.dump(dict(config=dict(product_directory=str(tmp_path)))))
    with pytest.raises(Exception, match="'timestream' section"):
        PipelineManager().load_configfile(str(f2))


def _product_dir(tmp_path):
    prod = tmp_path / "prod"
    prod.mkdir()
    conf = dict(config=dict(beamtransfers=False, kltransform=False, psfisher=False, output_directory=str(prod)),
                telescope=dict(type="UnpolarisedCylinder", num_freq=2, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=1.5)])
    (prod / "config.yaml").write_text(yaml.dump(conf))
    return prod


def test_pipeline_paths_and_instances(tmp_path, monkeypatch):
    from driftscan_amd.pipeline import PipelineManager, fixpath

    prod = _product_dir(tmp_path)
    home = tmp_path / "home"
    home.mkdir()
    monkeypatch.setenv("HOME", str(home))
    monkeypatch.setenv("DRIFT_TS_ROOT", str(tmp_path / "data"))
    assert fixpath("~/a/../b") == str(home / "b") and fixpath("$DRIFT_TS_ROOT/x//y") == str(tmp_path / "data" / "x" / "y")
    monkeypatch.setenv("DRIFT_PROD", str(prod))
    conf = dict(config=dict(product_directory="$DRIFT_PROD", klmodes=["kl"], nside=16, wiener=True, batched=False,
                            generate_maps=False, no_m_zero=False),
                timestreams=[dict(name="a", directory="$DRIFT_TS_ROOT/ts_a", output_directory="~/out_a"),
                             dict(name="b", directory="~/ts_b", simulate=dict(product_directory="$DRIFT_PROD", ndays=3, seed=1))],
                crosspower=[dict(psname="ps", klname="kl", timestreams=["a", "b"], psfile="~/xp.hdf5")])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = PipelineManager.from_configfile(str(cfile))
    assert p.product_directory == str(prod)
    assert p.klmodes == ["kl"] and p.nside == 16 and p.wiener is True and p.batched is False and p.generate_maps is False
    assert sorted(p.timestreams) == ["a", "b"] and list(p.simulations) == ["b"] and p.simulations["b"]["ndays"] == 3
    a, b = p.timestreams["a"], p.timestreams["b"]
    assert a.directory == str(tmp_path / "data" / "ts_a") and a.output_directory == str(home / "out_a")
    assert b.directory == str(home / "ts_b") and b.output_directory == b.directory
    assert a.no_m_zero is False and b.no_m_zero is False
    assert a.manager.kltransforms["kl"].threshold == 1.5 and a.telescope.nfreq == 2
    assert p.crosspower[0]["psfile"] == "~/xp.hdf5"
    # a second instance starts empty and leaves the first alone (the reference shares one class-level dictionary)
    q = PipelineManager()
    assert q.timestreams == {} and q.simulations == {} and q.crosspower == []
    q.timestreams["z"] = None
    assert "z" not in p.timestreams and "z" not in PipelineManager().timestreams


def test_pipeline_command_line_needs_a_file():
    from driftscan_amd import pipeline

    with pytest.raises(SystemExit):
        pipeline.main([])
