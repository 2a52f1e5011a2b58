"""The batched device route of the m-mode chain (`Timestream.generate_modes_batched`, `mapmake_svd_batched`,
`mapmake_kl_batched`) and `PipelineManager` against the per-m methods, which stay the oracle.

Values are compared stage by stage on the input the batched route itself produced, so bounds do not compound: a batched
result and the single-m operator fed the same input each lie within sqrt(2) gamma_{K+2} (|A| |x|) of the exact product,
hence within 4 (K + 2) eps (|A| |x|) of each other (the bound of tests/test_gpu_blockvec.py)."""
import json
import os
import time

import numpy as np
import pytest
import yaml

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def _conf(outdir):
    """The small polarised cylinder of tests/test_gpu_timestream.py, with a power-spectrum estimator."""
    return dict(config=dict(beamtransfers=True, kltransform=True, psfisher=True, output_directory=str(outdir), truncate=False),
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, inverse=True, use_foregrounds=False)],
                psfisher=[dict(type="Full", name="ps", klname="kl", threshold=0.0, bandtype="polar", num_theta=1,
                               k_bands=[dict(spacing="linear", start=0.0, stop=0.006, num=4)])])


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    from driftscan_amd import device, manager, timestream

    device.reset_context()
    d = tmp_path_factory.mktemp("mb")
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(_conf(d / "prod")))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    timestream.simulate(pm, str(d / "ts"), ndays=10, seed=5)
    return pm, d


def _tree(root):
    out = {}
    for dirpath, _, files in os.walk(root):
        for f in files:
            out[os.path.relpath(os.path.join(dirpath, f), root)] = os.path.join(dirpath, f)
    return out


def _contents(path):
    """{dataset: array} and the attributes of a product file."""
    from driftscan_amd import storage

    with storage.File(path, "r") as f:
        return {k: f[k][:] for k in f.keys()}, {k: f.attrs[k] for k in f.attrs.keys()}


def _bound(A, x):
    """4 (K + 2) eps (|A| |x|) for y = A x."""
    return 4.0 * (A.shape[1] + 2) * EPS * (np.abs(A) @ np.abs(x))


def _threshold_between(pm):
    """A KL threshold that some m pass with a few modes and others do not pass at all: the median over m of the largest
    eigenvalue."""
    kl = pm.kltransforms["kl"]
    tops = []
    for mi in range(pm.telescope.mmax + 1):
        ev = kl.evals_m(mi)
        tops.append(float(ev.max()) if ev is not None and ev.size else 0.0)
    return float(np.sort(np.array(tops))[len(tops) // 2])


def _stream(pm, d, out):
    from driftscan_amd import timestream

    ts = timestream.Timestream(str(d / "ts"), pm)
    ts.output_directory = str(d / out)
    os.makedirs(ts.output_directory, exist_ok=True)
    return ts


def test_batched_files_against_per_m_route(prod):
    pm, d = prod
    bt, tel, kl = pm.beamtransfer, pm.telescope, pm.kltransforms["kl"]
    thr = _threshold_between(pm)

    ref = _stream(pm, d, "out_per_m")
    ref.generate_mmodes()
    ref.generate_mmodes_svd()
    ref.set_kltransform("kl", threshold=thr)
    ref.generate_mmodes_kl()

    one = _stream(pm, d, "out_one_batch")
    one.generate_modes_batched([("kl", thr)], chunk_gb=64.0)
    each = _stream(pm, d, "out_one_m_per_batch")
    each.generate_modes_batched([("kl", thr)], chunk_gb=1e-9)

    fr, f1, fe = _tree(ref.output_directory), _tree(one.output_directory), _tree(each.output_directory)
    assert sorted(fr) == sorted(f1) == sorted(fe)
    assert "mmodes/COMPLETED_M" in f1 and len(f1) >= 1 + 3 * (tel.mmax + 1)
    empty = kept = 0
    for rel in sorted(fr):
        if rel.endswith("COMPLETED_M"):
            continue
        (dr, ar), (d1, a1), (de, ae) = _contents(fr[rel]), _contents(f1[rel]), _contents(fe[rel])
        assert sorted(dr) == sorted(d1) == sorted(de) and sorted(ar) == sorted(a1) == sorted(ae), rel
        for k in ar:
            assert np.array_equal(ar[k], a1[k]) and np.array_equal(ar[k], ae[k]), (rel, k)
        for k in dr:
            assert dr[k].shape == d1[k].shape and dr[k].dtype == d1[k].dtype, (rel, k, dr[k].shape, d1[k].shape)
            assert d1[k].tobytes() == de[k].tobytes() and d1[k].shape == de[k].shape, ("chunking changes " + rel, k)
        if "klmode_" in rel:
            n = d1["mmode_kl"].shape[0]
            empty += n == 0
            kept += n > 0
    assert empty > 0 and kept > 0, (empty, kept)     # the zero-length path and the ordinary one both ran

    # values, stage by stage, each on the input file the batched route wrote
    ntime = ref.ntime
    x = np.stack([ref.timestream_f(fi) for fi in range(tel.nfreq)])              # (F, npairs, ntime)
    fft = np.fft.fft(x, axis=-1) / ntime
    b_fft = 4.0 * (ntime + 2) * EPS * np.abs(x).sum(axis=-1) / ntime             # (F, npairs)
    one.set_kltransform("kl", threshold=thr)
    for mi in range(tel.mmax + 1):
        mm = one.mmode(mi)
        want = np.zeros_like(mm)
        want[:, 0] = fft[..., mi]
        if mi:
            want[:, 1] = fft[..., ntime - mi].conj()
        assert np.all(np.abs(mm - want) <= b_fft[:, None, :]), ("mmode", mi)
        # telescope -> SVD
        sv = one.mmode_svd(mi)
        tm = mm.reshape(tel.nfreq, bt.ntel)
        single = bt.project_vector_telescope_to_svd(mi, tm)
        svnum, svbounds = bt._svd_num(mi)
        but = bt.beam_ut(mi)
        bound = np.concatenate([_bound(but[fi, : svnum[fi]], tm[fi]) for fi in range(tel.nfreq)] + [np.zeros(0)])
        assert sv.shape == single.shape == bound.shape and np.all(np.abs(sv - single) <= bound), ("svd", mi)
        # SVD -> KL
        klm = one.mmode_kl(mi)
        single = kl.project_vector_svd_to_kl(mi, sv, threshold=thr)
        evals, evecs = kl.modes_m(mi, thr)
        assert klm.shape == single.shape == ((0,) if evals is None else (evals.size,)), ("kl", mi)
        if evals is not None:
            assert np.all(np.abs(klm - single) <= _bound(evecs, sv)), ("kl", mi)

    # a second call writes nothing
    before = {rel: os.stat(p).st_mtime_ns for rel, p in f1.items()}
    time.sleep(0.05)
    one.generate_modes_batched([("kl", thr)], chunk_gb=64.0)
    assert {rel: os.stat(p).st_mtime_ns for rel, p in _tree(one.output_directory).items()} == before


def test_batched_map_makers_stage_by_stage(prod):
    from driftscan_amd import device, healpix

    pm, d = prod
    bt, tel, kl = pm.beamtransfer, pm.telescope, pm.kltransforms["kl"]
    ctx = device.get_context()
    nside = 16
    ts = _stream(pm, d, "out_maps")
    ts.set_kltransform("kl")
    thr = ts.klthreshold
    ts.generate_modes_batched(["kl"])
    ms = list(range(tel.mmax + 1))

    def to_array(parts):
        alm = np.zeros((tel.nfreq, tel.num_pol_sky, tel.lmax + 1, tel.lmax + 1), dtype=np.complex128)
        for mi, a in parts:
            alm[..., mi] = a
        return alm

    def sky_bound(mi, sv):
        svnum, svbounds = bt._svd_num(mi)
        inv = bt.invbeam_svd(mi)
        out = np.zeros((tel.nfreq, tel.num_pol_sky, tel.lmax + 1))
        for fi in range(tel.nfreq):
            for pi in range(tel.num_pol_sky):
                out[fi, pi] = _bound(inv[fi, pi, :, : svnum[fi]], sv[svbounds[fi] : svbounds[fi + 1]])
        return out

    # SVD map: a_lm against the per-m operator fed the same SVD vectors, then the file against the synthesis of that array
    parts = ts.alm_svd_batched()
    assert [mi for mi, _ in parts] == ms
    for mi, a in parts:
        sv = ts.mmode_svd(mi)
        assert np.all(np.abs(a - bt.project_vector_svd_to_sky(mi, sv)) <= sky_bound(mi, sv)), ("svd map", mi)
    ts.mapmake_svd_batched(nside, "map_svd.hdf5")
    mp = _contents(ts.output_directory + "/map_svd.hdf5")[0]["map"]
    assert mp.tobytes() == healpix.sphtrans_inv_sky(to_array(parts), nside).tobytes()
    stamp = os.stat(ts.output_directory + "/map_svd.hdf5").st_mtime_ns
    ts.mapmake_svd_batched(nside, "map_svd.hdf5")
    assert os.stat(ts.output_directory + "/map_svd.hdf5").st_mtime_ns == stamp      # an existing map is left alone

    # KL maps
    for wiener in (False, True):
        assert ts.no_m_zero
        parts = ts.alm_kl_batched(wiener=wiener)
        assert [mi for mi, _ in parts] == ms[1:]                                    # m = 0 is left out
        for mi, a in parts:
            klm = ts.mmode_kl(mi)
            if klm.size == 0:
                assert not a.any()
                continue
            if wiener:
                ev = kl.evals_m(mi, thr)
                klm = klm * (ev / (1.0 + ev))
            # stage 1 (KL -> SVD) of this m alone on the device: what stage 2 consumed inside the batch, bit for bit
            isvd, off = kl.project_vectors_kl_to_svd_device([mi], ctx.to_device(klm[:, None]), threshold=thr)
            isvd = isvd.cpu().numpy()[:, 0]
            single = kl.project_vector_kl_to_svd(mi, klm, threshold=thr)
            inv = kl.invmodes_m(mi, thr)
            assert np.all(np.abs(isvd - single) <= _bound(inv, klm)), ("kl -> svd", mi, wiener)
            # stage 2 (SVD -> sky)
            assert np.all(np.abs(a - bt.project_vector_svd_to_sky(mi, isvd)) <= sky_bound(mi, isvd)), ("kl map", mi, wiener)
        name = "map_kl_w%d.hdf5" % wiener
        ts.mapmake_kl_batched(nside, name, wiener=wiener)
        mp = _contents(ts.output_directory + "/" + name)[0]["map"]
        assert mp.tobytes() == healpix.sphtrans_inv_sky(to_array(parts), nside).tobytes()
    ts.no_m_zero = False
    assert [mi for mi, _ in ts.alm_kl_batched()] == ms
    ts.no_m_zero = True

    # a transform without the inverse is refused, as by mapmake_kl
    kl.inverse = False
    try:
        with pytest.raises(Exception, match="inverse"):
            ts.mapmake_kl_batched(nside, "map_refused.hdf5")
    finally:
        kl.inverse = True


class _FixtureTelescope(object):
    def __init__(self, F, B, P, lmax, npower):
        self.nfreq, self.nbase, self.npairs = F, B, B
        self.num_pol_sky = P
        self.lmax = self.mmax = lmax
        self.included_freq = np.arange(F)
        self.included_baseline = np.arange(B)
        self.included_pol = np.arange(P)
        self.frequencies = np.linspace(400.0, 450.0, F)
        self.baselines = np.zeros((B, 2))
        self.tsys_flat = 1.0
        self._npower = npower

    def noisepower(self, bl_indices, f_indices, ndays=None):
        bl, fi = np.broadcast_arrays(bl_indices, f_indices)
        return self._npower[fi, bl]


def test_reference_golden_through_the_batched_route(golden_dir, tmp_path):
    """tests/golden/timestream.npz (outputs of the unmodified reference class) through `generate_modes_batched`,
    `alm_svd_batched` and `alm_kl_batched`, set up as tests/test_gpu_timestream.py::test_against_reference_timestream
    does and with its tolerances."""
    from driftscan_amd import beamtransfer, device, kltransform, storage, timestream

    device.reset_context()
    g = np.load(os.path.join(golden_dir, "timestream.npz"))
    F, B, P, lmax = (int(x) for x in g["dims"])
    tel = _FixtureTelescope(F, B, P, lmax, g["npower"])
    bt = beamtransfer.BeamTransfer(str(tmp_path / "bt"), telescope=tel)
    bt.polsvcut, bt.svcut = float(g["polsvcut"]), float(g["svcut"])
    bt._generate_dirs()
    for mi in range(lmax + 1):
        with storage.File(bt._mfile(mi), "w") as f:
            f.create_dataset("beam_m", data=g["m%d_beam_m" % mi][..., mi:])
    bt._generate_svdfiles(regen=True)
    kl = kltransform.KLTransform.from_config(dict(threshold=0.0, inverse=True, use_foregrounds=False), bt, subdir="kl")
    kl._cvsg, kl._cvfg = g["cv_sg"], np.zeros_like(g["cv_sg"])
    kl.generate(regen=True)

    class PM(object):
        beamtransfer = bt
        kltransforms = {"kl": kl}

    ts = timestream.Timestream(str(tmp_path / "ts"), PM())
    data = g["timestream"]
    for fi in range(F):
        os.makedirs(ts._fdir(fi), exist_ok=True)
        with storage.File(ts._ffile(fi), "w") as f:
            f.create_dataset("timestream", data=data[fi])
            f.attrs["ntime"] = data.shape[-1]
    thr = float(g["kl_threshold"])
    ts.set_kltransform("kl", threshold=thr)
    ts.generate_modes_batched([("kl", thr)])
    ts.no_m_zero = False
    alm_svd = dict(ts.alm_svd_batched())
    alm_kl = dict(ts.alm_kl_batched(wiener=False))
    alm_klw = dict(ts.alm_kl_batched(wiener=True))
    for mi in range(lmax + 1):
        mm = ts.mmode(mi)
        ref = g["m%d_mmode" % mi]
        assert mm.shape == ref.shape and np.abs(mm - ref).max() <= 1e-13 * np.abs(ref).max(), mi
        sv = ts.mmode_svd(mi)
        assert abs(np.linalg.norm(sv) - g["svd_norm"][mi]) <= 1e-9 * max(g["svd_norm"][mi], 1e-300), mi
        assert np.abs(alm_svd[mi] - g["alm_svd"][..., mi]).max() <= 1e-8 * np.abs(g["alm_svd"]).max(), mi
        assert ts.mmode_kl(mi).size == int(g["nkl"][mi]), mi
        if mi >= 1:
            assert np.abs(alm_kl[mi] - g["alm_kl"][..., mi]).max() <= 1e-7 * np.abs(g["alm_kl"]).max(), mi
            assert np.abs(alm_klw[mi] - g["alm_kl_wiener"][..., mi]).max() <= 1e-7 * np.abs(g["alm_kl_wiener"]).max(), mi


def _pipeline_yaml(pm, d, tag, batched):
    return dict(config=dict(product_directory=pm.directory, klmodes=["kl"], powerspectra=[dict(psname="ps", klname="kl")],
                            klmaps=["kl"], nside=16, batched=batched),
                timestreams=[dict(name="a", directory=str(d / "ts"), output_directory=str(d / (tag + "_a"))),
                             dict(name="b", directory=str(d / (tag + "_sim")), output_directory=str(d / (tag + "_b")),
                                  simulate=dict(product_directory=pm.directory, ndays=10, seed=9))],
                crosspower=[dict(psname="ps", klname="kl", timestreams=["a", "b"], psfile=str(d / (tag + "_cross.hdf5")))])


def test_pipeline_manager_end_to_end(prod):
    from driftscan_amd import pipeline, timestream

    pm, d = prod
    tel, bt = pm.telescope, pm.beamtransfer
    trees = {}
    for tag, batched in (("pb", True), ("pp", False)):
        cfile = str(d / (tag + ".yaml"))
        open(cfile, "w").write(yaml.dump(_pipeline_yaml(pm, d, tag, batched)))
        pl = pipeline.PipelineManager.from_configfile(cfile)
        assert pl.batched is batched
        pl.simulate()
        assert os.path.exists(pl.timestreams["b"]._ffile(0))
        pl.run()
        trees[tag] = {n: sorted(_tree(str(d / (tag + "_" + n)))) for n in ("a", "b")}
        assert os.path.exists(str(d / (tag + "_cross.hdf5")))
    assert trees["pb"] == trees["pp"]                                               # both routes leave the same files

    thr = pm.kltransforms["kl"].threshold
    npix = 12 * 16 * 16
    for n in ("a", "b"):
        out = str(d / ("pb_" + n))
        dsets, _ = _contents(out + "/ps_ps.hdf5")
        assert sorted(dsets) == sorted(["fisher", "covariance", "error", "correlation", "bandpower", "powerspectrum"])
        nbands = dsets["powerspectrum"].shape[0]
        assert dsets["fisher"].shape == dsets["covariance"].shape == dsets["correlation"].shape == (nbands, nbands)
        assert dsets["error"].shape == dsets["bandpower"].shape == (nbands,)
        assert all(np.isfinite(v).all() for v in dsets.values())
        klmodes = _contents(out + ("/klmodes_kl_%f.hdf5" % thr))[0]["evals"]
        assert klmodes.shape == (tel.mmax + 1, bt.ndofmax) and np.isfinite(klmodes).all()
        for name in ("map_kl.hdf5", "map_svd.hdf5", "map_full.hdf5"):
            mp = _contents(out + "/" + name)[0]["map"]
            assert mp.shape == (tel.nfreq, tel.num_pol_sky, npix) and mp.dtype == np.float64 and np.isfinite(mp).all(), name
        # the estimator is unchanged code: called by hand on the KL-mode files of the run it gives the same bits
        again = timestream.Timestream(str(d / "ts"), pm)
        again.output_directory = out
        os.rename(out + "/ps_ps.hdf5", out + "/ps_ps_run.hdf5")
        again.set_kltransform("kl")
        again.set_psestimator("ps")
        assert again.powerspectrum().tobytes() == dsets["powerspectrum"].tobytes()
    cross = _contents(str(d / "pb_cross.hdf5"))[0]
    assert cross["powerspectrum"].shape == (2, 2, cross["fisher"].shape[0]) and np.isfinite(cross["powerspectrum"]).all()


# ---- production size ------------------------------------------------------------------------------------------------------
def test_batched_chain_production_size(tmp_path_factory, capsys):
    """BASELINE configs[1] (129 m, 16 frequencies), a simulated noisy timestream: wall time of the per-m route
    (`generate_mmodes` + `generate_mmodes_svd` + `generate_mmodes_kl`, unchanged code) against `generate_modes_batched`,
    each into a fresh output directory, file writing included, second of two runs.  Asserts the direction only: the per-m
    route pays an upload - launch - wait round trip per (m, frequency) and stage, the batched route one per batch.  The
    figures are printed, and written to $DRIFTMI_RECORD_DIR/modes_batched_configs1.json when that variable names a directory
    (profiles/modes_batched_configs1.json is the record of one run)."""
    import torch

    from benchlib.common import CFG2
    from driftscan_amd import device, manager, timestream

    device.reset_context()
    d = tmp_path_factory.mktemp("prodsize")
    conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=False, output_directory=str(d / "prod"), truncate=False),
                telescope=dict(type="UnpolarisedCylinder", **CFG2),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.1, use_foregrounds=False)])
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    bt, tel = pm.beamtransfer, pm.telescope
    bt._dev.clear()
    bt.__dict__.pop("_stack_memo", None)
    timestream.simulate(pm, str(d / "ts"), ndays=10, seed=5)
    ctx = device.get_context()
    chunk_gb = 2.0

    def stream(out):
        ts = timestream.Timestream(str(d / "ts"), pm)
        ts.output_directory = str(d / out)
        os.makedirs(ts.output_directory)
        ts.set_kltransform("kl")
        return ts

    def per_m(ts):
        ts.generate_mmodes()
        ts.generate_mmodes_svd()
        ts.generate_mmodes_kl()

    def batched(ts):
        ts.generate_modes_batched(["kl"], chunk_gb=chunk_gb)

    times = {}
    for run in range(2):
        for name, fn in (("per_m", per_m), ("batched", batched)):
            ts = stream("%s_%d" % (name, run))
            ctx.sync()
            if name == "batched":
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            fn(ts)
            ctx.sync()
            times[name] = time.perf_counter() - t0
            if name == "batched":
                peak = torch.cuda.max_memory_allocated() - base
            assert not bt._dev                                   # nothing stays resident behind a batch
    # where the batched route spends its time: one more run with the opt-in log (it waits for the device at every step)
    ts = stream("batched_split")
    ts.mode_log = {}
    t0 = time.perf_counter()
    batched(ts)
    split = dict(ts.mode_log, total=time.perf_counter() - t0)
    ndof = sum(int(bt.ndof(mi)) for mi in range(tel.mmax + 1))
    vectors = 16 * (tel.mmax + 1) * tel.nfreq * (bt.ntel + 2 * bt.svd_len)      # m-modes, SVD and KL vectors of ALL m
    rec = dict(nm=tel.mmax + 1, nfreq=tel.nfreq, ntel=bt.ntel, svd_len=bt.svd_len, ndof_total=ndof, chunk_gb=chunk_gb,
               per_m_s=times["per_m"], batched_s=times["batched"], ratio=times["per_m"] / times["batched"],
               peak_device_bytes=int(peak), batched_split_s=split)
    with capsys.disabled():
        print("\nmodes chain at configs[1]: " + json.dumps(rec))
    outdir = os.environ.get("DRIFTMI_RECORD_DIR", "")
    if outdir and os.path.isdir(outdir):
        with open(os.path.join(outdir, "modes_batched_configs1.json"), "w") as f:
            json.dump(rec, f, indent=1)
    assert peak <= chunk_gb * (1 << 30) + vectors, (peak, vectors)
    assert times["batched"] < times["per_m"], rec
