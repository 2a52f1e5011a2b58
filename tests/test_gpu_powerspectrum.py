"""GPU: Timestream.powerspectrum and cross_powerspectrum (drift/pipeline/timestream.py:463-523, :570-642) on a small
polarised cylinder with a psfisher section: the written file against p = F^-1 (sum_m q_m - bias) from per-m
q_estimator, the cross spectra of three timestreams, and a two-rank run against the one-rank file."""
import os
import shutil

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _conf(outdir):
    return dict(config=dict(beamtransfers=True, kltransform=True, psfisher=True, output_directory=str(outdir),
                            truncate=False),
                psfisher=[dict(type="Full", name="ps", klname="kl", threshold=0.0, bandtype="polar", num_theta=1,
                               k_bands=[dict(spacing="linear", start=0.0, stop=0.006, num=4)])],
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, use_foregrounds=False)])


@pytest.fixture(scope="module")
def prod(tmp_path_factory):
    import yaml

    from driftscan_amd import device, manager

    device.reset_context()
    d = tmp_path_factory.mktemp("ps")
    cfile = str(d / "params.yaml")
    open(cfile, "w").write(yaml.dump(_conf(d / "prod")))
    pm = manager.ProductManager.from_config(cfile)
    pm.generate()
    return pm, d, cfile


def _stream(pm, path, seed):
    from driftscan_amd import timestream

    ts = timestream.Timestream(str(path), pm)
    ts.set_kltransform("kl")
    for mi in range(pm.telescope.mmax + 1):   # the m-mode directories a simulated timestream would have
        os.makedirs(ts._mdir(mi), exist_ok=True)
    np.random.seed(seed)
    ts.fake_kl_data()
    ts.set_psestimator("ps")
    return ts


def _mlist(pm):
    return list(range(1, pm.telescope.mmax + 1))


def test_powerspectrum(prod):
    from driftscan_amd import storage

    pm, d, _ = prod
    ts = _stream(pm, d / "ts0", 1)
    p = ts.powerspectrum()
    ps = pm.psestimators["ps"]
    assert ps.clarray is None   # delbands ran
    with storage.File(ts._psfile, "r") as f:
        for k in ("fisher", "covariance", "error", "correlation", "bandpower", "powerspectrum"):
            assert k in f, k
        filed = f["powerspectrum"][:]
        fisher_f = f["fisher"][:]
    ps.genbands()
    qsum = sum(ps.q_estimator(mi, ts.mmode_kl(mi)) for mi in _mlist(pm))
    fisher, bias = ps.fisher_bias()
    ref = np.linalg.inv(fisher) @ (qsum - bias)
    ps.delbands()
    assert np.abs(fisher).max() > 0 and np.array_equal(fisher_f, fisher)
    assert np.abs(filed - ref).max() <= 1e-10 * np.abs(ref).max()
    assert np.array_equal(p, filed)
    assert ts.powerspectrum() is None   # an existing file is skipped
    with storage.File(ts._psfile, "r") as f:
        assert np.array_equal(f["powerspectrum"][:], filed)


def test_cross_powerspectrum(prod):
    from driftscan_amd import storage, timestream

    pm, d, _ = prod
    streams = [_stream(pm, d / ("x%d" % i), 10 + i) for i in range(3)]
    psfile = str(d / "cross.hdf5")
    p = timestream.cross_powerspectrum(streams, "ps", psfile)
    ps = pm.psestimators["ps"]
    nb = ps.nbands
    assert p.shape == (3, 3, nb)
    ps.genbands()
    fisher, bias = ps.fisher_bias()
    finv = np.linalg.inv(fisher)
    for i in range(3):
        assert not p[i, i].any()
        for j in range(i + 1, 3):
            qp = sum(ps.q_estimator(mi, streams[i].mmode_kl(mi), streams[j].mmode_kl(mi)) for mi in _mlist(pm))
            ref = finv @ (qp - bias)
            assert np.abs(p[i, j] - ref).max() <= 1e-10 * np.abs(ref).max(), (i, j)
            assert np.array_equal(p[i, j], p[j, i])
    ps.delbands()
    with storage.File(psfile, "r") as f:
        assert np.array_equal(f["powerspectrum"][:], p)
    assert timestream.cross_powerspectrum(streams, "ps", psfile) is None


_RANK_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group(backend="gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
from driftscan_amd import manager, timestream
pm = manager.ProductManager.from_config(%(cfile)r)
ts = timestream.Timestream(%(tsdir)r, pm)
ts.set_kltransform("kl")
ts.set_psestimator("ps")
ts.powerspectrum()
dist.barrier()
dist.destroy_process_group()
'''


def test_two_ranks_match_one(prod, tmp_path):
    import socket
    import subprocess
    import sys

    from driftscan_amd import storage

    pm, d, cfile = prod
    one = _stream(pm, d / "r1", 5)
    one.powerspectrum()
    two = tmp_path / "r2"
    shutil.copytree(str(d / "r1" / "mmodes"), str(two / "mmodes"))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % dict(root=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), port=port,
                                          cfile=cfile, tsdir=str(two)))
    env = dict(os.environ, DRIFTMI_DEVICE="0", DRIFTMI_WORKSPACE_GB="2")
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], env=env, stdout=subprocess.PIPE,
                              stderr=subprocess.STDOUT) for r in range(2)]
    outs = [p.communicate(timeout=300)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    with storage.File(one._psfile, "r") as fa, storage.File(str(two / "ps_ps.hdf5"), "r") as fb:
        for k in ("fisher", "covariance", "error", "correlation", "bandpower", "powerspectrum"):
            a, b = fa[k][:], fb[k][:]
            assert a.shape == b.shape and np.abs(a - b).max() <= 1e-12 * max(np.abs(a).max(), 1e-300), k
