"""Noise of the weighted m-modes of flagged timestreams on the host: the numpy restatement of the
inverse-diagonal scan of dm_toeplitz_solve_diag against a dense inverse in long double, the layout of the inflation, a
Monte-Carlo on noise that shows Cov(a) = noisepower * A^-1 with a diagonal m-block, and the files of the per-m pipeline
route on one rank and on two.  No GPU."""
import os

import numpy as np
import pytest

import flag_noise_cases as fn
import flags_cases as fc

EPS = fc.EPS


def _ts():
    from driftscan_amd import timestream

    return timestream


CASES = [("a", n, s) for n, s in ((1, 0), (2, 0), (3, 1), (17, 0), (64, 2), (65, 1), (129, 0), (257, 2))] + \
        [("b", 65, 0), ("c", 65, 0)] + [("d", n, 0) for n in (1, 17, 64)]


# ---- 1. the restatement against long double ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,seed", CASES)
def test_inverse_diag_host_against_long_double(kind, n, seed):
    cs = fn.diag_case(kind, n, seed)
    d, info = _ts().toeplitz_inverse_diag_host(cs["col"])
    assert info == 0 and d.shape == (n,) and d.dtype == np.float64
    # the restatement's own error sets e_ref; it has to be sound itself: within the project's factor of EPS cond
    print("(%s) n = %d: cond %.3g, error %.3g = %.3g EPS cond" % (kind, n, cs["cond"], cs["e_ref"], cs["e_ref"] / (EPS * cs["cond"])))
    assert cs["e_ref"] <= fc.FACTOR * EPS * cs["cond"]
    fn.check(d, cs, what="toeplitz_inverse_diag_host")
    # persymmetry d_i = d_{n-1-i}, which the antisymmetry of g gives without being imposed
    assert np.all(np.abs(d - d[::-1]) <= cs["bound"] * d)
    if kind == "d":
        assert np.all(d == 1.0)


def test_inverse_diag_host_batches_and_failure():
    ts = _ts()
    cols = np.stack([fc.column_of("a", 17, 0), fc.column_of("e", 17), fc.column_of("a", 17, 1), np.zeros(17)])
    d, info = ts.toeplitz_inverse_diag_host(cols)
    assert info.tolist() == [0, 1, 0, 17] and d.shape == (4, 17)
    assert not d[1].any() and not d[3].any()
    for s, seed in ((0, 0), (2, 1)):
        solo, i1 = ts.toeplitz_inverse_diag_host(cols[s])
        assert i1 == 0 and np.array_equal(solo, d[s])
        fn.check(d[s], fn.diag_case("a", 17, seed))
    # the diagonal goes with the solver: column i of the inverse from toeplitz_levinson_host
    x, _ = ts.toeplitz_levinson_host(cols[0], np.eye(17))
    assert np.all(np.abs(x.diagonal().real - d[0]) <= 2 * fn.diag_case("a", 17, 0)["bound"] * d[0])


def test_checker_rejects_a_moved_element():
    for kind, n in (("a", 65), ("b", 65), ("a", 257)):
        cs = fn.diag_case(kind, n, 0)
        good = np.asarray(cs["dref"], dtype=np.float64)
        fn.check(good, cs)
        for i in (0, n // 2, n - 1):
            bad = good.copy()
            bad[i] += 2.0 * cs["bound"] * bad[i]
            with pytest.raises(AssertionError):
                fn.check(bad, cs)
        nan = good.copy()
        nan[1] = np.nan
        with pytest.raises(AssertionError):
            fn.check(nan, cs)


# ---- 2. the layout of the inflation -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mmax,ntime,nf,npairs", [(0, 1, 1, 1), (2, 9, 2, 3), (8, 40, 3, 5)])
def test_inflation_layout(mmax, ntime, nf, npairs):
    ts = _ts()
    N = 2 * mmax + 1
    rng = np.random.default_rng(mmax)
    x = rng.standard_normal((nf, npairs, ntime)) + 1j * rng.standard_normal((nf, npairs, ntime))
    w = np.stack([fc.random_mask(ntime, 0.25 if ntime > 1 else 0.0, 10 * f + p) for f in range(nf) for p in range(npairs)])
    w = w.reshape(nf, npairs, ntime)
    if npairs >= 3:
        w[0, 1] = 1.0                                            # complete data
        w[-1, 0] = 0.0                                           # not solved
        w[-1, 2] = 0.5                                           # constant weight
    modes, info, infl = ts.mmodes_weighted_host(x, w, mmax, inflation=True)
    m2, i2 = ts.mmodes_weighted_host(x, w, mmax)
    assert np.array_equal(modes, m2) and np.array_equal(info, i2)
    assert infl.shape == (mmax + 1, nf, 2, npairs) and infl.dtype == np.float64
    d = np.zeros((nf, npairs, N))
    for f in range(nf):
        for p in range(npairs):
            if info[f, p] == 0:
                d[f, p], li = ts.toeplitz_inverse_diag_host(fc.column(w[f, p], N))
                assert li == 0
    want = fn.inflation_of(d, mmax)
    ev = [np.linalg.eigvalsh(fc.toeplitz(fc.column(w[f, p], N))) for f in range(nf) for p in range(npairs) if info[f, p] == 0]
    tol = 2 * fc.FACTOR * EPS * max(e[-1] / e[0] for e in ev)    # two algorithms, each within FACTOR EPS cond
    assert np.all(np.abs(infl - want) <= tol * np.abs(want))
    assert np.all(infl[0, :, 1] == 1.0)
    if npairs >= 3:
        assert info[-1, 0] == -1 and np.all(infl[:, -1, 0, 0] == 0.0) and np.all(infl[1:, -1, 1, 0] == 0.0)
        assert np.all(infl[:, 0, 0, 1] == 1.0) and np.all(infl[:, 0, 1, 1] == 1.0)
        assert np.all(infl[:, -1, 0, 2] == 2.0) and np.all(infl[1:, -1, 1, 2] == 2.0)
    # weights without a pair axis: one system, its diagonal for every baseline
    _, _, one = ts.mmodes_weighted_host(x, w[:, 0], mmax, inflation=True)
    _, _, full = ts.mmodes_weighted_host(x, np.repeat(w[:, :1], npairs, axis=1), mmax, inflation=True)
    assert np.array_equal(one, full)
    assert np.all(ts.mmodes_weighted_host(x, np.ones(ntime), mmax, inflation=True)[2] == 1.0)


# ---- 3. Monte-Carlo on noise ----------------------------------------------------------------------------------------------------
def test_noise_variance_of_the_modes_is_the_inverse_diagonal():
    from driftscan_amd import skysim

    ts = _ts()
    mmax, ntime, R = 8, 40, 20000
    N = 2 * mmax + 1
    w = skysim.FlagModel(fraction=0.4, burst=3, seed=4).mask(ntime, [0])[0]
    assert N <= np.count_nonzero(w) < ntime
    rng = np.random.default_rng(2024)
    # circular white noise of per-sample variance ntime * noisepower, noisepower = 1: what the simulators draw
    x = np.sqrt(ntime / 2.0) * (rng.standard_normal((1, R, ntime)) + 1j * rng.standard_normal((1, R, ntime)))
    x = x * w
    _, info, infl = ts.mmodes_weighted_host(x[:, :1], w, mmax, inflation=True)
    assert not info.any()
    d = infl[:, 0, :, 0]                                                       # (mmax + 1, 2)
    real = np.ones((mmax + 1, 2), dtype=bool)
    real[0, 1] = False                                                         # (m = 0, slot 1) holds no mode
    # why neither shortcut would do: the inflation is large, and it is not the same for every m
    assert np.max(np.abs(d[real] - 1.0)) > 0.5
    assert np.max(np.abs(d[real] * w.mean() - 1.0)) > 0.05
    modes, _ = ts.mmodes_weighted_host(x, w, mmax)                             # (mmax + 1, 1, 2, R)
    var = (np.abs(modes[:, 0]) ** 2).mean(axis=-1)                             # (mmax + 1, 2)
    dev = np.abs(var[real] / d[real] - 1.0)
    print("variance / d - 1: worst %.3g of %.3g allowed" % (dev.max(), 5 / np.sqrt(R)))
    assert np.all(dev <= 5.0 / np.sqrt(R))
    assert not modes[0, 0, 1].any()
    # slots 0 and 1 of an m, a_{+m} and conj(a_{-m}), are uncorrelated: the m-block of the noise stays diagonal
    cross = np.abs((modes[1:, 0, 0] * modes[1:, 0, 1].conj()).mean(axis=-1))
    allowed = 5.0 * np.sqrt(d[1:, 0] * d[1:, 1] / R)
    print("pseudo-covariance: worst %.3g of the allowed" % (cross / allowed).max())
    assert np.all(cross <= allowed)
    # while a_{+m} and a_{-m} themselves are correlated in general (the Hermitian covariance A^-1 is not diagonal)
    k = np.arange(-mmax, mmax + 1)
    F = np.exp(2j * np.pi * ((np.arange(ntime)[:, None] * k[None, :]) % ntime) / ntime)
    Ainv = np.linalg.inv((F.conj().T * w[None, :]) @ F / ntime)
    m1 = int(np.argmax(np.abs(Ainv[mmax + np.arange(1, mmax + 1), mmax - np.arange(1, mmax + 1)]))) + 1
    herm = (modes[m1, 0, 0] * modes[m1, 0, 1]).mean()                          # E[a_{+m} conj(a_{-m})]
    assert abs(herm - Ainv[mmax + m1, mmax - m1]) <= 5.0 * np.sqrt(d[m1, 0] * d[m1, 1] / R)
    # with a ridge the diagonal of A_rho^-1 bounds the variance from above
    rho = 1e-2
    mr, _, ir = ts.mmodes_weighted_host(x[:, :1], w, mmax, ridge=rho, inflation=True)
    dr = ir[:, 0, :, 0]
    modes_r, _ = ts.mmodes_weighted_host(x, w, mmax, ridge=rho)
    var_r = (np.abs(modes_r[:, 0]) ** 2).mean(axis=-1)
    assert np.all(var_r[real] <= dr[real] * (1.0 + 5.0 / np.sqrt(R)))
    assert np.all(dr[real] < d[real])


# ---- 4. the files of the per-m route ----------------------------------------------------------------------------------------------
def _product_dir(tmp_path):
    import yaml

    prod = tmp_path / "prod"
    prod.mkdir()
    conf = dict(config=dict(beamtransfers=False, kltransform=False, psfisher=False, output_directory=str(prod)),
                telescope=dict(type="UnpolarisedCylinder", num_freq=2, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4, tsys=1.0))
    (prod / "config.yaml").write_text(yaml.dump(conf))
    return prod


def _write_timestream(ts, x, w=None):
    from driftscan_amd import storage

    for fi in range(x.shape[0]):
        os.makedirs(ts._fdir(fi), exist_ok=True)
        with storage.File(ts._ffile(fi), "w") as f:
            f.create_dataset("timestream", data=np.ascontiguousarray(x[fi]))
            if w is not None:
                f.create_dataset("weight", data=np.ascontiguousarray(w[fi]))
            f.attrs["ntime"] = x.shape[-1]


def test_host_route_writes_the_inflation_files(tmp_path):
    from driftscan_amd import manager, storage, timestream

    pm = manager.ProductManager.from_config(str(_product_dir(tmp_path)))
    tel = pm.telescope
    mmax, nfreq, npairs = int(tel.mmax), int(tel.nfreq), int(tel.npairs)
    N = 2 * mmax + 1
    ntime = int(np.ceil(2.5 * N))
    rng = np.random.default_rng(9)
    x, _ = fc.band_limited(rng, nfreq, npairs, mmax, ntime)
    w = np.stack([fc.random_mask(ntime, 0.25, 3 * f + p) for f in range(nfreq) for p in range(npairs)]).reshape(x.shape)
    w[0, 0] = 0.0                                                # a dead baseline
    w[1, 1] = 1.0                                                # and a complete one
    flagged = timestream.Timestream(str(tmp_path / "ts_w"), pm)
    _write_timestream(flagged, x * w, w)
    flagged.generate_mmodes()
    modes, info, infl = timestream.mmodes_weighted_host(x * w, w, mmax, inflation=True)
    for mi in range(mmax + 1):
        assert np.array_equal(flagged.mmode(mi), modes[mi])      # the modes keep their bits
        got = flagged.noise_inflation(mi)
        assert got.shape == (nfreq, 2, npairs) and got.dtype == np.float64
        assert np.array_equal(got, infl[mi])
        with storage.File(flagged._mdir(mi) + "/inflation.hdf5", "r") as f:
            assert np.array_equal(f["noise_inflation"][:], infl[mi]) and int(f.attrs["m"]) == mi
    assert np.all(infl[:, 1, 0, 1] == 1.0) and not infl[:, 0, 0, 0].any()
    per_mode = np.concatenate([infl[:, :, 0], infl[1:, :, 1]], axis=0)
    with storage.File(flagged.output_directory + "/mmodes/weights.hdf5", "r") as f:
        assert np.array_equal(f["info"][:], info)
        assert np.array_equal(f["inflation_mean"][:], per_mode.mean(axis=0))
        assert np.array_equal(f["inflation_max"][:], per_mode.max(axis=0))
        assert f["inflation_max"][:][1, 1] == 1.0 and f["inflation_max"][:][0, 0] == 0.0
        assert f["inflation_max"][:][1, 0] > 1.0
    # files without `weight`: no inflation file, and ones from the reader
    plain = timestream.Timestream(str(tmp_path / "ts_c"), pm)
    _write_timestream(plain, x)
    plain.generate_mmodes()
    for mi in range(mmax + 1):
        assert not os.path.exists(plain._mdir(mi) + "/inflation.hdf5")
        assert sorted(os.listdir(plain._mdir(mi))) == ["mode.hdf5"]
        ones = plain.noise_inflation(mi)
        assert ones.shape == (nfreq, 2, npairs) and np.all(ones == 1.0)
    assert not os.path.exists(plain.output_directory + "/mmodes/weights.hdf5")


def test_pipeline_reads_the_bias_switch(tmp_path):
    import yaml

    from driftscan_amd import timestream
    from driftscan_amd.pipeline import PipelineManager

    prod = _product_dir(tmp_path)
    conf = dict(config=dict(product_directory=str(prod)),
                timestreams=[dict(name="a", directory=str(tmp_path / "ts_a"), flag_noise_bias_correct=True),
                             dict(name="b", directory=str(tmp_path / "ts_b"))])
    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf))
    p = PipelineManager.from_configfile(str(cfile))
    assert timestream.Timestream.flag_noise_bias_correct is False
    assert p.timestreams["a"].flag_noise_bias_correct is True and p.timestreams["b"].flag_noise_bias_correct is False


_RANK_SCRIPT = r'''
import sys
sys.path.insert(0, %(root)r)
import torch.distributed as dist
dist.init_process_group(backend="gloo", init_method="tcp://127.0.0.1:%(port)d", rank=int(sys.argv[1]), world_size=2)
from driftscan_amd import manager, timestream
pm = manager.ProductManager.from_config(%(prod)r)
ts = timestream.Timestream(%(tsdir)r, pm)
ts.output_directory = %(outdir)r
ts.generate_mmodes()
dist.barrier()
dist.destroy_process_group()
'''


def test_two_ranks_regroup_the_inflation_as_the_modes(tmp_path):
    """Two ranks (gloo, CPU) split the frequencies and the m; the files are those of one rank."""
    import socket
    import subprocess
    import sys

    from driftscan_amd import manager, storage, timestream

    prod = _product_dir(tmp_path)
    pm = manager.ProductManager.from_config(str(prod))
    tel = pm.telescope
    mmax, nfreq, npairs = int(tel.mmax), int(tel.nfreq), int(tel.npairs)
    ntime = int(np.ceil(2.5 * (2 * mmax + 1)))
    rng = np.random.default_rng(10)
    x, _ = fc.band_limited(rng, nfreq, npairs, mmax, ntime)
    w = np.stack([fc.random_mask(ntime, 0.25, 7 * f + p) for f in range(nfreq) for p in range(npairs)]).reshape(x.shape)
    one = timestream.Timestream(str(tmp_path / "ts_w"), pm)
    _write_timestream(one, x * w, w)
    one.output_directory = str(tmp_path / "out1")
    one.generate_mmodes()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    script = tmp_path / "rank.py"
    script.write_text(_RANK_SCRIPT % dict(root=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), port=port,
                                          prod=str(prod), tsdir=str(tmp_path / "ts_w"), outdir=str(tmp_path / "out2")))
    procs = [subprocess.Popen([sys.executable, str(script), str(r)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
             for r in range(2)]
    outs = [p.communicate(timeout=180)[0].decode() for p in procs]
    assert all(p.returncode == 0 for p in procs), "\n".join(outs)
    two = timestream.Timestream(str(tmp_path / "ts_w"), pm)
    two.output_directory = str(tmp_path / "out2")
    for mi in range(mmax + 1):
        assert np.array_equal(two.mmode(mi), one.mmode(mi))
        assert np.array_equal(two.noise_inflation(mi), one.noise_inflation(mi)) and one.noise_inflation(mi).max() > 1.0
    with storage.File(str(tmp_path / "out1/mmodes/weights.hdf5"), "r") as fa, \
            storage.File(str(tmp_path / "out2/mmodes/weights.hdf5"), "r") as fb:
        for k in ("nkept", "info", "inflation_mean", "inflation_max"):
            assert np.array_equal(fa[k][:], fb[k][:]), k
