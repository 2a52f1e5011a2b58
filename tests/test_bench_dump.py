"""bench.py --dump-outputs: what `dump_outputs` writes for one pass of the hot path, on host tensors standing in for the
device products (CPU only)."""
import os

import numpy as np
import pytest
import torch

import bench


def _pass(rng, ms, F=3, K=4, L=5, T=4):
    """A stand-in BeamTransfer with SVD products in `_dev` and hot_path_step's return value for the m-blocks `ms`."""
    class _BT:
        _dev = {}

    bt, products = _BT(), []
    for mi in ms:
        cplx = lambda *s: torch.from_numpy(rng.standard_normal(s) + 1j * rng.standard_normal(s))
        bt._dev[mi] = dict(beam_svd=cplx(F, K, 1, L), beam_ut=cplx(F, K, T))
        n = 2 + mi
        products.append((mi, rng.random((F, K)), (torch.from_numpy(rng.random(n)), cplx(n, n), None, {"ac": 0.0})))
    return bt, products[::-1]   # any order: the dump sorts by m


def test_dump_outputs_writes_float64_files_with_a_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 50)
    bt, products = _pass(np.random.default_rng(1), [0, 1, 2])
    nbytes = bench.dump_outputs(str(tmp_path / "a"), bt, products)
    bench.dump_outputs(str(tmp_path / "b"), bt, products)
    names = {"m", "singular_values", "kl_ndof", "kl_evals", "beam_svd", "beam_ut", "kl_evecs"}
    assert set(os.listdir(tmp_path / "a")) == {n + ".npy" for n in names}
    got = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in names}
    assert all(a.dtype == np.float64 for a in got.values())
    assert nbytes == sum(a.nbytes for a in got.values()) <= bench.DUMP_BYTES
    for n in names:   # the same pass gives the same files
        assert np.array_equal(got[n], np.load(tmp_path / "b" / (n + ".npy")))
    by_m = sorted(products, key=lambda r: r[0])
    assert got["m"].tolist() == [0, 1, 2] and got["kl_ndof"].tolist() == [2, 3, 4]
    assert np.array_equal(got["singular_values"], np.stack([r[1] for r in by_m]))
    assert np.array_equal(got["kl_evals"], np.concatenate([r[2][0].numpy() for r in by_m]))
    # beam_ut (36 elements per m, 108 in all) is sampled; the KL eigenvectors (4 + 9 + 16 = 29) are written whole
    flat = {"beam_ut": np.concatenate([bt._dev[m]["beam_ut"].numpy().ravel() for m in (0, 1, 2)]),
            "kl_evecs": np.concatenate([r[2][1].numpy().ravel() for r in by_m])}
    pick = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(flat["beam_ut"].size, 50, replace=False))
    assert np.array_equal(got["beam_ut"], np.stack([flat["beam_ut"][pick].real, flat["beam_ut"][pick].imag], axis=-1))
    assert np.array_equal(got["kl_evecs"], np.stack([flat["kl_evecs"].real, flat["kl_evecs"].imag], axis=-1))
    assert got["beam_svd"].shape == (50, 2)


def test_steps_must_be_positive_and_dump_is_for_the_default_workload():
    assert bench.parse_args(["--steps", "3", "--dump-outputs", "d"]).steps == 3
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args(["--workload", "configs2", "--dump-outputs", "d"])


def test_full_legs_are_off_by_default():
    """A plain run measures the headline figure only; the per-stage passes, roofline, CPU baseline and north-star leg run
    behind --full, where --no-cpu-baseline / --no-north-star still leave either out."""
    assert not bench.parse_args([]).full
    args = bench.parse_args(["--full", "--no-north-star"])
    assert args.full and args.no_north_star and not args.no_cpu_baseline
