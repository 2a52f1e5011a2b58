"""The I/O stages the Timestream routes share: the chunk reader and its rule for weights, the
row chunks and their refusal, the rewriter and `weight_input`, the product and root writers.  Directories of nf = 3,
nrow = 4, nt = 5 written with `storage.File`; no device."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from driftscan_amd import storage, timestream

NF, NROW, NT = 3, 4, 5
FREQS = [400.0, 405.0, 410.0]


def _manager(npairs=NROW):
    tel = SimpleNamespace(nfreq=NF, npairs=npairs, frequencies=np.array(FREQS))
    return SimpleNamespace(beamtransfer=SimpleNamespace(telescope=tel))


def _directory(path, weighted=(), shapes=None, unstacked=False):
    """A directory whose file fi holds `timestream`, `weight` (float32: the reader converts) for fi in `weighted`, a foreign
    dataset and attributes; returns (the Timestream, the arrays written per file)."""
    ts = timestream.Timestream(str(path), _manager())
    rng = np.random.default_rng(5)
    wrote = []
    for fi in range(NF):
        shape = (NROW, NT) if shapes is None else shapes[fi]
        d = dict(timestream=rng.standard_normal(shape) + 1j * rng.standard_normal(shape), foreign=np.arange(3, dtype=np.int32) + fi)
        if fi in weighted:
            d["weight"] = rng.integers(0, 3, shape).astype(np.float32)
        os.makedirs(ts._fdir(fi), exist_ok=True)
        with storage.File(ts._ffile(fi), "w") as f:
            for k, v in d.items():
                f.create_dataset(k, data=v)
            f.attrs["ntime"] = NT
            f.attrs["note"] = "file %d" % fi
            if unstacked:
                f.attrs["unstacked"] = 1
        wrote.append(d)
    return ts, wrote


def _contents(path):
    with storage.File(path, "r") as f:
        return {k: np.asarray(f[k][:]) for k in f.keys()}, dict(f.attrs)


def test_open_reports_the_shape_and_refuses(tmp_path):
    ts, _ = _directory(tmp_path / "a")
    src, nrow, nt = timestream._route_open("route", _manager(), ts.directory)
    assert (src.directory, nrow, nt) == (ts.directory, NROW, NT)
    with pytest.raises(ValueError, match="route: .* holds 4 rows, the telescope has 6 baselines"):
        timestream._route_open("route", _manager(npairs=6), ts.directory)
    assert timestream._route_open("route", _manager(npairs=6), ts.directory, rows=False)[1:] == (NROW, NT)
    un, _ = _directory(tmp_path / "b", unstacked=True)
    with pytest.raises(ValueError, match="unstacked"):
        timestream._route_open("route", _manager(), un.directory)
    assert timestream._route_open("route", _manager(), un.directory, stacked_only=False)[1:] == (NROW, NT)


def test_reader_weights_rule(tmp_path):
    """No file weighted: w is None.  One of three: ones for the other two, float64; the rule holds per chunk."""
    ts, wrote = _directory(tmp_path / "a")
    c = timestream._route_read("route", ts, range(NF), NROW, NT)
    assert c.w is None and c.files is None and c.fs == [0, 1, 2]
    assert all(a.dtype == np.complex128 and a.shape == (NROW, NT) for a in c.x)
    assert all(np.array_equal(a, d["timestream"].astype(np.complex128)) for a, d in zip(c.x, wrote))
    ts, wrote = _directory(tmp_path / "b", weighted=(1,))
    c = timestream._route_read("route", ts, range(NF), NROW, NT)
    assert all(a.dtype == np.float64 and a.shape == (NROW, NT) for a in c.w)
    assert np.all(c.w[0] == 1) and np.all(c.w[2] == 1) and np.array_equal(c.w[1], wrote[1]["weight"].astype(np.float64))
    assert timestream._route_read("route", ts, [0], NROW, NT).w is None
    assert timestream._route_read("route", ts, [2, 1], NROW, NT).fs == [2, 1]


def test_reader_opens_each_file_once_and_keeps_it_whole(tmp_path, monkeypatch):
    ts, wrote = _directory(tmp_path / "a", weighted=(0, 2))
    opened, real = [], storage.File

    def counting(path, mode="r", **kw):
        opened.append(path)
        return real(path, mode, **kw)

    monkeypatch.setattr(storage, "File", counting)
    for whole in (False, True):
        del opened[:]
        c = timestream._route_read("route", ts, range(NF), NROW, NT, whole=whole)
        assert opened == [ts._ffile(fi) for fi in range(NF)]
    for fi, (data, attrs) in enumerate(c.files):
        assert set(data) == set(wrote[fi])
        assert all(data[k].dtype == wrote[fi][k].dtype and np.array_equal(data[k], wrote[fi][k]) for k in data)
        assert attrs["note"] == "file %d" % fi and int(attrs["ntime"]) == NT


def test_reader_names_the_file_of_another_shape(tmp_path):
    ts, _ = _directory(tmp_path / "a", shapes=[(NROW, NT), (NROW, NT + 1), (NROW, NT)])
    for whole in (False, True):
        with pytest.raises(ValueError, match="route: ") as e:
            timestream._route_read("route", ts, range(NF), NROW, NT, whole=whole)
        assert ts._ffile(1) in str(e.value) and ts._ffile(0) not in str(e.value) and "(4, 5)" in str(e.value)


def test_row_chunks():
    per_row = 48.0 * NF * NT
    for nrow, rows_fit in ((NROW, 1), (NROW, 3), (NROW, 4), (NROW, 9), (7, 2), (0, 1)):
        budget = rows_fit * per_row / 2.0**30
        ranges = timestream._row_chunks("route", nrow, budget, per_row)
        assert [r0 for r0, _ in ranges] == [0] * bool(nrow) + [r1 for _, r1 in ranges[:-1]]   # no gap, no overlap
        assert (ranges[-1][1] if ranges else 0) == nrow
        assert all(0 < (r1 - r0) * per_row <= budget * 2.0**30 for r0, r1 in ranges)
    with pytest.raises(ValueError, match=r"route: one row over all frequencies needs chunk_gb >= ") as e:
        timestream._row_chunks("route", NROW, 1e-9, per_row)
    need = float(re.search(r"chunk_gb >= ([0-9.e+-]+) \(given: 1e-09\)", str(e.value)).group(1))
    assert timestream._row_chunks("route", NROW, need, per_row) == [(r, r + 1) for r in range(NROW)]


def test_rewriter_keeps_the_first_input_weight(tmp_path):
    ts, wrote = _directory(tmp_path / "a", weighted=(1,))
    dst = timestream.Timestream(str(tmp_path / "out"), _manager())
    new_w = np.arange(NF * NROW * NT, dtype=np.float64).reshape(NF, NROW, NT)
    extra = np.arange(NF * NROW, dtype=np.int32).reshape(NF, NROW)
    chunk = timestream._route_read("route", ts, range(NF), NROW, NT, whole=True)
    timestream._route_rewrite(dst, chunk, dict(weight=new_w[:, ::-1], added=extra))
    for fi in range(NF):
        data, attrs = _contents(dst._ffile(fi))
        assert set(data) == {"timestream", "foreign", "weight", "added"} | ({"weight_input"} if fi == 1 else set())
        assert np.array_equal(data["weight"], new_w[fi, ::-1]) and data["weight"].dtype == np.float64
        assert np.array_equal(data["added"], extra[fi]) and data["added"].dtype == np.int32
        for k in ("timestream", "foreign"):   # foreign datasets and the data itself survive, dtype and all
            assert data[k].dtype == wrote[fi][k].dtype and np.array_equal(data[k], wrote[fi][k])
        assert attrs["note"] == "file %d" % fi and int(attrs["ntime"]) == NT
    first = _contents(dst._ffile(1))[0]["weight_input"]
    assert first.dtype == np.float32 and np.array_equal(first, wrote[1]["weight"])
    # a second pass, in place: every file is weighted now, and weight_input stays what the first pass kept
    chunk = timestream._route_read("route", dst, range(NF), NROW, NT, whole=True)
    assert np.array_equal(chunk.w[0], new_w[0, ::-1])
    timestream._route_rewrite(dst, chunk, dict(weight=2 * new_w))
    for fi in range(NF):
        data, _ = _contents(dst._ffile(fi))
        assert np.array_equal(data["weight"], 2 * new_w[fi]) and np.array_equal(data["added"], extra[fi])
        assert np.array_equal(data["weight_input"], wrote[1]["weight"] if fi == 1 else new_w[fi, ::-1])


def test_product_and_root_writers(tmp_path):
    ts, _ = _directory(tmp_path / "a")
    big = np.arange(NF * 2 * 6, dtype=np.float64).reshape(NF, 2, 6)
    data = dict(map=big[:, :, ::2], hits=np.arange(NF * 2, dtype=np.int32).reshape(NF, 2))   # a strided slice
    timestream._route_write_products(ts, [2, 0], "ringmap", "one", {k: v[[2, 0]] for k, v in data.items()})
    assert not os.path.exists(timestream._product_file(ts, 1, "ringmap", "one"))
    for fi in (0, 2):
        path = os.path.join(ts._fdir(fi), "ringmap_one.hdf5")
        assert path == timestream._product_file(ts, fi, "ringmap", "one")
        got, attrs = _contents(path)
        assert set(got) == {"map", "hits"} and set(attrs) == {"frequency"} and float(attrs["frequency"]) == FREQS[fi]
        assert got["map"].dtype == np.float64 and got["hits"].dtype == np.int32
        assert np.array_equal(got["map"], data["map"][fi]) and np.array_equal(got["hits"], data["hits"][fi])
    root = os.path.join(ts.directory, "ringmap_one.hdf5")
    timestream._write_hdf5(root, dict(beam=big[:, 1], pol=np.array([[0, 1]], dtype=np.int32).T),
                           dict(parts=2, window="none", ha_max=0.05))
    got, attrs = _contents(root)
    assert set(got) == {"beam", "pol"} and got["pol"].dtype == np.int32 and got["pol"].shape == (2, 1)
    assert np.array_equal(got["beam"], big[:, 1]) and np.array_equal(got["pol"], [[0], [1]])
    assert int(attrs["parts"]) == 2 and float(attrs["ha_max"]) == 0.05
    assert (attrs["window"].decode() if isinstance(attrs["window"], bytes) else attrs["window"]) == "none"
