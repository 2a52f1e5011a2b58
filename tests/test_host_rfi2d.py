"""RFI flagging along frequency and the dilation of flags on the host:
`timestream.rfi_flag_freq_host` as the transposition of `rfi_flag_host`, `timestream.rfi_dilate_host` against the brute
force over all windows of tests/rfi2d_cases.py, the comparison against doctored answers, the parameter dicts, the
pipeline's `rfi_freq:` and `rfi_dilate:` keys, and the two refusals of the steps along frequency."""
import numpy as np
import pytest

import rfi2d_cases as r2
import rfi_cases as rc
from driftscan_amd import parallel, timestream


def test_freq_pass_is_the_transposition():
    """Every output and every detail of `rfi_flag_freq_host` is that of `rfi_flag_host` on the data transposed to
    (nt, nrow, nf), transposed back, with and without w and with the occupancy step."""
    rng = np.random.default_rng(61)
    nf, nrow, nt = 150, 3, 4
    x, w = r2.freq_data(rng, nf, nrow, nt, runs=((60, 9),), frac=0.05)
    for wv, p in ((w, rc.params(segment=64)), (None, rc.params(segment=64, niter=1)), (w, rc.params(segment=150, row_share=0.5))):
        xv = x if wv is not None else np.where(np.isfinite(x), x, 0)
        got = timestream.rfi_flag_freq_host(xv, wv, details=True, **p)
        want = timestream.rfi_flag_host(xv.transpose(2, 1, 0), None if wv is None else wv.transpose(2, 1, 0), details=True, **p)
        nseg = -(-nf // p["segment"])
        assert got[0].shape == (nf, nrow, nt) and got[1].shape == (nseg, nrow, nt)
        assert got[2].shape == (nrow, nt) and got[3].shape == (nf, nt) and got[2].dtype == np.int32
        for a, b in zip(got[:4], want[:4]):
            assert np.array_equal(a, b.transpose(), equal_nan=True)
        assert sorted(got[4]) == sorted(want[4])
        for name in want[4]:
            assert np.array_equal(got[4][name], want[4][name].transpose())
        assert (got[0] == 0).any() and not (got[0] == 0).all()
        plain = timestream.rfi_flag_freq_host(xv, wv, **p)
        assert len(plain) == 4 and np.array_equal(plain[0], got[0], equal_nan=True)
    # a series along frequency sees its own samples only: the flags of one (row, j) alone
    alone = timestream.rfi_flag_freq_host(x[:, 1:2, 2:3], w[:, 1:2, 2:3], **rc.params(segment=64))
    full = timestream.rfi_flag_freq_host(x, w, **rc.params(segment=64))
    assert np.array_equal(alone[0][:, 0, 0], full[0][:, 1, 2], equal_nan=True)
    with pytest.raises(ValueError):
        timestream.rfi_flag_freq_host(x[0], None)


def _random_series(rng, count=300, nmax=70):
    for _ in range(count):
        n = int(rng.integers(1, nmax + 1))
        yield n, float(rng.choice([0.0, 0.05, 0.15, 0.4, 0.8]))


@pytest.mark.parametrize("axis", ("time", "freq"))
@pytest.mark.parametrize("missing", (False, True))
def test_dilation_against_all_windows(axis, missing):
    """300 random series of 1 to 70 samples, each with every eta: the two-scan form flags what the brute force over all
    windows flags, keeps every other weight bit for bit and counts the new flags; eta = 0 changes nothing."""
    rng = np.random.default_rng(67 + (axis == "freq") + 2 * missing)
    for n, frac in _random_series(rng):
        shape = (1, 2, n) if axis == "time" else (n, 2, 1)
        w = r2.flag_weights(rng, shape, frac, run=5) if frac else rng.uniform(0.5, 1.5, shape)
        ref = r2.flag_weights(rng, shape, 0.15, run=7) if missing else None
        for eta in r2.ETAS:
            got = timestream.rfi_dilate_host(w, eta, axis=axis, ref=ref)
            assert got[1].dtype == np.int32 and got[1].shape == (shape[:2] if axis == "time" else shape[1:])
            assert r2.same(r2.dilate_brute(w, eta, axis=axis, ref=ref), got) == [], (n, eta)
            if eta == 0:
                assert np.array_equal(got[0].view(np.int64), w.view(np.int64)) and not got[1].any()
            if ref is not None:   # a missing sample stays as it is
                gone = ~(ref > 0)
                assert np.array_equal(got[0][gone].view(np.int64), w[gone].view(np.int64))


def test_dilation_by_hand():
    """A run of 10 at eta = 0.2 grows by two on each side; with the samples beside it missing it grows past them by the
    same two; eta close to 1 flags the whole series once one sample is flagged; the refusals."""
    w = np.ones((1, 1, 40))
    w[0, 0, 15:25] = 0.0
    out, n = timestream.rfi_dilate_host(w, 0.2)
    assert np.array_equal(np.nonzero(out[0, 0] == 0)[0], np.arange(13, 27)) and n[0, 0] == 4
    ref = np.ones_like(w)
    ref[0, 0, 12:15] = 0.0
    ref[0, 0, 25:27] = np.nan
    out, n = timestream.rfi_dilate_host(w, 0.2, ref=ref)
    assert np.array_equal(np.nonzero(out[0, 0] == 0)[0], np.r_[10:12, 15:25, 27:29]) and n[0, 0] == 4
    assert np.array_equal(out[0, 0, 12:15], w[0, 0, 12:15])
    # the flags the data arrived with as the missing set: nothing is left to dilate
    out, n = timestream.rfi_dilate_host(w, 0.2, ref=w)
    assert np.array_equal(out, w) and n[0, 0] == 0
    one = np.ones((1, 1, 40))
    one[0, 0, 7] = -1.0
    out, n = timestream.rfi_dilate_host(one, 1.0 - 1.0 / 65536)
    assert n[0, 0] == 39 and out[0, 0, 7] == -1.0 and np.all(np.delete(out[0, 0], 7) == 0)
    assert timestream.rfi_dilate_kappa(0.0) == 65536 and timestream.rfi_dilate_kappa(0.2) == 52429
    for bad in (-0.1, 1.0, np.nan, np.inf, 1.0 - 2.0**-18):
        with pytest.raises(ValueError, match="rfi_dilate"):
            timestream.rfi_dilate_host(w, bad)
    with pytest.raises(ValueError):
        timestream.rfi_dilate_host(w, 0.2, axis="row")
    with pytest.raises(ValueError):
        timestream.rfi_dilate_host(w, 0.2, ref=np.ones((1, 1, 39)))


def test_the_comparison_rejects_doctored_answers():
    """One flipped flag, one miscounted series, kappa off by one in either direction and missing samples counted as
    length: each fails the comparison that the honest answer passes.  kappa + 1 shows at eta = 0.5 on a window with
    exactly half its samples flagged; kappa - 1 at eta = 0.2, where kappa = 52429 is just above 4 / 5 of 65536 and a
    window with exactly four of five flagged does not reach it."""
    rng = np.random.default_rng(71)
    shape = (2, 3, 64)
    w = r2.flag_weights(rng, shape, 0.2, run=5)
    w[0, 0, :8] = [1.0, 0.0, 1.0, 0.0, 1.0, 1.0, 1.0, 1.0]
    w[0, 1, :12] = [0.0, 0.0, 0.0, 0.0] + [1.0] * 8
    ref = r2.flag_weights(rng, shape, 0.15, run=7)
    ref[0, :2, :12] = 1.0
    for eta, doctors in ((0.5, (dict(kappa_shift=1), dict(missing_counts=True))), (0.2, (dict(kappa_shift=-1),))):
        honest = timestream.rfi_dilate_host(w, eta, ref=ref)
        want = r2.dilate_brute(w, eta, ref=ref)
        assert r2.same(want, honest) == []
        flipped = honest[0].copy()
        j = int(np.nonzero(flipped[1, 2] > 0)[0][0])
        flipped[1, 2, j] = 0.0
        assert r2.same(want, (flipped, honest[1]))
        count = honest[1].copy()
        count[0, 1] += 1
        assert r2.same(want, (honest[0], count))
        for doctor in doctors:
            assert r2.same(want, r2.dilate_brute(w, eta, ref=ref, **doctor)), doctor
    # without missing samples the third doctor has nothing to get wrong
    assert r2.same(r2.dilate_brute(w, 0.5), r2.dilate_brute(w, 0.5, missing_counts=True)) == []


def test_parameter_dicts():
    """`rfi_dilate_params` fills `time`, `freq` and `new_only`; an unknown key and an eta outside [0, 1) raise
    ValueError; the frequency pass takes the keys of the time pass through the same `rfi_params`."""
    assert timestream.rfi_dilate_params(None) == dict(time=0.0, freq=0.0, new_only=True)
    assert timestream.rfi_dilate_params(dict(time=0.2)) == dict(time=0.2, freq=0.0, new_only=True)
    assert timestream.rfi_dilate_params(dict(freq=0.1, new_only=False)) == dict(time=0.0, freq=0.1, new_only=False)
    with pytest.raises(ValueError, match="unknown key"):
        timestream.rfi_dilate_params(dict(eta=0.2))
    for bad in (dict(time=1.0), dict(freq=-0.5), dict(time=np.nan)):
        with pytest.raises(ValueError, match="rfi_dilate"):
            timestream.rfi_dilate_params(bad)
    assert timestream.rfi_params(dict(segment=256)) == dict(rc.DEFAULTS, segment=256)
    assert timestream.RFI_DEFAULTS == rc.DEFAULTS


def _products(tmp_path, num_freq=2):
    import yaml

    prod = tmp_path / "prod"
    prod.mkdir()
    (prod / "config.yaml").write_text(yaml.dump(dict(
        config=dict(beamtransfers=False, kltransform=False, psfisher=False, output_directory=str(prod)),
        telescope=dict(type="UnpolarisedCylinder", num_freq=num_freq, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                       num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4, tsys=1.0))))
    return prod


def test_pipeline_keys(tmp_path, monkeypatch):
    """`rfi_freq: {...}` and `rfi_dilate: {...}` beside `rfi:` in `stack_from` and `sidereal_from` reach
    `stack_baselines` and `sidereal_stack` with the defaults filled in, and only when present; an unknown key is refused
    when the file is read."""
    import yaml

    from driftscan_amd.pipeline import PipelineManager

    prod = _products(tmp_path)

    def conf(sid, stack):
        return dict(config=dict(product_directory=str(prod)),
                    timestreams=[dict(name="d0", directory=str(tmp_path / "d0"),
                                      stack_from=dict(directory=str(tmp_path / "u0"), **stack)),
                                 dict(name="sid", directory=str(tmp_path / "sid"),
                                      sidereal_from=dict(days=[str(tmp_path / "d0")], **sid))])

    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf(dict(rfi=dict(chi1=5.0), rfi_freq=dict(segment=256, windows=[1, 2]), rfi_dilate=dict(time=0.2)),
                                    dict(rfi_dilate=dict(freq=0.1, new_only=False)))))
    p = PipelineManager.from_configfile(str(cfile))
    seen = {}
    monkeypatch.setattr(timestream, "stack_baselines", lambda m, indir, outdir, **kw: seen.update(stack=kw))
    monkeypatch.setattr(timestream, "sidereal_stack", lambda m, days, outdir, **kw: seen.update(sidereal=kw))
    p.stack()
    assert seen["sidereal"]["rfi"] == dict(rc.DEFAULTS, chi1=5.0)
    assert seen["sidereal"]["rfi_freq"] == dict(rc.DEFAULTS, segment=256, windows=(1, 2))
    assert seen["sidereal"]["rfi_dilate"] == dict(time=0.2, freq=0.0, new_only=True)
    assert seen["stack"]["rfi_dilate"] == dict(time=0.0, freq=0.1, new_only=False)
    assert "rfi" not in seen["stack"] and "rfi_freq" not in seen["stack"]
    cfile.write_text(yaml.dump(conf(dict(rfi_freq={}), {})))
    p = PipelineManager.from_configfile(str(cfile))
    seen.clear()
    p.stack()
    assert seen["sidereal"]["rfi_freq"] == rc.DEFAULTS and "rfi_dilate" not in seen["sidereal"]
    assert not {"rfi", "rfi_freq", "rfi_dilate"} & set(seen["stack"])
    for bad in (conf(dict(rfi_freq=dict(chi=5.0)), {}), conf({}, dict(rfi_dilate=dict(eta=0.2))),
                conf({}, dict(rfi_freq=dict(threshold=3))), conf(dict(rfi_dilate=dict(time=0.2, axis="time")), {})):
        cfile.write_text(yaml.dump(bad))
        with pytest.raises(ValueError, match="unknown key"):
            PipelineManager.from_configfile(str(cfile))


def test_frequency_steps_need_one_chunk_on_one_rank(tmp_path):
    """A step along frequency with a `chunk_gb` that does not hold every frequency raises ValueError naming the
    `chunk_gb` it needs, and so does more than one rank; dilation along time alone asks for neither (it gets as far as
    asking for a device)."""
    from driftscan_amd import manager

    nfreq, nrow, nt = 4, 6, 50
    pm = manager.ProductManager.from_config(str(_products(tmp_path, nfreq)))
    ts = timestream.Timestream(str(tmp_path / "day"), pm)
    rng = np.random.default_rng(73)
    for fi in range(nfreq):
        timestream._write_sim_file(ts, fi, rc.crandn(rng, nrow, nt), np.linspace(0, 1, nt, endpoint=False))
    ts.save()
    small = 3 * nrow * nt * 48.0 / 2.0**30   # three of the four frequencies
    calls = [lambda **kw: timestream.rfi_flag(pm, ts.directory, str(tmp_path / "out"), **kw),
             lambda **kw: timestream.sidereal_stack(pm, [ts.directory], str(tmp_path / "sid"), ntime=8, **{
                 dict(freq="rfi_freq", dilate="rfi_dilate").get(k, k): v for k, v in kw.items()})]
    for call in calls:
        for step in (dict(freq={}), dict(dilate=dict(freq=0.1)), dict(freq=dict(segment=2), dilate=dict(time=0.2))):
            with pytest.raises(ValueError, match="chunk_gb >= ") as e:
                call(chunk_gb=small, **step)
            need = float(str(e.value).split("chunk_gb >= ")[1].split()[0])
            assert small < need <= 2 * small
            parallel.set_virtual(0, 2)
            try:
                with pytest.raises(ValueError, match="2 ranks"):
                    call(**step)
            finally:
                parallel.set_virtual(None)
    import torch

    if not torch.cuda.is_available():
        from driftscan_amd import _lib

        with pytest.raises(_lib.DriftMIError):   # no refusal of its own: the next thing it asks for is the device
            calls[0](chunk_gb=small, dilate=dict(time=0.2))
