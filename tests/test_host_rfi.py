"""The RFI flagger on the host: `timestream.rfi_flag_host` against a second statement with one
loop per sample, double against long double on the decided segments, the checker of tests/rfi_cases.py against doctored
answers, `skysim.RFIModel`, the share flagged on pure noise, and the pipeline's `rfi:` keys."""
import numpy as np
import pytest

import rfi_cases as rc
from driftscan_amd import skysim, timestream


def _small(rng, nrow=3, nt=150, frac=0.05, runs=((60, 9),)):
    x = rc.fringing_sky(rng, rc.NF, nrow, nt)
    rc.add_bursts(rng, x, 2)
    w = rc.input_flags(rng, x.shape, frac, runs)
    return rc.poison(x, w), w


SMALL = [rc.params(segment=64), rc.params(segment=64, niter=1), rc.params(segment=150, kernel_sigma=0.4),
         rc.params(segment=40, windows=(1, 4, 64), min_good=30), rc.params(segment=64, kernel_sigma=10.6, chi1=4.0, rho=1.2)]


@pytest.mark.parametrize("dtype", (np.float64, np.longdouble))
def test_restatement_against_the_loop_statement(dtype):
    """Flags equal sample for sample and noise within eps / sqrt(ln 2), for every series of every small case, with and
    without w."""
    rng = np.random.default_rng(41)
    for p in SMALL:
        x, w = _small(rng)
        for wv in (w, None):
            xv = x if wv is not None else np.where(np.isfinite(x), x, 0)
            w_out, noise, nflag, occ, det = timestream.rfi_flag_host(xv, wv, dtype=dtype, details=True, **p)
            inflag = np.zeros(x.shape, dtype=bool) if wv is None else ~(wv > 0)
            for f in range(x.shape[0]):
                for r in range(x.shape[1]):
                    fl, nz = rc.flag_loop(xv[f, r], None if wv is None else wv[f, r], p, real=dtype)
                    assert np.array_equal(fl, w_out[f, r] == 0), (p, f, r)
                    assert np.all(np.abs(nz - noise[f, r]) <= det["eps"][f, r] / rc.SQRT_LN2)
            new = (w_out == 0) & ~inflag
            assert np.array_equal(nflag, new.sum(axis=2)) and np.array_equal(occ, new.sum(axis=1))
            keep = w_out != 0
            assert np.array_equal(w_out[keep], (np.ones(x.shape) if wv is None else wv)[keep])
            assert np.array_equal(det["row_flags"], w_out == 0)   # row_share = 1: no occupancy step


def test_tables():
    """Both statements of the tables agree to the bit, the thresholds fall with the window length and with the
    iteration, and the parameter refusals are those of the entry point."""
    for p in SMALL + [rc.params()]:
        g, t = timestream.rfi_tables_host(p["kernel_sigma"], p["windows"], p["chi1"], p["rho"], p["niter"], p["base"])
        H, g2, t2 = rc.tables(p)
        assert g.shape == (H + 1,) and np.array_equal(g, np.array(g2)) and np.array_equal(t, np.array(t2))
        assert np.all(np.diff(t, axis=1) <= 0) and np.all(np.diff(t, axis=0) <= 0) and g[0] == 1.0
    alpha, beta = np.sqrt(np.pi / (4 * np.log(2))), np.sqrt((1 - np.pi / 4) / np.log(2))
    assert abs(timestream.rfi_tables_host()[1][2, 0] - (alpha + 6 * beta)) < 1e-14
    for bad in (dict(kernel_sigma=0.0), dict(kernel_sigma=10.7), dict(windows=(3,)), dict(windows=(2, 1)), dict(windows=()),
                dict(windows=(128,)), dict(chi1=0.0), dict(rho=0.9), dict(base=0.5), dict(niter=0), dict(niter=9)):
        with pytest.raises(ValueError, match="rfi"):
            timestream.rfi_tables_host(**bad)
    assert timestream.rfi_segments(385, 128) == [(0, 96), (96, 192), (192, 288), (288, 385)]


def test_double_and_long_double_decide_alike():
    """400 segments of 256 samples: a fringing sky of 30 sigma, 3 % input flags, bursts of 3 to 40 sigma lasting 1 to 8
    samples.  At most 1 % of the segments are undecided (a condition on the inputs), and on every decided one the flags
    of the two precisions are identical."""
    rng = np.random.default_rng(43)
    x = rc.fringing_sky(rng, rc.NF, 100, 512)
    truth = rc.add_bursts(rng, x, 4)
    w = rc.input_flags(rng, x.shape, 0.03)
    x = rc.poison(x, w)
    p = rc.params(segment=256)
    ref = rc.reference(x, w, p)
    w_out, noise = timestream.rfi_flag_host(x, w, **p)[:2]
    assert ref["decided"].size == 400
    bad, und = rc.check(ref, w_out == 0, noise, p, 512)
    differing = int((ref["row_flags"] != (w_out == 0)).any(axis=-1).sum())
    ok = w > 0
    strong = truth & ok
    print("undecided %d of 400, differing series %d; bursts found %.3f, flagged outside bursts %.3f"
          % (int((~ref["decided"]).sum()), differing, (w_out == 0)[strong].mean(), (w_out == 0)[ok & ~truth].mean()))
    assert not bad, bad


def test_the_checker_rejects_doctored_answers():
    """One flipped flag, a median of the wrong rank, flags carried over between iterations instead of restarted, and a
    window pass that sees its own new flags: each fails the comparison that the honest answer passes."""
    rng = np.random.default_rng(47)
    nt, p = 256, rc.params(segment=128)
    x = rc.fringing_sky(rng, rc.NF, 4, nt)
    rc.add_bursts(rng, x, 5)
    w = rc.input_flags(rng, x.shape, 0.03)
    x = rc.poison(x, w)
    ref = rc.reference(x, w, p)

    def answer(**doctor):
        fl, nz = np.zeros(x.shape, dtype=bool), np.zeros(x.shape[:2] + (2,))
        for f in range(x.shape[0]):
            for r in range(x.shape[1]):
                fl[f, r], nz[f, r] = rc.flag_loop(x[f, r], w[f, r], p, **doctor)
        return fl, nz

    fl, nz = answer()
    assert rc.check(ref, fl, nz, p, nt)[0] == []
    flipped = fl.copy()
    flipped[1, 2, 77] ^= True
    assert rc.check(ref, flipped, nz, p, nt)[0]
    off = nz.copy()
    off[0, 1, 1] *= 1 + 1e-12
    assert rc.check(ref, fl, off, p, nt)[0]
    for doctor in (dict(median_shift=1), dict(carry=True), dict(live=True)):
        assert rc.check(ref, *answer(**doctor), p, nt)[0], doctor


def test_rfi_model():
    """Frequency subsets reproduce the rows of the full call, the same samples are hit in every row with one phase per
    (row, burst), and stream 28 shares no draw with FlagModel's placement for the same seed."""
    m = skysim.RFIModel(fraction=0.1, burst=4, amplitude=20.0, seed=9)
    nt, nrow = 300, 6
    fg = [0, 3, 7]
    full, mask = m.bursts(nt, fg, nrow), m.mask(nt, fg)
    assert full.shape == (3, nrow, nt) and mask.shape == (3, nt) and mask.dtype == bool
    assert np.array_equal(m.bursts(nt, [7, 0], nrow), full[[2, 0]]) and np.array_equal(m.mask(nt, [3]), mask[1:2])
    assert np.all(mask[:, None, :] | (full == 0)) and np.all((np.abs(full) > 0).any(axis=1) == mask)
    assert 0.03 < mask.mean() < 0.25
    start = m.starts(nt, fg)
    f0, s0 = (int(v[0]) for v in np.nonzero(start & ~np.roll(mask, 1, axis=1)))   # a burst that no other runs into
    run = full[f0, :, s0]
    assert np.allclose(np.abs(run), 20.0) and len(set(np.round(np.angle(run), 9))) == nrow
    flag = skysim.FlagModel(fraction=0.1, burst=4, seed=9).mask(nt, fg) == 0
    assert not np.array_equal(flag, mask)
    # the draws themselves: no uniform of stream 28 is one of stream 27
    f, s = np.meshgrid(np.array(fg, dtype=np.uint64), np.arange(nt, dtype=np.uint64), indexing="ij")
    u = []
    for stream in (skysim.STREAM_TS_FLAG, skysim.STREAM_TS_RFI):
        wd = skysim._philox4x32_10([s, f, np.zeros_like(s), np.full_like(s, stream)], (9, 0))
        u.append(skysim._u53(wd[0], wd[1]).ravel())
    assert skysim.STREAM_TS_RFI == 28 and not np.intersect1d(u[0], u[1]).size
    for bad in (dict(fraction=1.0), dict(burst=0), dict(amplitude=-1.0)):
        with pytest.raises(ValueError):
            skysim.RFIModel(**bad)
    with pytest.raises(ValueError, match="unknown"):
        skysim.RFIModel.from_config(dict(fraction=0.1, length=3))
    assert skysim.RFIModel.from_config(dict(fraction=0.1, burst=2, amplitude=5.0, seed=1)).burst == 2


# The share of pure complex noise that the default parameters flag, from 8 192 000 samples (2 x 4000 series of 1024) on
# the host at development time.
PURE_NOISE_SHARE = 3.551e-4   # 2909 of 8 192 000


def test_pure_noise():
    """The flagged share of 204 800 samples of pure noise against PURE_NOISE_SHARE.  Flags come in runs of up to 16 (the
    longest window), so the samples are not independent draws: the binomial standard deviation is taken for
    N / 16 independent units, and five of them are allowed."""
    rng = np.random.default_rng(53)
    x = rc.crandn(rng, rc.NF, 100, 1024)
    w_out = timestream.rfi_flag_host(x, None)[0]
    share = float((w_out == 0).mean())
    sd = np.sqrt(PURE_NOISE_SHARE * (1 - PURE_NOISE_SHARE) / (x.size / 16.0))
    print("pure noise: %.5f flagged, expected %.5f +- %.5f" % (share, PURE_NOISE_SHARE, sd))
    assert abs(share - PURE_NOISE_SHARE) <= 5 * sd


def test_pipeline_keys(tmp_path, monkeypatch):
    """`sidereal_from: {..., rfi: {...}}` and `stack_from: {..., rfi: {...}}` reach `sidereal_stack` and `stack_baselines`
    with the defaults filled in; an unknown key is refused when the file is read."""
    import yaml

    from driftscan_amd.pipeline import PipelineManager

    prod = tmp_path / "prod"
    prod.mkdir()
    (prod / "config.yaml").write_text(yaml.dump(dict(
        config=dict(beamtransfers=False, kltransform=False, psfisher=False, output_directory=str(prod)),
        telescope=dict(type="UnpolarisedCylinder", num_freq=2, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                       num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4, tsys=1.0))))

    def conf(sid_rfi, stack_rfi):
        return dict(config=dict(product_directory=str(prod)),
                    timestreams=[dict(name="d0", directory=str(tmp_path / "d0"),
                                      stack_from=dict(directory=str(tmp_path / "u0"), rfi=stack_rfi)),
                                 dict(name="sid", directory=str(tmp_path / "sid"),
                                      sidereal_from=dict(days=[str(tmp_path / "d0")], rfi=sid_rfi))])

    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf(dict(chi1=5.0, windows=[1, 2, 4]), dict(segment=512, row_share=0.5))))
    p = PipelineManager.from_configfile(str(cfile))
    seen = {}
    monkeypatch.setattr(timestream, "stack_baselines", lambda m, indir, outdir, **kw: seen.update(stack=kw))
    monkeypatch.setattr(timestream, "sidereal_stack", lambda m, days, outdir, **kw: seen.update(sidereal=kw))
    p.stack()
    assert seen["stack"]["rfi"] == dict(rc.DEFAULTS, segment=512, row_share=0.5)
    assert seen["sidereal"]["rfi"] == dict(rc.DEFAULTS, chi1=5.0, windows=(1, 2, 4))
    cfile.write_text(yaml.dump(conf({}, None)))
    p = PipelineManager.from_configfile(str(cfile))
    seen.clear()
    p.stack()
    assert seen["sidereal"]["rfi"] == rc.DEFAULTS and "rfi" not in seen["stack"]
    for bad in (conf(dict(chi=5.0), None), conf(None, dict(threshold=3))):
        cfile.write_text(yaml.dump(bad))
        with pytest.raises(ValueError, match="unknown key"):
            PipelineManager.from_configfile(str(cfile))
    with pytest.raises(ValueError, match="unknown key"):
        timestream.rfi_params(dict(sigma=2.0))
    assert timestream.rfi_params(None) == rc.DEFAULTS
