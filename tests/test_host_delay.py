"""The delay fit along frequency on the host: the float64 statement with LAPACK against the
long-double one under the bound of the section, on the cases the device is held to; kappa_2(G) <= 1e8 for every sample of
every element-wise case; the doctored answers the checker must reject; `delay_basis`, `delay_classes` and the
parameters of the routes."""
import numpy as np
import pytest

import delay_cases as dc
from driftscan_amd import timestream

_REF = {}


def _case(name):
    if name not in _REF:
        c = dc.make(name)
        _REF[name] = (c, dc.reference(c))
    return _REF[name]


@pytest.mark.parametrize("name", sorted(dc.CASES))
def test_float64_statement_within_the_bound(name):
    """Every mode of every case: the float64 statement is within the bound of the long-double one, info is equal, the
    exact parts are exact, and no solved sample has kappa_2(G) > 1e8 (so none is excused).  The patterns of the case are
    all there: series solved, series with too few samples, NaN, negative and zero flags."""
    c, ref = _case(name)
    solved = ref["info"] == 0
    assert solved.any()
    print("%s: kappa_2(G) up to %.3g, %d of %d series solved" % (name, ref["kappa"][solved].max(), solved.sum(), solved.size))
    assert np.all(ref["kappa"][solved] <= dc.KAPPA_MAX)
    assert set(np.unique(ref["info"])) <= {0, -1}
    if c["nt"] >= 5:
        assert (ref["info"] == -1).any() and np.isnan(c["w"]).any() and (c["w"] < 0).any() and (c["w"] == 0).any()
    # the signal dominates what lies outside the span, which the derivation of the bound assumes (theta <= 2)
    om = np.where(ref["kept"], c["w"], 0.0)
    num = np.sqrt((om * np.abs(np.where(ref["kept"], c["x"], 0.0)) ** 2).sum(axis=0))
    den = np.sqrt((om * np.abs(ref["model"]).astype(np.float64) ** 2).sum(axis=0))
    assert np.all(num[solved] <= 2.0 * den[solved])
    for mode in dc.MODES:
        x_out, w_out, info = timestream.delay_fit_host(c["x"], c["w"], c["bases"], c["basis_of"], mode, 0.0, None)
        bad, worst = dc.check(c, ref, mode, x_out, w_out, info)
        print("  %s: worst error %.3g of its bound" % (mode, worst))
        assert not bad, bad


def test_exact_parts_and_min_valid_boundary():
    """Kept samples of inpaint are x bit for bit, kept weights w bit for bit, flagged samples of filter 0; a series with
    r - 1 kept samples gives info = -1 and one with r is solved; min_valid moves the boundary; w = None keeps all."""
    c, ref = _case("nf 64")
    x_out, w_out, info = timestream.delay_fit_host(c["x"], c["w"], c["bases"], c["basis_of"], "inpaint")
    kept = ref["kept"]
    assert np.array_equal(x_out[kept].view(np.int64), c["x"][kept].view(np.int64))
    assert np.array_equal(w_out[kept].view(np.int64), c["w"][kept].view(np.int64))
    nvalid = kept.sum(axis=0)
    ranks = np.array([c["ranks"][k] for k in c["basis_of"]])[:, None]
    assert np.array_equal(info == -1, (nvalid < ranks) | (nvalid == 0))
    assert ((nvalid == ranks - 1) & (ranks > 1)).any() and (nvalid == ranks).any()
    assert np.all(info[nvalid == ranks] == 0)
    xf, wf, _ = timestream.delay_fit_host(c["x"], c["w"], c["bases"], c["basis_of"], "filter")
    assert np.all(xf[~kept] == 0) and np.all(wf[~kept] == 0) and np.all(np.isfinite(xf.real))
    info40 = timestream.delay_fit_host(c["x"], c["w"], c["bases"], c["basis_of"], "model", min_valid=40)[2]
    assert np.array_equal(info40 == -1, nvalid < 40)
    c2 = dc.make("nf 7", w_none=True)
    x2, w2, i2 = timestream.delay_fit_host(c2["x"], None, c2["bases"], c2["basis_of"], "inpaint")
    assert not i2.any() and np.all(w2 == 1) and np.array_equal(x2, c2["x"])
    bad = np.array(c["basis_of"])
    bad[1] = len(c["bases"])
    ib = timestream.delay_fit_host(c["x"], c["w"], c["bases"], bad, "inpaint")[2]
    assert np.all(ib[1] == -2) and np.array_equal(ib[[0, 2, 3, 4]], info[[0, 2, 3, 4]])


def test_rank_deficient_basis():
    """A basis with one vector twice and ridge = 0: the pivot of the second copy is exactly 0, info = 3; with a ridge the
    series are solved, in both arithmetics, within the bound."""
    c = dc.deficient()
    for dtype in (np.float64, np.longdouble):
        info = timestream.delay_fit_host(c["x"], c["w"], c["bases"], c["basis_of"], "model", 0.0, None, dtype=dtype)[2]
        assert np.all(info[[0, 2]] == 3) and np.all(info[1] == 0)
    ref = dc.reference(c, ridge=0.5)
    assert not ref["info"].any() and np.all(ref["kappa"] <= dc.KAPPA_MAX)
    for mode in dc.MODES:
        out = timestream.delay_fit_host(c["x"], c["w"], c["bases"], c["basis_of"], mode, 0.5, None)
        bad, _ = dc.check(c, ref, mode, *out)
        assert not bad, bad


def test_wide_gap_scaled_bound_only():
    """A gap wider than 1 / tau: kappa_2(G) is large and the fill is poor, but the float64 answer stays within the
    scaled bound."""
    c = dc.wide_gap()
    ref = dc.reference(c)
    assert not ref["info"].any()
    print("wide gap: kappa_2(G) %.3g .. %.3g" % (ref["kappa"].min(), ref["kappa"].max()))
    assert ref["kappa"].min() > dc.KAPPA_MAX
    for mode in dc.MODES:
        out = timestream.delay_fit_host(c["x"], c["w"], c["bases"], c["basis_of"], mode)
        bad, worst = dc.check(c, ref, mode, *out)
        print("  %s: worst error %.3g of its bound" % (mode, worst))
        assert not bad, bad


def test_checker_rejects_doctored_answers():
    """Planted into the float64 answer: a flagged x leaking in with weight, one basis column of the neighbouring class,
    the ridge dropped, 1 / v replaced by the mean weight, filter not zeroing flagged samples."""
    c, _ = _case("nf 64")
    ridge = 1e-3
    ref = dc.reference(c, ridge=ridge)
    args = (c["bases"], c["basis_of"])
    for mode in dc.MODES:
        good = timestream.delay_fit_host(c["x"], c["w"], *args, mode, ridge, None)
        assert not dc.check(c, ref, mode, *good)[0]
    kept = ref["kept"]
    solved = np.broadcast_to((ref["info"] == 0)[None], kept.shape)
    # a flagged x leaks in with weight (only where the series stays solved the same way: info must not be what differs)
    leak_w = c["w"].copy()
    leak_x = np.where(kept, c["x"], c["x_clean"] + 0.1)
    some = ~kept & solved
    some[:, :, 1::2] = False
    leak_w[some] = 0.7
    xl, _, il = timestream.delay_fit_host(leak_x, leak_w, *args, "model", ridge, None)
    assert np.array_equal(il, ref["info"])
    assert dc.check(c, ref, "model", xl, np.where(kept, c["w"], 0.0), il)[0]
    # one basis column of the neighbouring class
    swapped = [a.copy() for a in c["bases"]]
    swapped[0][:, 1] = c["bases"][1][:, 1]
    xs, ws, i_s = timestream.delay_fit_host(c["x"], c["w"], swapped, c["basis_of"], "model", ridge, None)
    assert dc.check(c, ref, "model", xs, ws, i_s)[0]
    # the ridge dropped
    xr, wr, ir = timestream.delay_fit_host(c["x"], c["w"], *args, "model", 0.0, None)
    assert dc.check(c, ref, "model", xr, wr, ir)[0]
    # 1 / v replaced by the mean weight of the series
    xi, wi, ii = timestream.delay_fit_host(c["x"], c["w"], *args, "inpaint", ridge, None)
    om = np.where(kept, c["w"], 0.0)
    wbar = np.broadcast_to(om.sum(axis=0) / np.maximum(kept.sum(axis=0), 1), kept.shape)
    wd = np.where(~kept & solved, wbar, wi)
    assert dc.check(c, ref, "inpaint", xi, wd, ii)[0]
    # filter that leaves the model under the flags
    xf, wf, i_f = timestream.delay_fit_host(c["x"], c["w"], *args, "filter", ridge, None)
    xd = np.where(~kept & solved, -ref["model"].astype(np.complex128), xf)
    assert dc.check(c, ref, "filter", xd, wf, i_f)[0]


def test_host_statement_refusals():
    c, _ = _case("nf 7")
    a = (c["x"], c["w"], c["bases"], c["basis_of"])
    with pytest.raises(ValueError):
        timestream.delay_fit_host(*a, mode="fill")
    with pytest.raises(ValueError):
        timestream.delay_fit_host(*a, ridge=-1.0)
    with pytest.raises(ValueError):
        timestream.delay_fit_host(*a, ridge=np.nan)
    with pytest.raises(ValueError):
        timestream.delay_fit_host(*a, dtype=np.float32)
    with pytest.raises(ValueError):
        timestream.delay_fit_host(c["x"], c["w"][:, :2], c["bases"], c["basis_of"])
    with pytest.raises(ValueError):
        timestream.delay_fit_host(c["x"], c["w"], [np.ones((6, 1))], c["basis_of"])


# ---- delay_basis and delay_classes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,tau,gaps", ((64, 0.05, False), (256, 0.03, False), (65, 0.2, True), (7, 0.1, False)))
def test_delay_basis(nf, tau, gaps):
    """Orthonormal to 1e-13, eigenvalues descending and above the cut, and the span holds exp(2 pi i tau' nu) for
    |tau'| <= 0.9 tau.  S is the mean of e e^H over the band |tau'| <= tau, so the mean over the band of the squared
    residual |(1 - A A^T) e|^2 / nf is the sum of the dropped eigenvalues / nf; the tolerance on the residual of a single
    tau' is 4 times its square root (measured: the worst single tau' is 1.5 to 1.7 times that root at eigencut 1e-10,
    3e-6 to 6e-6 of |e|), with the dropped eigenvalues from the long-double residual S - A diag(lambda) A^T."""
    nu = dc.grid(nf)
    if gaps:
        nu = np.delete(nu, [10, 11, 30])
    cut = 1e-10
    A, lam = timestream.delay_basis(nu, tau, cut)
    r = A.shape[1]
    assert A.shape[0] == nu.size and lam.shape == (r,) and 1 <= r <= nu.size
    assert np.abs(A.T @ A - np.eye(r)).max() <= 1e-13
    assert np.all(np.diff(lam) <= 0) and lam[-1] >= cut * lam[0]
    L = np.longdouble
    S = np.sinc(2.0 * tau * (nu[:, None] - nu[None, :])).astype(L)
    dropped = float(np.trace(S - (A.astype(L) * lam.astype(L)) @ A.T.astype(L)))
    dropped = max(dropped, nu.size * 2.0**-52 * float(lam[0]))
    tol = 4.0 * np.sqrt(dropped / nu.size)
    worst = 0.0
    for tp in np.linspace(-0.9 * tau, 0.9 * tau, 41):
        e = np.exp(2j * np.pi * tp * nu).astype(np.clongdouble)
        res = e - A.astype(L) @ (A.T.astype(L) @ e)
        worst = max(worst, float(np.sqrt((np.abs(res) ** 2).sum() / nu.size)))
    print("nf %d tau %g: rank %d, residual %.3g of |e|, tolerance %.3g" % (nu.size, tau, r, worst, tol))
    assert worst <= tol
    # more eigenvectors with a lower cut, fewer with a smaller band
    assert timestream.delay_basis(nu, tau, 1e-14)[0].shape[1] >= r >= timestream.delay_basis(nu, tau / 2, cut)[0].shape[1]


def test_delay_basis_rank_refusal():
    nfmax, rmax = dc.limits()
    assert rmax >= 64 and nfmax >= 256
    nu = dc.grid(256)
    with pytest.raises(ValueError, match="bandwidth x delay product"):
        timestream.delay_basis(nu, 1.0)
    with pytest.raises(ValueError):
        timestream.delay_basis(nu, -0.1)
    with pytest.raises(ValueError):
        timestream.delay_basis(nu, 0.1, eigencut=0.0)
    A, _ = timestream.delay_basis(nu[:1], 0.1)
    assert A.shape == (1, 1) and abs(abs(A[0, 0]) - 1) < 1e-15


class _Tel(object):
    def __init__(self, nf, baselines):
        self.frequencies = dc.grid(nf)
        self.baselines = np.asarray(baselines, dtype=np.float64)


def test_delay_classes():
    """tau_row = horizon |b| / c + buffer / (nf dnu); every row's ceiling is >= its tau; at most nclass ceilings,
    equally spaced; the table is packed as the device reads it."""
    rng = np.random.default_rng(3)
    b = rng.uniform(-60.0, 60.0, (37, 2))
    b[5] = 0.0
    tel = _Tel(64, b)
    table, ranks, basis_of, tau = timestream.delay_classes(tel, horizon=1.0, buffer=2.0, nclass=4)
    blen = np.sqrt((b**2).sum(axis=1))
    assert np.allclose(tau, blen / 299.792458 + 2.0 / (64 * 0.390625), rtol=1e-14)
    ceil, of2 = timestream.delay_class_ceilings(tau, 4)
    assert np.array_equal(of2, basis_of) and basis_of.dtype == np.int32 and len(ceil) == len(ranks) <= 4
    assert np.all(ceil[basis_of] >= tau) and ceil[-1] == tau.max()
    lo, hi = tau.min(), tau.max()
    assert np.allclose(ceil, [c for c in lo + (hi - lo) * np.arange(1, 5) / 4 if np.any(np.isclose(c, ceil))])
    for k in range(1, len(ceil)):   # the smallest ceiling that holds the row
        rows = basis_of == k
        assert np.all(tau[rows] > ceil[k - 1])
    assert np.all(np.diff(ranks) >= 0) and table.shape == (64 * ranks.sum(),)
    off = 0
    for k, r in enumerate(ranks):
        A, _ = timestream.delay_basis(tel.frequencies, ceil[k])
        assert np.array_equal(table[off : off + 64 * r].reshape(r, 64), A.T)
        off += 64 * r
    # one row, or rows of one length: one class
    assert np.array_equal(timestream.delay_classes(_Tel(8, [[3.0, 4.0]] * 3))[2], [0, 0, 0])
    with pytest.raises(ValueError):
        timestream.delay_classes(_Tel(1, [[3.0, 4.0]]))
    with pytest.raises(ValueError):
        timestream.delay_classes(tel, nclass=0)
    with pytest.raises(ValueError, match="bandwidth x delay product"):
        timestream.delay_classes(_Tel(256, [[3000.0, 0.0]]))


def test_delay_params_and_pipeline_key(tmp_path, monkeypatch):
    """`delay_params` fills the defaults and refuses unknown keys and bad values; `delay: {...}` in `stack_from` and
    `sidereal_from` reaches `stack_baselines` and `sidereal_stack` with the defaults filled in, only when present."""
    import yaml

    from driftscan_amd.pipeline import PipelineManager

    assert timestream.delay_params() == timestream.DELAY_DEFAULTS
    assert timestream.delay_params(dict(mode="filter", nclass=3))["nclass"] == 3
    for bad in (dict(modes="x"), dict(mode="fill"), dict(ridge=-1), dict(nclass=0), dict(eigencut=2.0), dict(buffer=-1.0)):
        with pytest.raises(ValueError):
            timestream.delay_params(bad)
    prod = tmp_path / "prod"
    prod.mkdir()
    (prod / "config.yaml").write_text(yaml.dump(dict(
        config=dict(beamtransfers=False, kltransform=False, psfisher=False, output_directory=str(prod)),
        telescope=dict(type="UnpolarisedCylinder", num_freq=8, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                       num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4, tsys=1.0))))

    def conf(sid, stack):
        return dict(config=dict(product_directory=str(prod)),
                    timestreams=[dict(name="d0", directory=str(tmp_path / "d0"),
                                      stack_from=dict(directory=str(tmp_path / "u0"), **stack)),
                                 dict(name="sid", directory=str(tmp_path / "sid"),
                                      sidereal_from=dict(days=[str(tmp_path / "d0")], **sid))])

    cfile = tmp_path / "pipe.yaml"
    cfile.write_text(yaml.dump(conf(dict(delay=dict(mode="inpaint", buffer=1.0)), dict(delay={}))))
    p = PipelineManager.from_configfile(str(cfile))
    seen = {}
    monkeypatch.setattr(timestream, "stack_baselines", lambda m, indir, outdir, **kw: seen.update(stack=kw))
    monkeypatch.setattr(timestream, "sidereal_stack", lambda m, days, outdir, **kw: seen.update(sidereal=kw))
    p.stack()
    assert seen["sidereal"]["delay"] == dict(timestream.DELAY_DEFAULTS, buffer=1.0)
    assert seen["stack"]["delay"] == timestream.DELAY_DEFAULTS
    cfile.write_text(yaml.dump(conf({}, {})))
    p = PipelineManager.from_configfile(str(cfile))
    seen.clear()
    p.stack()
    assert "delay" not in seen["stack"] and "delay" not in seen["sidereal"]
    cfile.write_text(yaml.dump(conf(dict(delay=dict(tau=1.0)), {})))
    with pytest.raises(ValueError, match="unknown key"):
        PipelineManager.from_configfile(str(cfile))


def test_delay_filter_refusals(tmp_path):
    """More than one rank and a `chunk_gb` that does not hold one row over all frequencies raise ValueError before the
    device is asked for; unknown keywords are refused."""
    import yaml

    from driftscan_amd import manager, parallel

    prod = tmp_path / "prod"
    prod.mkdir()
    (prod / "config.yaml").write_text(yaml.dump(dict(
        config=dict(beamtransfers=False, kltransform=False, psfisher=False, output_directory=str(prod)),
        telescope=dict(type="UnpolarisedCylinder", num_freq=8, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                       num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4, tsys=1.0))))
    pm = manager.ProductManager.from_config(str(prod))
    nrow, nt = int(pm.telescope.npairs), 20
    ts = timestream.Timestream(str(tmp_path / "day"), pm)
    rng = np.random.default_rng(1)
    for fi in range(8):
        timestream._write_sim_file(ts, fi, rng.standard_normal((nrow, nt)) + 0j, np.linspace(0, 1, nt, endpoint=False))
    ts.save()
    with pytest.raises(ValueError, match="chunk_gb >= "):
        timestream.delay_filter(pm, ts.directory, str(tmp_path / "out"), chunk_gb=1e-9)
    with pytest.raises(ValueError, match="unknown key"):
        timestream.delay_filter(pm, ts.directory, str(tmp_path / "out"), taper=1)
    parallel.set_virtual(0, 2)
    try:
        with pytest.raises(ValueError, match="2 ranks"):
            timestream.delay_filter(pm, ts.directory, str(tmp_path / "out"))
        # the routes refuse before they stack or regrid anything: nothing is written
        with pytest.raises(ValueError, match="2 ranks"):
            timestream.sidereal_stack(pm, [ts.directory], str(tmp_path / "sid"), ntime=8, delay={})
        with pytest.raises(ValueError, match="2 ranks"):
            timestream.stack_baselines(pm, ts.directory, str(tmp_path / "stk"), delay={})
        assert not (tmp_path / "sid").exists() and not (tmp_path / "stk").exists()
    finally:
        parallel.set_virtual(None)
