"""RFI flagging along frequency and the dilation of flags on the device:
`Context.rfi_flag_freq` against the long-double statement on the decided segments and bit for bit against
`Context.rfi_flag` on the transposed copy, on the edges of every tile width; `Context.rfi_dilate` against the host
statement exactly, on both axes; guards, determinism, refusals; and `timestream.rfi_flag(freq=, dilate=)` on a directory
against the host chain."""
import numpy as np
import pytest

import rfi2d_cases as r2
import rfi_cases as rc

pytestmark = pytest.mark.gpu


def _ctx():
    from driftscan_amd import device

    return device.get_context()


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else a.dtype)


def _guarded(ctx, shapes):
    """Buffers with one NaN (int32: -77) guard plane on each side of the first axis; the inside is poisoned too."""
    return [ctx.to_device(np.full((s[0] + 2,) + tuple(s[1:]), -77 if dt is np.int32 else np.nan, dtype=dt)) for s, dt in shapes]


def _poisoned(ctx, bufs, inside=False):
    for b in bufs:
        h = ctx.to_host(b)
        h = h if inside else np.stack([h[0], h[-1]])
        if not (np.all(h == -77) if h.dtype == np.int32 else np.all(np.isnan(h))):
            return False
    return True


def _freq_shapes(nf, nrow, nt, nseg):
    return (((nf, nrow, nt), np.float64), ((nseg, nrow, nt), np.float64), ((nrow, nt), np.int32), ((nf, nt), np.int32))


def _run_freq(ctx, x, w, p):
    nf, nrow, nt = x.shape
    bufs = _guarded(ctx, _freq_shapes(nf, nrow, nt, -(-nf // p["segment"])))
    out = tuple(b[1:-1] for b in bufs)
    got = ctx.rfi_flag_freq(ctx.to_device(x), w=None if w is None else ctx.to_device(w), out=out, **p)
    assert all(g.data_ptr() == t.data_ptr() for g, t in zip(got, out))
    ctx.sync()
    assert _poisoned(ctx, bufs)
    return [ctx.to_host(t) for t in out]


def _run_time_transposed(ctx, x, w, p):
    """`Context.rfi_flag` on the contiguous copy transposed to (nt, nrow, nf), its outputs transposed back."""
    back = lambda a: np.ascontiguousarray(np.transpose(a))
    out = ctx.rfi_flag(ctx.to_device(back(x)), w=None if w is None else ctx.to_device(back(w)), **p)
    return [back(ctx.to_host(t)) for t in out]


def _tile(ctx, nf, p):
    nseg = -(-nf // p["segment"])
    return ctx.lib.dm_rfi_freq_tile(-(-nf // nseg))


# name: (nf, the data's keywords, the parameters)
FREQ_CASES = {
    "nf 15 < min_good": (15, dict(bursts=1), {}),
    "nf 37": (37, dict(bursts=1), {}),
    "nf 64": (64, {}, {}),
    "nf 65": (65, {}, {}),
    "nf 256": (256, {}, {}),
    "nf 257": (257, {}, {}),
    "nf 512": (512, dict(bursts=4), {}),
    "nf 513": (513, dict(bursts=4), {}),
    "nf 1025": (1025, dict(bursts=8), dict(segment=2048)),
    "short last segment": (385, dict(bursts=4), dict(segment=128)),
    "segment 600": (600, dict(bursts=4), dict(segment=1024)),
    "max segment": (2048, dict(bursts=12), dict(segment=2048)),
    "windows 1..64": (257, dict(bursts=3), dict(windows=(1, 2, 4, 8, 16, 32, 64))),
    "no w": (257, dict(bursts=3, w=False), {}),
    "all input flagged": (65, {}, {}),
    "long flag runs": (257, dict(bursts=3, runs=((20, 18), (100, 40), (240, 17))), {}),
}


def test_tile_widths():
    """`dm_rfi_freq_tile`: 8 series up to 512 samples, 4 up to 1024, 2 up to the longest segment, 0 otherwise."""
    lib = _ctx().lib
    mx = lib.dm_rfi_max_segment()
    assert [lib.dm_rfi_freq_tile(n) for n in (-1, 0, 1, 512, 513, 1024, 1025, mx, mx + 1)] == [0, 0, 8, 8, 4, 4, 2, 2, 0]
    assert lib.dm_rfi_dilate_max_length(0) >= 16384 and lib.dm_rfi_dilate_max_length(1) >= mx
    assert lib.dm_rfi_dilate_max_length(2) == 0


@pytest.mark.parametrize("nrow", (1, 5))
@pytest.mark.parametrize("name", sorted(FREQ_CASES))
def test_freq_pass(name, nrow):
    """Every case at nt = 1, TJ - 1, TJ, TJ + 1 and 2 TJ + 3 for the TJ of its segment length: the flags are those of the
    long-double statement on every decided segment (at most 1 % undecided, asserted on the reference first), noise is
    within eps / sqrt(ln 2), all four outputs equal those of `Context.rfi_flag` on the transposed contiguous copy bit for
    bit, kept weights are the input's bits, nflag and occupancy count the new flags, the guards stay, and a second call
    gives the same bits."""
    ctx = _ctx()
    nf, kw, pk = FREQ_CASES[name]
    assert ctx.lib.dm_rfi_max_segment() == 2048
    p = rc.params(**pk)
    TJ = _tile(ctx, nf, p)
    assert TJ == (2 if name in ("max segment", "nf 1025") else 4 if name in ("segment 600", "nf 513") else 8)
    rng = np.random.default_rng(sum(map(ord, name)) + nrow)
    ntmax = 2 * TJ + 3
    x, w = r2.freq_data(rng, nf, nrow, ntmax, **kw)
    if name == "all input flagged":
        w = np.zeros_like(w)
    back = lambda a: np.ascontiguousarray(np.transpose(a))
    ref = rc.reference(back(x), None if w is None else back(w), p)   # on (nt, nrow, nf): series are independent
    und = 1.0 - float(ref["decided"].mean())
    assert und <= 0.01, (name, und)
    for nt in sorted({1, TJ - 1, TJ, TJ + 1, ntmax}):
        xs = np.ascontiguousarray(x[:, :, :nt])
        ws = None if w is None else np.ascontiguousarray(w[:, :, :nt])
        w_out, noise, nflag, occ = got = _run_freq(ctx, xs, ws, p)
        assert np.all(np.isfinite(w_out)) and np.all(np.isfinite(noise))
        win = np.ones(xs.shape) if ws is None else ws
        inflag = ~(win > 0)
        flags = w_out == 0
        assert np.all(flags[inflag]), (name, nt)
        assert np.array_equal(_bits(w_out[~flags]), _bits(win[~flags])), (name, nt)
        sub = {k: v[:nt] for k, v in ref.items()}
        bad, _ = rc.check(sub, back(flags), back(noise), p, nf)
        new = flags & ~inflag
        print("%-20s nf %4d rows %d nt %2d (TJ %d): new flags %.3f (reference %.3f), undecided %.3f"
              % (name, nf, nrow, nt, TJ, new.mean(), (sub["row_flags"] & ~back(inflag)).mean(), und))
        assert not bad, (name, nt, bad)
        assert np.array_equal(nflag, new.sum(axis=0)) and np.array_equal(occ, new.sum(axis=1)), (name, nt)
        for a, b in zip(got, _run_time_transposed(ctx, xs, ws, p)):
            assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (name, nt)
        for a, b in zip(got, _run_freq(ctx, xs, ws, p)):
            assert np.array_equal(_bits(a), _bits(b)), (name, nt)
        if name in ("nf 15 < min_good", "all input flagged"):
            assert flags.all() and np.all(noise == 0)
        if name == "long flag runs":
            assert not flags.all()


@pytest.mark.parametrize("row_share", (0.5, 1.0))
def test_freq_occupancy_in_integers(row_share):
    """The occupancy rule applied in numpy to the device's own row flags gives the device's occupancy and final w_out,
    and both equal `Context.rfi_flag` on the transposed copy; in place (w_out = w) gives the same bits."""
    ctx = _ctx()
    rng = np.random.default_rng(37)
    nf, nrow, nt = 257, 5, 11
    x, w = r2.freq_data(rng, nf, nrow, nt, bursts=3, frac=0.1)
    # bursts in the same frequencies of every row of some samples
    for j in (2, 7):
        f0 = int(rng.integers(10, nf - 20))
        x[f0 : f0 + 5, :, j] += 25.0 * np.exp(2j * np.pi * rng.random((1, nrow)))
    x = np.ascontiguousarray(np.transpose(rc.poison(np.transpose(x), np.transpose(w))))
    p1, p = rc.params(segment=128), rc.params(segment=128, row_share=row_share)
    rows = _run_freq(ctx, x, w, p1)
    got = _run_freq(ctx, x, w, p)
    inflag = ~(w > 0)
    new = (rows[0] == 0) & ~inflag
    n_new, n_in = new.sum(axis=1), (~inflag).sum(axis=1)
    col = (n_in > 0) & (n_new.astype(np.float64) > np.float64(row_share) * n_in.astype(np.float64))
    want = np.where((rows[0] == 0) | col[:, None, :], 0.0, w)
    assert np.array_equal(got[3], n_new) and np.array_equal(got[2], new.sum(axis=0))
    assert np.array_equal(_bits(got[0]), _bits(want)) and np.array_equal(_bits(got[1]), _bits(rows[1]))
    if row_share < 1:
        assert col.any() and not col.all() and np.any((got[0] == 0) & (rows[0] != 0))
    else:
        assert not col.any()
    for a, b in zip(got, _run_time_transposed(ctx, x, w, p)):
        assert np.array_equal(_bits(a), _bits(b))
    xd, wd = ctx.to_device(x), ctx.to_device(w)
    fresh = ctx.rfi_flag_freq(xd, w=wd, **p)
    same = ctx.rfi_flag_freq(xd, w=wd, out=(wd,) + tuple(fresh[1:]), **p)
    assert same[0].data_ptr() == wd.data_ptr() and np.array_equal(_bits(ctx.to_host(wd)), _bits(got[0]))


def test_freq_refusals_launch_nothing():
    """Every refusal of dm_rfi_flag_freq returns nonzero with the context's error set, and the outputs keep their
    poison; the wrapper's own checks; nothing to do is not refused."""
    from driftscan_amd import _lib

    ctx = _ctx()
    rng = np.random.default_rng(9)
    nf, nrow, nt = 65, 3, 5
    xd = ctx.to_device(rc.crandn(rng, nf, nrow, nt))
    wd = ctx.to_device(np.ones((nf, nrow, nt)))
    mx = ctx.lib.dm_rfi_max_segment()
    good = dict(nf=nf, nrow=nrow, nt=nt, segment=64, sigma=2.5, windows=(1, 2, 4), chi1=6.0, rho=1.5, niter=3, base=2.0,
                min_good=16, row_share=1.0, x=xd, w=wd)
    bads = [dict(nf=-1), dict(nt=-1), dict(nrow=-1), dict(segment=0), dict(segment=mx + 1), dict(sigma=0.0),
            dict(sigma=np.nan), dict(sigma=10.7), dict(windows=()), dict(windows=(1, 2, 4, 8, 16, 32, 64, 128)),
            dict(windows=(3,)), dict(windows=(2, 1)), dict(windows=(128,)), dict(chi1=0.0), dict(chi1=np.inf), dict(rho=0.5),
            dict(base=0.9), dict(niter=0), dict(niter=9), dict(min_good=0), dict(row_share=0.0), dict(row_share=1.5),
            dict(row_share=np.nan), dict(x=None), dict(out0="x"), dict(out1="w"), dict(out0=None), dict(out3="out2")]
    for bad in bads:
        a = dict(good, **bad)
        bufs = _guarded(ctx, _freq_shapes(nf, nrow, nt, 2))
        out = [b[1:-1] for b in bufs]
        ptr = {"x": ctx.ptr(xd), "w": ctx.ptr(wd), "out2": ctx.ptr(out[2]), None: None}
        op = [ctx.ptr(t) for t in out]
        for i in range(4):
            if "out%d" % i in bad:
                op[i] = ptr[bad["out%d" % i]]
        win = (_lib.c_int * max(len(a["windows"]), 1))(*a["windows"])
        rcode = ctx.lib.dm_rfi_flag_freq(ctx.h, a["nf"], a["nrow"], a["nt"], a["segment"], a["sigma"], len(a["windows"]), win,
                                         a["chi1"], a["rho"], a["niter"], a["base"], a["min_good"], a["row_share"],
                                         None if a["x"] is None else ctx.ptr(a["x"]), ctx.ptr(a["w"]), *op)
        assert rcode != 0, bad
        with pytest.raises(_lib.DriftMIError, match="dm_rfi_flag_freq"):
            ctx.check(rcode, "dm_rfi_flag_freq")
        ctx.sync()
        assert _poisoned(ctx, bufs, inside=True), bad
    with pytest.raises(ValueError):
        ctx.rfi_flag_freq(xd.real.contiguous())
    with pytest.raises(ValueError):
        ctx.rfi_flag_freq(xd, w=wd[:, :2].contiguous())
    with pytest.raises(ValueError):
        ctx.rfi_flag_freq(xd, out=(wd, wd, wd, wd))
    # a tensor on the host is refused before anything is launched
    xs, ws = ctx.to_device(np.ones((2, 3, 8), dtype=np.complex128)), ctx.to_device(np.ones((2, 3, 8)))
    with pytest.raises(ValueError, match="one GPU"):
        ctx.rfi_flag_freq(xs, w=ws.cpu())
    empty = ctx.rfi_flag_freq(xd[:, :0].contiguous())
    assert tuple(empty[0].shape) == (nf, 0, nt) and tuple(empty[2].shape) == (0, nt)


# ---- dilation -----------------------------------------------------------------------------------------------------
def _dilate_shapes(shape, axis):
    return ((shape, np.float64), ((shape[:2] if axis == "time" else shape[1:]), np.int32))


def _run_dilate(ctx, w, eta, axis, ref):
    bufs = _guarded(ctx, _dilate_shapes(w.shape, axis))
    out = tuple(b[1:-1] for b in bufs)
    got = ctx.rfi_dilate(ctx.to_device(w), eta, axis=axis, ref=None if ref is None else ctx.to_device(ref), out=out)
    assert all(g.data_ptr() == t.data_ptr() for g, t in zip(got, out))
    ctx.sync()
    assert _poisoned(ctx, bufs)
    return [ctx.to_host(t) for t in out]


def _dilate_inputs(rng, shape, axis):
    """Weights with runs of flags and a reference with missing runs; series 0, 1 and 2 along `axis` (where there are that
    many) are all flagged, not flagged at all and missing throughout."""
    w = r2.flag_weights(rng, shape, 0.08, run=6)
    ref = r2.flag_weights(rng, shape, 0.1, run=9)
    sl = [(lambda k: (0, k)), (lambda k: (k, 0))][axis == "freq"]
    series = (lambda k: (sl(k)[0], sl(k)[1], slice(None))) if axis == "time" else (lambda k: (slice(None), sl(k)[1], sl(k)[0]))
    nser = shape[1] if axis == "time" else shape[2]
    if nser > 0:
        w[series(0)] = 0.0
    if nser > 1:
        w[series(1)] = 1.25
    if nser > 2:
        ref[series(2)] = np.nan
    return w, ref


DILATE_SHAPES = [("time", (2, 4, n)) for n in (1, 2, 63, 64, 65, 257, 1025)] + [("time", (1, 1, 16384))] + \
    [("freq", (nf, 2, nt)) for nf, nt in ((1, 5), (37, 1), (37, 63), (257, 64), (257, 65), (2048, 3))]


@pytest.mark.parametrize("axis,shape", DILATE_SHAPES)
def test_dilation_equals_the_host_statement(axis, shape):
    """`Context.rfi_dilate` equals `timestream.rfi_dilate_host` exactly — flags, kept bits and counts — for eta 0 (a
    bit-identical copy), 0.2 and 0.9, with and without a reference, out of place and in place, with series that are all
    flagged, not flagged and missing throughout; the guards stay and a second call gives the same bits."""
    from driftscan_amd import timestream

    ctx = _ctx()
    assert shape[2 if axis == "time" else 0] <= ctx.lib.dm_rfi_dilate_max_length(0 if axis == "time" else 1)
    rng = np.random.default_rng(shape[0] + 7 * shape[2])
    w, ref = _dilate_inputs(rng, shape, axis)
    for eta in (0.0, 0.2, 0.9):
        for rv in (None, ref):
            want = timestream.rfi_dilate_host(w, eta, axis=axis, ref=rv)
            got = _run_dilate(ctx, w, eta, axis, rv)
            assert r2.same(want, got) == [], (eta, rv is not None)
            assert r2.same(got, _run_dilate(ctx, w, eta, axis, rv)) == []
            if eta == 0:
                assert np.array_equal(_bits(got[0]), _bits(w)) and not got[1].any()
            wd = ctx.to_device(w)
            inplace = ctx.rfi_dilate(wd, eta, axis=axis, ref=None if rv is None else ctx.to_device(rv), out=(wd, ctx.to_device(got[1] * 0 - 1)))
            assert inplace[0].data_ptr() == wd.data_ptr()
            assert r2.same(want, [ctx.to_host(t) for t in inplace]) == [], (eta, "in place")
    grown = timestream.rfi_dilate_host(w, 0.9, axis=axis)[1]
    if min(shape) > 2 and shape[2 if axis == "time" else 0] > 16:
        assert grown.any()


def test_dilation_by_hand_and_the_flags_of_the_input_as_reference():
    """A run of 10 at eta = 0.2 grows by two on each side on both axes; with the input's own flags as the reference
    nothing is added."""
    ctx = _ctx()
    w = np.ones((40, 1, 40))
    w[5, 0, 15:25] = 0.0
    w[15:25, 0, 30] = 0.0
    wd = ctx.to_device(w)
    out, n = (ctx.to_host(t) for t in ctx.rfi_dilate(wd, 0.2))
    assert np.array_equal(np.nonzero(out[5, 0] == 0)[0], np.arange(13, 27)) and n[5, 0] == 4 and n.sum() == 4
    out, n = (ctx.to_host(t) for t in ctx.rfi_dilate(wd, 0.2, axis="freq"))
    assert np.array_equal(np.nonzero(out[:, 0, 30] == 0)[0], np.arange(13, 27)) and n[0, 30] == 4 and n.sum() == 4
    for axis in ("time", "freq"):
        out, n = (ctx.to_host(t) for t in ctx.rfi_dilate(wd, 0.2, axis=axis, ref=wd))
        assert np.array_equal(out, w) and not n.any()


def test_dilation_refusals_launch_nothing():
    """Every refusal of dm_rfi_dilate returns nonzero with the context's error set and leaves the poison: eta outside
    [0, 1) or NaN, kappa < 1, another axis, a series over the exported limit, overlaps, null pointers."""
    from driftscan_amd import _lib

    ctx = _ctx()
    nf, nrow, nt = 6, 3, 9
    wd, rd = ctx.to_device(np.ones((nf, nrow, nt))), ctx.to_device(np.ones((nf, nrow, nt)))
    tmax, fmax = ctx.lib.dm_rfi_dilate_max_length(0), ctx.lib.dm_rfi_dilate_max_length(1)
    long_t, long_f = ctx.to_device(np.ones((1, 1, tmax + 1))), ctx.to_device(np.ones((fmax + 1, 1, 1)))
    good = dict(nf=nf, nrow=nrow, nt=nt, axis=0, eta=0.2, w=wd, ref=rd)
    bads = [dict(eta=-0.1), dict(eta=1.0), dict(eta=np.nan), dict(eta=np.inf), dict(eta=1.0 - 2.0**-18), dict(axis=2),
            dict(axis=-1), dict(nf=-1), dict(nrow=-1), dict(nt=-1), dict(w=None), dict(out0=None), dict(out1=None),
            dict(out0="ref"), dict(out1="w"), dict(out1="ref"), dict(out1="out0"),
            dict(nf=1, nrow=1, nt=tmax + 1, w=long_t, ref=None), dict(nf=fmax + 1, nrow=1, nt=1, axis=1, w=long_f, ref=None)]
    for bad in bads:
        a = dict(good, **bad)
        bufs = _guarded(ctx, _dilate_shapes((nf, nrow, nt), "time"))
        out = [b[1:-1] for b in bufs]
        op = [ctx.ptr(t) for t in out]
        ptr = {"w": ctx.ptr(wd), "ref": ctx.ptr(rd), "out0": op[0], None: None}
        for i in range(2):
            if "out%d" % i in bad:
                op[i] = ptr[bad["out%d" % i]]
        rcode = ctx.lib.dm_rfi_dilate(ctx.h, a["nf"], a["nrow"], a["nt"], a["axis"], a["eta"],
                                      None if a["w"] is None else ctx.ptr(a["w"]), None if a["ref"] is None else ctx.ptr(a["ref"]), *op)
        assert rcode != 0, bad
        with pytest.raises(_lib.DriftMIError, match="dm_rfi_dilate"):
            ctx.check(rcode, "dm_rfi_dilate")
        ctx.sync()
        assert _poisoned(ctx, bufs, inside=True), bad
    assert np.all(ctx.to_host(wd) == 1) and np.all(ctx.to_host(rd) == 1)
    with pytest.raises(ValueError):
        ctx.rfi_dilate(wd, 0.2, axis="row")
    with pytest.raises(ValueError):
        ctx.rfi_dilate(wd.to(ctx.torch.float32), 0.2)
    with pytest.raises(ValueError):
        ctx.rfi_dilate(wd, 0.2, ref=rd[:, :2].contiguous())
    with pytest.raises(ValueError):
        ctx.rfi_dilate(wd, 0.2, out=(wd, wd))
    # a tensor on the host is refused before anything is launched
    ws = ctx.to_device(np.ones((2, 3, 8)))
    for axis in ("time", "freq"):
        with pytest.raises(ValueError, match="one GPU"):
            ctx.rfi_dilate(ws, 0.2, axis=axis, ref=ws.cpu())
    # the length limit is inclusive; nothing to do is not refused
    edge = ctx.rfi_dilate(long_t[:, :, :tmax].contiguous(), 0.2)
    assert not ctx.to_host(edge[1]).any()
    empty = ctx.rfi_dilate(wd[:, :0].contiguous(), 0.2, axis="freq")
    assert tuple(empty[1].shape) == (0, nt)


# ---- the directory call ---------------------------------------------------------------------------------------------
def test_directory_call_against_the_host_chain(tmp_path):
    """32 frequencies, 6 rows of 200 samples: a smooth spectrum per row plus unit noise, one channel with a 30 sigma
    carrier for the whole day, and a broadband burst of 4 samples at 30 sigma with shoulders of 2 samples at 5 sigma.
    `timestream.rfi_flag(freq=..., dilate=dict(time=0.2))` equals the host chain `rfi_flag_host` ->
    `rfi_flag_freq_host` -> `rfi_dilate_host` on the decided segments; the time pass alone keeps the carrier channel, the
    whole chain flags it and the shoulders.  The shares are printed; the only conditions are these set relations."""
    import yaml

    from driftscan_amd import manager, storage, timestream

    nfreq, nrow, nt = 32, 6, 200
    prod = tmp_path / "prod"
    prod.mkdir()
    (prod / "config.yaml").write_text(yaml.dump(dict(
        config=dict(beamtransfers=False, kltransform=False, psfisher=False, output_directory=str(prod)),
        telescope=dict(type="UnpolarisedCylinder", num_freq=nfreq, freq_start=400.0, freq_end=420.0, freq_mode="edge",
                       num_cylinders=2, cylinder_width=2.0, num_feeds=2, feed_spacing=0.4, tsys=1.0))))
    pm = manager.ProductManager.from_config(str(prod))
    rng = np.random.default_rng(83)
    f = np.arange(nfreq)[:, None, None]
    x = rc.crandn(rng, nfreq, nrow, nt) + 20.0 * np.exp(2j * np.pi * rng.random((1, nrow, 1))) * (1.0 + 0.3 * np.cos(f / 9.0 + rng.random((1, nrow, 1))))
    chan, t0 = 11, 120
    x[chan] += 30.0 * np.exp(2j * np.pi * rng.random((nrow, 1)))
    x[:, :, t0 : t0 + 4] += 30.0 * np.exp(2j * np.pi * rng.random((nfreq, nrow, 1)))
    for sl in (slice(t0 - 2, t0), slice(t0 + 4, t0 + 6)):
        x[:, :, sl] += 5.0 * np.exp(2j * np.pi * rng.random((nfreq, nrow, 1)))
    src = timestream.Timestream(str(tmp_path / "day"), pm)
    for fi in range(nfreq):
        timestream._write_sim_file(src, fi, x[fi], np.linspace(0, 2 * np.pi, nt, endpoint=False))
    src.save()
    tp, fp, dil = dict(segment=200), dict(segment=32, kernel_sigma=1.5, min_good=12), dict(time=0.2)
    only = timestream.rfi_flag(pm, src.directory, str(tmp_path / "time_only"), **tp)
    full = timestream.rfi_flag(pm, src.directory, str(tmp_path / "full"), freq=fp, dilate=dil, **tp)

    def read(ts, name):
        out = []
        for fi in range(nfreq):
            with storage.File(ts._ffile(fi), "r") as fh:
                out.append(None if name not in fh else np.asarray(fh[name][:]))
        return out

    w_only, w_full = np.stack(read(only, "weight")), np.stack(read(full, "weight"))
    assert all(v is None for v in read(only, "rfi_freq_nflag")) and all(v is None for v in read(only, "rfi_dilate_nflag"))
    # the host chain, with the decided series of both passes
    pt, pf = timestream.rfi_params(tp), timestream.rfi_params(fp)
    w1, _, _, _, d1 = timestream.rfi_flag_host(x, None, dtype=np.longdouble, details=True, **pt)
    w2, _, _, _, d2 = timestream.rfi_flag_freq_host(x, w1, dtype=np.longdouble, details=True, **pf)
    w3, _ = timestream.rfi_dilate_host(w2, 0.2, axis="time", ref=None)   # the day came without weights: nothing is missing
    assert d1["decided"].all() and d2["decided"].all(), "the inputs of this test leave a segment undecided"
    assert np.array_equal(w_only, w1) and np.array_equal(w_full, w3)
    nfq, ndl = np.stack(read(full, "rfi_freq_nflag")), np.stack(read(full, "rfi_dilate_nflag"))
    assert nfq.dtype == np.int32 and nfq.shape == (nfreq, nrow)
    assert np.array_equal(nfq, ((w2 == 0) & (w1 > 0)).sum(axis=2)) and np.array_equal(ndl, ((w3 == 0) & (w2 > 0)).sum(axis=2))
    shoulders = np.r_[t0 - 2 : t0, t0 + 4 : t0 + 6]
    others = np.ones(nfreq, dtype=bool)
    others[chan] = False
    print("carrier channel flagged: %.3f by the time pass, %.3f by the chain; shoulders %.3f and %.3f; burst %.3f and %.3f; "
          "the rest %.4f and %.4f" % ((w_only[chan] == 0).mean(), (w_full[chan] == 0).mean(), (w_only[:, :, shoulders] == 0).mean(),
                                      (w_full[:, :, shoulders] == 0).mean(), (w_only[:, :, t0 : t0 + 4] == 0).mean(),
                                      (w_full[:, :, t0 : t0 + 4] == 0).mean(),
                                      (np.delete(w_only[others], np.r_[t0 - 2 : t0 + 6], axis=2) == 0).mean(),
                                      (np.delete(w_full[others], np.r_[t0 - 2 : t0 + 6], axis=2) == 0).mean()))
    assert (w_only[chan] == 0).mean() < 0.5 and np.all(w_full[chan] == 0)
    assert np.all(w_full[:, :, shoulders] == 0) and np.all(w_full[w_only == 0] == 0)
