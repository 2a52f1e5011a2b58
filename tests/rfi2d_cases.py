"""Shared by tests/test_host_rfi2d.py and tests/test_gpu_rfi2d.py: inputs for the frequency pass
in the layout (nf, nrow, nt), the dilation of flags as a brute force over all windows, written without
`timestream.rfi_dilate_host`, and the comparison that every answer is held to."""
import numpy as np

import rfi_cases as rc

ONE = 65536
ETAS = (0.0, 0.1, 0.2, 0.5, 0.9)


def freq_data(rng, nf, nrow, nt, bursts=2, w=True, runs=(), frac=0.03):
    """x (nf, nrow, nt) and w (or None) whose series along frequency are those of tests/rfi_cases.py along time: a
    fringing sky with bursts, `frac` input flags (0, negative, NaN), the runs (f0, length) of input flags, and NaN and
    Inf under every input flag."""
    xt = rc.fringing_sky(rng, nt, nrow, nf)
    rc.add_bursts(rng, xt, bursts)
    wt = rc.input_flags(rng, xt.shape, frac, runs) if w else None
    if w:
        xt = rc.poison(xt, wt)
    back = lambda a: np.ascontiguousarray(np.transpose(a))
    return back(xt), (back(wt) if w else None)


def kappa(eta):
    return int(np.rint((1.0 - float(eta)) * ONE))


def dilate_series(flagged, missing, k, missing_counts=False):
    """One series: flagged, missing (n,) bool; a sample outside `missing` comes out flagged iff some window [a, b) with
    a <= j < b has 65536 (flagged present samples) >= k (present samples).  missing_counts=True makes the doctored
    answer in which missing samples count as length."""
    n = len(flagged)
    out = np.zeros(n, dtype=bool)
    fl = np.asarray(flagged, dtype=bool) & ~np.asarray(missing, dtype=bool)
    present = np.ones(n, dtype=bool) if missing_counts else ~np.asarray(missing, dtype=bool)
    cf, cp = np.concatenate([[0], np.cumsum(fl)]), np.concatenate([[0], np.cumsum(present)])
    cf, cp = cf.astype(np.int64), cp.astype(np.int64)
    for j in range(n):
        if missing[j]:
            continue
        nfl = cf[None, j + 1 :] - cf[: j + 1, None]   # every window [a, b) with a <= j < b
        npr = cp[None, j + 1 :] - cp[: j + 1, None]
        out[j] = bool(np.any(ONE * nfl >= k * npr))
    return out


def dilate_brute(w, eta, axis="time", ref=None, kappa_shift=0, missing_counts=False):
    """(w_out, nadded) of the dilation of w (nf, nrow, nt) by the brute force over all windows of every series."""
    w = np.asarray(w, dtype=np.float64)
    ax = 2 if axis == "time" else 0
    F = np.moveaxis(~(w > 0), ax, -1)
    I = np.zeros(F.shape, dtype=bool) if ref is None else np.moveaxis(~(np.asarray(ref) > 0), ax, -1)
    k = kappa(eta) + kappa_shift
    new = np.zeros(F.shape, dtype=bool)
    for i in np.ndindex(F.shape[:-1]):
        new[i] = dilate_series(F[i], I[i], k, missing_counts) & ~F[i]
    nadded = new.sum(axis=-1).astype(np.int32)
    return np.where(np.moveaxis(new, -1, ax), 0.0, w), nadded


def flag_weights(rng, shape, frac=0.08, run=6):
    """Weights in (0.5, 1.5) with runs of 1 .. `run` flags (0, negative, NaN) along both axes, `frac` of the samples."""
    nf, nrow, nt = shape
    w = rng.uniform(0.5, 1.5, shape)
    n = max(1, int(frac * w.size / (0.5 * run + 0.5)))
    for _ in range(n):
        f, r, t, ln = int(rng.integers(nf)), int(rng.integers(nrow)), int(rng.integers(nt)), int(rng.integers(1, run + 1))
        v = rng.choice([0.0, -1.0, np.nan])
        if rng.random() < 0.5:
            w[f, r, t : t + ln] = v
        else:
            w[f : f + ln, r, t] = v
    return w


def same(want, got, what=""):
    """Complaints about an answer (w_out, nadded) against the expected one: flags, kept bits, counts."""
    bad = []
    (w0, n0), (w1, n1) = want, got
    if not np.array_equal(w0 == 0, w1 == 0):
        bad.append("%s flags differ in %d samples" % (what, int(((w0 == 0) != (w1 == 0)).sum())))
    if not np.array_equal(np.asarray(w0).view(np.int64), np.asarray(w1).view(np.int64)):
        bad.append("%s w_out differs in its bits" % what)
    if not np.array_equal(n0, n1):
        bad.append("%s nadded differs" % what)
    return bad
