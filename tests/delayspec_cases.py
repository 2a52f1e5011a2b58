"""The cases of the delay-spectrum tests, their long-double reference, the bound and the checker.

A case is one launch: nf frequencies, five rows with amplitudes graded over six decades, a step of either sign with
max |phi| of about 300 turns, a taper, weights with zeros, negatives and NaN, NaN and Inf in x under every flag, and a
bin table with unequal bins, an empty bin, a bin whose series all fall under min_valid, and samples outside every bin.
The shapes sit at the edges of the 16 x 16 x 4 MFMA tile, of the workgroup tile of the kernel (128 delays, 64 samples,
chunks of 16 frequencies: no nf, nd or nt of a case is a multiple of its tile, unless it is 1) and of its bin split (a
bin of more than 128 samples is cut into 2 .. 4 segments).

The bound.  For a used series t let A(t) = sum_f |y_f| |x_f| and c = 2^-53 (6 pi max|phi| + 8 + 2 nf): each of Re D_a(t)
and Im D_a(t) is off by at most e = c A (the ring-map bound of section 4.25 without its normalisation: 2 pi |phi| 2^-53 from
the rounded product step_f k, the rest of the 6 pi for sincospi and the reduction, 8 for the roundings of T omega, y x and
the two products of a frequency, 2 nf for the accumulation).  With |D| <= A,
    | |D^|^2 - |D|^2 | <= 2 e (|Re D| + |Im D|) + 2 e^2 <= (2 sqrt(2) c + 2 c^2) A^2,
the two squares and their sum add 2 2^-53 |D^|^2 <= 2 2^-53 (1 + 2 c)^2 A^2, and a sum of n_t such non-negative terms in any
order adds at most n_t 2^-53 of the sum.  So
    |q^ - q| <= (2 sqrt(2) c + 2 c^2 + (n_t + 2) 2^-53 (1 + 2 c)^2) sum_t A(t)^2,
and the same for h with x = 1.  s1 and s2 are sums of nf n_t non-negative terms of three roundings each: (nf n_t + 2)
2^-53 relative.  count and the zeros of a bin without a used series are exact."""
import numpy as np

from driftscan_amd.timestream import delay_spectrum_host

U = 2.0 ** -53
NROW = 5

# name: (nf, nd, nt, a0 ("lo", "mid", "hi"), bin table or None, weighting, min_valid)
CASES = {
    "one": (1, 1, 1, "lo", None, "mask", 1),
    "edges": (3, 15, 37, "lo", (1, 9, 9, 20, 24, 36), "mask", 2),
    "four": (4, 16, 37, "mid", (0, 5, 37), "weight", 1),
    "five": (5, 17, 130, "hi", None, "mask", 3),                       # one bin in two segments
    "seventeen": (17, 33, 130, "mid", (2, 2, 50, 57, 129), "weight", 9),
    "wide": (67, 129, 130, "mid", (0, 129, 130), "mask", 30),          # two delay blocks, a bin in two segments
    "long": (5, 17, 300, "mid", (0, 260, 300), "weight", 2),           # a bin in three segments (beyond the issue's list)
}
DROPPED = {"edges": (20, 24), "seventeen": (50, 57)}   # the bin whose series all fall under min_valid


def make(name, w_none=False, taper_none=False, weighting=None, min_valid=None):
    nf, nd, nt, where, bins, wt, need = CASES[name]
    rng = np.random.default_rng(sum(ord(ch) for ch in name) + 11)
    a0 = {"lo": 0, "mid": nd // 2, "hi": nd - 1}[where]
    kmax = max(nd - 1, 1)
    step = (np.linspace(-1.0, 0.83, nf) if nf > 1 else np.array([0.77])) * 300.0 / kmax
    taper = None if taper_none else rng.uniform(0.5, 3.0, nf)
    amp = 10.0 ** (-6.0 * np.arange(NROW) / (NROW - 1))
    x = (rng.standard_normal((nf, NROW, nt)) + 1j * rng.standard_normal((nf, NROW, nt))) * amp[None, :, None]
    w = None
    if not w_none:
        w = rng.uniform(0.5, 2.0, (nf, NROW, nt))
        drop = rng.random((nf, NROW, nt))
        if nt > 1:
            w[drop < 0.2] = 0.0
            w[(drop >= 0.2) & (drop < 0.25)] = -1.0
            w[(drop >= 0.25) & (drop < 0.3)] = np.nan
        if name in DROPPED:
            t0, t1 = DROPPED[name]
            w[1:, :, t0:t1] = 0.0          # one kept channel at the most: under min_valid
        bad = ~(w > 0)
        x[bad] = np.where(rng.random(int(bad.sum())) < 0.5, np.nan, np.inf)   # a sample that is not kept reaches nothing
    off = np.array([0, nt] if bins is None else bins, dtype=np.int32)
    return dict(name=name, nf=nf, nrow=NROW, nt=nt, nd=nd, a0=a0, step=step, taper=taper, x=x, w=w, bin_off=off,
                weighting=wt if weighting is None else weighting, min_valid=need if min_valid is None else min_valid)


def reference(c, dtype=np.longdouble):
    """`delay_spectrum_host` in long double: (q, h, s1, s2, count)."""
    return delay_spectrum_host(c["x"], c["w"], c["taper"], c["step"], c["nd"], c["a0"], c["weighting"], c["min_valid"],
                               c["bin_off"], dtype=dtype)


def bound(c):
    """(bq, bh) (nrow, nbin) long double, the bounds of q and h of the module docstring, and n_t (nrow, nbin)."""
    ld = np.longdouble
    nf, nrow, nt, nd = c["nf"], c["nrow"], c["nt"], c["nd"]
    off = c["bin_off"]
    nbin = off.size - 1
    kept = np.ones(c["x"].shape, dtype=bool) if c["w"] is None else c["w"] > 0
    T = np.ones(nf, dtype=ld) if c["taper"] is None else c["taper"].astype(ld)
    om = kept.astype(ld) if (c["w"] is None or c["weighting"] == "mask") else np.where(kept, c["w"], 0.0).astype(ld)
    y = np.abs(T[:, None, None] * om)
    ax = np.where(kept, np.abs(np.where(kept, c["x"], 0.0)), 0.0).astype(ld)
    used = kept.sum(axis=0) >= c["min_valid"]
    A = np.where(used, (y * ax).sum(axis=0), 0)       # (nrow, nt)
    Aw = np.where(used, y.sum(axis=0), 0)
    kmax = max(c["a0"], nd - 1 - c["a0"], nd - 1)
    cc = ld(U) * (6 * np.pi * np.abs(c["step"]).max() * kmax + 8 + 2 * nf)
    bq, bh, n = np.zeros((nrow, nbin), dtype=ld), np.zeros((nrow, nbin), dtype=ld), np.zeros((nrow, nbin), dtype=np.int64)
    for b in range(nbin):
        sl = slice(off[b], off[b + 1])
        n[:, b] = used[:, sl].sum(axis=1)
        fac = 2 * np.sqrt(ld(2)) * cc + 2 * cc * cc + (n[:, b] + 2) * ld(U) * (1 + 2 * cc) ** 2
        bq[:, b] = fac * (A[:, sl] ** 2).sum(axis=1)
        bh[:, b] = fac * (Aw[:, sl] ** 2).sum(axis=1)
    return bq, bh, n


def check(c, got, ref):
    """got = (q, h, s1, s2, count) (h, s1, s2, count may be None) against ref in long double: q and h under `bound`, s1
    and s2 to (nf n_t + 2) 2^-53 relative, count and the zeros of the bins without a used series exactly.  Returns
    (complaints, the worst error of q and h in units of its bound)."""
    bad = []
    bq, bh, n = bound(c)
    worst = 0.0
    if not np.array_equal(n, ref[4]):
        bad.append("the reference does not count the series of the bound")
    empty = ref[4] == 0
    for name, g, r, lim in (("q", got[0], ref[0], bq), ("h", got[1], ref[1], bh)):
        if g is None:
            continue
        g = np.asarray(g)
        if g.shape != r.shape:
            bad.append("%s has shape %s, not %s" % (name, g.shape, r.shape))
            continue
        err = np.abs(g.astype(np.longdouble) - r)
        lim3 = np.broadcast_to(lim[:, :, None], err.shape)
        over = ~(err <= lim3)
        if over.any():
            i = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err - lim3)), err.shape)
            bad.append("%s: %d elements over the bound, first (row, bin, delay) = %s: error %.3g, bound %.3g"
                       % (name, over.sum(), i, err[i], lim3[i]))
        if np.any(g[empty] != 0) or np.any(np.signbit(g[empty])):
            bad.append("%s is not exactly +0 in a bin without a used series" % name)
        with np.errstate(invalid="ignore", divide="ignore"):
            if err.size:
                worst = max(worst, float(np.max(np.where(lim3 > 0, err / np.where(lim3 > 0, lim3, 1), 0))))
    for name, g, r in (("s1", got[2], ref[2]), ("s2", got[3], ref[3])):
        if g is None:
            continue
        g = np.asarray(g)
        if g.shape != r.shape:
            bad.append("%s has shape %s, not %s" % (name, g.shape, r.shape))
            continue
        tol = (c["nf"] * n + 2) * np.longdouble(U) * np.abs(r)
        if np.any(~(np.abs(g.astype(np.longdouble) - r) <= tol)):
            bad.append("%s is outside (nf n_t + 2) 2^-53 relative" % name)
        if np.any(g[empty] != 0):
            bad.append("%s is not exactly 0 in a bin without a used series" % name)
    if got[4] is not None:
        g = np.asarray(got[4])
        if g.shape != ref[4].shape or g.dtype != np.int32 or not np.array_equal(g, ref[4]):
            bad.append("count differs")
    return bad, worst
