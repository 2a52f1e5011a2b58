"""Shared by tests/test_host_delay.py and tests/test_gpu_delay.py: inputs for the delay fit
along frequency, the long-double reference and the checker that holds an answer to the bound of that section."""
import numpy as np

import rfi_cases as rc
from driftscan_amd import timestream

# gamma = (C1 nf + C2 r^2) 2^-53, derived in DESIGN.md section 4.23 (not fitted to any answer)
C1, C2 = 176.0, 8.0
U = 2.0**-53
KAPPA_MAX = 1e8
MODES = ("model", "filter", "inpaint")


def limits():
    return timestream._delay_limits()


def gamma(nf, r):
    return (C1 * nf + C2 * r * r) * U


def grid(nf):
    """nf channel centres in MHz, 0.39 MHz apart from 400 MHz."""
    return 400.0 + 0.390625 * np.arange(nf)


def delay_basis_of_rank(nf, r, eigencut=1e-10):
    """`timestream.delay_basis` on `grid(nf)` with tau bisected until the rank is r."""
    nu = grid(nf)

    def rank(tau):
        lam = np.linalg.eigvalsh(np.sinc(2.0 * tau * (nu[:, None] - nu[None, :])))[::-1]
        return int((lam >= eigencut * lam[0]).sum())

    band = max(nu[-1] - nu[0], 1.0)
    lo, hi = 0.0, 2.0 * nf / band
    # the rank is 2 B tau plus 7 to 9 at this cut: start from that bracket where it holds (each step is an eigenproblem)
    near = max(0.0, (r - 12) / (2.0 * band)), max(0.5, r - 4.0) / (2.0 * band)
    if nf > 256 and rank(near[0]) < r < rank(near[1]):
        lo, hi = near
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        k = rank(mid)
        if k == r:
            A, _ = timestream.delay_basis(nu, mid, eigencut)
            assert A.shape == (nf, r)
            return A
        if k < r:
            lo = mid
        else:
            hi = mid
    raise AssertionError("no tau gives rank %d on %d channels" % (r, nf))


def random_basis(rng, nf, r):
    """r orthonormal columns with no structure."""
    return np.ascontiguousarray(np.linalg.qr(rng.standard_normal((nf, r)))[0])


# name: (nf, nt, [(kind, rank)] of the table, basis_of) — classes of different ranks, basis_of not sorted
CASES = {
    "nf 1": (1, 5, [("random", 1)], (0, 0, 0)),
    "nf 2": (2, 1, [("random", 1), ("delay", 2)], (1, 0, 1)),
    "nf 7": (7, 67, [("delay", 2), ("random", 1), ("delay", 5)], (2, 0, 1, 2)),
    "nf 64": (64, 67, [("delay", 17), ("delay", 2), ("random", 32), ("delay", 9)], (2, 0, 3, 1, 0)),
    "nf 65": (65, 5, [("random", 64), ("delay", 17), ("random", 1)], (1, 2, 0)),
    "nf 256": (256, 5, [("delay", 32), ("delay", 17), ("delay", 64), ("delay", 2)], (2, 0, 3, 1)),
    # one sample, one delay basis: the long-double reference and the eigenproblems of 2048 channels are the cost
    "nf max": (None, 1, [("random", 64), ("delay", 2)], (1, 0, 1)),
}


def _flag_value(i):
    return (0.0, -1.0, np.nan)[i % 3]


def weights(rng, nf, ranks_of_row, nt, none_flagged=False):
    """(nf, nrow, nt) weights: non-binary in (0.5, 1.5), and per (row, t) one of the patterns — nothing flagged, one
    channel, a run in the middle, runs at both edges, the whole series, nvalid = r - 1, nvalid = r, graded over
    1e-6 .. 1e6 — with channel 3 of row 0 flagged for every t.  The flags are 0, negative and NaN in turn.  The patterns
    that leave exactly r - 1 or r samples, and the graded weights, fall on rows of rank <= 2 only (elsewhere a run):
    with r samples of a larger basis, or weights over twelve decades on it, kappa_2(G) is past the 1e8 the element-wise
    bound is stated for."""
    nrow = len(ranks_of_row)
    w = rng.uniform(0.5, 1.5, (nf, nrow, nt))
    if none_flagged:
        return w
    n = 0
    for row, r in enumerate(ranks_of_row):
        for t in range(nt):
            p = (t + 3 * row) % 8
            run = max(1, min(8, nf // 8))
            idx = np.zeros(nf, dtype=bool)
            if p == 1:
                idx[int(rng.integers(nf))] = True
            elif p == 2 or (p in (5, 6, 7) and r > 2):
                j0 = max(0, nf // 2 - run // 2)
                idx[j0 : j0 + run] = True
            elif p == 3:
                idx[: max(1, run // 2)] = True
                idx[nf - max(1, run // 2) :] = True
            elif p == 4:
                idx[:] = True
            elif p in (5, 6):
                keep = r - 1 if p == 5 else r
                idx[:] = True
                if keep > 0:
                    idx[np.unique(np.round(np.linspace(0, nf - 1, keep)).astype(int))] = False
                    if int((~idx).sum()) != keep:   # nf too short for `keep` distinct channels
                        idx[:] = False
            elif p == 7:
                w[:, row, t] = 10.0 ** np.linspace(-6.0, 6.0, nf)
            for f in np.nonzero(idx)[0]:
                w[f, row, t] = _flag_value(n)
                n += 1
    if nf > 3:
        w[3, 0, :] = 0.0
    return w


def make(name, seed=0, w_none=False, none_flagged=False):
    """The inputs of a case: dict(nf, nrow, nt, bases, ranks, basis_of, x (poisoned under the flags), w, x_clean)."""
    nf, nt, table, basis_of = CASES[name]
    if nf is None:
        nf = limits()[0]
    rng = np.random.default_rng(sum(map(ord, name)) + 1000 * seed)
    bases = [delay_basis_of_rank(nf, r) if kind == "delay" else random_basis(rng, nf, r) for kind, r in table]
    return build(rng, bases, basis_of, nt, w_none=w_none, none_flagged=none_flagged)


def build(rng, bases, basis_of, nt, w_none=False, none_flagged=False, noise=1e-3):
    nf = bases[0].shape[0]
    nrow = len(basis_of)
    ranks = [int(a.shape[1]) for a in bases]
    x = np.empty((nf, nrow, nt), dtype=np.complex128)
    for row, k in enumerate(basis_of):
        x[:, row] = bases[k] @ rc.crandn(rng, ranks[k], nt) + noise * rc.crandn(rng, nf, nt)
    w = None if w_none else weights(rng, nf, [ranks[k] for k in basis_of], nt, none_flagged=none_flagged)
    xp = x if w is None else rc.poison(x, w)
    return dict(nf=nf, nrow=nrow, nt=nt, bases=bases, ranks=ranks, basis_of=np.asarray(basis_of, dtype=np.int32), x=xp, w=w,
                x_clean=x)


def deficient(nt=5):
    """Basis 0 has its second vector twice, in numbers that make every sum exact (indicator vectors of four channels,
    unit weights): the pivot of column 2 is exactly 0, on every arithmetic.  Basis 1 is regular."""
    nf = 8
    a = np.zeros((nf, 3))
    a[:4, 0] = 1.0
    a[4:, 1] = 1.0
    a[4:, 2] = 1.0
    rng = np.random.default_rng(5)
    b = random_basis(rng, nf, 2)
    c = build(rng, [a, b], (0, 1, 0), nt, w_none=True)
    return c


def wide_gap(nt=5):
    """One class of rank 17 on 64 channels with a gap of 32 channels, several times 1 / tau (about 8 channels;
    kappa_2(G) grows by about 20 per 4 channels of gap, past 1e8 here): held to the scaled bound only."""
    rng = np.random.default_rng(9)
    a = delay_basis_of_rank(64, 17)
    c = build(rng, [a], (0, 0), nt, none_flagged=True)
    c["w"][16:48] = 0.0
    c["x"] = rc.poison(c["x_clean"], c["w"])
    return c


def reference(c, ridge=0.0, min_valid=None):
    """The long-double statement with its details: what every answer is held against."""
    _, _, info, det = timestream.delay_fit_host(c["x"], c["w"], c["bases"], c["basis_of"], "model", ridge, min_valid,
                                                dtype=np.longdouble, details=True)
    cn = np.sqrt((np.abs(det["c"]) ** 2).sum(axis=-1)).astype(np.float64)
    return dict(det, info=info, cnorm=cn)


def expected(c, ref, mode):
    """(x_out, w_out) of `mode` from the reference, in long double."""
    kept, solved = ref["kept"], (ref["info"] == 0)[None]
    w = np.ones(c["x"].shape) if c["w"] is None else c["w"]
    xk = np.where(kept, c["x"], 0.0).astype(np.clongdouble)
    w_out = np.where(kept, w, 0.0).astype(np.longdouble)
    if mode == "model":
        x_out = np.where(solved, ref["model"], 0.0)
    elif mode == "filter":
        x_out = np.where(solved & kept, xk - ref["model"], xk)
    else:
        x_out = np.where(solved & ~kept, ref["model"], xk)
        with np.errstate(divide="ignore", invalid="ignore"):
            fill = np.where((ref["v"] > 0) & np.isfinite(ref["v"]), 1 / ref["v"], 0)
        w_out = np.where(solved & ~kept, fill, w_out)
    return x_out, w_out


def check(c, ref, mode, x_out, w_out, info):
    """An answer against the reference: list of complaints and the worst error as a share of its bound.  info is equal;
    where the answer is exact by definition (kept samples of inpaint, kept weights, zeros, series that are not solved)
    it is equal bit for bit; every model value is within gamma kappa_2(G) |a_f| |c| (in filter mode plus the rounding of
    the subtraction), every fill weight within gamma kappa_2(G) of itself."""
    bad = []
    nf = c["nf"]
    if not np.array_equal(info, ref["info"]):
        bad.append("info differs in %d series" % int((info != ref["info"]).sum()))
        return bad, np.inf
    ex, ew = expected(c, ref, mode)
    kept, solved = ref["kept"], np.broadcast_to((ref["info"] == 0)[None], ref["kept"].shape)
    r_row = np.array([c["ranks"][k] if 0 <= k < len(c["ranks"]) else 1 for k in c["basis_of"]], dtype=np.float64)
    g = (C1 * nf + C2 * r_row**2)[None, :, None] * U * ref["kappa"][None]
    tol = g * ref["anorm"][:, :, None] * ref["cnorm"][None]
    if mode == "filter":
        tol = tol + 2.0 * U * (np.abs(ex) + np.abs(ref["model"])).astype(np.float64)
    fitted = solved if mode == "model" else solved & kept if mode == "filter" else solved & ~kept
    err = np.abs(x_out.astype(np.clongdouble) - ex).astype(np.float64)
    exact = ~fitted
    same = (x_out.real == ex.real.astype(np.float64)) & (x_out.imag == ex.imag.astype(np.float64))
    if np.any(exact & ~same):
        bad.append("x_out differs in %d samples that are exact by definition" % int((exact & ~same).sum()))
    worst = 0.0
    if fitted.any():
        if not np.all(np.isfinite(x_out.real[fitted]) & np.isfinite(x_out.imag[fitted])):
            bad.append("x_out is not finite in a fitted sample")
        share = err[fitted] / np.maximum(tol[fitted], 1e-300)
        worst = float(np.nanmax(share))
        if np.any(~(err[fitted] <= tol[fitted])):
            bad.append("model off by %.3g of its bound" % worst)
    filled = solved & ~kept if mode == "inpaint" else np.zeros_like(kept)
    wsame = w_out == ew.astype(np.float64)
    if np.any(~filled & ~wsame):
        bad.append("w_out differs in %d samples that are exact by definition" % int((~filled & ~wsame).sum()))
    if filled.any():
        werr = np.abs(w_out.astype(np.longdouble) - ew).astype(np.float64)
        wtol = np.broadcast_to(g, kept.shape) * ew.astype(np.float64)
        share = float(np.nanmax(werr[filled] / np.maximum(wtol[filled], 1e-300)))
        worst = max(worst, share)
        if np.any(~(werr[filled] <= wtol[filled])):
            bad.append("fill weight off by %.3g of its bound" % share)
    return bad, worst
