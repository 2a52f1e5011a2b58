"""Case tables, long-double residuals and derived error bounds for the batched Cholesky and the triangular solves
(driftscan_amd/csrc/dm_chol.hip).

Nothing here needs a GPU.  `POTRF_CASES`, `TRSM_CASES` and `INFO_CASES` list the problems, `potrf_layout` / `trsm_layout`
lay a list of them out in one NaN-poisoned host buffer each (in the given order, with gaps, with padded leading
dimensions), `check_potrf` / `check_trsm` compare result buffers with the exact conditions and the bounds, and
`run_potrf` / `run_trsm` send a layout through `Context.zpotrf_problems` / `Context.ztrsm_problems`.

Bounds (derived, nothing measured): componentwise backward errors in the style of the (2K + 8) 2^-53 bound of
gemm_cases.py.  Element (i, j) of a factor or of a solution closes an inner product of at most K = n complex terms,
2K fma-rounded real products per part, whose moduli |L| |L|^T (or |op(L)| |X|) bounds; the subtraction from A (or B)
and the division by the pivot — here a square root and a multiplication by a reciprocal, two roundings more than the
one of a division — add a constant number of roundings:

    factor:  |L^ L^^H - A|_ij    <= (2n + 10) 2^-53 (|L^| |L^|^T)_ij       on i >= j
    solve:   |op(L) X^ - B|_ij   <= (2n + 10) 2^-53 (|op(L)| |X^|)_ij      (upper_only: on i <= j)

The residuals are formed from the device's own result in np.longdouble (64-bit mantissa: their own rounding is 2^-11
of the bound).  With upper_only row i of the residual uses X^_kj with k <= i <= j only, the valid entries.

Exact conditions: the strictly upper triangle of a factor is 0, its diagonal real and positive, info == 0; everything
outside a problem's window (ld padding, rows beyond n, the gaps between problems, columns >= nrhs of B) keeps the bits
of its NaN poison; the strictly upper triangle of L handed to a solve is NaN (it is not to be read).
"""
import zlib

import numpy as np

from gemm_cases import LD, LD_OK, U  # noqa: F401  (LD_OK is re-exported for the test modules)

NB = 32
FAMILIES = ("wishart", "spec10", "spec14", "graded")
POTRF_N = (0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 193, 257)
LD_PADS = (0, 1, 7)
TRSM_N = (1, 31, 32, 33, 64, 65, 80, 96, 97, 128, 129, 200, 257, 385, 449)
TRSM_NRHS = (1, 63, 64, 255, 256, 257, 300)
TRSM_NRHS_N = (33, 97)          # every nrhs is run at these n
TRSM_BIG_N, TRSM_BIG_NRHS = 385, (1, 63, 64)   # from here on nrhs <= 64: the long-double residual stays cheap
TRSM_MIXED = ((449, 64), (80, 300), (200, 257), (64, 63), (1, 1))
TRSM_EMPTY = ((65, 33), (0, 5), (33, 0), (97, 64))
UPPER_N = (1, 33, 64, 65, 129, 257, 320)
UPPER_GRAM_N = 129              # this one takes B = (L^-1 A)^H, as dm_eigh_gen forms it
INFO_N = (1, 33, 65, 97, 130)
INFO_J = (0, 31, 32, 63, 64, 95, 96)   # and n - 1
GAP = 5                          # poisoned elements in front of every problem of a buffer
POISON = complex(np.nan, np.nan)


def factor_of(n):
    return (2 * n + 10) * U


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- matrix families -----------------------------------------------------------------------------------------------
def hpd(family, n):
    """The Hermitian positive definite matrix of a family at size n: exactly Hermitian, real diagonal."""
    rng = _rng("hpd", family, n)
    if n == 0:
        return np.zeros((0, 0), dtype=np.complex128)
    if family == "wishart":
        X = _crand(rng, n, n + 3)
        A = X @ X.conj().T + 0.1 * np.eye(n)
    elif family in ("spec10", "spec14"):
        Q, _ = np.linalg.qr(_crand(rng, n, n))
        A = (Q * np.logspace(0, -float(family[4:]), n)) @ Q.conj().T
    elif family == "graded":
        X = _crand(rng, n, n)
        D = np.logspace(6, -6, n)
        A = D[:, None] * (X @ X.conj().T / n + np.eye(n)) * D[None, :]
    else:
        raise ValueError(family)
    A = 0.5 * (A + A.conj().T)   # exact: the two sums commute, and a + conj(a) is real
    assert np.array_equal(A, A.conj().T) and not A.diagonal().imag.any()
    return A


_LCACHE = {}


def lower_of(family, n):
    """LAPACK's factor of hpd(family, n) (numpy.linalg.cholesky): the L of the solve cases, which are tested on their own
    and not through the device's factor.  Never written to."""
    if (family, n) not in _LCACHE:
        L = np.linalg.cholesky(hpd(family, n)) if n else np.zeros((0, 0), dtype=np.complex128)
        L.setflags(write=False)
        _LCACHE[(family, n)] = L
    return _LCACHE[(family, n)]


# ---- case tables ---------------------------------------------------------------------------------------------------
def potrf_case(family, n, pad, variant=None):
    """variant: None (the upper triangle mirrors the lower), 'nan_upper' (strictly upper triangle NaN), 'imag_diag'
    (the diagonal carries an imaginary part that is not to be read)."""
    return dict(kind="potrf", family=family, n=n, ld=n + pad, variant=variant, expect_info=0,
                name="potrf_%s_%d_ld%d%s" % (family, n, n + pad, "_" + variant if variant else ""))


POTRF_CASES = [potrf_case(f, n, pad) for f in FAMILIES for pad in LD_PADS for n in POTRF_N]


def potrf_group(family, pad, variant=None):
    return [potrf_case(family, n, pad, variant) for n in POTRF_N]


def mixed_order(cases):
    """The order of a mixed launch: a fixed shuffle that is not sorted by size."""
    perm = _rng("order", len(cases)).permutation(len(cases))
    return [cases[i] for i in perm]


def trsm_case(family, n, nrhs, conjtrans, padded, upper_only=False, gram=False):
    return dict(kind="trsm", family=family, n=n, nrhs=nrhs, conjtrans=conjtrans, upper_only=upper_only, gram=gram,
                ldl=n + (3 if padded else 0), ldb=nrhs + (5 if padded else 0),
                name="trsm_%s_%dx%d_%s%s%s" % (family, n, nrhs, "H" if conjtrans else "N", "_pad" if padded else "",
                                               "_upper" if upper_only else ""))


def _build_trsm():
    pairs = []
    for i, n in enumerate(TRSM_N):
        pool = TRSM_BIG_NRHS if n >= TRSM_BIG_N else TRSM_NRHS
        pairs += [(n, pool[i % len(pool)]), (n, pool[(i + 3) % len(pool)] if len(pool) > 3 else pool[(i + 1) % len(pool)])]
    pairs += [(n, r) for n in TRSM_NRHS_N for r in TRSM_NRHS]
    pairs = sorted(set(pairs))
    out = []
    for conj in (False, True):
        for i, (n, r) in enumerate(pairs):
            out.append(trsm_case(FAMILIES[(i + conj) % 4], n, r, conj, padded=(i + conj) % 2 == 1))
    return out


TRSM_CASES = _build_trsm()


def trsm_mixed(conjtrans):
    """{449, 80, 200, 64, 1} in one launch: the backward launch starts the small problems late, and 80 and 200 have an
    odd number of 32-row blocks."""
    return [trsm_case(FAMILIES[i % 4], n, r, conjtrans, padded=i % 2 == 0) for i, (n, r) in enumerate(TRSM_MIXED)]


def trsm_empty(conjtrans):
    """One n = 0 and one nrhs = 0 member among non-empty ones."""
    return [trsm_case(FAMILIES[(i + 1) % 4], n, r, conjtrans, padded=i % 2 == 1) for i, (n, r) in enumerate(TRSM_EMPTY)]


UPPER_CASES = [trsm_case(FAMILIES[i % 4], n, n, False, padded=i % 2 == 1, upper_only=True, gram=n == UPPER_GRAM_N)
               for i, n in enumerate(UPPER_N)]


def info_matrix(n, kind, i, j):
    """(A, expected info).  kind 'pivot': A0 = L0 L0^H with the diagonal of L0 in [1, 2) and A[j, j] -= 2 L0[j, j]^2, so
    that the pivot at j is -L0[j, j]^2; 'zero': the zero matrix; 'nan': A0 with a NaN at (i, j), i > j; 'inf': A0 with
    +Inf on the diagonal at j."""
    rng = _rng("info", n)
    L0 = np.tril(_crand(rng, n, n), -1) / np.sqrt(2.0 * max(n, 1))
    L0[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    A = L0 @ L0.conj().T
    A = 0.5 * (A + A.conj().T)
    if kind == "pivot":
        A[j, j] -= 2.0 * L0[j, j].real ** 2
        return A, j + 1
    if kind == "zero":
        return np.zeros_like(A), 1
    if kind == "nan":
        assert i > j
        A[i, j] = A[j, i] = POISON
        return A, i + 1
    if kind == "inf":
        A[j, j] = np.inf
        return A, j + 1
    raise ValueError(kind)


def info_case(n, kind, i=0, j=0, pad=0):
    return dict(kind="info", n=n, ld=n + pad, what=kind, i=i, j=j, variant=None,
                expect_info=info_matrix(n, kind, i, j)[1], name="info_%s_%d_%d_%d" % (kind, n, i, j))


def _build_info():
    out = []
    for k, n in enumerate(INFO_N):
        for j in sorted({jj for jj in INFO_J if jj < n} | {n - 1}):
            out.append(info_case(n, "pivot", j=j, pad=(k + j) % 2))
    out += [info_case(33, "zero"), info_case(1, "zero"), info_case(97, "zero", pad=1),
            info_case(33, "nan", 20, 5), info_case(65, "nan", 40, 3, pad=1), info_case(130, "nan", 100, 70),
            info_case(130, "nan", 129, 0), info_case(65, "inf", j=0), info_case(65, "inf", j=40, pad=7),
            info_case(130, "inf", j=129)]
    return out


INFO_CASES = _build_info()


def case_matrix(c):
    """The full Hermitian input of a potrf or info case (before its variant is applied)."""
    if c["kind"] == "info":
        return info_matrix(c["n"], c["what"], c["i"], c["j"])[0]
    return hpd(c["family"], c["n"])


# ---- layouts -------------------------------------------------------------------------------------------------------
class Layout(object):
    """cases, the poisoned host buffer(s), and per problem the element offset and the integer index array of its window."""


def _window(off, rows, cols, ld):
    return off + np.arange(rows)[:, None] * ld + np.arange(cols)[None, :]


def _place(sizes):
    """Offsets of windows of (rows, cols, ld) in one buffer: GAP poisoned elements in front of each, two poisoned rows
    behind each; returns (offsets, total)."""
    offs, at = [], 0
    for rows, cols, ld in sizes:
        at += GAP
        offs.append(at)
        at += (rows + 2) * ld + GAP
    return offs, at + GAP


def potrf_layout(cases):
    lay = Layout()
    lay.cases = list(cases)
    lay.off, total = _place([(c["n"], c["n"], c["ld"]) for c in cases])
    lay.buf = np.full(total, POISON, dtype=np.complex128)
    lay.win, lay.A = [], []
    for c, off in zip(cases, lay.off):
        n = c["n"]
        A = case_matrix(c)
        w = _window(off, n, n, c["ld"])
        V = A.copy()
        if c["variant"] == "nan_upper":
            V[np.triu_indices(n, 1)] = POISON
        elif c["variant"] == "imag_diag":
            V[np.arange(n), np.arange(n)] += 1j * (0.37 + np.arange(n))
        lay.buf[w] = V
        lay.win.append(w)
        lay.A.append(A)
    lay.in_window = np.zeros(total, dtype=bool)
    for w in lay.win:
        lay.in_window[w] = True
    return lay


def potrf_problems(lay):
    return [dict(n=c["n"], ld=c["ld"], a_off=off) for c, off in zip(lay.cases, lay.off)]


def trsm_rhs(c):
    """The right-hand sides of a solve case (n x nrhs)."""
    n, nrhs = c["n"], c["nrhs"]
    if c["gram"]:   # B = (L^-1 A)^H with A Hermitian, what the second solve of dm_eigh_gen is handed
        import scipy.linalg

        rng = _rng("gram", c["name"])
        S = _crand(rng, n, n)
        S = 0.5 * (S + S.conj().T)
        return np.ascontiguousarray(scipy.linalg.solve_triangular(lower_of(c["family"], n), S, lower=True).conj().T)
    return _crand(_rng("rhs", c["name"]), n, nrhs)


def trsm_layout(cases):
    """L_buf holds every L with its strictly upper triangle NaN, B_buf every right-hand side."""
    lay = Layout()
    lay.cases = list(cases)
    lay.l_off, nl = _place([(c["n"], c["n"], c["ldl"]) for c in cases])
    lay.b_off, nb = _place([(c["n"], c["nrhs"], c["ldb"]) for c in cases])
    lay.L_buf = np.full(nl, POISON, dtype=np.complex128)
    lay.B_buf = np.full(nb, POISON, dtype=np.complex128)
    lay.wL, lay.wB, lay.L, lay.B = [], [], [], []
    for c, lo, bo in zip(cases, lay.l_off, lay.b_off):
        n = c["n"]
        L, B = lower_of(c["family"], n), trsm_rhs(c)
        wl, wb = _window(lo, n, n, c["ldl"]), _window(bo, n, c["nrhs"], c["ldb"])
        V = L.copy()
        V[np.triu_indices(n, 1)] = POISON
        lay.L_buf[wl] = V
        lay.B_buf[wb] = B
        lay.wL.append(wl); lay.wB.append(wb); lay.L.append(L); lay.B.append(B)
    lay.in_window = np.zeros(nb, dtype=bool)
    for w in lay.wB:
        lay.in_window[w] = True
    return lay


def trsm_problems(lay):
    return [dict(n=c["n"], nrhs=c["nrhs"], ldl=c["ldl"], ldb=c["ldb"], l_off=lo, b_off=bo)
            for c, lo, bo in zip(lay.cases, lay.l_off, lay.b_off)]


# ---- checks ---------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1, 2)


def outside_changed(before, after, in_window):
    """Number of elements outside every window whose bits changed."""
    return int(((_bits(before) != _bits(after)).any(axis=1) & ~in_window).sum())


def _split(a):
    return np.ascontiguousarray(a.real).astype(LD), np.ascontiguousarray(a.imag).astype(LD)


_MEMO = {}


def _memo(key, arr, fn):
    """fn() once per (key, bits of arr): a launch that reproduces a result bit for bit is not measured again."""
    k = (key, zlib.crc32(np.ascontiguousarray(arr).tobytes()), arr.shape)
    if k not in _MEMO:
        _MEMO[k] = fn()
    return _MEMO[k]


def factor_residual(A, Lh):
    """(failures, worst ratio to the bound) of a candidate factor Lh of the Hermitian A (its lower triangle and the real
    part of its diagonal are the input)."""
    n = A.shape[0]
    fails = []
    if n == 0:
        return fails, 0.0
    if np.triu(Lh, 1).real.any() or np.triu(Lh, 1).imag.any() or np.isnan(np.triu(Lh, 1)).any():
        fails.append("the strictly upper triangle is not exactly 0")
    d = Lh.diagonal()
    if d.imag.any() or not (d.real > 0.0).all():
        fails.append("the diagonal is not real and positive")
    Lt = np.tril(Lh)
    if not np.isfinite(Lt.real).all() or not np.isfinite(Lt.imag).all():
        return fails + ["the factor is not finite"], np.inf
    lr, li = _split(Lt)
    ar, ai = _split(np.tril(A))
    ai[np.arange(n), np.arange(n)] = 0
    rr = lr @ lr.T + li @ li.T - ar
    ri = li @ lr.T - lr @ li.T - ai
    absl = np.abs(Lt).astype(LD)
    bound = factor_of(n) * (absl @ absl.T)
    low = np.tril(np.ones((n, n), dtype=bool))
    err = np.hypot(rr, ri)
    bad = ~(err <= bound) & low
    ratio = float(np.max(np.where(low & (bound > 0), err / np.where(bound > 0, bound, 1), 0)))
    if bad.any():
        i, j = (int(x[0]) for x in np.nonzero(bad))
        fails.append("%d of %d elements outside the bound, first (%d, %d): |res| %.3e, bound %.3e"
                     % (bad.sum(), low.sum(), i, j, float(err[i, j]), float(bound[i, j])))
    return fails, ratio


def solve_residual(L, B, Xh, conjtrans, upper_only=False):
    """(failures, worst ratio to the bound) of a candidate solution Xh of op(L) X = B."""
    n, nrhs = B.shape
    if n == 0 or nrhs == 0:
        return [], 0.0
    M = np.tril(L).copy()
    M[np.arange(n), np.arange(n)] = M.diagonal().real
    if conjtrans:
        M = M.conj().T
    mask = np.ones((n, nrhs), dtype=bool)
    X = Xh
    if upper_only:
        mask = np.triu(mask)
        X = np.triu(Xh)   # what lies below the diagonal is undefined and enters no residual on or above it
    if not (np.isfinite(X.real).all() and np.isfinite(X.imag).all()):
        return ["the solution is not finite"], np.inf
    mr, mi = _split(M)
    xr, xi = _split(X)
    br, bi = _split(B)
    rr = mr @ xr - mi @ xi - br
    ri = mr @ xi + mi @ xr - bi
    bound = factor_of(n) * (np.abs(M).astype(LD) @ np.abs(X).astype(LD))
    err = np.hypot(rr, ri)
    bad = ~(err <= bound) & mask
    ratio = float(np.max(np.where(mask & (bound > 0), err / np.where(bound > 0, bound, 1), 0)))
    fails = []
    if bad.any():
        i, j = (int(x[0]) for x in np.nonzero(bad))
        fails.append("%d of %d elements outside the bound, first (%d, %d): |res| %.3e, bound %.3e"
                     % (bad.sum(), mask.sum(), i, j, float(err[i, j]), float(bound[i, j])))
    return fails, ratio


def check_potrf(lay, out, info):
    """(failures, worst ratio) of the result buffer and the info array of a factorisation launch."""
    fails, worst = [], 0.0
    if out.shape != lay.buf.shape:
        return ["buffer shape changed"], np.inf
    moved = outside_changed(lay.buf, out, lay.in_window)
    if moved:
        fails.append("%d elements outside the windows changed" % moved)
    for k, c in enumerate(lay.cases):
        if int(info[k]) != c["expect_info"]:
            fails.append("%s: info %d, expected %d" % (c["name"], int(info[k]), c["expect_info"]))
        if c["expect_info"] != 0:
            continue
        Lh = out[lay.win[k]]
        f, r = _memo(("potrf", c["kind"], c.get("family"), c["n"]), Lh, lambda: factor_residual(lay.A[k], Lh))
        fails += ["%s: %s" % (c["name"], x) for x in f]
        worst = max(worst, r)
    return fails, worst


def check_trsm(lay, out):
    """(failures, worst ratio) of the result buffer of B of a solve launch."""
    fails, worst = [], 0.0
    if out.shape != lay.B_buf.shape:
        return ["buffer shape changed"], np.inf
    moved = outside_changed(lay.B_buf, out, lay.in_window)
    if moved:
        fails.append("%d elements outside the windows of B changed" % moved)
    for k, c in enumerate(lay.cases):
        Xh = out[lay.wB[k]]
        f, r = _memo(("trsm", c["name"]), Xh,
                     lambda: solve_residual(lay.L[k], lay.B[k], Xh, c["conjtrans"], c["upper_only"]))
        fails += ["%s: %s" % (c["name"], x) for x in f]
        worst = max(worst, r)
    return fails, worst


# ---- device glue ---------------------------------------------------------------------------------------------------
def run_potrf(ctx, lay):
    """One `zpotrf_problems` call for the whole layout on a fresh device copy; (result buffer on the host, info)."""
    dA = ctx.to_device(lay.buf)
    info = ctx.zpotrf_problems([dict(p, A=dA) for p in potrf_problems(lay)])
    return dA.cpu().numpy(), info


def run_trsm(ctx, lay, conjtrans, upper_only=False):
    """One `ztrsm_problems` call for the whole layout on fresh device copies; the result buffer of B on the host."""
    dL, dB = ctx.to_device(lay.L_buf), ctx.to_device(lay.B_buf)
    ctx.ztrsm_problems([dict(p, L=dL, B=dB) for p in trsm_problems(lay)], conjtrans=conjtrans, upper_only=upper_only)
    ctx.sync()
    assert np.array_equal(_bits(dL.cpu().numpy()), _bits(lay.L_buf)), "L was written to"
    return dB.cpu().numpy()
