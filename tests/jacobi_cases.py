"""Inputs, a float64 reference solver and the contract of the one-sided row-Jacobi engine (`dm_jacobi_rows`), numpy only.

What the engine is held to is `check_rows_result`: conditions a to f of DESIGN.md section 4.2 ("what the engine
promises").  `hestenes_rows` is a textbook Hestenes one-sided Jacobi in float64, the reference solver of the same
accuracy class (scipy here exposes neither zgesvj nor dgesvj): tests/test_host_jacobi_cases.py holds it to the same
contract on the CPU, tests/test_gpu_jacobi_rows.py holds the device to it.
TEST INFRASTRUCTURE — never imported by the product."""
import os

import numpy as np

U = 1.11e-16                         # unit roundoff of float64
EPS = 2.220446049250313e-16
FLOOR = 2.0 * (4.0 * EPS) ** 2       # x max_i |a_i|^2: the engine's noise floor (jac_rows_setup), doubled
GUARD = 4096                         # sentinel elements in front of and behind a packed buffer
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "jacobi_exact.npz")


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _unitary(rng, n, k):
    """n x k with orthonormal columns."""
    return np.linalg.qr(crand(rng, n, k))[0]


# ---- generators: seeded, complex128 (rows x cols) -------------------------------------------------------------------
def graded(rows, cols, decades, seed=0):
    """D B: B with unit-norm random rows, D = 10^(-decades perm / (rows - 1)) — the rows graded over `decades`, shuffled."""
    rng = np.random.default_rng([1, rows, cols, int(decades * 8), seed])
    B = crand(rng, rows, cols)
    B /= np.linalg.norm(B, axis=1, keepdims=True)
    D = 10.0 ** (-decades * rng.permutation(rows) / max(rows - 1, 1))
    return D[:, None] * B


def smooth_deficient(rows, cols, decades, rank, seed=0):
    """U diag(s) V^H of the given rank, s = 10^linspace(0, -decades): the wide-dynamic-range block of test_gpu_svdkl."""
    rng = np.random.default_rng([2, rows, cols, int(decades * 8), rank, seed])
    u, v = _unitary(rng, rows, rank), _unitary(rng, cols, rank)
    return (u * 10.0 ** np.linspace(0.0, -decades, rank)) @ v.conj().T


def clustered(rows, cols, group=7, decades=9, seed=0):
    """Singular values in groups of `group` exactly equal values, the groups spread over `decades`."""
    rng = np.random.default_rng([3, rows, cols, group, decades, seed])
    k = min(rows, cols)
    ng = (k + group - 1) // group
    s = np.repeat(10.0 ** (-decades * np.arange(ng) / max(ng - 1, 1)), group)[:k]
    return (_unitary(rng, rows, k) * s) @ _unitary(rng, cols, k).conj().T


def orthogonal_rows(rows, cols, decades=6, seed=0):
    """D Q, Q from a QR: rows that are orthogonal already (to rounding), graded and shuffled."""
    rng = np.random.default_rng([4, rows, cols, int(decades * 8), seed])
    Q = _unitary(rng, cols, rows).T
    D = 10.0 ** (-decades * rng.permutation(rows) / max(rows - 1, 1))
    return D[:, None] * Q


def with_zero_rows(rows, cols, nzero, rank=None, seed=0):
    """Random rows of rank `rank` (None: full), `nzero` of them exactly zero."""
    rng = np.random.default_rng([5, rows, cols, nzero, rank or 0, seed])
    A = crand(rng, rows, cols) if rank is None else crand(rng, rows, rank) @ crand(rng, rank, cols)
    A[rng.permutation(rows)[:nzero]] = 0.0
    return A


def duplicate_rows(rows, cols, seed=0):
    """Rank 1: every row the same vector, half of them with a factor of their own."""
    rng = np.random.default_rng([6, rows, cols, seed])
    f = np.ones(rows, dtype=np.complex128)
    f[rows // 2:] = crand(rng, rows - rows // 2)
    return f[:, None] * crand(rng, 1, cols)


def gapped(rows, cols, cut, gap_decades, seed=0):
    """A spectrum from 1 down to 1e-4 cut with an empty band of `gap_decades` centred (in the logarithm) on cut * sigma_0:
    half of the values above the band, half below."""
    rng = np.random.default_rng([7, rows, cols, int(-np.log10(cut) * 8), int(gap_decades * 8), seed])
    k = min(rows, cols)
    lc, h = np.log10(cut), 0.5 * gap_decades
    s = 10.0 ** np.concatenate([np.linspace(0.0, lc + h, k // 2), np.linspace(lc - h, lc - 4.0, k - k // 2)])
    return (_unitary(rng, rows, k) * s) @ _unitary(rng, cols, k).conj().T


FAMILIES = dict(graded=graded, smooth_deficient=smooth_deficient, clustered=clustered, orthogonal_rows=orthogonal_rows,
                with_zero_rows=with_zero_rows, duplicate_rows=duplicate_rows, gapped=gapped)


def make(family, args):
    return FAMILIES[family](*args)


# The ragged batch of tests/test_gpu_jacobi_rows.py (group ii): (nrows, acols, row0, ld - ncols, gc0, gc1) of problems that go
# to the engine in ONE call; ncols = acols + nrows runs from 40 to 300.  A = graded(nrows, acols, 3, 100 + nrows).
RAGGED = ((0, 40, 7, 1, 0, 40), (1, 45, 0, 5, 3, 20), (2, 60, 32, 0, 10, 11), (31, 50, 7, 1, 5, 21), (32, 40, 0, 0, 0, 40),
          (33, 70, 32, 5, 3, 20), (63, 64, 7, 0, 10, 11), (64, 100, 32, 1, 5, 21), (65, 90, 0, 5, 0, 90),
          (97, 120, 7, 5, 3, 20), (130, 170, 32, 1, 0, 170))


def ragged_case(k):
    n, acols, _, _, gc0, gc1 = RAGGED[k]
    return ("graded", (n, acols, 3, 100 + n), gc0, gc1)


# The cases with an exact spectrum in tests/golden/jacobi_exact.npz (at most 96 rows): (family, args, gc0, gc1), gc1 = None
# for all columns.  tests/gen_golden_jacobi.py evaluates them; the tests look them up with `exact_sigma`.
EXACT_CASES = (
    [("graded", (r, c, d, seed), 0, None) for r, c, d in ((48, 64, 8), (96, 128, 12), (70, 30, 6)) for seed in (0, 1, 2)]
    + [("orthogonal_rows", (70, 90), 0, None), ("clustered", (70, 90), 0, None), ("with_zero_rows", (70, 90, 20), 0, None),
       ("with_zero_rows", (70, 90, 20, 1), 0, None), ("duplicate_rows", (70, 90), 0, None), ("gapped", (60, 80, 1e-4, 2), 0, None)]
    + [ragged_case(k) for k in range(len(RAGGED)) if 1 <= RAGGED[k][0] <= 96])


def case_key(family, args, gc0, gc1):
    return "%s%r[%d:%s]" % (family, tuple(args), gc0, "" if gc1 is None else gc1)


_golden = None


def exact_sigma(family, args, gc0=0, gc1=None):
    """(s_ref float64 descending, e_ref) of a fixture case."""
    global _golden
    if _golden is None:
        g = np.load(GOLDEN)
        keys = [str(k) for k in g["keys"]]
        _golden = ({k: g["s_ref"][g["off"][i]:g["off"][i + 1]] for i, k in enumerate(keys)}, float(g["e_ref"]))
    return _golden[0][case_key(family, args, gc0, gc1)], _golden[1]


# ---- the float64 reference solver ------------------------------------------------------------------------------------
def hestenes_rows(Z, gc0, gc1, tol=1e-15, max_sweeps=60):
    """Textbook Hestenes one-sided Jacobi on the rows of Z (n x ncols, a copy is returned): the pairs (i, j > i) of a
    row-cyclic sweep are rotated, until a sweep finds every cosine over the columns [gc0, gc1) <= tol.  Norms and inner
    product are taken afresh from the rows each time: that is what keeps the small rows accurate to their own size.  A
    rotation leaves the larger row of its pair on top (de Rijk): the rows sort themselves while they converge, 14 sweeps
    instead of 24 on a clustered spectrum, and as much less rounding.  Pairs whose inner product is below the noise floor
    (4 eps)^2 max_i |a_i|^2 — the residue rows of a rank-deficient input, more of them than dimensions left — are left
    alone.  Rows come back sorted by descending norm.  Returns (Z, sigma, sweeps that rotated)."""
    Z = np.array(Z, dtype=np.complex128)
    n = Z.shape[0]
    G = slice(gc0, gc1)
    floor = 0.5 * FLOOR * (np.abs(Z[:, G]) ** 2).sum(axis=1).max(initial=0.0)
    for sweeps in range(max_sweeps + 1):
        rotated = False
        for i in range(n - 1):
            for j in range(i + 1, n):
                x, y = Z[i], Z[j]
                xg, yg = x[G], y[G]
                # (numpy's own pairwise sums, not BLAS dot products: the same bits on every CPU)
                a, b = (xg.real ** 2 + xg.imag ** 2).sum(), (yg.real ** 2 + yg.imag ** 2).sum()
                g = (xg * yg.conj()).sum()
                ga = abs(g)
                if ga <= tol * np.sqrt(a * b) or ga <= floor:
                    continue
                rotated = True
                y = y * (g / ga)                                # <x, y> real and positive
                zeta = (b - a) / (2.0 * ga)
                t = (1.0 if zeta >= 0 else -1.0) / (abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                Z[i], Z[j] = (c * x - s * y, s * x + c * y) if a >= b else (s * x + c * y, c * x - s * y)
        if not rotated:
            break
    sig = np.sqrt((np.abs(Z[:, G]) ** 2).sum(axis=1))
    order = np.argsort(-sig, kind="stable")
    return Z[order], sig[order], sweeps


# ---- packed, guarded buffers -----------------------------------------------------------------------------------------
def pack(items, guard=GUARD, gap=17, below=2):
    """One flat complex128 buffer of NaN sentinels that holds every problem's Z = [A | I] (the identity in the LAST nrows
    columns; the columns of A outside the Gram range are passengers too): items are dicts with A (nrows x acols), and
    optionally row0 (sentinel rows above), ldx (ld - ncols), gc0, gc1 (default: all of A).  `below` sentinel rows follow
    each matrix, `gap` elements separate two matrices.  Returns (buffer, problems): dicts with off, ld, row0, nrows, ncols, gc0,
    gc1, acols — what `Context.jacobi_rows_problems` and `check_rows_result` take."""
    probs, chunks, pos = [], [], guard
    chunks.append(np.full(guard, np.nan + 1j * np.nan, dtype=np.complex128))
    for it in items:
        A = np.asarray(it["A"], dtype=np.complex128)
        nrows, acols = A.shape
        ncols = acols + nrows
        ld, row0 = ncols + int(it.get("ldx", 0)), int(it.get("row0", 0))
        M = np.full((row0 + nrows + below, ld), np.nan + 1j * np.nan, dtype=np.complex128)
        M[row0:row0 + nrows, :acols] = A
        M[row0:row0 + nrows, acols:ncols] = np.eye(nrows)
        gc1 = it.get("gc1")
        probs.append(dict(off=pos, ld=ld, row0=row0, nrows=nrows, ncols=ncols, gc0=int(it.get("gc0", 0)),
                          gc1=acols if gc1 is None else int(gc1), acols=acols))
        chunks += [M.reshape(-1), np.full(gap, np.nan + 1j * np.nan, dtype=np.complex128)]
        pos += M.size + gap
    chunks.append(np.full(guard, np.nan + 1j * np.nan, dtype=np.complex128))
    return np.concatenate(chunks), probs


def region(buf, prob):
    """The (nrows x ncols) block of a problem inside a packed buffer (a copy)."""
    o, ld = prob["off"] + prob["row0"] * prob["ld"], prob["ld"]
    idx = o + ld * np.arange(prob["nrows"])[:, None] + np.arange(prob["ncols"])[None, :]
    return buf[idx.reshape(-1)].reshape(prob["nrows"], prob["ncols"])


def put(buf, prob, M):
    """Write the (nrows x ncols) block of a problem into a packed buffer."""
    o, ld = prob["off"] + prob["row0"] * prob["ld"], prob["ld"]
    idx = o + ld * np.arange(prob["nrows"])[:, None] + np.arange(prob["ncols"])[None, :]
    buf[idx.reshape(-1)] = np.asarray(M).reshape(-1)


def check_guards(Zin, Zout, probs):
    """f: every element outside rows [row0, row0 + nrows) x columns [0, ncols) of the problems is bit-identical to what was
    uploaded — the rows above and below, the ld slack, the gaps between problems, the guards."""
    assert Zin.shape == Zout.shape and Zin.dtype == Zout.dtype == np.complex128
    fixed = np.ones(Zin.size, dtype=bool)
    for p in probs:
        o = p["off"] + p["row0"] * p["ld"]
        idx = o + p["ld"] * np.arange(p["nrows"])[:, None] + np.arange(p["ncols"])[None, :]
        fixed[idx.reshape(-1)] = False
    a, b = Zin.view(np.uint64).reshape(-1, 2)[fixed], Zout.view(np.uint64).reshape(-1, 2)[fixed]
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, "f: %d elements outside the problems were overwritten, the first at %d" % (
        bad.size, np.flatnonzero(fixed)[bad[0]])
    return 0.0


def simulate(Zin, probs, solver=hestenes_rows):
    """What a correct engine hands back for a packed buffer, by the reference solver: (Zout, sigma list, sweeps)."""
    Zout, sig, sw = Zin.copy(), [], 0
    for p in probs:
        Y, s, k = solver(region(Zin, p), p["gc0"], p["gc1"])
        put(Zout, p, Y)
        sig.append(s)
        sw = max(sw, k)
    return Zout, sig, sw


def old_absolute_check(Y):
    """The orthogonality test of test_jacobi_rows before the contract: |G_ij| <= 1e-11 sigma_0^2."""
    G = Y @ Y.conj().T
    return np.abs(G - np.diag(np.diag(G))).max() / (1e-11 * np.abs(np.diag(G)).max())


# ---- the contract ----------------------------------------------------------------------------------------------------
def check_rows_result(A, Zin, Zout, sigma, prob, sweeps, opts=None, others=(), s_ref=None, e_ref=None, parts=None):
    """Conditions a to f on one problem of a packed buffer.  A: the (nrows x acols) input left of the identity; Zin / Zout:
    the buffer as uploaded / as downloaded; sigma: the problem's reported norms; prob: its descriptor (`pack`); opts: the
    engine's options (dict); others: the other problems of the same buffer (for f).  s_ref / e_ref: an exact spectrum and
    numpy's own worst error on the fixture (`exact_sigma`); without them e is held to numpy.linalg.svd at 1e-12 sigma_0.
    parts: the conditions to ASSERT (all are measured); default "abcdef", without c and e for a subspace split that no
    sweep ordered (subspace_cut > 0 and sweeps == 0: the rows are not singular vectors then, only split at the cut).
    Returns the measured ratios value / bound per condition (<= 1 passes)."""
    opts = dict(opts or {})
    if parts is None:
        parts = "abdf" if opts.get("subspace_cut", 0.0) > 0.0 and sweeps == 0 else "abcdef"
    n, ncols, acols, gc0, gc1 = prob["nrows"], prob["ncols"], prob["acols"], prob["gc0"], prob["gc1"]
    A = np.asarray(A, dtype=np.complex128).reshape(n, acols)
    sigma = np.asarray(sigma, dtype=np.float64)[:n]
    r = {}
    assert sweeps >= 0
    zi, zo = region(Zin, prob), region(Zout, prob)
    has_w = acols < ncols        # (a buffer without the identity columns, acols == ncols, has no W: a and b are not measured)
    assert np.array_equal(zi[:, :acols], A) and (not has_w or np.array_equal(zi[:, acols:], np.eye(n))), \
        "the buffer does not hold [A | I]"
    assert np.isfinite(zo.view(np.float64)).all() and np.isfinite(sigma).all(), "NaN or Inf in the result"
    Y, W = zo[:, :acols], zo[:, acols:]
    YG = Y[:, gc0:gc1]
    r["a"] = r["b"] = 0.0
    if has_w:
        # a. unitarity
        r["a"] = np.abs(W @ W.conj().T - np.eye(n)).max(initial=0.0) / 1e-12
        # b. backward error over every carried column
        a2 = np.linalg.norm(A, 2) if A.size else 0.0
        r["b"] = np.abs(W @ A - Y).max(initial=0.0) / (1e-11 * a2) if a2 > 0.0 else float(np.abs(Y).max(initial=0.0) > 0.0)
    # c. relative orthogonality, the Gram matrix in extended precision (a float64 Gram carries K u of its own)
    K = gc1 - gc0
    tol = max(1e-13, K * U)
    yl = YG.astype(np.clongdouble)
    g = yl @ yl.conj().T
    d = np.real(np.diag(g)).astype(np.float64)
    s0sq = d.max(initial=0.0)
    floor = FLOOR * (np.abs(A[:, gc0:gc1]) ** 2).sum(axis=1).max(initial=0.0)
    rel = 4.0 * tol * np.sqrt(np.outer(d, d))
    bound = np.maximum(rel, floor)
    drop = float(opts.get("drop_below", 0.0))
    if drop > 0.0:
        low = np.sqrt(d) < drop * np.sqrt(s0sq)
        bound = np.where(low[:, None] | low[None, :], 1e-11 * s0sq, bound)
    off = np.abs(g).astype(np.float64)
    np.fill_diagonal(off, 0.0)
    np.fill_diagonal(bound, 1.0)
    ratio = np.where(off > 0.0, off / np.where(bound > 0.0, bound, np.finfo(float).tiny), 0.0)
    r["c"] = ratio.max(initial=0.0)
    with np.errstate(divide="ignore"):      # (how far the floor term reaches above the relative one: > 1 where residue rows are)
        r["c_floor_over_rel"] = (floor / rel[~np.eye(n, dtype=bool)]).max(initial=0.0) if s0sq > 0.0 and n > 1 else 0.0
    # d. the reported norms: descending, the row norms of Y_G
    nrm = np.sqrt(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        r["d"] = np.where(nrm > 0.0, np.abs(sigma - nrm) / (1e-14 * nrm), np.where(sigma == 0.0, 0.0, np.inf)).max(initial=0.0)
    descending = bool((np.diff(sigma) <= 0.0).all())
    # e. singular values, absolutely
    k = min(n, K)
    s_np = np.zeros(n)
    if k:
        s_np[:k] = np.linalg.svd(A[:, gc0:gc1], compute_uv=False)
    s0 = s_np[0] if n else 0.0
    if drop > 0.0:
        # Weyl: leaving rows out of the sweeps moves the other singular values by at most their Frobenius norm
        fro = np.sqrt((nrm[nrm < drop * nrm.max(initial=0.0)] ** 2).sum())
        big = sigma > 1e-10 * s0
        r["e"] = (np.abs(sigma - s_np)[big] / (1e-12 * s0 + fro)).max(initial=0.0) if s0 > 0.0 else 0.0
    elif s_ref is not None:
        ref = np.zeros(n)
        ref[:len(s_ref)] = s_ref
        r["e"] = np.abs(sigma - ref).max(initial=0.0) / (8.0 * e_ref * s0) if s0 > 0.0 else float(np.abs(sigma).max(initial=0.0) > 0)
    else:
        r["e"] = np.abs(sigma - s_np).max(initial=0.0) / (1e-12 * s0) if s0 > 0.0 else float(np.abs(sigma).max(initial=0.0) > 0)
    # f. nothing outside the problems was written
    if "f" in parts:
        r["f"] = check_guards(Zin, Zout, [prob] + list(others))
    for p in "abcde":
        if p in parts:
            assert r[p] <= 1.0, "%s: %.3g times the bound (%r, opts %r, sweeps %d)" % (p, r[p], {
                k_: v for k_, v in prob.items() if k_ != "off"}, opts, sweeps)
    if "d" in parts:
        assert descending, "d: sigma is not descending"
    return r
