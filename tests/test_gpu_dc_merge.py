"""The merge kernels of the tridiagonal divide & conquer (dc_setup, dc_secular, dc_zhat, dc_ubuild) at the sizes where their
code changes path and at the extremes of the deflation, through `Context.herm_eig` / `Context.eigh_gen`.

The inputs are real symmetric tridiagonal matrices handed in as Hermitian ones: the reductions leave them as they are up
to the signs of the off-diagonals, so the tree of the D&C is known on the host.  A matrix of n rows has depth D, the
smallest D with ceil(n / 2^D) <= 32, its node j of level l covers the rows [bound(l, j), bound(l, j + 1)) with
bound(l, i) = (i n) >> l, and is torn between the rows mid - 1 and mid, mid = bound(l + 1, 2 j + 1): the off-diagonal
element e[mid - 1].

Eigenvalues against numpy.linalg.eigvalsh (1e-13 of the norm), eigenvectors against the matrix with the bounds of
eig_cases.py (LAPACK's own ratios on the tables of test_gpu_eigensolver.py).
"""
import functools

import numpy as np
import pytest

import eig_cases as ec
import test_gpu_eigensolver as te

LEAF = 32
SMALL_NS = (33, 34, 63, 64, 65)              # root sizes around one wave of roots and the lane groups
PANEL_NS = (255, 256, 257, 513, 1025)        # ... around the 256-root tile, two and four of them
PANEL_ROUTES = ("two_pos", "one32")
DEFL_SIZES = (("small", 64), ("two_pos", 200), ("one32", 200))
KEEP = (0, 1, 16, 17)                        # and n - 1, n


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 30)
    yield c
    c.close()


# ---- the tree ------------------------------------------------------------------------------------------------------------
def depth(n):
    D = 0
    while ((n + (1 << D) - 1) >> D) > LEAF:
        D += 1
    return D


def bound(n, l, i):
    return (i * n) >> l


def tear(n, l, j):
    """Row `mid` of node j of level l: the node is torn at the off-diagonal element e[mid - 1]."""
    return bound(n, l + 1, 2 * j + 1)


def all_tears(n):
    return sorted({tear(n, l, j) for l in range(depth(n)) for j in range(1 << l)})


# ---- matrices ------------------------------------------------------------------------------------------------------------
def tridiag(d, e):
    d, e = np.asarray(d, dtype=np.float64), np.asarray(e, dtype=np.float64)
    C = (np.diag(d) + np.diag(e, 1) + np.diag(e, -1)).astype(np.complex128)
    C.setflags(write=False)
    return C


def _random_de(n, seed):
    rng = np.random.default_rng([7, n, seed])
    return rng.uniform(-1.0, 1.0, n), rng.uniform(0.25, 1.0, max(n - 1, 0))


@functools.lru_cache(maxsize=None)
def toeplitz121(n):
    return tridiag(2.0 * np.ones(n), np.ones(n - 1))


@functools.lru_cache(maxsize=None)
def random_tridiag(n, seed=0):
    return tridiag(*_random_de(n, seed))


@functools.lru_cache(maxsize=None)
def tear_zero(n, l, j, seed=0):
    """A random tridiagonal whose off-diagonal element at the tear of node (l, j) is zero: rho = 0 there, the whole node
    deflates (k = 0)."""
    d, e = _random_de(n, seed)
    e[tear(n, l, j) - 1] = 0.0
    return tridiag(d, e)


@functools.lru_cache(maxsize=None)
def constant_diagonal(n, eps):
    """d = 1, couplings eps (1 +- 1/4): at eps ~ 1e-14 the poles of a node lie within a few ulp of each other while the
    weights are not small, so the close-pole test passes pair after pair (chains of rotations)."""
    return tridiag(np.ones(n), eps * (1.0 + 0.25 * np.cos(np.arange(n - 1))))


@functools.lru_cache(maxsize=None)
def tiny_couplings(n):
    """diag(1 .. n) with off-diagonals 1e-20: every weight is tiny."""
    return tridiag(np.arange(1.0, n + 1.0), 1e-20 * np.ones(n - 1))


def k_de(n, k):
    """(d, e) of a matrix that is diagonal but for the element at the root tear: the children of the root deflate
    completely and hand up identity vectors, so the root sees two non-zero weights.  With different poles under them it
    keeps both (k = 2, the last root reads d[j - 1]); with equal poles one rotation merges them (k = 1)."""
    assert k in (1, 2)
    mid = tear(n, 0, 0)
    d = np.arange(1.0, n + 1.0) / n
    if k == 1:
        d[mid] = d[mid - 1]
    e = np.zeros(n - 1)
    e[mid - 1] = 0.3
    return d, e


@functools.lru_cache(maxsize=None)
def k_case(n, k):
    return tridiag(*k_de(n, k))


def _glued_de(nblk, seed):
    """Wilkinson blocks |i - 10| of 21 rows, glued with 1e-9; block b is lifted by b / 8 and the diagonal tilted, which
    separates the eigenvalues a plain glued Wilkinson matrix has in near-equal groups, so that a threshold between any
    two of them is well defined.  The tiny glue still deflates most of every node that a glue element falls into."""
    m = 21
    n = nblk * m
    rng = np.random.default_rng([11, nblk, seed])
    d = np.tile(np.abs(np.arange(m) - 10.0), nblk) + np.repeat(np.arange(nblk) / 8.0, m) + 0.013 * np.arange(n)
    d += rng.uniform(0.0, 0.05, n)
    e = np.ones(n - 1)
    e[m - 1:: m] = 1e-9
    return d, e


def _gapped(make, n, seeds=200):
    """The first matrix make(seed) whose spectrum has gaps of 2 MIN_GAP of the norm after 0, 1, 16, 17, n - 1 and n
    eigenvalues from either end: (C, ascending eigenvalues)."""
    counts = sorted({k for k in KEEP + (n - 1, n) if 0 <= k <= n})
    belows = sorted(set(counts) | {n - k for k in counts})
    for seed in range(seeds):
        C = tridiag(*make(seed))
        lam = np.linalg.eigvalsh(C)
        if all(ec.gap_around(lam, ec.threshold_below(lam, j)) >= 2 * ec.MIN_GAP for j in belows):
            lam.setflags(write=False)
            return C, lam
    raise AssertionError("no draw with the gaps wanted")


@functools.lru_cache(maxsize=None)
def select_case(name, n):
    if name == "tear_zero":      # every vector of the root is a deflated copy

        def make(seed):
            d, e = _random_de(n, 100 + seed)
            e[tear(n, 0, 0) - 1] = 0.0
            return d, e
    elif name == "glued":        # the selection mixes deflated and computed vectors
        assert n % 21 == 0

        def make(seed):
            return _glued_de(n // 21, seed)
    else:
        raise ValueError(name)
    return _gapped(make, n)


BATCH_NS = (1, 2, 32, 33, 64, 65, 130)      # 1, 2, 32: no merge level; the others one to three
BATCH_THR = 0.125


@functools.lru_cache(maxsize=None)
def select_batch():
    """[(A, ascending eigenvalues, number below 4 BATCH_THR)]: random tridiagonals moved along the identity so that the
    threshold falls into the widest gap of the middle half of each spectrum."""
    out = []
    for n in BATCH_NS:
        d, e = _random_de(n, 200)
        lam = np.linalg.eigvalsh(tridiag(d, e))
        if n == 1:
            below, mid = 0, lam[0] - 0.5
        else:
            lo, hi = (n // 4, max(n // 4 + 1, 3 * n // 4)) if n > 2 else (0, 1)
            g = int(np.argmax(np.diff(lam)[lo:hi])) + lo
            below, mid = g + 1, 0.5 * (lam[g] + lam[g + 1])
        A = tridiag(d + (4.0 * BATCH_THR - mid), e)
        lamA = np.linalg.eigvalsh(A)
        assert ec.gap_around(lamA, 4.0 * BATCH_THR) >= 2 * ec.MIN_GAP, n
        lamA.setflags(write=False)
        out.append((A, lamA, below))
    return tuple(out)


_REF = {}


def ref_evals(C):
    """numpy.linalg.eigvalsh of a write-protected matrix, once."""
    assert C.shape[0] <= 1025 and not C.flags.writeable
    if id(C) not in _REF:
        ev = np.linalg.eigvalsh(C)
        ev.setflags(write=False)
        _REF[id(C)] = (C, ev)
    return _REF[id(C)][1]


def _offdiag(C):
    return np.real(np.diag(C, 1))


# ---- host: the constructors put their zeros at the tears -------------------------------------------------------------------
def test_tear_positions_of_the_constructors():
    assert [depth(n) for n in (32, 33, 64, 65, 128, 129, 200, 1025)] == [0, 1, 1, 2, 2, 3, 3, 6]
    for n in (64, 200):
        D = depth(n)
        # the leaves tile the rows, none above 32 rows; the root is torn at n >> 1
        b = [bound(n, D, i) for i in range((1 << D) + 1)]
        assert b[0] == 0 and b[-1] == n and max(np.diff(b)) <= LEAF
        assert tear(n, 0, 0) == n >> 1
        assert set(all_tears(n)) == set(b[1:-1])
        e = _offdiag(tear_zero(n, 0, 0))
        assert np.flatnonzero(e == 0.0).tolist() == [(n >> 1) - 1]
        for k in (1, 2):
            d, e = k_de(n, k)
            assert np.flatnonzero(e).tolist() == [(n >> 1) - 1]
            assert (d[n >> 1] == d[(n >> 1) - 1]) == (k == 1)
    n = 200   # second level: the nodes [0, 100) and [100, 200) are torn at 50 and 150
    assert (tear(n, 1, 0), tear(n, 1, 1)) == (50, 150)
    assert np.flatnonzero(_offdiag(tear_zero(n, 1, 1)) == 0.0).tolist() == [149]
    C, _ = select_case("tear_zero", 64)
    assert np.flatnonzero(_offdiag(C) == 0.0).tolist() == [31]


# ---- 1. group and tile boundaries --------------------------------------------------------------------------------------------
def _pair(n):
    mats = [toeplitz121(n), random_tridiag(n)]
    return mats, [ref_evals(C) for C in mats]


@pytest.mark.gpu
@pytest.mark.parametrize("n", SMALL_NS)
def test_boundaries_small(ctx, monkeypatch, n):
    te.set_route(monkeypatch, "small")
    mats, refs = _pair(n)
    te.check_batch(ctx, mats, refs, "dc small n=%d" % n)


@pytest.mark.gpu
@pytest.mark.parametrize("n", PANEL_NS)
@pytest.mark.parametrize("route", PANEL_ROUTES)
def test_boundaries_panel(ctx, monkeypatch, route, n):
    te.set_route(monkeypatch, route)
    mats, refs = _pair(n)
    te.check_batch(ctx, mats, refs, "dc %s n=%d" % (route, n))


# ---- 2. deflation extremes ----------------------------------------------------------------------------------------------------
def _deflation_cases(n):
    return [("root tear zero", tear_zero(n, 0, 0)),
            ("second-level tear zero", tear_zero(n, 1, 1) if depth(n) > 1 else None),
            ("constant diagonal 1e-14", constant_diagonal(n, 1e-14)),
            ("constant diagonal 3e-15", constant_diagonal(n, 3e-15)),
            ("tiny couplings", tiny_couplings(n)),
            ("k = 1", k_case(n, 1)),
            ("k = 2", k_case(n, 2))]


@pytest.mark.gpu
@pytest.mark.parametrize("route,n", DEFL_SIZES)
def test_deflation_extremes(ctx, monkeypatch, route, n):
    """One batch of all the cases of a size (n = 64 has one merge level: its second-level case is the n = 200 one's)."""
    te.set_route(monkeypatch, route)
    cases = [(name, C) for name, C in _deflation_cases(n) if C is not None]
    mats = [C for _, C in cases]
    ev, W = te.solve(ctx, mats)
    for b, (name, C) in enumerate(cases):
        te.check(C, ev[b], W[b], ref_evals(C), "dc %s n=%d %s" % (route, n, name))


# ---- 3. selection at the root ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("side", ["upper", "lower"])
@pytest.mark.parametrize("route,name,n", [("small", "tear_zero", 64), ("two_pos", "tear_zero", 200),
                                          ("small", "glued", 63), ("one32", "glued", 105)])
def test_selection_at_the_root(ctx, monkeypatch, route, name, n, side):
    te.set_route(monkeypatch, route)
    A, lam = select_case(name, n)
    for k in sorted({k for k in KEEP + (n - 1, n)}):
        thr = ec.threshold_below(lam, ec.below_for(side, n, k)) / 4.0
        evs, Es, nkeep = te._eigh_gen_4I(ctx, [A], cut=(side, thr))
        assert nkeep.tolist() == [k], (side, k, nkeep)
        te._check_pencil_block(A, evs[0], Es[0], lam, te._rows(side, n, k), "dc %s %s n=%d %s keep %d" % (route, name, n, side, k))


@pytest.mark.gpu
@pytest.mark.parametrize("side", ["upper", "lower"])
@pytest.mark.parametrize("route", PANEL_ROUTES)
def test_selection_mixed_depths(ctx, monkeypatch, route, side):
    """Sizes 1, 2, 32, 33, 64, 65 and 130 under one threshold: matrices without a merge level beside matrices with one,
    two and three."""
    te.set_route(monkeypatch, route)
    cases = select_batch()
    mats = [A for A, _, _ in cases]
    evs, Es, nkeep = te._eigh_gen_4I(ctx, mats, cut=(side, BATCH_THR))
    want = [(A.shape[0] - below) if side == "upper" else below for A, _, below in cases]
    assert nkeep.tolist() == want
    for i, (A, lam, _) in enumerate(cases):
        n = A.shape[0]
        te._check_pencil_block(A, evs[i], Es[i], lam, te._rows(side, n, want[i]), "dc %s batch %s n=%d" % (route, side, n))


# ---- 4. a matrix that cannot be solved fails alone, with its index, and nothing is addressed from its data --------------------
@pytest.mark.gpu
@pytest.mark.parametrize("route,n", [("small", 64), ("two_pos", 200)])
def test_non_finite_matrix_is_reported(ctx, monkeypatch, route, n):
    """One NaN in the second of three matrices: the leaves of its tridiagonal do not converge (or hand up non-finite
    poles), the matrix is flagged on the device and not merged — the merge kernels take their column indices from sorted
    poles — and the call returns 1000 + 1.  The context then solves the healthy matrices as before."""
    from driftscan_amd._lib import DriftMIError

    te.set_route(monkeypatch, route)
    good = [random_tridiag(n), toeplitz121(n)]
    bad = np.array(random_tridiag(n, 1))
    bad[5, 5] = np.nan
    with pytest.raises(DriftMIError, match=r"\(1001\)"):
        te.solve(ctx, [good[0], bad, good[1]])
    te.check_batch(ctx, good, [ref_evals(C) for C in good], "dc %s n=%d after a failed call" % (route, n))
