"""The Hermitian eigensolver (dm_herm_eig_batched, and through dm_eigh_gen its eigenvector selection) on every route
production takes, against the matrix it was given: residual C V = V diag(ev), orthogonality, eigenvalues — with the bounds
of eig_cases.py, which come from LAPACK's own ratios on the same matrices (tests/test_host_eigcases.py).

Routes (all three variables are read per call):
    small      batch maxn <= 96 (QL for maxn <= 32, divide & conquer above)
    one32      DM_TRD_TWOSTAGE=0, 97 <= maxn <= 2048: one-stage reduction, 32-wide panels (64-wide above 2048)
    two_pos    DM_TRD_TWOSTAGE=1: two-stage reduction, bulge chase by band position
    two_pairs  DM_TRD_TWOSTAGE=1 DM_SB_CHASE=pairs: two-stage reduction, sweep-owning chase
"""
import ctypes

import numpy as np
import pytest

import eig_cases as ec

pytestmark = pytest.mark.gpu

ROUTE_ENV = {
    "small": {},
    "one32": {"DM_TRD_TWOSTAGE": "0"},
    "two_pos": {"DM_TRD_TWOSTAGE": "1"},
    "two_pairs": {"DM_TRD_TWOSTAGE": "1", "DM_SB_CHASE": "pairs"},
}
ROUTE_VARS = ("DM_TRD_TWOSTAGE", "DM_SB_CHASE", "DM_SB_POS_CAP")
PANEL_ROUTES = ("one32", "two_pos", "two_pairs")


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ref_evals():
    """numpy.linalg.eigvalsh of a matrix of the case table (n <= 1000), computed once per matrix and write-protected."""
    cache = {}

    def get(C):
        assert C.shape[0] <= 1000 and not C.flags.writeable
        if id(C) not in cache:
            ev = np.linalg.eigvalsh(C) if C.shape[0] else np.zeros(0)
            ev.setflags(write=False)
            cache[id(C)] = (C, ev)
        return cache[id(C)][1]

    return get


def set_route(monkeypatch, route, **extra):
    for v in ROUTE_VARS:
        monkeypatch.delenv(v, raising=False)
    for k, v in dict(ROUTE_ENV[route], **extra).items():
        monkeypatch.setenv(k, v)


def solve(ctx, mats):
    """dm_herm_eig_batched on copies of same-sized matrices: (ev (nb, n) in the solver's order, W (nb, n, n))."""
    n, nb = mats[0].shape[0], len(mats)
    ev, W = ctx.herm_eig(ctx.to_device(np.stack(mats)), n, n, strideC=n * n, batch=nb)
    return ev.cpu().numpy()[:, :n], W.cpu().numpy()


def check(C, ev, W, ref, what, tol=1e-13):
    """Finite output, eigenvalues against `ref` (ascending), residual and orthogonality of V = W^H."""
    assert np.isfinite(ev).all() and np.isfinite(W).all(), what
    ec.assert_eigvals(ev, ref, tol, what)
    return ec.assert_eigvecs(C, W.conj().T, ev, np.abs(ref).max() if len(ref) else 0.0, what)


def check_batch(ctx, mats, refs, what, tol=1e-13):
    ev, W = solve(ctx, mats)
    for b, (C, ref) in enumerate(zip(mats, refs)):
        check(C, ev[b], W[b], ref, "%s [%d]" % (what, b), tol)
    return ev


# ---- a. residuals per route -----------------------------------------------------------------------------------------------
def _kinds_batch(n, ref_evals):
    mats = [ec.random_case(kind, n)[1] for kind in ec.kinds_for(n)]
    return mats, [ref_evals(C) for C in mats]


@pytest.mark.parametrize("n", ec.SMALL_NS)
def test_residuals_small(ctx, monkeypatch, ref_evals, n):
    """One matrix of every spectrum kind in one batch on the small route: n <= 32 takes QL, above it divide & conquer."""
    set_route(monkeypatch, "small")
    mats, refs = _kinds_batch(n, ref_evals)
    check_batch(ctx, mats, refs, "small n=%d" % n)


@pytest.mark.parametrize("n", ec.PANEL_NS)
@pytest.mark.parametrize("route", PANEL_ROUTES)
def test_residuals_panel(ctx, monkeypatch, ref_evals, route, n):
    """The same on the three panel routes.  129 | 130 straddle one block of 128 one-stage reflectors (n - 1 of them),
    161 | 162 the same boundary of the two-stage count n - 33; 97 is the smallest panel size."""
    set_route(monkeypatch, route)
    mats, refs = _kinds_batch(n, ref_evals)
    check_batch(ctx, mats, refs, "%s n=%d" % (route, n))


# ---- b. the 64-wide build and the two-stage route above 2048 --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["graded", "clustered"])
@pytest.mark.parametrize("twostage", ["0", "1"])
def test_residuals_above_2048(ctx, monkeypatch, twostage, kind):
    """n = 2049: DM_TRD_TWOSTAGE=0 is the one-stage reduction with 64-wide panels (dm_trd64), =1 the two-stage route of a
    matrix past the narrow-panel range.  The spectrum is prescribed, so no LAPACK call is needed."""
    set_route(monkeypatch, "small", DM_TRD_TWOSTAGE=twostage)
    lam, C = ec.random_case(kind, ec.WIDE_N)
    check_batch(ctx, [C], [np.sort(lam)], "n=2049 twostage=%s %s" % (twostage, kind), tol=2e-13)


# ---- c. matrices that arrive tridiagonal or diagonal ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ec.STRUCTURED)
@pytest.mark.parametrize("route", PANEL_ROUTES)
def test_structured_panel(ctx, monkeypatch, ref_evals, route, name):
    """Glued Wilkinson matrices, the 1-2-1 Toeplitz matrix, a diagonal matrix, the identity and the zero matrix: every
    reflector of the reduction meets a zero column (DM_REFL_TINY), and the glued ones deflate heavily."""
    set_route(monkeypatch, route)
    C = ec.structured(name)
    ev = check_batch(ctx, [C], [ref_evals(C)], "%s %s" % (route, name))
    if name == "zero":
        assert (ev == 0.0).all()


@pytest.mark.parametrize("name", ec.STRUCTURED_SMALL)
def test_structured_small(ctx, monkeypatch, ref_evals, name):
    set_route(monkeypatch, "small")
    C = ec.structured(name)
    ev = check_batch(ctx, [C], [ref_evals(C)], "small %s" % name)
    if name == "zero_small":
        assert (ev == 0.0).all()


# ---- d. the by-position chase declines ----------------------------------------------------------------------------------
def test_position_chase_falls_back_to_pairs(ctx, monkeypatch, ref_evals):
    """DM_SB_POS_CAP=1: a matrix of 452 rows needs more resident workgroups than the cap, so the by-position chase declines
    and the sweep-owning chase runs, as for a matrix too large for it.  Same bounds; same eigenvalues as DM_SB_CHASE=pairs."""
    mats = [ec.random_case(kind, 452)[1] for kind in ("graded", "uniform")]
    refs = [ref_evals(C) for C in mats]
    set_route(monkeypatch, "two_pos", DM_SB_POS_CAP="1")
    got = np.sort(check_batch(ctx, mats, refs, "two_pos capped n=452"), axis=1)
    set_route(monkeypatch, "two_pairs")
    pairs = np.sort(solve(ctx, mats)[0], axis=1)
    for b, ref in enumerate(refs):
        assert np.abs(got[b] - pairs[b]).max() <= 1e-13 * np.abs(ref).max()


# ---- e. leading dimensions and strides with slack ---------------------------------------------------------------------------
SENTINEL = complex(12345.678, -8765.4321)
GUARD = 4096


def _guarded(ctx, n, ld, stride, nb, mats=None):
    """A device buffer [guard | nb matrices of n rows, leading dimension ld, `stride` apart | guard], all sentinel except
    the matrix entries; returns (tensor, pointer to the first matrix, host copy)."""
    span = (nb - 1) * stride + n * ld
    host = np.full(GUARD + span + GUARD, SENTINEL, dtype=np.complex128)
    if mats is not None:
        for b, C in enumerate(mats):
            for i in range(n):
                o = GUARD + b * stride + i * ld
                host[o: o + n] = C[i]
    t = ctx.to_device(host)
    return t, ctypes.c_void_p(t.data_ptr() + 16 * GUARD), host


def _unpack(buf, n, ld, stride, nb):
    return np.stack([np.stack([buf[GUARD + b * stride + i * ld: GUARD + b * stride + i * ld + n] for i in range(n)])
                     for b in range(nb)])


@pytest.mark.parametrize("route,n", [("small", 40)] + [(r, n) for r in PANEL_ROUTES for n in (130, 300)])
def test_leading_dimensions_and_slack(ctx, monkeypatch, ref_evals, route, n):
    """ldc = n + 5, strideC = n ldc + 7, ldw = n + 3, strideW = n ldw + 11, C and W inside larger buffers: the results meet
    the bounds and the guards around both are untouched, bit for bit.  (C is destroyed, so nothing is asked of the
    padding between its rows.)"""
    set_route(monkeypatch, route)
    nb = 3
    kinds = ("graded", "clustered", "uniform")
    mats = [ec.random_case(kind, n)[1] for kind in kinds]
    ldc, ldw = n + 5, n + 3
    strideC, strideW = n * ldc + 7, n * ldw + 11
    dC, pC, hC = _guarded(ctx, n, ldc, strideC, nb, mats)
    dW, pW, hW = _guarded(ctx, n, ldw, strideW, nb)
    ev = ctx.empty((nb, n), np.float64)
    rc = ctx.lib.dm_herm_eig_batched(ctx.h, n, pC, ldc, strideC, pW, ldw, strideW, nb, ctx.ptr(ev))
    ctx.check(rc, "dm_herm_eig_batched")
    outC, outW = dC.cpu().numpy(), dW.cpu().numpy()
    for out, host, name in ((outC, hC, "C"), (outW, hW, "W")):
        for sl in (slice(0, GUARD), slice(len(host) - GUARD, len(host))):
            assert np.array_equal(out[sl].view(np.uint64), host[sl].view(np.uint64)), "guard of %s overwritten" % name
    W = _unpack(outW, n, ldw, strideW, nb)
    ev = ev.cpu().numpy()
    for b, C in enumerate(mats):
        check(C, ev[b], W[b], ref_evals(C), "%s n=%d ld [%d]" % (route, n, b))


# ---- eigh_gen with B = 4 I: L = 2 I exactly, E = W / 2, pencil eigenvalues lam / 4 — all scalings exact ------------------------
def _eigh_gen_4I(ctx, mats, cut=None):
    """dm_eigh_gen on the pencils (A_b, 4 I): (ev per block (ascending), E per block (rows = modes), last_nkeep)."""
    from driftscan_amd._lib import block_offsets

    ns = [A.shape[0] for A in mats]
    off, _ = block_offsets(ns)
    A = np.concatenate([a.ravel() for a in mats])
    B = np.concatenate([(4.0 * np.eye(n, dtype=np.complex128)).ravel() for n in ns])
    evals, evoff, evecs, ac, _ = ctx.eigh_gen(ctx.to_device(A), ctx.to_device(B), ns, off, cut=cut)
    assert (ac == 0.0).all()
    ev, E = evals.cpu().numpy(), evecs.cpu().numpy()
    return ([ev[evoff[i]: evoff[i] + n] for i, n in enumerate(ns)],
            [E[off[i]: off[i] + n * n].reshape(n, n) for i, n in enumerate(ns)], ctx.last_nkeep.copy())


def _check_pencil_block(A, ev, E, ref, rows, what):
    """Block of a pencil (A, 4 I): all eigenvalues ascending against ref / 4, the modes `rows` against A (V = 2 E^H), every
    other row exactly zero."""
    n = A.shape[0]
    assert np.isfinite(ev).all() and np.isfinite(E).all(), what
    assert (np.diff(ev) >= 0).all(), what
    ec.assert_eigvals(ev, ref / 4.0, 1e-13, what)
    other = np.ones(n, dtype=bool)
    other[rows] = False
    assert not E[other].any(), "%s: rows outside the selection are not zero" % what
    if n:
        ec.assert_eigvecs(A, 2.0 * E[rows].conj().T, 4.0 * ev[rows], np.abs(ref).max(), what)


# ---- f. mixed sizes in one batch ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", PANEL_ROUTES)
def test_mixed_sizes_in_one_batch(ctx, monkeypatch, ref_evals, route):
    """Sizes from 0 to 161 in one call (the KL use: ndof varies with m): the blocks below 34 rows have no first-stage
    panel, the empty one has nothing.  E A E^H = diag(ev) to the 5e-13 of the norm test_herm_eig_tridiag asks of the
    same product up to n = 517."""
    set_route(monkeypatch, route)
    kinds = ("graded", "clustered", "uniform")
    mats = [ec.random_case(kinds[i % 3], n)[1] if n else np.zeros((0, 0), dtype=np.complex128)
            for i, n in enumerate(ec.MIXED_NS)]
    evs, Es, nkeep = _eigh_gen_4I(ctx, mats)
    assert (nkeep == np.array(ec.MIXED_NS)).all()
    for i, (A, ev, E) in enumerate(zip(mats, evs, Es)):
        n = A.shape[0]
        if n == 0:
            assert ev.size == 0 and E.size == 0
            continue
        ref = ref_evals(A)
        _check_pencil_block(A, ev, E, ref, slice(0, n), "%s mixed n=%d" % (route, n))
        assert np.abs(E @ A @ E.conj().T - np.diag(ev)).max() <= 5e-13 * np.abs(ref).max() / 4.0, n


# ---- g. selection ---------------------------------------------------------------------------------------------------------
def _rows(side, n, k):
    return slice(n - k, n) if side == "upper" else slice(0, k)


@pytest.mark.parametrize("side", ["upper", "lower"])
@pytest.mark.parametrize("route,n", [("small", 64)] + [(r, 200) for r in PANEL_ROUTES])
def test_selection_counts(ctx, monkeypatch, ref_evals, route, n, side):
    """Threshold cuts that keep 0, 1, 15, 16, 17 (one slab of 16 columns, one more), 63, 64, 65 (one workgroup of four
    slabs, one more), n - 1 and n modes from either end: the count, the rows formed, their residuals against the matrix,
    exact zeros elsewhere, and all n eigenvalues."""
    set_route(monkeypatch, route)
    lam, A = ec.select_case(n)
    ref = ref_evals(A)
    for k in ec.keep_counts(n):
        thr = ec.threshold_below(lam, ec.below_for(side, n, k)) / 4.0
        evs, Es, nkeep = _eigh_gen_4I(ctx, [A], cut=(side, thr))
        assert nkeep.tolist() == [k], (side, k, nkeep)
        _check_pencil_block(A, evs[0], Es[0], ref, _rows(side, n, k), "%s n=%d %s keep %d" % (route, n, side, k))


@pytest.mark.parametrize("side", ["upper", "lower"])
@pytest.mark.parametrize("route", ["two_pos", "one32"])
def test_selection_mixed_batch(ctx, monkeypatch, ref_evals, route, side):
    """One threshold over blocks of 200, 130, 97, 64 and 200 rows that keep none, all, 17, - and 65 modes; the fourth
    block is all zero and takes the shortcut of dm_eigh_gen (zero eigenvalues; all of them are 0, so it reports 0 or n
    modes by the side of the threshold 0 falls on: the identity where they are kept, zero rows where the cut drops them,
    as include/driftmi.h promises for every block)."""
    set_route(monkeypatch, route)
    cases = ec.select_batch(side)
    mats = [A for _, A, _ in cases]
    mats[3] = np.zeros_like(mats[3])
    evs, Es, nkeep = _eigh_gen_4I(ctx, mats, cut=(side, ec.SELECT_BATCH_THR))
    want = [k for _, _, k in cases]
    assert ec.SELECT_BATCH_THR > 0.0
    want[3] = 0 if side == "upper" else 64          # searchsorted(zeros, thr > 0) = n: nothing above, everything below
    assert nkeep.tolist() == want
    for i, (A, ev, E) in enumerate(zip(mats, evs, Es)):
        n = A.shape[0]
        if i == 3:
            assert (ev == 0.0).all() and np.array_equal(E, np.eye(n) if want[3] == n else np.zeros((n, n)))
            continue
        _check_pencil_block(A, ev, E, ref_evals(cases[i][1]), _rows(side, n, want[i]),
                            "%s batch %s block %d" % (route, side, i))


# ---- h. the route the policy picks, and the threaded selection callback ---------------------------------------------------
def test_policy_batch_with_selection(ctx, monkeypatch, ref_evals):
    """64 matrices of 256 rows with no variable set: trd_policy_of sends the batch to the two-stage route, and the
    selection callback runs on several host threads (sum n = 16384, 64 matrices).  Whatever route it takes: residuals of
    the kept modes of every block, and the number kept."""
    set_route(monkeypatch, "small")
    batch = ec.policy_batch()
    mats = [A for _, _, A in batch]
    evs, Es, nkeep = _eigh_gen_4I(ctx, mats, cut=("upper", ec.POLICY_THR))
    n = ec.POLICY_N
    for i, (kind, lam, A) in enumerate(batch):
        k = int((lam >= 4.0 * ec.POLICY_THR).sum())
        if kind == "placed":
            assert k == ec.POLICY_KEEP
        assert nkeep[i] == k, (i, kind, nkeep[i], k)
        _check_pencil_block(A, evs[i], Es[i], ref_evals(A), _rows("upper", n, k), "policy block %d (%s)" % (i, kind))
