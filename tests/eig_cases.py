"""Matrices, checkers and bounds for the Hermitian eigensolver tests (host only, numpy; shared by the CPU and GPU tests).

A device result is measured against the matrix it was given, never against another device result: with eigenvectors as
the columns of V (n x k, all of them or a selected subset) and nrm = max |ev| over the whole spectrum,

    res  = max |C V - V diag(ev)| / (n eps nrm)
    orth = max |V^H V - I|        / (n eps)

and what is allowed is MARGIN times the worst ratio `numpy.linalg.eigh` (LAPACK zheevd) reaches over the same table of
matrices (`table()`), recorded below as REF_RES / REF_ORTH and re-measured by tests/test_host_eigcases.py.  MARGIN = 8 =
2 (the two-stage route applies about twice as many unitary transformations as zheevd) x 4 (another summation order:
MFMA-blocked products, the explicit Q of the small route).  LAPACK's worst ratios belong to n = 2, where three units of
rounding are 1.5 n eps; from the smallest panel size on (n >= PANEL_MIN = 97) its ratios are twenty times smaller, and a
result of that size is held to MARGIN times those (REF_RES_PANEL / REF_ORTH_PANEL) — `bounds(n)`.  A back-transformation that is wrong but still unitary —
reflectors applied in the wrong order, a block shifted by one row — passes `orth` and every W W^H = I check; `res` is
what rejects it.
"""
import functools

import numpy as np

EPS = 2.220446049250313e-16
MARGIN = 8.0
# worst ratios of numpy.linalg.eigh over table(); both are reached at the smallest sizes and fall with n
REF_RES = 1.60
REF_ORTH = 1.01
# the same over the matrices of the table with n >= PANEL_MIN (the sizes of the panel routes)
PANEL_MIN = 97
REF_RES_PANEL = 0.078
REF_ORTH_PANEL = 0.20

KINDS = ("graded", "clustered", "uniform", "lowrank")
SMALL_NS = (1, 2, 3, 31, 32, 33, 64, 95, 96)                    # QL up to 32, divide & conquer above
PANEL_NS = (97, 128, 129, 130, 160, 161, 162, 257, 452, 1000)   # 129 | 130 and 161 | 162: one block of 128 reflectors
LD_NS = (40, 130, 300)
MIXED_NS = (161, 1, 2, 33, 34, 35, 66, 97, 130, 0)
SELECT_NS = (64, 200)
SELECT_KEEP = (0, 1, 15, 16, 17, 63, 64, 65)                     # and n - 1, n; see keep_counts
SELECT_BATCH = ((200, 0), (130, 130), (97, 17), (64, 1), (200, 65))   # (n, modes kept); the 64 block is zeroed on the device side
SELECT_BATCH_THR = 0.125                                         # pencil threshold of that batch (B = 4 I)
POLICY_N, POLICY_NB, POLICY_KEEP, POLICY_THR = 256, 64, 40, 0.26
WIDE_N = 2049


def crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


# ---- generators --------------------------------------------------------------------------------------------------------
def spectrum(rng, kind, n):
    if kind == "graded":
        return 10.0 ** rng.uniform(-12, 0, n) * rng.choice([1.0, 1.0, -1.0], n)
    if kind == "clustered":
        return rng.choice(np.linspace(0.5, 3.0, 40), n)  # heavy deflation
    if kind == "uniform":
        return np.sort(rng.uniform(-1.0, 1.0, n))
    if kind == "lowrank":
        lam = np.zeros(n)
        lam[rng.permutation(n)[: n // 20]] = rng.uniform(0.5, 2.0, n // 20)
        return lam
    raise ValueError(kind)


def from_spectrum(rng, lam):
    """H diag(lam) H^H with H a product of three Householder reflectors (dense, unitary to rounding), symmetrised."""
    n = len(lam)
    C = np.diag(np.asarray(lam, dtype=np.float64)).astype(np.complex128)
    for _ in range(3):
        u = crand(rng, n)
        u /= np.linalg.norm(u)
        C -= 2.0 * np.outer(u, u.conj() @ C)
        C -= 2.0 * np.outer(C @ u, u.conj())
    return 0.5 * (C + C.conj().T)


def _seed(kind, n, salt=0):
    return [KINDS.index(kind), n, salt]


def _frozen(*arrs):
    for a in arrs:
        a.setflags(write=False)
    return arrs if len(arrs) > 1 else arrs[0]


@functools.lru_cache(maxsize=None)
def random_case(kind, n, salt=0):
    """(lam, C) of one kind and size, the same arrays (write-protected) on every call."""
    rng = np.random.default_rng(_seed(kind, n, salt))
    lam = spectrum(rng, kind, n)
    return _frozen(lam, from_spectrum(rng, lam))


def kinds_for(n):
    """The spectrum kinds that exist at size n (`lowrank` has n / 20 non-zero eigenvalues)."""
    return tuple(k for k in KINDS if k != "lowrank" or n >= 20)


def _wilkinson_glued(nblk, glue, seed):
    m = 21
    n = nblk * m
    rng = np.random.default_rng(seed)
    d = np.tile(np.abs(np.arange(m) - 10.0), nblk)
    e = np.ones(n - 1)
    e[m - 1:: m] = glue
    e = e * np.exp(2j * np.pi * rng.uniform(0, 1, n - 1))
    return np.diag(d).astype(np.complex128) + np.diag(e, -1) + np.diag(e.conj(), 1)


@functools.lru_cache(maxsize=None)
def structured(name):
    """Matrices that arrive tridiagonal or diagonal: every reflector of the reduction meets a zero column."""
    if name == "wilkinson5":      # 5 x W21, glue 1e-8
        C = _wilkinson_glued(5, 1e-8, 105)
    elif name == "wilkinson8":    # 8 x W21, glue 1e-14
        C = _wilkinson_glued(8, 1e-14, 168)
    elif name == "toeplitz121":
        n = 200
        C = (2.0 * np.eye(n) + np.eye(n, k=1) + np.eye(n, k=-1)).astype(np.complex128)
    elif name == "diagonal":
        C = np.diag(np.linspace(-1.0, 1.0, 130)).astype(np.complex128)
    elif name == "identity":
        C = np.eye(161, dtype=np.complex128)
    elif name == "zero":
        C = np.zeros((100, 100), dtype=np.complex128)
    elif name == "diagonal_small":
        C = np.diag(np.linspace(-1.0, 1.0, 96)).astype(np.complex128)
    elif name == "identity_small":
        C = np.eye(95, dtype=np.complex128)
    elif name == "zero_small":
        C = np.zeros((64, 64), dtype=np.complex128)
    else:
        raise ValueError(name)
    return _frozen(C)


STRUCTURED = ("wilkinson5", "wilkinson8", "toeplitz121", "diagonal", "identity", "zero")
STRUCTURED_SMALL = ("diagonal_small", "identity_small", "zero_small")


# ---- selection: thresholds in known gaps ----------------------------------------------------------------------------------
def keep_counts(n):
    return tuple(sorted({k for k in SELECT_KEEP + (n - 1, n) if 0 <= k <= n}))


def threshold_below(lam, j):
    """A threshold with exactly j eigenvalues of `lam` below it, in the middle of the gap (a quarter of the norm outside
    the spectrum for j = 0 and j = n)."""
    s = np.sort(np.asarray(lam))
    n = len(s)
    nrm = np.abs(s).max()
    if j == 0:
        return float(s[0] - 0.25 * nrm)
    if j == n:
        return float(s[-1] + 0.25 * nrm)
    return float(0.5 * (s[j - 1] + s[j]))


def below_for(side, n, k):
    """Number of eigenvalues below the threshold that keeps k modes on `side`."""
    return n - k if side == "upper" else k


def gap_around(lam, thr):
    """Width of the gap of the spectrum that thr lies in, relative to max |lam| (0 if thr is an eigenvalue; the distance to
    the spectrum if thr lies outside it)."""
    lam = np.asarray(lam)
    lo, hi = lam[lam <= thr], lam[lam >= thr]
    if lo.size and hi.size:
        return float((hi.min() - lo.max()) / np.abs(lam).max())
    return float(np.abs(lam - thr).min() / np.abs(lam).max())


MIN_GAP = 1e-3


@functools.lru_cache(maxsize=None)
def gapped_uniform(n, belows, salt):
    """(lam, C) of the `uniform` kind whose gaps after `belows` eigenvalues are each at least 2 MIN_GAP of the norm wide:
    the first of the seeds salt, salt + 10000, ... whose draw has them (a sorted uniform draw of 200 has a mean gap of
    0.01 but some of 1e-5)."""
    for t in range(1000):
        rng = np.random.default_rng(_seed("uniform", n, salt + 10000 * t))
        lam = spectrum(rng, "uniform", n)
        if all(gap_around(lam, threshold_below(lam, j)) >= 2 * MIN_GAP for j in belows):
            return random_case("uniform", n, salt + 10000 * t)
    raise AssertionError("no draw with the gaps wanted")


def select_case(n):
    """The matrix of the single-block selection tests: gaps at every count of keep_counts(n), from either end."""
    ks = keep_counts(n)
    return gapped_uniform(n, tuple(sorted({k for k in ks} | {n - k for k in ks})), 0)


@functools.lru_cache(maxsize=None)
def shifted_case(n, below, thr, salt):
    """A `uniform` matrix moved along the identity so that `thr` lies in the gap with `below` eigenvalues under it."""
    lam0, _ = gapped_uniform(n, (below,), salt)
    rng = np.random.default_rng(_seed("uniform", n, 5000 + salt))
    lam = lam0 + (thr - threshold_below(lam0, below))
    return _frozen(lam, from_spectrum(rng, lam))


@functools.lru_cache(maxsize=None)
def select_batch(side):
    """The mixed batch of the selection test: [(lam, A, kept)], pencil (A, 4 I) cut at SELECT_BATCH_THR."""
    out = []
    for i, (n, k) in enumerate(SELECT_BATCH):
        lam, A = shifted_case(n, below_for(side, n, k), 4.0 * SELECT_BATCH_THR, 10 + i)
        out.append((lam, A, k))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def policy_batch():
    """64 matrices of n = 256: two of each kind, then `uniform` ones placed to keep POLICY_KEEP modes above POLICY_THR.
    [(kind, lam, A)]."""
    out = []
    for kind in KINDS:
        for r in range(2):
            lam, A = random_case(kind, POLICY_N, 1 + r)
            out.append((kind, lam, A))
    for i in range(POLICY_NB - len(out)):
        lam, A = shifted_case(POLICY_N, POLICY_N - POLICY_KEEP, 4.0 * POLICY_THR, 100 + i)
        out.append(("placed", lam, A))
    return tuple(out)


def cut_thresholds():
    """Every (spectrum, threshold) pair the selection tests use, in the units of the matrix (4 x the pencil threshold)."""
    for n in SELECT_NS:
        lam, _ = select_case(n)
        for side in ("upper", "lower"):
            for k in keep_counts(n):
                yield "select n=%d %s k=%d" % (n, side, k), lam, threshold_below(lam, below_for(side, n, k))
    for side in ("upper", "lower"):
        for i, (lam, _, k) in enumerate(select_batch(side)):
            yield "batch %s block %d" % (side, i), lam, 4.0 * SELECT_BATCH_THR
    for i, (kind, lam, _) in enumerate(policy_batch()):
        yield "policy block %d (%s)" % (i, kind), lam, 4.0 * POLICY_THR


# ---- the case table the reference constants are measured over (n <= 1000) -------------------------------------------------
def table():
    """(name, C) of every matrix of tests/test_gpu_eigensolver.py with n <= 1000 (each once)."""
    seen = set()
    for n in sorted(set(SMALL_NS + PANEL_NS + LD_NS + tuple(m for m in MIXED_NS if m > 0))):
        for kind in kinds_for(n):
            seen.add((kind, n, 0))
            yield "%s n=%d" % (kind, n), random_case(kind, n)[1]
    for n in SELECT_NS:
        yield "select n=%d" % n, select_case(n)[1]
    for name in STRUCTURED + STRUCTURED_SMALL:
        yield name, structured(name)
    for side in ("upper", "lower"):
        for i, (_, A, _) in enumerate(select_batch(side)):
            yield "batch %s block %d" % (side, i), A
    for i, (kind, _, A) in enumerate(policy_batch()):
        yield "policy block %d (%s)" % (i, kind), A


# ---- checkers ----------------------------------------------------------------------------------------------------------
def res_ratio(C, V, ev, nrm=None):
    """max |C V - V diag(ev)| / (n eps nrm) for the columns of V (n x k) and their eigenvalues ev (k).  `nrm` is
    max |eigenvalue| of the whole spectrum (default: of ev).  A zero matrix allows no residual at all."""
    n, k = V.shape
    if n == 0 or k == 0:
        return 0.0
    ev = np.asarray(ev, dtype=np.float64)
    if nrm is None:
        nrm = np.abs(ev).max()
    err = np.abs(C @ V - V * ev[None, :]).max()
    if nrm == 0.0:
        return 0.0 if err == 0.0 else np.inf
    return float(err / (n * EPS * nrm))


def res_ratio_pencil(A, B, X, ev):
    """The same ratio for the pencil (A, B) with B = L L^H and B-orthonormal columns X: L^-1 (A X - B X diag(ev)) is the
    residual C V - V diag(ev) of the standard problem C = L^-1 A L^-H, V = L^H X.  The reduction itself carries a backward
    error of order eps cond(B) in any implementation (parity_util.pencil_tol), so a caller allows cond(B) times the
    bound of the standard problem."""
    n, k = X.shape
    if n == 0 or k == 0:
        return 0.0
    ev = np.asarray(ev, dtype=np.float64)
    L = np.linalg.cholesky(B)
    R = np.linalg.solve(L, A @ X - (B @ X) * ev[None, :])
    return float(np.abs(R).max() / (n * EPS * np.abs(ev).max()))


def orth_ratio(V):
    """max |V^H V - I| / (n eps) for the columns of V (n x k)."""
    n, k = V.shape
    if n == 0 or k == 0:
        return 0.0
    return float(np.abs(V.conj().T @ V - np.eye(k)).max() / (n * EPS))


def ratios(C, V, ev, nrm=None):
    return res_ratio(C, V, ev, nrm), orth_ratio(V)


def reference(n):
    """(REF_RES, REF_ORTH) for a matrix of n rows."""
    return (REF_RES_PANEL, REF_ORTH_PANEL) if n >= PANEL_MIN else (REF_RES, REF_ORTH)


def bounds(n):
    """The (res, orth) ratios a device result of n rows may reach."""
    r, o = reference(n)
    return MARGIN * r, MARGIN * o


def assert_eigvecs(C, V, ev, nrm=None, what=""):
    """The bounds every device result must meet; the ratios are printed first so a run shows them."""
    assert np.isfinite(V).all() and np.isfinite(ev).all(), "%s: non-finite output" % what
    res, orth = ratios(C, V, ev, nrm)
    max_res, max_orth = bounds(C.shape[0])
    print("%s: res %.3g orth %.3g (allowed %.3g / %.3g)" % (what, res, orth, max_res, max_orth))
    assert res <= max_res, "%s: residual ratio %.3g > %.3g" % (what, res, max_res)
    assert orth <= max_orth, "%s: orthogonality ratio %.3g > %.3g" % (what, orth, max_orth)
    return res, orth


def assert_eigvals(ev, ref, tol=1e-13, what=""):
    """|sort(ev) - ref| <= tol max |ref| (ref ascending)."""
    ev, ref = np.sort(np.asarray(ev)), np.asarray(ref)
    assert ev.shape == ref.shape, "%s: %s eigenvalues for %s" % (what, ev.shape, ref.shape)
    if ev.size == 0:
        return
    err = np.abs(ev - ref).max()
    assert err <= tol * np.abs(ref).max(), "%s: eigenvalue error %.3g, norm %.3g" % (what, err, np.abs(ref).max())
