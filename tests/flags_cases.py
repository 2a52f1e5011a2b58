"""Shared cases and checkers of the flagged-timestream tests: Hermitian positive-definite Toeplitz
systems built from masks with fixed seeds, their reference solutions in extended precision, and the error bound.

The bound.  The forward error ||x - x_ref||_2 / ||x_ref||_2 of a solver is taken against a dense solve in np.clongdouble
of the system whose right-hand side was formed in long double from a known x (and rounded to double, which is what every
solver is handed).  A solver passes when it stays within FACTOR * max(e_ref, EPS * cond_2(A)), with e_ref the error of
scipy.linalg.solve_toeplitz on the same system and cond_2 from eigvalsh; the inputs are sound when scipy alone stays
within E_REF_MAX.

Systems: (a) random flags of 20-30 % of ntime = ceil(2.5 n) samples, (b) a contiguous gap of 10 of 160 samples at n = 65,
(c) a gap of 16 of 160 with ridge 1e-6 at n = 65, (d) the identity (w = 1), (e) c = (1, 2, 0, ...), not positive definite.
(b) and (c) exist at n = 65 only: a gap of the same relative width at larger n has a condition number beyond 1 / EPS and
fails the soundness condition, so the mixed batches of other orders hold (a) with several seeds and (d).
"""
import functools

import numpy as np

EPS = np.finfo(np.float64).eps
FACTOR = 4.0
E_REF_MAX = 1e-8
NRHS_MAX = 8


def random_mask(ntime, fraction, seed):
    """0/1 weights with exactly round(fraction * ntime) samples flagged, chosen by a seeded permutation."""
    w = np.ones(ntime)
    w[np.random.default_rng(seed).permutation(ntime)[: int(round(fraction * ntime))]] = 0.0
    return w


def gap_mask(ntime, start, length):
    w = np.ones(ntime)
    w[(start + np.arange(length)) % ntime] = 0.0
    return w


def column(w, n, ridge=0.0):
    """c_d = (1 / ntime) sum_t w_t e^{-2 pi i d t / ntime}, d < n, with ridge * c_0 added to c_0."""
    ntime = w.shape[0]
    t, d = np.arange(ntime), np.arange(n)
    c = (w[:, None] * np.exp(-2j * np.pi * ((t[:, None] * d[None, :]) % ntime) / ntime)).sum(axis=0) / ntime
    c[0] = c[0].real * (1.0 + ridge)
    return c


def toeplitz(col, dtype=np.complex128):
    n = col.shape[0]
    k = np.arange(n)
    d = k[:, None] - k[None, :]
    c = col.astype(dtype)
    c[0] = c[0].real
    return np.where(d >= 0, c[np.abs(d)], c[np.abs(d)].conj())


def dense_solve_ld(T, B):
    """T X = B by blocked Gaussian elimination without pivoting (T Hermitian positive definite) in T's precision:
    T (n, n), B (n, r) np.clongdouble."""
    A, X = T.copy(), B.copy()
    n, nb = A.shape[0], 32
    for k0 in range(0, n, nb):
        k1 = min(n, k0 + nb)
        for k in range(k0, k1):
            A[k + 1 :, k] /= A[k, k]
            if k + 1 < k1:
                A[k + 1 :, k + 1 : k1] -= A[k + 1 :, k : k + 1] * A[k : k + 1, k + 1 : k1]
        if k1 < n:
            for k in range(k0, k1):
                A[k + 1 : k1, k1:] -= A[k + 1 : k1, k : k + 1] * A[k : k + 1, k1:]
            A[k1:, k1:] -= A[k1:, k0:k1] @ A[k0:k1, k1:]
    for k in range(n):
        X[k + 1 :] -= A[k + 1 :, k : k + 1] * X[k : k + 1]
    for k in range(n - 1, -1, -1):
        X[k] /= A[k, k]
        X[:k] -= A[:k, k : k + 1] * X[k : k + 1]
    return X


def forward_error(x, xref):
    """||x - xref||_2 / ||xref||_2 along the last axis, in long double."""
    x, xref = np.asarray(x, dtype=np.clongdouble), np.asarray(xref, dtype=np.clongdouble)
    return (np.sqrt((np.abs(x - xref) ** 2).sum(axis=-1)) / np.sqrt((np.abs(xref) ** 2).sum(axis=-1))).astype(np.float64)


def column_of(kind, n, seed=0):
    if kind == "a":
        return column(random_mask(int(np.ceil(2.5 * n)), 0.2 + 0.05 * (seed % 3), 100 + seed), n)
    if kind == "b":
        assert n == 65
        return column(gap_mask(160, 40, 10), n)
    if kind == "c":
        assert n == 65
        return column(gap_mask(160, 40, 16), n, ridge=1e-6)
    if kind == "d":
        c = np.zeros(n, dtype=np.complex128)
        c[0] = 1.0
        return c
    if kind == "e":
        c = np.zeros(n, dtype=np.complex128)
        c[0] = 1.0
        if n > 1:
            c[1] = 2.0
        return c
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def case(kind, n, seed=0):
    """One system with NRHS_MAX right-hand sides: col (n,), B (NRHS_MAX, n) double, Xref (NRHS_MAX, n) clongdouble,
    cond, e_ref (NRHS_MAX,) of scipy and bound (NRHS_MAX,).  Computed once and shared; do not write to it."""
    import scipy.linalg

    col = column_of(kind, n, seed)
    rng = np.random.default_rng(1000 * n + 10 * seed + ord(kind))
    X0 = rng.standard_normal((NRHS_MAX, n)) + 1j * rng.standard_normal((NRHS_MAX, n))
    Tld = toeplitz(col, np.clongdouble)
    B = (Tld @ X0.astype(np.clongdouble).T).T.astype(np.complex128)
    Xref = dense_solve_ld(Tld, B.astype(np.clongdouble).T).T
    ev = np.linalg.eigvalsh(toeplitz(col))
    cond = float(ev[-1] / ev[0])
    xs = scipy.linalg.solve_toeplitz(col, B.T).T
    e_ref = forward_error(xs, Xref)
    out = dict(kind=kind, n=n, col=col, B=B, Xref=Xref, cond=cond, e_ref=e_ref,
               bound=FACTOR * np.maximum(e_ref, EPS * cond))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def pool(n):
    """The distinct systems of the mixed batches of order n."""
    kinds = [("a", 0), ("a", 1), ("d", 0), ("a", 2)]
    if n == 65:
        kinds += [("b", 0), ("c", 0)]
    return [case(k, n, s) for k, s in kinds]


def check(x, cs, nrhs=None, what=""):
    """Assert that x (nrhs, n) solves case `cs` within the bound and that the case is sound; returns (errors, bounds)."""
    nrhs = x.shape[0] if nrhs is None else nrhs
    assert float(cs["e_ref"].max()) <= E_REF_MAX, "%s: scipy itself is off by %.3g on system (%s) of order %d" % (
        what, cs["e_ref"].max(), cs["kind"], cs["n"])
    err = forward_error(x[:nrhs], cs["Xref"][:nrhs])
    assert np.all(np.isfinite(err)) and np.all(err <= cs["bound"][:nrhs]), \
        "%s: system (%s) n = %d: forward error %s beyond %s (cond %.3g, e_ref %.3g)" % (
            what, cs["kind"], cs["n"], err, cs["bound"][:nrhs], cs["cond"], cs["e_ref"].max())
    return err, cs["bound"][:nrhs]


# ---- signals and weights of the m-mode tests -----------------------------------------------------------------------------
def band_limited(rng, nf, npairs, mmax, ntime):
    """(x (nf, npairs, ntime), a (nf, npairs, 2 mmax + 1)): x_t = sum_k a_k e^{2 pi i k t / ntime}, k = -mmax .. mmax."""
    N = 2 * mmax + 1
    a = rng.standard_normal((nf, npairs, N)) + 1j * rng.standard_normal((nf, npairs, N))
    k, t = np.arange(-mmax, mmax + 1), np.arange(ntime)
    F = np.exp(2j * np.pi * ((t[:, None] * k[None, :]) % ntime) / ntime)
    return a @ F.T, a


def modes_layout(a, mmax):
    """Coefficients a (nf, npairs, 2 mmax + 1) in k = -mmax .. mmax order as (mmax + 1, nf, 2, npairs) mode files."""
    nf, npairs, _ = a.shape
    out = np.zeros((mmax + 1, nf, 2, npairs), dtype=a.dtype)
    out[:, :, 0] = a[:, :, mmax:].transpose(2, 0, 1)
    out[1:, :, 1] = a[:, :, :mmax][:, :, ::-1].conj().transpose(2, 0, 1)
    return out


def modes_unlayout(v):
    """The inverse of `modes_layout`: (nf, npairs, 2 mmax + 1)."""
    mmax = v.shape[0] - 1
    return np.concatenate([v[1:, :, 1][::-1].conj().transpose(1, 2, 0), v[:, :, 0].transpose(1, 2, 0)], axis=-1)


def row_bounds(x, w, mmax, ridge=0.0):
    """Per (frequency, pair) the allowed ||device - host||_2 of the weighted modes (nf, npairs):
    FACTOR * max(e_ref, EPS cond) ||a||_2 for the Toeplitz solve — e_ref the distance of scipy's Toeplitz solve from the
    dense host solution of the same system — plus 4 (ntime + 2) EPS sum_t |w x| / ntime for the transform of w x."""
    import scipy.linalg

    from driftscan_amd import timestream

    nf, npairs, ntime = x.shape
    N = 2 * mmax + 1
    wb = np.broadcast_to(w[:, None, :] if w.ndim == 2 else w, x.shape)
    host, info = timestream.mmodes_weighted_host(x, w, mmax, ridge=ridge)
    a = modes_unlayout(host)
    k, t = np.arange(-mmax, mmax + 1), np.arange(ntime)
    F = np.exp(2j * np.pi * ((t[:, None] * k[None, :]) % ntime) / ntime)
    out = np.zeros((nf, npairs))
    for f in range(nf):
        for p in range(npairs):
            if info[f, p] != 0:
                continue
            col = column(wb[f, p], N, ridge=ridge)
            b = F.conj().T @ (wb[f, p] * x[f, p]) / ntime
            ev = np.linalg.eigvalsh(toeplitz(col))
            e_ref = float(forward_error(scipy.linalg.solve_toeplitz(col, b), a[f, p]))
            out[f, p] = (FACTOR * max(e_ref, EPS * ev[-1] / ev[0]) * np.linalg.norm(a[f, p])
                         + 4.0 * (ntime + 2) * EPS * np.abs(wb[f, p] * x[f, p]).sum() / ntime)
    return host, info, out
