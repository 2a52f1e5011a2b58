"""Shared cases and the checker of the noise-inflation tests: the diagonal of the inverse of the
Toeplitz systems of tests/flags_cases.py in extended precision, and the bound a solver's diagonal must stay within.

The bound.  Every element of a diagonal d is compared with the dense inverse in np.clongdouble (`flags_cases.dense_solve_ld`
on the identity) of the system as rounded to double: |d_i - dref_i| <= K * max(e_ref, EPS * cond_2(A)) * dref_i, with e_ref
the largest such relative error of `timestream.toeplitz_inverse_diag_host` on the same system and cond_2 from eigvalsh.
K is 8: at the project's 4 (`flags_cases.FACTOR`) the solver alone stays below 0.25 of the bound at every order tested,
but the inflation of `mmode_transform_weighted`, whose first columns come out of a ZGEMM and carry its rounding into a
system of condition cond_2, reached 0.77; the rule fixed with these tests is the next power of two that brings the worst
ratio under 0.5 (never beyond 64).  The measured ratios are in DESIGN.md section 4.16.
"""
import functools

import numpy as np

import flags_cases as fc

EPS = fc.EPS
K = 8.0


@functools.lru_cache(maxsize=None)
def diag_case(kind, n, seed=0):
    """One system: col (n,), dref (n,) longdouble diagonal of the inverse, cond, e_ref and bound (relative, per element).
    Computed once and shared; do not write to it."""
    from driftscan_amd import timestream

    col = fc.column_of(kind, n, seed)
    if kind == "d":
        dref = np.ones(n, dtype=np.longdouble)
    else:
        inv = fc.dense_solve_ld(fc.toeplitz(col, np.clongdouble), np.eye(n, dtype=np.clongdouble))
        dref = inv.diagonal().real.copy()
    ev = np.linalg.eigvalsh(fc.toeplitz(col))
    cond = float(ev[-1] / ev[0])
    dh, info = timestream.toeplitz_inverse_diag_host(col)
    assert info == 0
    e_ref = float(np.max(np.abs(dh.astype(np.longdouble) - dref) / dref))
    out = dict(kind=kind, n=n, col=col, dref=dref, cond=cond, e_ref=e_ref, host=dh, bound=K * max(e_ref, EPS * cond))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def pool(n):
    """The distinct systems of the mixed batches of order n, those of `flags_cases.pool`."""
    kinds = [("a", 0), ("a", 1), ("d", 0), ("a", 2)]
    if n == 65:
        kinds += [("b", 0), ("c", 0)]
    return [diag_case(k, n, s) for k, s in kinds]


def rel_error(d, cs):
    """Per-element relative error of d (n,) against the long-double diagonal of case `cs`."""
    return (np.abs(np.asarray(d, dtype=np.longdouble) - cs["dref"]) / cs["dref"]).astype(np.float64)


def check(d, cs, what=""):
    """Assert that d is the diagonal of the inverse of case `cs` within the bound; returns the worst error / bound."""
    err = rel_error(d, cs)
    assert np.all(np.isfinite(err)) and np.all(err <= cs["bound"]), \
        "%s: system (%s) n = %d: relative error %.3g beyond %.3g (cond %.3g, e_ref %.3g)" % (
            what, cs["kind"], cs["n"], np.nanmax(err), cs["bound"], cs["cond"], cs["e_ref"])
    return float(err.max() / cs["bound"])


def inflation_of(d, mmax):
    """Diagonals d (nf, npairs, 2 mmax + 1) in k = -mmax .. mmax order in the layout of the mode files, 1.0 at
    (m = 0, slot 1)."""
    nf, npairs, _ = d.shape
    out = np.zeros((mmax + 1, nf, 2, npairs), dtype=np.float64)
    out[:, :, 0] = d[:, :, mmax:].transpose(2, 0, 1)
    out[1:, :, 1] = d[:, :, :mmax][:, :, ::-1].transpose(2, 0, 1)
    out[0, :, 1] = 1.0
    return out
