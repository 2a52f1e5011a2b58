"""CPU-only checks of the Cholesky / triangular-solve case tables (tests/chol_cases.py): the tables cover what they
claim, LAPACK's results pass every bound and every exact condition, planted errors are rejected, and the host-only
argument checkers of the library refuse what they must."""
import numpy as np
import pytest
import scipy.linalg
import scipy.linalg.lapack

import chol_cases as cc
from driftscan_amd import _lib

pytestmark = pytest.mark.skipif(not cc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")

EARG = -1


# ---- LAPACK as the stand-in for a correct device --------------------------------------------------------------------
def lapack_potrf(lay):
    out, info = lay.buf.copy(), []
    for c, w in zip(lay.cases, lay.win):
        if c["n"] == 0:
            info.append(0)
            continue
        # the lower triangle and the real part of the diagonal are the input, as for the device
        V = np.tril(lay.buf[w])
        V[np.arange(c["n"]), np.arange(c["n"])] = V.diagonal().real
        L, i = scipy.linalg.lapack.zpotrf(V, lower=1, clean=1)
        info.append(int(i))
        if i == 0:
            out[w] = L
    return out, np.array(info)


def lapack_trsm(lay, mutate=None):
    out = lay.B_buf.copy()
    for k, (c, w) in enumerate(zip(lay.cases, lay.wB)):
        if c["n"] == 0 or c["nrhs"] == 0:
            continue
        X = scipy.linalg.solve_triangular(lay.L[k], lay.B[k], lower=True, trans="C" if c["conjtrans"] else "N")
        out[w] = mutate(k, c, X) if mutate else X
    return out


# ---- coverage -------------------------------------------------------------------------------------------------------
def test_tables_are_reproducible_and_cover_their_lists():
    assert [c["name"] for c in cc._build_trsm()] == [c["name"] for c in cc.TRSM_CASES]
    assert np.array_equal(cc.hpd("spec10", 33), cc.hpd("spec10", 33))
    names = [c["name"] for c in cc.POTRF_CASES + cc.TRSM_CASES + cc.UPPER_CASES + cc.INFO_CASES]
    assert len(set(names)) == len(names)
    # factorisation: every family at every size and padding; every residue of n around 32 and 64
    assert {(c["family"], c["n"], c["ld"] - c["n"]) for c in cc.POTRF_CASES} == {
        (f, n, p) for f in cc.FAMILIES for n in cc.POTRF_N for p in cc.LD_PADS}
    assert set(cc.POTRF_N) == {0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 160, 193, 257}
    assert set(cc.LD_PADS) == {0, 1, 7}
    for m in (32, 64):
        assert {n % m for n in cc.POTRF_N if n > 2} >= {m - 1, 0, 1}
    assert {n % 32 for n in cc.TRSM_N} >= {31, 0, 1} and {n % 64 for n in cc.TRSM_N} >= {0, 1}
    order = [c["n"] for c in cc.mixed_order(cc.potrf_group("wishart", 1))]
    assert sorted(order) == sorted(cc.POTRF_N) and order != sorted(order) and order != sorted(order, reverse=True)
    lay = cc.potrf_layout(cc.mixed_order(cc.potrf_group("wishart", 7)))
    ends = [o + max(c["n"] - 1, 0) * c["ld"] + c["n"] for c, o in zip(lay.cases, lay.off)]
    assert all(o2 - e1 >= cc.GAP for e1, o2 in zip(ends, lay.off[1:]))   # gaps between the problems of one buffer
    # solves
    for conj in (False, True):
        cs = [c for c in cc.TRSM_CASES if c["conjtrans"] == conj]
        per_n = {n: {c["nrhs"] for c in cs if c["n"] == n} for n in cc.TRSM_N}
        assert all(len(v) >= 2 for v in per_n.values()), per_n
        for n in cc.TRSM_NRHS_N:
            assert per_n[n] == set(cc.TRSM_NRHS)
        assert all(c["nrhs"] <= 64 for c in cs if c["n"] >= 385)
        pads = [c["ldl"] > c["n"] for c in cs]
        assert abs(sum(pads) - len(pads) / 2) <= 1 and all((c["ldl"] > c["n"]) == (c["ldb"] > c["nrhs"]) for c in cs)
        assert {c["family"] for c in cs} == set(cc.FAMILIES)
    assert set(cc.TRSM_N) == {1, 31, 32, 33, 64, 65, 80, 96, 97, 128, 129, 200, 257, 385, 449}
    assert set(cc.TRSM_NRHS) == {1, 63, 64, 255, 256, 257, 300}
    # both 256-column workgroups of the substitution kernel, and their edges
    assert {(r + 255) // 256 for r in cc.TRSM_NRHS} == {1, 2} and {255, 256, 257} <= set(cc.TRSM_NRHS)
    # the recursive update reaches s = 6 and s = 7 (64-row super blocks), sizes 1, 2 and 4
    smax = {n: (n + 63) // 64 - 1 for n in cc.TRSM_N}
    assert smax[385] == 6 and smax[449] == 7 and max(smax.values()) == 7
    assert min(n for n in range(1, 500) if (n + 63) // 64 - 1 >= 6) == 385
    assert min(n for n in range(1, 500) if (n + 63) // 64 - 1 >= 7) == 449
    assert {s & -s for s in range(1, 8)} == {1, 2, 4}
    # one backward launch with odd and even numbers of 32-row blocks, the small problems starting late
    for conj in (False, True):
        mixed = cc.trsm_mixed(conj)
        assert [c["n"] for c in mixed] == [449, 80, 200, 64, 1]
        assert {((c["n"] + 31) // 32) % 2 for c in mixed} == {0, 1}
        assert ((80 + 31) // 32) % 2 == 1 and ((200 + 31) // 32) % 2 == 1
        empty = cc.trsm_empty(conj)
        assert sum(c["n"] == 0 for c in empty) == 1 and sum(c["nrhs"] == 0 and c["n"] > 0 for c in empty) == 1
        assert sum(c["n"] > 0 and c["nrhs"] > 0 for c in empty) >= 2
    # upper_only: nrhs == n, first_col at the start of the second 256-column workgroup, the Gram-shaped B
    assert [c["n"] for c in cc.UPPER_CASES] == [1, 33, 64, 65, 129, 257, 320]
    assert all(c["nrhs"] == c["n"] and c["upper_only"] and not c["conjtrans"] for c in cc.UPPER_CASES)
    assert ((320 - 1) // 64) * 64 == 256
    assert sum(c["gram"] for c in cc.UPPER_CASES) == 1
    # info
    got = {(c["n"], c["j"]) for c in cc.INFO_CASES if c["what"] == "pivot"}
    assert got == {(n, j) for n in cc.INFO_N for j in (0, 31, 32, 63, 64, 95, 96, n - 1) if j < n}
    assert {c["what"] for c in cc.INFO_CASES} == {"pivot", "zero", "nan", "inf"}
    assert all(c["i"] > c["j"] for c in cc.INFO_CASES if c["what"] == "nan")


# ---- LAPACK passes ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_lapack_factor_within_bound(family):
    worst = 0.0
    for variant in (None, "nan_upper", "imag_diag"):
        lay = cc.potrf_layout(cc.mixed_order(cc.potrf_group(family, 1, variant)))
        out, info = lapack_potrf(lay)
        fails, r = cc.check_potrf(lay, out, info)
        assert not fails, "\n".join(fails[:10])
        worst = max(worst, r)
    print("LAPACK zpotrf, %s: worst ratio to the bound %.3f" % (family, worst))
    assert 0.0 < worst < 1.0


@pytest.mark.parametrize("which", ["forward", "backward", "upper_only", "mixed"])
def test_lapack_solves_within_bound(which):
    worst = {}
    if which == "mixed":
        groups = [cc.trsm_mixed(False), cc.trsm_mixed(True), cc.trsm_empty(False), cc.trsm_empty(True), cc.UPPER_CASES]
        for g in groups:   # the layout of a whole launch, then one by one: the worst ratio is kept per family
            lay = cc.trsm_layout(g)
            assert not cc.check_trsm(lay, lapack_trsm(lay))[0]
        groups = [[c] for g in groups for c in g]
    elif which == "upper_only":
        groups = [[c] for c in cc.UPPER_CASES]
    else:
        groups = [[c] for c in cc.TRSM_CASES if c["conjtrans"] == (which == "backward")]
    for g in groups:
        lay = cc.trsm_layout(g)
        fails, r = cc.check_trsm(lay, lapack_trsm(lay))
        assert not fails, "\n".join(fails[:10])
        worst[g[0]["family"]] = max(worst.get(g[0]["family"], 0.0), r)
    for f in cc.FAMILIES:
        print("LAPACK ztrsm, %s, %s: worst ratio to the bound %.3f" % (which, f, worst[f]))
        assert 0.0 < worst[f] < 1.0


def test_lapack_info_matches_the_expected_index():
    """LAPACK returns exactly the planted index for the pivot and the zero cases (the NaN and Inf rules are the
    project's own contract and are not compared)."""
    cases = [c for c in cc.INFO_CASES if c["what"] in ("pivot", "zero")]
    lay = cc.potrf_layout(cases)
    out, info = lapack_potrf(lay)
    assert [int(i) for i in info] == [c["expect_info"] for c in cases]
    fails, _ = cc.check_potrf(lay, out, info)
    assert not fails, fails[:5]


# ---- planted errors ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", cc.FAMILIES)
@pytest.mark.parametrize("n", [33, 129, 257])
def test_planted_factor_errors_are_rejected(family, n):
    lay = cc.potrf_layout([cc.potrf_case(family, n, 1)])
    good, info = lapack_potrf(lay)
    assert not cc.check_potrf(lay, good, info)[0]
    w = lay.win[0]
    # one element off by 1e-12 relative: (n - 1, 0), whose inner product has the one term L[n-1, 0] L[0, 0], so that
    # the bound there is (2n + 10) 2^-53 of that term in every family (an element deep inside a row of an
    # ill-conditioned factor is allowed more than 1e-12 of itself by a backward bound)
    bad = good.copy()
    bad[w[n - 1, 0]] *= 1.0 + 1e-12
    assert cc.check_potrf(lay, bad, info)[0]
    # one dropped term of one inner product: L[i, j] as if the term k had not been subtracted
    L = good[w]
    i, j, k = n - 2, n // 2, n // 4
    bad = good.copy()
    bad[w[i, j]] += L[i, k] * np.conj(L[j, k]) / L[j, j]
    assert cc.check_potrf(lay, bad, info)[0]
    # exact conditions: a non-zero in the upper triangle, an imaginary part on the diagonal, a changed element of the
    # ld padding, info off by one
    for idx, val in ((w[0, n - 1], 1e-300), (w[1, 1], good[w[1, 1]] + 1e-300j), (w[0, n - 1] + 1, 0.0)):
        bad = good.copy()
        bad[idx] = val
        assert cc.check_potrf(lay, bad, info)[0]
    assert cc.check_potrf(lay, good, info + 1)[0]


def test_planted_info_errors_are_rejected():
    cases = [c for c in cc.INFO_CASES if c["what"] == "pivot"]
    lay = cc.potrf_layout(cases)
    out, info = lapack_potrf(lay)
    assert not cc.check_potrf(lay, out, info)[0]
    for d in (1, -1):
        for k in (0, len(cases) - 1):
            off = info.copy()
            off[k] += d
            assert cc.check_potrf(lay, out, off)[0]


@pytest.mark.parametrize("conj", [False, True])
def test_planted_solve_errors_are_rejected(conj):
    for c in [c for c in cc.TRSM_CASES if c["conjtrans"] == conj and c["n"] in (65, 97, 200, 449)]:
        lay = cc.trsm_layout([c])
        good = lapack_trsm(lay)
        assert not cc.check_trsm(lay, good)[0]
        n = c["n"]
        last = slice(((n - 1) // 32) * 32, n) if not conj else slice(0, min(32, n))   # the block solved last

        def skip_last(k, c, X):
            X = X.copy()
            X[last] = lay.B[k][last]
            return X

        def wrong_op(k, c, X):
            return scipy.linalg.solve_triangular(lay.L[k], lay.B[k], lower=True, trans="N" if conj else "C")

        def one_off(k, c, X):
            X = X.copy()
            X[n // 2, c["nrhs"] - 1] *= 1.0 + 1e-11
            return X

        for mut in (skip_last, wrong_op, one_off):
            assert cc.check_trsm(lay, lapack_trsm(lay, mut))[0], (c["name"], mut.__name__)
        # one poisoned element outside the window: right of the last column, and behind the last row
        w = lay.wB[0]
        for idx in (w[0, -1] + 1 if c["ldb"] > c["nrhs"] else w[-1, -1] + 1, w[-1, -1] + c["ldb"]):
            bad = good.copy()
            bad[idx] = 0.0
            assert cc.check_trsm(lay, bad)[0], c["name"]


def test_planted_upper_only_errors_are_rejected():
    for c in cc.UPPER_CASES:
        lay = cc.trsm_layout([c])
        n = c["n"]
        garbage = lambda k, c, X: np.triu(X) + np.tril(np.full_like(X, cc.POISON), -1)   # noqa: E731
        good = lapack_trsm(lay, garbage)
        assert not cc.check_trsm(lay, good)[0], c["name"]   # what lies below the diagonal is not looked at

        def wrong_diag(k, c, X):
            X = garbage(k, c, X)
            X[n // 2, n // 2] *= 1.0 + 1e-11
            return X

        assert cc.check_trsm(lay, lapack_trsm(lay, wrong_diag))[0], c["name"]
        if n > 1:
            def wrong_corner(k, c, X):
                X = garbage(k, c, X)
                X[0, n - 1] *= 1.0 + 1e-11
                return X

            assert cc.check_trsm(lay, lapack_trsm(lay, wrong_corner))[0], c["name"]


# ---- the library's host-only argument checks ----------------------------------------------------------------------------
def test_checkers_accept_every_case_of_the_module():
    for pad in cc.LD_PADS:
        lay = cc.potrf_layout(cc.mixed_order(cc.potrf_group("graded", pad)))
        assert _lib.zpotrf_problems_check(cc.potrf_problems(lay)) == 0
    assert _lib.zpotrf_problems_check(cc.potrf_problems(cc.potrf_layout(cc.INFO_CASES))) == 0
    assert _lib.zpotrf_problems_check([]) == 0 and _lib.ztrsm_problems_check([]) == 0
    for conj in (False, True):
        groups = [[c for c in cc.TRSM_CASES if c["conjtrans"] == conj], cc.trsm_mixed(conj), cc.trsm_empty(conj)]
        for g in groups:
            assert _lib.ztrsm_problems_check(cc.trsm_problems(cc.trsm_layout(g)), conjtrans=conj) == 0
    assert _lib.ztrsm_problems_check(cc.trsm_problems(cc.trsm_layout(cc.UPPER_CASES)), upper_only=True) == 0
    # empty problems may come without their matrices
    assert _lib.zpotrf_problems_check([dict(n=0, ld=0, a_null=True)]) == 0
    assert _lib.ztrsm_problems_check([dict(n=0, nrhs=4, ldl=0, ldb=4, l_null=True, b_null=True),
                                      dict(n=4, nrhs=0, ldl=4, ldb=0, l_null=True, b_null=True)]) == 0


def test_checkers_refuse_bad_arguments():
    good = dict(n=8, ld=8)
    for bad in (dict(n=-1, ld=8), dict(n=8, ld=7), dict(n=8, ld=-8), dict(n=1, ld=0), dict(n=8, ld=8, a_null=True)):
        assert _lib.zpotrf_problems_check([bad]) == EARG, bad
        assert _lib.zpotrf_problems_check([good, bad]) == EARG, bad
    assert _lib.zpotrf_problems_check([good, dict(n=0, ld=0)]) == 0
    tg = dict(n=8, nrhs=5, ldl=8, ldb=5)
    for bad in (dict(tg, n=-1), dict(tg, nrhs=-1), dict(tg, ldl=7), dict(tg, ldb=4), dict(tg, ldl=-8), dict(tg, ldb=-5),
                dict(tg, l_null=True), dict(tg, b_null=True)):
        for conj in (False, True):
            assert _lib.ztrsm_problems_check([bad], conjtrans=conj) == EARG, bad
            assert _lib.ztrsm_problems_check([tg, bad], conjtrans=conj) == EARG, bad
    sq = dict(n=8, nrhs=8, ldl=8, ldb=9)
    assert _lib.ztrsm_problems_check([sq], upper_only=True) == 0
    assert _lib.ztrsm_problems_check([sq], conjtrans=True, upper_only=True) == EARG   # upper_only with conjtrans
    assert _lib.ztrsm_problems_check([sq, tg], upper_only=True) == EARG               # upper_only with nrhs != n
    assert _lib.ztrsm_problems_check([dict(sq, nrhs=9, ldb=9)], upper_only=True) == EARG
    assert _lib.ztrsm_problems_check([sq, dict(n=0, nrhs=3, ldl=0, ldb=3)], upper_only=True) == EARG
    lib = _lib.load()
    assert lib.dm_zpotrf_problems_check(-1, None) == EARG and lib.dm_zpotrf_problems_check(1, None) == EARG
    assert lib.dm_ztrsm_problems_check(-1, None, 0, 0) == EARG and lib.dm_ztrsm_problems_check(1, None, 0, 0) == EARG


def test_view_checks_refuse_a_view_that_runs_past_its_tensor():
    """Host arithmetic of `zpotrf_check_view` / `ztrsm_check_views` (nothing reaches the library): the exact extent
    passes, one element less does not."""
    p = dict(n=5, ld=8, a_off=3)
    need = 3 + 4 * 8 + 5
    _lib.zpotrf_check_view(p, need)
    with pytest.raises(ValueError):
        _lib.zpotrf_check_view(p, need - 1)
    for bad in (dict(p, n=-1), dict(p, ld=-1), dict(p, a_off=-1)):
        with pytest.raises(ValueError):
            _lib.zpotrf_check_view(bad, 1000)
    _lib.zpotrf_check_view(dict(n=0, ld=0, a_off=7), 0)   # nothing is touched
    t = dict(n=5, nrhs=3, ldl=6, ldb=4, l_off=2, b_off=1)
    nl, nb = 2 + 4 * 6 + 5, 1 + 4 * 4 + 3
    _lib.ztrsm_check_views(t, nl, nb)
    for short in ((nl - 1, nb), (nl, nb - 1)):
        with pytest.raises(ValueError):
            _lib.ztrsm_check_views(t, *short)
    for bad in (dict(t, n=-1), dict(t, nrhs=-1), dict(t, l_off=-1), dict(t, b_off=-1), dict(t, ldb=-4)):
        with pytest.raises(ValueError):
            _lib.ztrsm_check_views(bad, 1000, 1000)
    _lib.ztrsm_check_views(dict(t, n=0), 0, 0)
    _lib.ztrsm_check_views(dict(t, nrhs=0), 0, 0)
    # every layout of the module lies inside its buffers, and not one element to spare is assumed
    lay = cc.potrf_layout(cc.mixed_order(cc.potrf_group("wishart", 7)))
    for q in cc.potrf_problems(lay):
        _lib.zpotrf_check_view(q, lay.buf.size)
    lay = cc.trsm_layout(cc.trsm_mixed(True))
    for q in cc.trsm_problems(lay):
        _lib.ztrsm_check_views(q, lay.L_buf.size, lay.B_buf.size)
        with pytest.raises(ValueError):
            _lib.ztrsm_check_views(q, lay.L_buf.size, q["b_off"] + (q["n"] - 1) * q["ldb"] + q["nrhs"] - 1)
