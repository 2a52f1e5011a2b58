"""Every kernel path of the batched Cholesky and of the triangular solves (dm_chol.hip) against the exact conditions and
the derived per-element bounds of tests/chol_cases.py, through dm_zpotrf_problems / dm_ztrsm_problems: every case in a
launch of its own and in its mixed launch.  The long-double residuals are formed once per distinct result (a launch that
reproduces a result bit for bit is not measured again).  Each test prints its worst ratio to the bound."""
import numpy as np
import pytest

import chol_cases as cc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not cc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")]

WORST = {}


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 28)
    yield c
    c.close()


def _note(kind, ratio):
    WORST[kind] = max(WORST.get(kind, 0.0), ratio)
    print("%s: worst ratio to the bound %.3f (so far %.3f)" % (kind, ratio, WORST[kind]))


# ---- factorisation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", cc.LD_PADS)
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_factor_each_size_alone(ctx, family, pad):
    fails, worst = [], 0.0
    for c in cc.potrf_group(family, pad):
        lay = cc.potrf_layout([c])
        f, r = cc.check_potrf(lay, *cc.run_potrf(ctx, lay))
        fails += f
        worst = max(worst, r)
    _note("factor", worst)
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("pad", cc.LD_PADS)
@pytest.mark.parametrize("family", cc.FAMILIES)
def test_factor_mixed_launch(ctx, family, pad):
    """All sizes in one launch, not in size order, with gaps between them in one buffer."""
    lay = cc.potrf_layout(cc.mixed_order(cc.potrf_group(family, pad)))
    fails, worst = cc.check_potrf(lay, *cc.run_potrf(ctx, lay))
    _note("factor", worst)
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("family", cc.FAMILIES)
def test_factor_reads_neither_the_upper_triangle_nor_the_imaginary_diagonal(ctx, family):
    """The factor is bit-identical with the strictly upper triangle of the input NaN instead of mirrored, and with a
    non-zero imaginary part on the input's diagonal."""
    outs = {}
    for variant in (None, "nan_upper", "imag_diag"):
        lay = cc.potrf_layout(cc.mixed_order(cc.potrf_group(family, 1, variant)))
        out, info = cc.run_potrf(ctx, lay)
        fails, _ = cc.check_potrf(lay, out, info)
        assert not fails, "%s: %s" % (variant, "\n".join(fails[:20]))
        outs[variant] = [out[w] for w in lay.win]
    for variant in ("nan_upper", "imag_diag"):
        for c, a, b in zip(lay.cases, outs[None], outs[variant]):
            assert np.array_equal(cc._bits(a), cc._bits(b)), "%s differs with %s" % (c["name"], variant)


def test_info_is_the_first_failing_pivot(ctx):
    """Exactly j + 1 for a negative pivot at j (what LAPACK returns on these matrices), 1 for the zero matrix, i + 1 for
    a NaN at (i, j) below the diagonal, j + 1 for +Inf on the diagonal; alone and all in one launch."""
    fails = []
    for c in cc.INFO_CASES:
        lay = cc.potrf_layout([c])
        fails += cc.check_potrf(lay, *cc.run_potrf(ctx, lay))[0]
    lay = cc.potrf_layout(cc.INFO_CASES)
    fails += cc.check_potrf(lay, *cc.run_potrf(ctx, lay))[0]
    assert not fails, "\n".join(fails[:20])


def test_failing_members_leave_the_others_alone(ctx):
    """The factors and the info of the good members of a mixed launch are bit-identical to a launch without the failing
    ones."""
    good = cc.mixed_order(cc.potrf_group("spec10", 1))
    lay0 = cc.potrf_layout(good)
    out0, info0 = cc.run_potrf(ctx, lay0)
    assert not cc.check_potrf(lay0, out0, info0)[0]
    bad = [c for c in cc.INFO_CASES if (c["what"], c["n"], c["j"]) in
           {("pivot", 97, 32), ("pivot", 130, 129), ("zero", 33, 0), ("nan", 65, 3), ("inf", 65, 40)}]
    assert len(bad) == 5
    mixed = list(good)
    for k, b in enumerate(bad):
        mixed.insert(3 * k + 1, b)
    lay1 = cc.potrf_layout(mixed)
    out1, info1 = cc.run_potrf(ctx, lay1)
    fails, _ = cc.check_potrf(lay1, out1, info1)
    assert not fails, "\n".join(fails[:20])
    at = {c["name"]: k for k, c in enumerate(mixed)}
    for k, c in enumerate(good):
        assert info1[at[c["name"]]] == info0[k] == 0
        assert np.array_equal(cc._bits(out1[lay1.win[at[c["name"]]]]), cc._bits(out0[lay0.win[k]])), c["name"]


def test_launches_of_empty_matrices(ctx):
    """n = 0 for every member is a valid launch with info = 0 (it used to ask for an empty grid), through both entry
    points; so is an empty list."""
    lay = cc.potrf_layout([cc.potrf_case("wishart", 0, p) for p in cc.LD_PADS])
    out, info = cc.run_potrf(ctx, lay)
    assert list(info) == [0, 0, 0] and cc.outside_changed(lay.buf, out, lay.in_window) == 0
    assert len(ctx.zpotrf_problems([])) == 0
    ctx.ztrsm_problems([])
    A = ctx.to_device(np.full(8, cc.POISON))
    assert list(ctx.zpotrf(A, 0, 0, stride=0, batch=3)) == [0, 0, 0]
    ctx.sync()
    assert np.isnan(A.cpu().numpy().real).all()


# ---- solves --------------------------------------------------------------------------------------------------------------
def _solve_groups(ctx, groups, conj, upper_only, kind):
    fails, worst = [], 0.0
    for g in groups:
        lay = cc.trsm_layout(g)
        f, r = cc.check_trsm(lay, cc.run_trsm(ctx, lay, conj, upper_only))
        fails += f
        worst = max(worst, r)
    _note(kind, worst)
    assert not fails, "\n".join(fails[:20])


@pytest.mark.parametrize("conj", [False, True], ids=["forward", "backward"])
def test_solve_each_case_alone(ctx, conj):
    _solve_groups(ctx, [[c] for c in cc.TRSM_CASES if c["conjtrans"] == conj], conj, False,
                  "backward solve" if conj else "forward solve")


@pytest.mark.parametrize("conj", [False, True], ids=["forward", "backward"])
def test_solve_mixed_launches(ctx, conj):
    """{449, 80, 200, 64, 1} in one launch (the backward launch starts the small problems late; 80 and 200 have an odd
    number of 32-row blocks), a launch with an n = 0 and an nrhs = 0 member, and every case of the table in one launch."""
    groups = [cc.trsm_mixed(conj), cc.trsm_empty(conj), cc.mixed_order([c for c in cc.TRSM_CASES if c["conjtrans"] == conj])]
    _solve_groups(ctx, groups, conj, False, "backward solve" if conj else "forward solve")


def test_upper_only_alone_and_mixed(ctx):
    """nrhs == n, the result checked on and above the diagonal: each size alone (320 puts first_col at the start of the
    second 256-column workgroup; 129 takes B = (L^-1 A)^H) and all in one launch."""
    _solve_groups(ctx, [[c] for c in cc.UPPER_CASES] + [cc.mixed_order(cc.UPPER_CASES)], False, True, "upper_only")


# ---- refused arguments ---------------------------------------------------------------------------------------------------
def test_refused_arguments_touch_nothing(ctx):
    from driftscan_amd import _lib

    n = 8
    A = ctx.to_device(np.full(4 * n * n, 7.0 + 0j))
    B = ctx.to_device(np.full(4 * n * n, 7.0 + 0j))
    good = dict(A=A, n=n, ld=n, a_off=0)
    for bad in (dict(good, ld=n - 1), dict(good, n=-1)):
        for probs in ([bad], [good, bad]):
            with pytest.raises((_lib.DriftMIError, ValueError)):
                ctx.zpotrf_problems(probs)
    tg = dict(L=A, B=B, n=n, nrhs=5, ldl=n, ldb=5)
    sq = dict(L=A, B=B, n=n, nrhs=n, ldl=n, ldb=n)
    for probs, kw in (([dict(tg, ldl=n - 1)], {}), ([dict(tg, ldb=4)], {}), ([sq, tg], dict(upper_only=True)),
                      ([sq], dict(upper_only=True, conjtrans=True)), ([tg, dict(tg, nrhs=-1)], dict(conjtrans=True))):
        with pytest.raises((_lib.DriftMIError, ValueError)):
            ctx.ztrsm_problems(probs, **kw)
    # the uniform entry points refuse a leading dimension shorter than a row as well
    with pytest.raises(_lib.DriftMIError):
        ctx.zpotrf(A, n, n - 1, stride=n * n, batch=2)
    with pytest.raises(_lib.DriftMIError):
        ctx.ztrsm(A, B, n, 5, n - 1, 5, batch=1)
    with pytest.raises(_lib.DriftMIError):
        ctx.ztrsm(A, B, n, 5, n, 4, batch=1)
    ctx.sync()
    assert bool((A == 7.0).all()) and bool((B == 7.0).all())
