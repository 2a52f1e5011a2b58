"""CPU-only checks of the grouped-GEMM case table (tests/gemm_cases.py): the reference and its bound accept a correct
product and reject planted errors, and the table reaches every kernel class and tile kind that the planner of
dm_gemm.hip can produce — read from the library's own decisions through dm_zgemm_plan_info."""
import numpy as np
import pytest

import gemm_cases as gc
from driftscan_amd import _lib

pytestmark = pytest.mark.skipif(not gc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")

SOLO = [c["name"] for c in gc.CASES if c["solo"]]
ALL = [c["name"] for c in gc.CASES]


def test_table_size_and_edges():
    """About 150 problems (the four bulk entries of the chunk launch aside), the long K at M, N <= 130, and every
    edge of the issue's lists present."""
    assert 120 <= len(SOLO) <= 170
    E = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129}
    for cls in ("complex", "real_b", "all_real"):
        cs = [c for c in gc.CASES if c["cls"] == cls]
        assert E <= {c["M"] for c in cs} and E <= {c["N"] for c in cs}, cls
        assert {0, 1, 3, 4, 5, 15, 16, 17, 64, 129} <= {c["K"] for c in cs}, cls
    assert {159, 160, 255, 256, 257, 513} <= {c["N"] for c in gc.CASES if c["cls"] == "complex"}
    assert {160, 257, 513, 17, 129} <= {c["N"] for c in gc.CASES if c["cls"] == "real_b"}
    for c in gc.CASES:
        assert c["K"] < 512 or (c["M"] <= 130 and c["N"] <= 130), c["name"]
    deep = [c for c in gc.group_cases("deep")]
    for k in (512, 516, 520, 513, 518, 523):
        assert {(c["M"] % 64 == 0 and c["N"] % 64 == 0) for c in deep if c["K"] == k} == {True, False}, k
    cplx = [c for c in gc.CASES if c["cls"] != "all_real"]
    assert {(c["a_kfast"], c["b_kfast"], c["conjA"], c["conjB"]) for c in cplx if c["cls"] == "complex"} >= {
        (a, b, ca, cb) for a in (True, False) for b in (True, False) for ca, cb in ((False, False), (True, True))}
    assert {c["beta"] for c in cplx} >= {0.0, 1.0, -2.0} and {c["csc"] for c in cplx} == {1, 3}
    assert any(c["alpha"] == 0.0 and c["alpha_im"] != 0.0 for c in cplx)
    assert any(c["alpha"] != 0.0 and c["alpha_im"] != 0.0 for c in cplx)


@pytest.mark.parametrize("name", ALL)
def test_numpy_product_within_bound_and_mutants_outside(name):
    """numpy's own product passes the bound of the long-double reference; each mutant that the table does not list as
    inert for the case leaves the bound, and each inert one reproduces the product exactly."""
    d, ref = gc.cached(name)
    c = d.case
    mask = gc.tile_set(c)[None]
    re, im, _ = gc.reference(d, dtype=np.float64, want_bound=False)
    bad = gc.outside(d, ref, re, im) & mask
    assert not bad.any(), "%d elements of numpy's product outside the bound" % bad.sum()
    if c["beta"] == 0.0:
        assert np.isfinite(ref[0][np.broadcast_to(mask, ref[0].shape)].astype(np.float64)).all()
    for mut in gc.MUTANTS:
        mre, mim, _ = gc.reference(d, dtype=np.float64, mutant=mut, want_bound=False)
        if mut in c["inert"]:
            same = np.array_equal(mre, re, equal_nan=True) and (im is None or np.array_equal(mim, im, equal_nan=True))
            assert same, "%s is listed as inert for %s but changes the product" % (mut, name)
        else:
            assert (gc.outside(d, ref, mre, mim) & mask).any(), "mutant %s passes the bound on %s" % (mut, name)


def test_check_sees_poison_and_sentinels():
    """`check` itself: a clean result passes; a write outside the view, a NaN inside, a touched element outside the
    tile set of a triangular product each fail."""
    d, ref = gc.cached("c_lower_129")
    re, im, _ = gc.reference(d, dtype=np.float64, want_bound=False)
    good = d.C_buf.copy()
    good[d.iC] = re + 1j * im
    assert gc.check(d, ref, good) == []
    for where, value in ((0, 1.0), (int(d.iC[0, 0, 0]) + d.case["N"] * d.csc, 1.0), (int(d.iC[0, 5, 5]), np.nan),
                         (int(d.iC[0, 0, 100]), 0.0)):
        bad = good.copy()
        bad[where] = value
        assert len(gc.check(d, ref, bad)) == 1, where
    d, ref = gc.cached("c_aim_both_csc3")
    re, im, _ = gc.reference(d, dtype=np.float64, want_bound=False)
    good = d.C_buf.copy()
    good[d.iC] = re + 1j * im
    assert gc.check(d, ref, good) == []
    good[int(d.iC[0, 3, 3]) + 1] = 0.0   # between two columns of C
    assert len(gc.check(d, ref, good)) == 1


# ---- coverage, from the planner's own decisions --------------------------------------------------------------------
KINDS = ("complex", "complex_deep", "real_narrow", "real_wide", "gathered", "all_real")


def _kind(info, cls):
    if cls == 0:
        return "complex_deep" if info["deep"] else "complex"
    if cls == 1:
        return "real_wide" if info["wide_r"] else "real_narrow"
    return {2: "all_real", 3: "gathered"}[cls]


def _launches():
    """Every launch the GPU tests issue: each case alone, and each group."""
    out = [(n, gc.problems(gc.cached(n)[0])) for n in SOLO]
    for g in gc.GROUPS:
        out.append(("group " + g, sum((gc.problems(gc.cached(c["name"])[0]) for c in gc.group_cases(g)), [])))
    return out


def test_coverage_matrix():
    """{class} x {square, flat} x {interior, ragged} x {overwrite, read-modify-write}: every cell that
    dm_gemm_plan_build can produce holds at least one tile of the table, and the cells it cannot produce are empty:
    the all-real class has no flat tiles, and every tile of the gathered class is 'ragged' in the planner's sense
    (its operands are scaled, so the kernel takes its masked path).  Flat triangular products are the third
    impossible kind; the next test holds them."""
    cells = {k: np.zeros((2, 2, 2), dtype=np.int64) for k in KINDS}
    for _, probs in _launches():
        (info,) = _lib.zgemm_plan_info(probs)
        assert info["use4"], "the table is for the default (register-only) kernels"
        for cls in range(4):
            if info["tiles"][cls]:
                cells[_kind(info, cls)] += info["cells"][cls]
                assert info["cells"][cls].sum() == info["tiles"][cls]
                assert info["cells"][cls][1].sum() == info["flat"][cls]
    forbidden = {("all_real", 1, r, w) for r in (0, 1) for w in (0, 1)} | {("gathered", f, 0, w) for f in (0, 1) for w in (0, 1)}
    empty = []
    for k in KINDS:
        for f in (0, 1):
            for r in (0, 1):
                for w in (0, 1):
                    if (k, f, r, w) in forbidden:
                        assert cells[k][f, r, w] == 0, (k, f, r, w)
                    elif cells[k][f, r, w] == 0:
                        empty.append((k, "flat" if f else "square", "ragged" if r else "interior", "rmw" if w else "overwrite"))
    assert not empty, "cells without a tile: %s" % empty


def test_group_launch_decisions():
    """The per-launch decisions the groups are built for."""
    info = {g: _lib.zgemm_plan_info(sum((gc.problems(gc.cached(c["name"])[0]) for c in gc.group_cases(g)), []))[0]
            for g in gc.GROUPS}
    assert info["deep"]["deep"] and not info["complex"]["deep"]
    assert info["real_wide"]["wide_r"] and not info["real_narrow"]["wide_r"]
    assert any(c["N"] >= 160 for c in gc.group_cases("real_narrow")) and any(c["N"] < 160 for c in gc.group_cases("real_wide"))
    assert all(t > 0 for t in info["mixed"]["tiles"])
    assert info["chunk"]["tiles"] == [2050, 520, 520, 520]   # more than 8 x 256 and 8 x 64: a second round of chunks
    # every deep case alone is a deep launch, every K < 512 complex case is not
    for c in gc.CASES:
        if c["cls"] == "complex" and c["solo"] and c["M"] and c["N"]:
            assert _lib.zgemm_plan_info(gc.problems(gc.cached(c["name"])[0]))[0]["deep"] == (c["K"] >= 512), c["name"]


def test_triangular_products_are_square_tiles_of_the_tile_set():
    tri = [c for c in gc.CASES if c["tri"]]
    assert len(tri) == 12
    for c in tri:
        (info,) = _lib.zgemm_plan_info(gc.problems(gc.cached(c["name"])[0]))
        assert info["flat"] == [0, 0, 0, 0], c["name"]
        assert info["tiles"][0] == len(np.unique(np.argwhere(gc.tile_set(c)) // 64, axis=0)), c["name"]


# ---- refused flag combinations -------------------------------------------------------------------------------------
@pytest.mark.parametrize("label,prob", gc.refused_problems(), ids=[x[0] for x in gc.refused_problems()])
def test_plan_info_refuses(label, prob):
    with pytest.raises(_lib.DriftMIError):
        _lib.zgemm_plan_info([prob])
    # also behind a good launch, and the good one alone passes
    good = dict(M=8, N=8, K=4, rsA=4, csA=1, rsB=8, csB=1, ldc=8, launch=0)
    assert _lib.zgemm_plan_info([good])[0]["tiles"] == [1, 0, 0, 0]
    with pytest.raises(_lib.DriftMIError):
        _lib.zgemm_plan_info([good, dict(prob, launch=1)])


def test_wrapper_view_checks():
    """Host arithmetic of `zgemm_ex_check_views` (nothing reaches the library): the exact extent passes, one element
    less raises, for A, B, gathered B, kscale, gathered weights, and C through ldc and csc."""
    p = dict(M=5, N=7, K=3, rsA=4, csA=1, rsB=9, csB=1, ldc=30, csc=3, a_off=2, b_off=1, c_off=6, ks_off=2,
             has_kscale=True)
    nA, nB, nC, nks = 2 + 4 * 4 + 2 + 1, 1 + 2 * 9 + 6 + 1, 6 + 4 * 30 + 6 * 3 + 1, 2 + 3
    _lib.zgemm_ex_check_views(p, nA, nB, nC, nks)
    for short in ((nA - 1, nB, nC, nks), (nA, nB - 1, nC, nks), (nA, nB, nC - 1, nks), (nA, nB, nC, nks - 1)):
        with pytest.raises(ValueError):
            _lib.zgemm_ex_check_views(p, *short)
    g = np.array([[0, 4]] * 6 + [[10, 0]], dtype=np.int32)
    q = dict(p, flags=_lib.ZGEMM_B_GATHER, bgather=g, rsB=2, csB=0)
    nB, nks = 1 + 10 + 2 * 2 + 1, 2 + 4 + 3
    _lib.zgemm_ex_check_views(q, nA, nB, nC, nks)
    for short in ((nA, nB - 1, nC, nks), (nA, nB, nC, nks - 1)):
        with pytest.raises(ValueError):
            _lib.zgemm_ex_check_views(q, *short)
    for bad in (dict(q, bgather=g[:6]), dict(q, bgather=-g), dict(p, rsA=-1), dict(p, M=-1), dict(p, c_off=-1)):
        with pytest.raises(ValueError):
            _lib.zgemm_ex_check_views(bad, nA, nB, nC, nks)
    _lib.zgemm_ex_check_views(dict(p, M=0), 0, 0, 0, 0)   # nothing is touched
    _lib.zgemm_ex_check_views(dict(p, K=0), 0, 0, nC, 0)  # only C
    # every case of the table passes with its own buffers, and not with any of them one element shorter
    for c in gc.CASES:
        d = gc.cached(c["name"])[0]
        sizes = [d.A_buf.size, d.B_buf.size, d.C_buf.size, d.ks_buf.size if d.ks_buf is not None else 0]
        for pr in gc.problems(d)[-1:]:
            _lib.zgemm_ex_check_views(pr, *sizes)
            if c["M"] and c["N"]:
                with pytest.raises(ValueError):
                    _lib.zgemm_ex_check_views(pr, sizes[0], sizes[1], sizes[2] - d.csc - 2 * gc.PAD, sizes[3])
