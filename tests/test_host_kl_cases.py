"""CPU-only checks of the KL covariance-stage case tables (tests/kl_cases.py): the float64 restatements of the oracle
stay inside every bound and pin, every reference-level mutant leaves one on a named case, the tables reach every route of
the drivers, and the poison / layout helpers notice a flipped bit."""
import os

import numpy as np
import pytest

import kl_cases as kc
from oracle import kl as okl
from oracle import psfisher as opf

pytestmark = pytest.mark.skipif(not kc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")


# ---- float64 stand-ins for a correct device -------------------------------------------------------------------------
def _svbounds(sv):
    return np.concatenate([[0], np.cumsum(sv)]).astype(np.int64)


def _mirror_lower(sv, M):
    """What the mirror route does: the frequency blocks f' < f are the conjugate transposes of the others."""
    fr = np.repeat(np.arange(len(sv)), sv)
    low = fr[:, None] > fr[None, :]
    return np.where(low, np.conj(M.T), M)


def f64_cov(c):
    s = kc.SHAPES[c["shape"]]
    lay = kc.cov_layout(c)
    out = lay.buf.copy()
    beam, cl, sv, l0 = kc.beams(c["shape"]), kc.cl_table(c["shape"], c["sym_cl"]), kc.svnum_of(c["shape"]), kc.cov_l0(c)
    clm = np.zeros_like(cl)
    for pi, pj in kc.cov_pairs(c):
        clm[pi, pj] = cl[pi, pj]
    npol = s["P"] if c["npol"] is None else c["npol"]
    assert npol in (1, s["P"])
    for b in range(len(sv)):
        masked = beam[b].copy()
        masked[..., : min(max(int(l0[b]), 0), s["L"])] = 0.0
        val = okl.project_matrix_sky_to_svd(masked, sv[b], _svbounds(sv[b]), clm.transpose(0, 1, 4, 2, 3), temponly=npol == 1)
        if kc.cov_route(c) == "mirror":
            val = _mirror_lower(sv[b], val)
        v = kc.view(lay, out, b)
        v[...] = val if c["zero_first"] else v + val
    return out


def f64_diag(c):
    lay = kc.diag_layout(c)
    out = lay.buf.copy()
    ut, d = kc.diag_inputs(c["T"])
    sv = kc.svnum_of("tiles")
    for b in range(len(sv)):
        val = c["alpha"] * okl.project_matrix_diagonal_telescope_to_svd(ut[b], sv[b], _svbounds(sv[b]), d)
        v = kc.view(lay, out, b)
        if c["accumulate"]:
            fr = np.repeat(np.arange(len(sv[b])), sv[b])
            on = fr[:, None] == fr[None, :]
            v[on] = v[on] + val[on]
        else:
            v[...] = val
    return out


def f64_reg(c):
    lay = kc.reg_layout(c)
    out = lay.buf.copy()
    for b, n in enumerate(kc.REG_N):
        if n:
            v = kc.view(lay, out, b)
            v[np.diag_indices(n)] += c["reg"] * v.max()     # kltransform.py:289-290, as oracle.kl.sn_covariance has it
    return out


def f64_fisher():
    d = kc.fisher_inputs()
    L = kc.SHAPES["tiles"]["L"]
    out = []
    for b in range(len(d["ndof"])):
        masked = d["beam"][b].copy()
        masked[..., : min(max(int(d["l0"][b]), 0), L)] = 0.0
        out.append(opf.fisher_m(masked, d["svnum"][b], _svbounds(d["svnum"][b]), d["lam"][b], d["E"][b], d["cl"])[0])
    return np.stack(out)


# ---- the tables -----------------------------------------------------------------------------------------------------
def test_tables_cover_shapes_routes_and_edges(golden_dir):
    names = [c["name"] for c in kc.COV_CASES + kc.DIAG_CASES + kc.REG_CASES]
    assert len(set(names)) == len(names)
    assert kc.SHAPES == dict(small=dict(F=3, K=4, L=6, P=1), tiles=dict(F=5, K=30, L=7, P=1), pol=dict(F=3, K=12, L=6, P=4))
    for shape, s in kc.SHAPES.items():
        sv = kc.svnum_of(shape)
        assert sv.shape[1] == s["F"] and 4 <= len(sv) <= 5 and sv.max() == s["K"] and sv.min() == 0
    sv = kc.svnum_of("tiles")
    assert list(sv.sum(axis=1)) == [64, 65, 129, 150, 0]            # a tile, a tile + 1, two tiles + 1, ragged, empty
    live = sv[sv.sum(axis=1) > 0]
    assert (live[:, 0] == 0).any() and (live[:, -1] == 0).any() and (live[:, 1:-1] == 0).any()
    # the route rule of dm_project_cov: every route has a case, on "tiles" and, where pols matter, on "pol"
    routes = {}
    for c in kc.COV_CASES:
        routes.setdefault(kc.cov_route(c), set()).add(c["shape"])
    assert set(routes) == {"full", "mirror", "fallback", "accumulate"}
    assert routes["full"] >= {"tiles", "pol"} and routes["mirror"] >= {"tiles", "pol"} and routes["accumulate"] >= {"tiles", "pol"}
    by = kc.COV_BY_NAME
    assert kc.cov_route(by["pol_fallback_tq"]) == "fallback" and (0, 1) in kc.cov_pairs(by["pol_fallback_tq"])
    assert kc.cov_route(by["pol_dense_nomask_sym"]) == "fallback" and kc.cov_mask(by["pol_dense_nomask_sym"]) is None
    assert kc.cov_route(by["tiles_sym_accumulate"]) == "accumulate" and by["tiles_sym_accumulate"]["symmetric"]
    assert kc.cov_route(by["tiles_envfull"]) == "full" and kc.cov_route(dict(by["tiles_envfull"], env_full=False)) == "mirror"
    assert kc.cov_pairs(by["pol_npol1_nomask"]) == [(0, 0)] == kc.cov_pairs(by["pol_npol1_mask"])
    assert kc.cov_mask(by["pol_npol1_nomask"]) is None and kc.cov_mask(by["pol_npol1_mask"]) is not None
    assert len(kc.cov_pairs(by["pol_dense_nomask"])) == 16 and kc.cov_mask(by["pol_dense_nomask"]) is None
    for name in ("tiles_allmasked_zero", "tiles_allmasked_keep", "pol_allmasked_zero", "pol_allmasked_keep"):
        assert kc.cov_pairs(by[name]) == [] and by[name]["zero_first"] == name.endswith("zero")
    # l0: every value of the pool meets a non-empty block on the full, the mirror and the accumulate route
    for route in ("full", "mirror", "accumulate"):
        seen = set()
        for c in kc.COV_CASES:
            if kc.cov_route(c) == route and kc.cov_pairs(c):
                L = kc.SHAPES[c["shape"]]["L"]
                nd = kc.svnum_of(c["shape"]).sum(axis=1)
                seen |= {kc.l0_pool(L).index(int(v)) for v, n in zip(kc.cov_l0(c), nd) if n > 0}
        assert seen == set(range(6)), (route, seen)
    assert kc.l0_pool(7) == (0, 6, 7, -3, 9, 3)
    # project_diag and regularise
    assert {(c["T"], c["alpha"], c["accumulate"]) for c in kc.DIAG_CASES} == {
        (T, a, acc) for T in (1, 20, 67) for a in (1.0, 0.37) for acc in (False, True)}
    assert not kc.diag_inputs(20)[1][1].any() and (kc.diag_inputs(20)[1][0] != 0).all()
    assert sorted(kc.REG_N) == [0, 1, 2, 255, 256, 257, 300] and kc.REG_N[len(kc.REG_N) // 2] == 0
    assert {(c["design"], c["reg"]) for c in kc.REG_CASES} == {(d, r) for d in kc.REG_DESIGNS for r in (1e-14, 0.5)}
    for n in (255, 256, 257, 300):
        p, q = kc.tie_positions(n)
        assert p < kc.TIE_SPLIT <= q < n * n
        assert (p // 256) % 16 != (q // 256) % 16 and p // 4096 != q // 4096     # other workgroup, other stride pass
        for design, first_wins in (("tie_early", True), ("tie_late", False)):
            A = kc.reg_matrix(design, n).reshape(-1)
            assert A[p].real == A[q].real == A.real.max() and (A[p].imag > A[q].imag) == first_wins
            assert kc.lexmax(A) == (A[p] if first_wins else A[q]) == A.max()
    for n in (2, 255, 300):
        A = kc.reg_matrix("unique", n)
        i, j = np.unravel_index(int(np.argmax(A.real)), A.shape)
        assert i != j
        assert (kc.reg_matrix("negative", n).real < 0).all()
        assert int(np.argmax(kc.reg_matrix("last", n).real)) == n * n - 1
        assert not np.array_equal(A, A.conj().T)
    assert max(kc.REG_N) > 256      # the second workgroup of the diagonal update
    # fisher
    d = kc.fisher_inputs()
    assert list(zip(d["ndof"], d["nmodes"])) == [(150, 140), (129, 129), (65, 1), (64, 0), (0, 0)]
    assert list(d["l0"]) == [0, 3, 6, 0, 0] and d["cl"].shape[0] == 3
    assert np.array_equal(d["cl"], d["cl"].transpose(0, 1, 3, 2))
    assert set(kc.fisher_chunks()) == {0, 1, 2} and kc.fisher_chunks()[:2] == [2, 2]
    assert np.isnan(d["evecs_buf"][: kc.GAP]).all() and all(np.diff(d["evecs_off"]) >= kc.GAP)
    # eigh_gen
    assert kc.EIGH_NS == (33, 20, 0, 65, 7) and kc.EIGH_NS[kc.EIGH_ZERO] == 20
    g = np.load(os.path.join(golden_dir, "eigh_gen.npz"))
    spectra = [kc.pencil(n)[2] for i, n in enumerate(kc.EIGH_NS) if n and i != kc.EIGH_ZERO] + [g["npd_evals"]]
    for lam in spectra:     # the cut lies in a gap of every spectrum, 1e-3 lambda_max or more from each eigenvalue
        assert np.min(np.abs(lam - kc.EIGH_CUT)) >= 1e-3 * lam.max() and (np.diff(lam) > 0).all()
        assert 0 < np.searchsorted(lam, kc.EIGH_CUT) < lam.size
    for n in (33, 65, 7):
        A, B, _ = kc.pencil(n)
        assert np.array_equal(A, A.conj().T) and np.array_equal(B, B.conj().T) and np.linalg.cond(B) < 100
    assert not kc.pencil(20, zero=True)[0].any()


def test_layouts_have_gaps_and_notice_a_flipped_bit():
    c = kc.COV_BY_NAME["tiles_sym_accumulate"]
    lay = kc.cov_layout(c)
    ends = lay.off + np.array(lay.n) ** 2
    assert lay.off[0] == kc.GAP and all(lay.off[1:] - ends[:-1] == kc.GAP) and lay.buf.size == ends[-1] + kc.GAP
    assert np.isnan(lay.buf[~lay.in_view]).all() and np.isfinite(lay.buf[lay.in_view]).all()
    C0 = kc.view(lay, lay.buf, 2)
    assert not np.allclose(C0, C0.conj().T)
    assert np.isnan(kc.cov_layout(kc.COV_BY_NAME["tiles_full"]).buf).all()
    # a result equal to the reference passes; one flipped bit outside a view fails
    for c in (c, kc.COV_BY_NAME["small_full"]):
        good = kc.cov_refs_as_buffer(c)
        assert kc.check_cov(c, good) == ([], pytest.approx(0.0, abs=0.2))
        bad = good.copy()
        bits = bad.view(np.uint64)
        bits[2 * (kc.cov_layout(c).off[1] - 1)] ^= np.uint64(1)      # the real part of the element in front of block 1
        fails, _ = kc.check_cov(c, bad)
        assert len(fails) == 1 and "outside the views" in fails[0]
    c = kc.REG_CASES[0]
    good = kc.reg_expected(c)
    assert kc.check_reg(c, good) == []
    bad = good.copy()
    bad.view(np.uint64)[-1] ^= np.uint64(1)
    assert any("outside the views" in f for f in kc.check_reg(c, bad))
    bad = good.copy()
    kc.view(kc.reg_layout(c), bad, 2)[3, 4] += 1e-16      # an off-diagonal element moved by less than an ulp of 1
    assert bad[kc.reg_layout(c).off[2] + 3 * 255 + 4] != good[kc.reg_layout(c).off[2] + 3 * 255 + 4]
    assert any("off-diagonal" in f for f in kc.check_reg(c, bad))


# ---- the restatements stay inside every bound -----------------------------------------------------------------------
def test_float64_project_cov_is_inside_every_bound():
    worst = {}
    for c in kc.COV_CASES:
        fails, r = kc.check_cov(c, f64_cov(c))
        assert not fails, fails
        worst[c["name"]] = r
    print("project_cov, float64 restatement: worst err / bound %.3f (%s)" % (max(worst.values()), max(worst, key=worst.get)))
    assert 0.0 < max(worst.values()) <= 1.0
    # a block with l0 >= L is exactly zero, one with every pair masked too
    c = kc.COV_BY_NAME["tiles_full_rot0"]
    assert kc.cov_l0(c)[2] == 7 and not np.any(kc.cov_refs(c)[2][0]) and not np.any(kc.cov_refs(c)[2][1])
    assert all(not np.any(ref) for ref, _ in kc.cov_refs(kc.COV_BY_NAME["pol_allmasked_zero"]))


def test_float64_project_diag_is_inside_every_bound():
    worst = 0.0
    for c in kc.DIAG_CASES:
        fails, r = kc.check_diag(c, f64_diag(c))
        assert not fails, fails
        worst = max(worst, r)
    print("project_diag, float64 restatement: worst err / bound %.3f" % worst)
    assert 0.0 < worst <= 1.0
    # planted: an off-diagonal frequency block touched while accumulating, and one not cleared
    c = next(x for x in kc.DIAG_CASES if x["accumulate"] and x["T"] == 20)
    bad = f64_diag(c)
    lay = kc.diag_layout(c)
    kc.view(lay, bad, 3)[0, 149] *= 1.0 + 2.0 ** -52
    assert any("off-diagonal frequency" in f for f in kc.check_diag(c, bad)[0])
    c = next(x for x in kc.DIAG_CASES if not x["accumulate"] and x["T"] == 20)
    bad = f64_diag(c)
    kc.view(lay, bad, 3)[0, 149] = 1e-300
    assert kc.check_diag(c, bad)[0]


def test_numpy_regulariser_matches_every_case():
    for c in kc.REG_CASES:
        out = f64_reg(c)
        assert kc.check_reg(c, out) == [], c["name"]
        assert kc.same_bits(out, kc.reg_expected(c))
    # the single-rounding value differs from the two-rounding one somewhere, and is accepted as well
    c = next(x for x in kc.REG_CASES if x["design"] == "unique" and x["reg"] == 0.5)
    lay = kc.reg_layout(c)
    out = kc.reg_expected(c)
    for b, n in enumerate(kc.REG_N):
        two, one = kc.ref_regularise(kc.reg_matrix(c["design"], n), c["reg"])
        kc.view(lay, out, b)[np.arange(n), np.arange(n)] = one
    assert kc.check_reg(c, out) == []
    # (with reg = 0.5 the product is exact and with 1e-14 it is far below an ulp of the diagonal, so the two values agree
    # on the table; with a regulariser of order one they part in a few elements of a hundred)
    two, one = kc.ref_regularise(kc.reg_matrix("unique", 255), 0.3)
    assert 0 < (two != one).sum() < 128 and np.abs(two - one).max() <= 2.0 ** -51
    kc.view(lay, out, 6)[7, 7] += 2.0 ** -50
    assert any("neither" in f for f in kc.check_reg(c, out))


def test_float64_fisher_is_inside_the_pin():
    got = f64_fisher()
    fails, worst = kc.check_fisher(got)
    assert not fails, fails
    d = kc.fisher_inputs()
    dist = max(float(np.abs(got[b] - kc.ref_fisher(b)).max() / np.abs(kc.ref_fisher(b)).max()) for b in range(3))
    print("fisher: float64 restatement at %.2e max|F_ref| from the long-double value (pin 1e-12)" % dist)
    assert dist <= 1e-13 and worst <= 0.1
    assert not got[3].any() and not got[4].any() and d["nmodes"][3] == 0
    # the long-double value is Hermitian with a real diagonal, as a Gram matrix is
    F = kc.ref_fisher(0)
    assert np.abs(F - F.conj().T).max() <= 1e-18 * np.abs(F).max()


# ---- every mutant leaves a bound or the pin -------------------------------------------------------------------------
COV_MUTANT_CASE = dict(l0="tiles_full", lastl="tiles_full", mirror="tiles_mirror", weight_ff="tiles_full",
                       polswap="pol_fallback_tq", svoffset="tiles_full")


@pytest.mark.parametrize("mutant", kc.MUTANTS)
def test_every_mutant_is_caught(mutant):
    if mutant in COV_MUTANT_CASE:
        c = kc.COV_BY_NAME[COV_MUTANT_CASE[mutant]]
        fails, ratio = kc.check_cov(c, kc.cov_refs_as_buffer(c, mutant))
        print("mutant %s on %s: err / bound %.3g" % (mutant, c["name"], ratio))
        assert fails and ratio > 1e6
        if mutant == "weight_ff":    # invisible where the table is symmetric in the frequencies, as it must be
            sym = kc.COV_BY_NAME["tiles_envfull"]
            assert kc.check_cov(sym, kc.cov_refs_as_buffer(sym, mutant))[0] == []
        if mutant == "l0":           # one multipole off is caught at every clamped l0 that leaves a block standing
            for name in ("tiles_full_rot0", "tiles_mirror_rot1", "tiles_mirror_rot4"):
                cc = kc.COV_BY_NAME[name]
                assert kc.check_cov(cc, kc.cov_refs_as_buffer(cc, mutant))[0]
    elif mutant == "lexmax_re":
        late = next(x for x in kc.REG_CASES if x["design"] == "tie_late" and x["reg"] == 1e-14)
        early = next(x for x in kc.REG_CASES if x["design"] == "tie_early" and x["reg"] == 1e-14)
        assert kc.check_reg(late, kc.reg_expected(late, mutant))
        assert kc.check_reg(early, kc.reg_expected(early, mutant)) == []     # the earlier one wins either way
    else:
        good = np.stack([kc.ref_fisher(b).astype(np.complex128) for b in range(5)])
        assert kc.check_fisher(good)[0] == []
        fails, ratio = kc.check_fisher(good, mutant)
        print("mutant %s: err / pin %.3g" % (mutant, ratio))
        assert fails and any("block 0" in f for f in fails) and ratio > 1e6
        if mutant == "lastchunk":    # blocks with a single chunk cannot show it
            assert not any("block 2" in f for f in fails)


def test_safe_cut_and_driver_inputs():
    cut = kc.safe_cut([np.array([1.0, 2.0, 10.0]), np.array([0.5, 11.0])])
    assert 2.0 < cut < 10.0
    with pytest.raises(AssertionError):
        kc.safe_cut([np.array([1.0, 1.0001])])
    d = kc.driver_inputs()
    nd = d["svnum"].sum(axis=1)
    assert nd[0] > 0 and nd[1] == 0 and d["l0"][2] >= kc.DRV["L"] and (d["svnum"][3] == 0).any() and nd[3] > 0
