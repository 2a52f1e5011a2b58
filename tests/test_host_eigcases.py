"""The eigensolver test helpers of eig_cases.py against LAPACK on the host: the recorded reference ratios, the generators,
the checkers' power to reject wrong answers that stay unitary, and the gaps the selection thresholds sit in."""
import numpy as np
import pytest

import eig_cases as ec


@pytest.fixture(scope="module")
def reference_ratios():
    """(name, n, res, orth) of numpy.linalg.eigh on every matrix of the table, computed once."""
    out = []
    for name, C in ec.table():
        ev, V = np.linalg.eigh(C)
        res, orth = ec.ratios(C, V, ev)
        out.append((name, C.shape[0], res, orth))
    return tuple(out)


def test_reference_constants_cover_lapack(reference_ratios):
    """REF_RES / REF_ORTH are the worst ratios zheevd reaches over the table: no case exceeds them, and they are not
    padded beyond the rounding of the recorded figure."""
    worst_res = max(reference_ratios, key=lambda r: r[2])
    worst_orth = max(reference_ratios, key=lambda r: r[3])
    print("worst res %.4f (%s), worst orth %.4f (%s)" % (worst_res[2], worst_res[0], worst_orth[3], worst_orth[0]))
    for n in (1000, 452, 257):
        sub = [r for r in reference_ratios if r[1] == n]
        print("n = %d: res %.4f orth %.4f" % (n, max(r[2] for r in sub), max(r[3] for r in sub)))
    assert worst_res[2] <= ec.REF_RES, worst_res
    assert worst_orth[3] <= ec.REF_ORTH, worst_orth
    assert len(reference_ratios) > 150
    # ... and the pair for the sizes of the panel routes; every single case is inside what reference(n) says
    panel = [r for r in reference_ratios if r[1] >= ec.PANEL_MIN]
    worst_res, worst_orth = max(panel, key=lambda r: r[2]), max(panel, key=lambda r: r[3])
    print("n >= %d: worst res %.4f (%s), worst orth %.4f (%s)" % (ec.PANEL_MIN, worst_res[2], worst_res[0], worst_orth[3], worst_orth[0]))
    assert len(panel) > 100
    for name, n, res, orth in reference_ratios:
        assert res <= ec.reference(n)[0] and orth <= ec.reference(n)[1], (name, res, orth)
    # recorded figures, not padded ones: the worst case reaches each constant to within its last digit
    assert max(r[2] for r in reference_ratios) > ec.REF_RES - 0.01 and max(r[3] for r in reference_ratios) > ec.REF_ORTH - 0.01
    assert worst_res[2] > ec.REF_RES_PANEL - 0.001 and worst_orth[3] > ec.REF_ORTH_PANEL - 0.01


@pytest.mark.parametrize("kind,n", [(k, n) for n in (1, 2, 33, 130, 452) for k in ec.kinds_for(n)])
def test_from_spectrum_reproduces_the_spectrum(kind, n):
    lam, C = ec.random_case(kind, n)
    assert np.abs(C - C.conj().T).max() == 0.0
    got = np.linalg.eigvalsh(C)
    assert np.abs(got - np.sort(lam)).max() <= 1e-13 * np.abs(lam).max()


def test_cases_are_shared_and_write_protected():
    lam, C = ec.random_case("graded", 33)
    assert ec.random_case("graded", 33)[1] is C
    with pytest.raises(ValueError):
        C[0, 0] = 0.0
    with pytest.raises(ValueError):
        ec.structured("zero")[0, 0] = 1.0


def test_structured_matrices():
    W = ec.structured("wilkinson5")
    assert W.shape == (105, 105) and ec.structured("wilkinson8").shape == (168, 168)
    assert np.abs(W - W.conj().T).max() == 0.0 and np.abs(np.triu(W, 2)).max() == 0.0
    off = np.abs(np.diag(W, 1))
    assert np.allclose(off[20::21], 1e-8, rtol=1e-12, atol=0) and np.allclose(np.delete(off, np.s_[20::21]), 1.0, rtol=1e-12)
    assert np.allclose(np.abs(np.diag(ec.structured("wilkinson8"), 1))[20::21], 1e-14, rtol=1e-12, atol=0)
    assert (np.diag(W)[:21] == np.abs(np.arange(21) - 10.0)).all()
    T = ec.structured("toeplitz121")
    k = np.arange(1, 201)
    assert np.abs(np.linalg.eigvalsh(T) - np.sort(2.0 + 2.0 * np.cos(k * np.pi / 201))).max() <= 1e-13 * 4
    assert ec.structured("identity").shape == (161, 161) and not ec.structured("zero").any()


# ---- the checkers reject wrong answers that stay unitary ------------------------------------------------------------------
def _separated_pair(ev):
    nrm = np.abs(ev).max()
    for i in range(len(ev)):
        for j in range(i + 1, len(ev)):
            if abs(ev[i] - ev[j]) >= 0.1 * nrm:
                return i, j
    raise AssertionError("no separated pair")


def _mutations(ev, V):
    n = V.shape[0]
    i, j = _separated_pair(ev)
    swapped = V.copy()
    swapped[:, [i, j]] = swapped[:, [j, i]]
    yield "swapped columns", swapped
    rot = V.copy()
    c, s = np.cos(1e-9), np.sin(1e-9)
    rot[:, i], rot[:, j] = c * V[:, i] - s * V[:, j], s * V[:, i] + c * V[:, j]
    yield "rotated pair", rot
    rng = np.random.default_rng(n)
    u = ec.crand(rng, 32)
    u /= np.linalg.norm(u)
    refl = V.copy()
    refl[40:72] -= 2.0 * np.outer(u, u.conj() @ V[40:72])
    yield "stray reflector", refl


@pytest.mark.parametrize("kind", ec.KINDS)
@pytest.mark.parametrize("n", [130, 452])
def test_checkers_reject_unitary_mistakes(kind, n):
    lam, C = ec.random_case(kind, n)
    ev, V = np.linalg.eigh(C)
    res, orth = ec.ratios(C, V, ev)
    assert res <= ec.reference(n)[0] and orth <= ec.reference(n)[1]
    ec.assert_eigvecs(C, V, ev, what="lapack")
    for what, Vm in _mutations(ev, V):
        res, orth = ec.ratios(C, Vm, ev)
        print("%s %d %s: res %.3g orth %.3g" % (kind, n, what, res, orth))
        assert orth <= ec.bounds(n)[1], what
        assert res > ec.MARGIN * ec.REF_RES, what          # even at the bound of the smallest sizes
        with pytest.raises(AssertionError):
            ec.assert_eigvecs(C, Vm, ev, what=what)


def test_checkers_on_a_subset_and_on_the_zero_matrix():
    lam, C = ec.random_case("uniform", 200)
    ev, V = np.linalg.eigh(C)
    nrm = np.abs(ev).max()
    res, orth = ec.ratios(C, V[:, 183:], ev[183:], nrm)
    assert res <= ec.REF_RES_PANEL and orth <= ec.REF_ORTH_PANEL
    assert ec.res_ratio(C, V[:, 183:], ev[182:199], nrm) > ec.MARGIN * ec.REF_RES    # eigenvalues of the wrong rows
    assert ec.ratios(C, V[:, :0], ev[:0], nrm) == (0.0, 0.0)
    Z = ec.structured("zero")
    assert ec.res_ratio(Z, np.eye(100, dtype=complex), np.zeros(100)) == 0.0
    assert ec.res_ratio(Z, np.eye(100, dtype=complex), np.full(100, 1e-300)) > ec.MARGIN * ec.REF_RES
    with pytest.raises(AssertionError):
        ec.assert_eigvals(ev + 2e-13 * nrm, ev)
    with pytest.raises(AssertionError):
        ec.assert_eigvecs(C, np.full_like(V, np.nan), ev)


# ---- selection ------------------------------------------------------------------------------------------------------------
def test_cut_thresholds_sit_in_gaps():
    """Every threshold lies in a gap of its spectrum at least 1e-3 of the norm wide, so the number of modes a cut keeps
    does not depend on the solver's rounding (eigenvalues are right to 1e-13 of the norm)."""
    count = 0
    for what, lam, thr in ec.cut_thresholds():
        assert ec.gap_around(lam, thr) >= ec.MIN_GAP, (what, ec.gap_around(lam, thr))
        count += 1
    assert count == 2 * sum(len(ec.keep_counts(n)) for n in ec.SELECT_NS) + 2 * len(ec.SELECT_BATCH) + ec.POLICY_NB


def test_thresholds_keep_the_expected_number():
    for n in ec.SELECT_NS:
        lam, _ = ec.select_case(n)
        assert ec.keep_counts(n)[0] == 0 and ec.keep_counts(n)[-2:] == (n - 1, n)
        for k in ec.keep_counts(n):
            for side in ("upper", "lower"):
                thr = ec.threshold_below(lam, ec.below_for(side, n, k))
                i_ev = np.searchsorted(np.sort(lam), thr)
                assert (n - i_ev if side == "upper" else i_ev) == k
    for side in ("upper", "lower"):
        for (n, k), (lam, A, kept) in zip(ec.SELECT_BATCH, ec.select_batch(side)):
            i_ev = np.searchsorted(np.sort(lam), 4.0 * ec.SELECT_BATCH_THR)
            assert A.shape == (n, n) and kept == k and (n - i_ev if side == "upper" else i_ev) == k
    batch = ec.policy_batch()
    assert len(batch) == ec.POLICY_NB and [b[0] for b in batch[:8]] == [k for k in ec.KINDS for _ in range(2)]
    for kind, lam, A in batch[8:]:
        assert A.shape == (ec.POLICY_N, ec.POLICY_N) and (lam >= 4.0 * ec.POLICY_THR).sum() == ec.POLICY_KEEP
