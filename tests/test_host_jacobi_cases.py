"""CPU-only: the inputs, the float64 reference solver and the contract that tests/test_gpu_jacobi_rows.py holds the
row-Jacobi engine to (tests/jacobi_cases.py).  The generators are deterministic and have the spectra they claim; the
textbook Hestenes solver alone stays within every condition of `check_rows_result` on every family (so the conditions ask
nothing a float64 Jacobi cannot deliver); the checker turns down three doctored answers."""
import numpy as np
import pytest

import jacobi_cases as jc

FAMILY_CASES = [c for c in jc.EXACT_CASES if c[2] == 0 and c[3] is None]
# the family of the GPU groups iv and vi, at sizes the reference does in a second: 15 decades, rank-deficient and full rank
# (no exact spectrum in the fixture: held to numpy at 1e-12 sigma_0)
SMOOTH_CASES = [("smooth_deficient", (40, 50, 15, 20), 0, None), ("smooth_deficient", (100, 120, 15, 100), 0, None)]


def test_generators_are_deterministic_and_as_described():
    for fam, args, _, _ in FAMILY_CASES + [("smooth_deficient", (40, 50, 15, 20), 0, None)]:
        A = jc.make(fam, args)
        assert A.dtype == np.complex128 and A.shape == tuple(args[:2])
        assert np.array_equal(A, jc.make(fam, args)), fam
    assert not np.array_equal(jc.graded(48, 64, 8, 0), jc.graded(48, 64, 8, 1))
    n = np.linalg.norm(jc.graded(48, 64, 8), axis=1)
    assert np.allclose(np.sort(n), 10.0 ** (-8 * np.arange(47, -1, -1) / 47), rtol=1e-14) and n[0] != n.max()
    s = np.linalg.svd(jc.smooth_deficient(40, 50, 15, 20), compute_uv=False)
    assert np.abs(s[:20] - 10.0 ** np.linspace(0, -15, 20)).max() < 1e-14 and s[20:].max() < 1e-15
    s = np.linalg.svd(jc.clustered(70, 90), compute_uv=False).reshape(10, 7)
    assert np.abs(s - s[:, :1]).max() < 1e-14 and (s[1:, 0] < 0.2 * s[:-1, 0]).all()
    Q = jc.orthogonal_rows(70, 90)
    G = Q @ Q.conj().T
    d = np.sqrt(np.abs(np.diag(G)))
    assert np.abs(G / np.outer(d, d) - np.eye(70)).max() < 1e-14 and d.max() / d.min() > 0.9e6
    Z = jc.with_zero_rows(70, 90, 20)
    assert (np.abs(Z).max(axis=1) == 0).sum() == 20 and np.linalg.matrix_rank(Z) == 50
    assert np.linalg.matrix_rank(jc.with_zero_rows(70, 90, 20, 1)) == 1 and np.linalg.matrix_rank(jc.duplicate_rows(70, 90)) == 1
    for shape, cut in (((60, 80), 1e-4), ((300, 320), 1e-4), ((300, 320), 1e-10)):
        s = np.linalg.svd(jc.gapped(shape[0], shape[1], cut, 2), compute_uv=False)
        k = int((s > cut * s[0]).sum())
        assert k == shape[0] // 2 and s[k - 1] >= 9.99 * cut * s[0] and s[k] <= 0.1001 * cut * s[0]


def test_fixture_covers_the_cases():
    g = np.load(jc.GOLDEN)
    assert [str(k) for k in g["keys"]] == [jc.case_key(*c) for c in jc.EXACT_CASES]
    assert 1e-16 < float(g["e_ref"]) == g["e_case"].max() < 1e-14
    for fam, args, gc0, gc1 in jc.EXACT_CASES:
        s, e_ref = jc.exact_sigma(fam, args, gc0, gc1)
        X = jc.make(fam, args)[:, gc0:gc1]
        assert s.shape == (min(X.shape),) and (np.diff(s) <= 0).all()
        assert np.abs(np.linalg.svd(X, compute_uv=False) - s).max() <= 1e-14 * s[0]     # the generator's own self-check level


@pytest.mark.parametrize("case", FAMILY_CASES + SMOOTH_CASES, ids=lambda c: jc.case_key(*c))
def test_reference_solver_meets_the_contract(case):
    fam, args, gc0, gc1 = case
    A = jc.make(fam, args)
    Zin, probs = jc.pack([dict(A=A, row0=3, ldx=2)])
    Zout, sig, sweeps = jc.simulate(Zin, probs)
    s_ref, e_ref = jc.exact_sigma(fam, args) if case in FAMILY_CASES else (None, None)
    r = jc.check_rows_result(A, Zin, Zout, sig[0], probs[0], sweeps, s_ref=s_ref, e_ref=e_ref)
    print(jc.case_key(*case), "sweeps", sweeps, {k: float("%.3g" % v) for k, v in r.items()})
    if fam == "graded" and args[2] == 8:
        assert r["c_floor_over_rel"] < 1.0     # at 8 decades no pair falls under the floor term: c is purely relative here
    if fam == "orthogonal_rows":
        assert sweeps == 0


def test_reference_solver_meets_the_contract_on_the_ragged_batch():
    """The batch of the GPU test's group ii: row counts around the block sizes, offsets, ld slack, Gram sub-ranges."""
    mats = [jc.make(*jc.ragged_case(k)[:2]) for k in range(len(jc.RAGGED))]
    Zin, probs = jc.pack([dict(A=A, row0=c[2], ldx=c[3], gc0=c[4], gc1=c[5]) for A, c in zip(mats, jc.RAGGED)])
    assert sorted(p["ncols"] for p in probs)[::len(probs) - 1] == [40, 300]
    Zout, sig, sweeps = jc.simulate(Zin, probs)
    for k, (A, p) in enumerate(zip(mats, probs)):
        ex = jc.exact_sigma(*jc.ragged_case(k)) if 1 <= p["nrows"] <= 96 else (None, None)
        jc.check_rows_result(A, Zin, Zout, sig[k], p, sweeps, others=probs, s_ref=ex[0], e_ref=ex[1])


def test_reference_solver_meets_the_contract_under_the_options():
    """The branches of the checker that the options of the SVD chain select, on answers of the reference (a converged
    SVD meets them a fortiori).  drop_below: c absolute for the pairs with a row below drop_below sigma_0 — there are such
    rows — and e by Weyl's bound; a subspace split that no sweep ordered (sweeps == 0): a, b, d, f alone are asserted,
    c and e only measured; with sweeps > 0 the full contract again."""
    A = jc.smooth_deficient(40, 50, 15, 40)
    Zin, probs = jc.pack([dict(A=A, row0=3, ldx=2)])
    Zout, sig, sweeps = jc.simulate(Zin, probs)
    opts = dict(unconverged=True, drop_below=1e-12)
    assert (sig[0] < 1e-12 * sig[0][0]).sum() >= 5
    r = jc.check_rows_result(A, Zin, Zout, sig[0], probs[0], sweeps, opts)
    # the Weyl branch is the one that ran: against its bound, 1e-12 sigma_0 + |dropped rows|_F
    low = sig[0] < 1e-12 * sig[0][0]
    big = sig[0] > 1e-10 * sig[0][0]
    s_np = np.linalg.svd(A, compute_uv=False)
    assert np.isclose(r["e"], (np.abs(sig[0] - s_np)[big] / (1e-12 * s_np[0] + np.sqrt((sig[0][low] ** 2).sum()))).max())
    # ... and an answer whose dropped rows were left unorthogonalised still passes c there, but not among the rows above
    out = jc.region(Zout, probs[0])
    mixed = out.copy()
    mixed[-1], mixed[-2] = (out[-1] + out[-2]) / np.sqrt(2.0), (out[-1] - out[-2]) / np.sqrt(2.0)
    bad = Zout.copy()
    jc.put(bad, probs[0], mixed)
    nrm = np.linalg.norm(mixed[:, :50], axis=1)
    jc.check_rows_result(A, Zin, bad, nrm, probs[0], sweeps, opts, parts="abcf")
    with pytest.raises(AssertionError, match="^c: "):
        jc.check_rows_result(A, Zin, bad, nrm, probs[0], sweeps, parts="abcf")
    A = jc.gapped(60, 80, 1e-4, 2)
    Zin, probs = jc.pack([dict(A=A, row0=3, ldx=2)])
    Zout, sig, sweeps = jc.simulate(Zin, probs)
    opts = dict(unconverged=True, subspace_cut=1e-4, subspace_margin=100.0)
    assert set(jc.check_rows_result(A, Zin, Zout, sig[0], probs[0], 0, opts)) >= set("abcdef")
    jc.check_rows_result(A, Zin, Zout, sig[0], probs[0], sweeps, opts)
    # an unordered split is what parts "abdf" lets through: the two sides mixed inside, not across the cut
    out = jc.region(Zout, probs[0])
    q = np.linalg.qr(jc.crand(np.random.default_rng(5), 30, 30))[0]
    mixed = np.concatenate([q @ out[:30], q @ out[30:]])
    nrm = np.linalg.norm(mixed[:, :80], axis=1)
    order = np.argsort(-nrm, kind="stable")
    jc.put(Zout, probs[0], mixed[order])
    assert int((nrm[order] > 1e-4 * nrm.max()).sum()) == 30
    r = jc.check_rows_result(A, Zin, Zout, nrm[order], probs[0], 0, opts)
    assert r["c"] > 1.0
    with pytest.raises(AssertionError, match="^c: "):
        jc.check_rows_result(A, Zin, Zout, nrm[order], probs[0], 1, opts)


def _answer(A, gc1=None, solver=jc.hestenes_rows):
    Zin, probs = jc.pack([dict(A=A, gc1=gc1)])
    Zout, sig, sweeps = jc.simulate(Zin, probs, solver)
    return Zin, Zout, sig[0], probs[0], sweeps


def test_checker_rejects_lost_relative_orthogonality():
    """A norm-wise backward-stable answer — numpy.linalg.svd's U^H A, two of its small rows then mixed by an angle of
    1e-9 — passes the absolute orthogonality check the suite had (|G_ij| <= 1e-11 sigma_0^2) and fails c."""
    A = jc.graded(48, 64, 8)

    def lapack(Z, gc0, gc1):
        u, s, _ = np.linalg.svd(Z[:, gc0:gc1])
        Y = u.conj().T @ Z
        x, y = Y[-3].copy(), Y[-2].copy()
        Y[-3], Y[-2] = np.cos(1e-9) * x - np.sin(1e-9) * y, np.sin(1e-9) * x + np.cos(1e-9) * y
        sig = np.linalg.norm(Y[:, gc0:gc1], axis=1)
        order = np.argsort(-sig, kind="stable")
        return Y[order], sig[order], 1

    Zin, Zout, sig, prob, sweeps = _answer(A, solver=lapack)
    assert jc.old_absolute_check(jc.region(Zout, prob)[:, :64]) < 1e-3
    r = jc.check_rows_result(A, Zin, Zout, sig, prob, sweeps, parts="abdef")      # everything but c is in order
    assert r["c"] > 100.0
    with pytest.raises(AssertionError, match="^c: "):
        jc.check_rows_result(A, Zin, Zout, sig, prob, sweeps)


def test_checker_rejects_a_scaled_row_of_w():
    A = jc.graded(48, 64, 8)
    Zin, Zout, sig, prob, sweeps = _answer(A)
    jc.check_rows_result(A, Zin, Zout, sig, prob, sweeps)
    out = jc.region(Zout, prob)
    out[5, 64:] *= 1.0 + 1e-10
    jc.put(Zout, prob, out)
    with pytest.raises(AssertionError, match="^a: "):
        jc.check_rows_result(A, Zin, Zout, sig, prob, sweeps)


def test_checker_rejects_an_untransformed_passenger_column():
    """Column 1500 of 2049, in the second chunk of `jac_apply` (1024 columns each), left as it was uploaded."""
    A = jc.graded(40, 2009, 2, 5)
    Zin, Zout, sig, prob, sweeps = _answer(A, gc1=64)
    assert prob["ncols"] == 2049
    jc.check_rows_result(A, Zin, Zout, sig, prob, sweeps)
    out = jc.region(Zout, prob)
    out[:, 1500] = A[:, 1500]
    jc.put(Zout, prob, out)
    with pytest.raises(AssertionError, match="^b: "):
        jc.check_rows_result(A, Zin, Zout, sig, prob, sweeps)


def test_checker_rejects_a_write_outside_the_problem():
    A = jc.graded(20, 30, 2)
    Zin, probs = jc.pack([dict(A=A, row0=2, ldx=3), dict(A=A, row0=0, ldx=1)])
    Zout, sig, sweeps = jc.simulate(Zin, probs)
    jc.check_rows_result(A, Zin, Zout, sig[0], probs[0], sweeps, others=probs[1:])
    for where in (probs[0]["off"] + 2 * probs[0]["ld"] + 50,       # ld slack of a row of problem 0
                  probs[0]["off"] + 5,                             # a row above it
                  probs[1]["off"] - 3,                             # the gap between the two
                  jc.GUARD - 1):
        bad = Zout.copy()
        bad[where] = 0.0
        with pytest.raises(AssertionError, match="^f: "):
            jc.check_rows_result(A, Zin, bad, sig[0], probs[0], sweeps, others=probs[1:])
