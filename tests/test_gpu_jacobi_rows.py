"""The one-sided row-Jacobi engine (`dm_jacobi_rows`, through dm_jacobi_rows_problems) against its contract: conditions a to f
of `jacobi_cases.check_rows_result` on graded rows, ragged and offset batches, wide passenger
blocks, the deeper preconditioner levels, degenerate inputs and the options of the SVD chain.  Every bound is the
engine's documented stopping rule, the suite's existing level or the error of the float64 reference — none was read off
the device.  The lines `[contract]` that the tests print are the figures of the table in DESIGN.md."""
import re

import numpy as np
import pytest

import jacobi_cases as jc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 30)
    yield c
    c.close()


def run(ctx, items, **opts):
    """One call of the engine on a packed, guarded buffer: (Zin, Zout, problems, sigma (nprob, stride), sweeps)."""
    Zin, probs = jc.pack(items)
    dZ = ctx.to_device(Zin)
    sigma, sweeps = ctx.jacobi_rows_problems(dZ, probs, **opts)
    return Zin, dZ.cpu().numpy(), probs, sigma.cpu().numpy(), sweeps


def report(group, ratios, sweeps):
    worst = {k: max(r[k] for r in ratios) for k in "abcde"}
    print("[contract] %-28s sweeps %2d  " % (group, sweeps) + "  ".join("%s %.3g" % (k, worst[k]) for k in "abcde"))


def check_all(mats, res, opts=None, exact=None, **kw):
    Zin, Zout, probs, sigma, sweeps = res
    out = []
    for k, (A, p) in enumerate(zip(mats, probs)):
        ex = exact[k] if exact and exact[k] is not None else (None, None)
        out.append(jc.check_rows_result(A, Zin, Zout, sigma[k], p, sweeps, opts, others=probs, s_ref=ex[0], e_ref=ex[1], **kw))
    return out


# ---- i. relative orthogonality on graded rows ----------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,decades", [(48, 64, 8), (96, 128, 12), (70, 30, 6)])
def test_graded_rows_relative_orthogonality(ctx, rows, cols, decades):
    """Rows graded over many decades: |g_ij| <= 4 tol |y_i| |y_j| down to the smallest rows (what `beam_svd . pinv = 1`
    at kappa = 1 / svcut rests on; a solver that is only norm-wise backward stable is 1e-5 off here), the singular
    values against the exact ones."""
    args = [(rows, cols, decades, seed) for seed in (0, 1, 2)]
    mats = [jc.graded(*a) for a in args]
    res = run(ctx, [dict(A=A, row0=1, ldx=3) for A in mats])
    r = check_all(mats, res, exact=[jc.exact_sigma("graded", a) for a in args])
    report("i graded %dx%d/%d" % (rows, cols, decades), r, res[4])
    if decades == 8:      # no pair under the floor term: the relative bound alone decides
        assert max(x["c_floor_over_rel"] for x in r) < 1.0
    assert res[4] < 30


# ---- ii. row-count edges and a ragged batch in one call --------------------------------------------------------------
def test_ragged_batch_in_one_call(ctx):
    """Row counts around the 32-row blocks and the 64-row pairs, 0 included; row0 in {0, 7, 32}; ld = ncols + {0, 1, 5};
    Gram ranges of width 1, 16, 17 and the whole of A, gc0 off the 16-column tiles — as `svd_phase3` hands them over."""
    mats = [jc.make(*jc.ragged_case(k)[:2]) for k in range(len(jc.RAGGED))]
    items = [dict(A=A, row0=c[2], ldx=c[3], gc0=c[4], gc1=c[5]) for A, c in zip(mats, jc.RAGGED)]
    res = run(ctx, items)
    exact = [jc.exact_sigma(*jc.ragged_case(k)) if 1 <= c[0] <= 96 else None for k, c in enumerate(jc.RAGGED)]
    r = check_all(mats, res, exact=exact)
    report("ii ragged batch", r, res[4])
    assert res[4] < 30
    # the same problem on its own: the batch around it changes nothing
    k = [c[0] for c in jc.RAGGED].index(130)
    alone = run(ctx, [items[k]])
    check_all([mats[k]], alone)
    assert np.abs(alone[3][0, :130] - res[3][k, :130]).max() <= 1e-12 * alone[3][0, 0]
    # nothing to do: every problem empty, and no problem at all
    empty = [dict(A=np.zeros((0, c[1]), dtype=np.complex128), row0=c[2], ldx=c[3], gc0=c[4], gc1=c[5]) for c in jc.RAGGED[:4]]
    Zin, Zout, probs, _, sweeps = run(ctx, empty)
    assert sweeps == 0 and jc.check_guards(Zin, Zout, []) == 0.0
    dZ = ctx.to_device(Zin)
    _, sweeps = ctx.jacobi_rows_problems(dZ, [])
    assert sweeps == 0 and jc.check_guards(Zin, dZ.cpu().numpy(), []) == 0.0


# ---- iii. column chunks of jac_apply -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ncols", [1024, 1025, 2049])
def test_passenger_columns_beyond_one_chunk(ctx, ncols):
    """40 rows, Gram over the first 64 columns, the identity in the LAST 40 of `ncols`: every carried column — the second
    and third 1024-column chunk of `jac_apply` too — is transformed with the Gram columns (b over all columns)."""
    A = jc.graded(40, ncols - 40, 2, ncols)
    res = run(ctx, [dict(A=A, row0=2, ldx=1, gc1=64)])
    assert res[2][0]["ncols"] == ncols
    report("iii ncols %d" % ncols, check_all([A], res), res[4])


# ---- iv. the deeper preconditioner levels ------------------------------------------------------------------------------
def test_preconditioner_levels(ctx, monkeypatch, capfd):
    """15 decades over 300 rows, full rank and rank 150: the rows below 3e-5 sigma_0 get a preconditioner level of their
    own, cleaned against the rows above it first (`jac_level_clean`) — the debug line proves the level was opened."""
    mats = [jc.smooth_deficient(300, 320, 15, 300), jc.smooth_deficient(300, 320, 15, 150)]
    items = [dict(A=A, row0=1, ldx=1) for A in mats]
    capfd.readouterr()
    monkeypatch.setenv("DM_DEBUG", "1")
    res = run(ctx, items, unconverged=True)
    monkeypatch.delenv("DM_DEBUG")
    err = capfd.readouterr().err
    lines = [ln for ln in err.splitlines() if "preconditioner level" in ln or "[jacobi_rows] sweep " in ln]
    print("\n".join(lines))
    down = re.search(r"preconditioner level 0 done; (\d+) problems go one level down", err)
    assert down and int(down.group(1)) >= 1, err
    # a problem that goes down is rotated at level 1, and the level loop reports every level but the last
    assert "[jacobi_rows] preconditioner level 1 done" in err, err
    opts = dict(unconverged=True)
    report("iv levels 300x320/15", check_all(mats, res, opts), res[4])
    assert res[4] <= 6      # plain sweeps need 12 to 20
    one = run(ctx, items, unconverged=True, one_stage_eig=True)
    report("iv one_stage_eig", check_all(mats, one, dict(opts, one_stage_eig=True)), one[4])
    assert one[4] <= 6
    for k in range(2):
        assert np.abs(one[3][k] - res[3][k]).max() <= 1e-12 * res[3][k, 0]


# ---- v. degenerate inputs ----------------------------------------------------------------------------------------------
def test_orthogonal_rows_are_only_sorted(ctx):
    """Rows that are orthogonal already: the measuring pass retires the problem — no sweep, the rows only permuted."""
    A = jc.orthogonal_rows(70, 90)
    res = run(ctx, [dict(A=A, row0=7, ldx=5)])
    ex = [jc.exact_sigma("orthogonal_rows", (70, 90))]
    report("v orthogonal_rows", check_all([A], res, exact=ex), res[4])
    assert res[4] == 0
    zi, zo = jc.region(res[0], res[2][0]), jc.region(res[1], res[2][0])
    assert sorted(row.tobytes() for row in zi) == sorted(row.tobytes() for row in zo)
    forced = run(ctx, [dict(A=A, row0=7, ldx=5)], unconverged=True)
    report("v orthogonal, unconverged", check_all([A], forced, dict(unconverged=True), exact=ex), forced[4])


@pytest.mark.parametrize("family,args", [("clustered", (70, 90)), ("with_zero_rows", (70, 90, 20)),
                                         ("with_zero_rows", (70, 90, 20, 1)), ("duplicate_rows", (70, 90))])
def test_degenerate_spectra(ctx, family, args):
    """Exactly equal singular values; exactly zero rows; rank 1: c's floor term carries the residue rows."""
    A = jc.make(family, args)
    res = run(ctx, [dict(A=A, row0=7, ldx=5)])
    r = check_all([A], res, exact=[jc.exact_sigma(family, args)])
    report("v %s%r" % (family, args[2:]), r, res[4])
    assert res[4] < 30
    s_np = np.linalg.svd(A, compute_uv=False)
    assert np.abs(res[3][0, :70] - s_np).max() <= 1e-12 * s_np[0]


def test_zero_matrix_and_empty_gram_range(ctx):
    Z0 = np.zeros((70, 90), dtype=np.complex128)
    res = run(ctx, [dict(A=Z0, row0=7, ldx=5)])
    check_all([Z0], res)
    assert (res[3][0, :70] == 0.0).all()
    A = jc.graded(20, 30, 2)
    res = run(ctx, [dict(A=A, row0=7, ldx=5, gc0=5, gc1=5)])
    check_all([A], res)
    assert (res[3][0, :20] == 0.0).all()


# ---- vi. drop_below, SVD1's setting --------------------------------------------------------------------------------------
def test_drop_below(ctx):
    """Rows that end below 1e-12 sigma_0 stay out of the sweeps: a, b, d, f as ever, c in full among the rows above, the
    singular values above 1e-10 sigma_0 within Weyl's bound — the Frobenius norm of what was dropped."""
    A = jc.smooth_deficient(200, 240, 16, 200)
    opts = dict(unconverged=True, drop_below=1e-12)
    res = run(ctx, [dict(A=A, row0=1, ldx=1)], **opts)
    report("vi drop_below 1e-12", check_all([A], res, opts), res[4])
    assert res[4] < 30


# ---- vii. subspace_cut ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut,margin", [(1e-10, None), (1e-4, 100.0)])
def test_subspace_cut_is_placed_without_sweeps(ctx, monkeypatch, capfd, cut, margin):
    """The settings of `svd_phase1` and `svd_phase2`: a preconditioner level places the cut and no sweep follows.  The two
    sides are those of a converged SVD: their own singular values are the upper and the lower part of the spectrum."""
    A = jc.gapped(300, 320, cut, 2)
    s_np = np.linalg.svd(A, compute_uv=False)
    k = int((s_np > cut * s_np[0]).sum())
    assert k == 150 and s_np[k - 1] > 9.9 * cut * s_np[0] and s_np[k] < 0.101 * cut * s_np[0]     # the gap is there
    opts = dict(unconverged=True, subspace_cut=cut)
    if margin is not None:
        opts["subspace_margin"] = margin
    capfd.readouterr()
    monkeypatch.setenv("DM_DEBUG", "1")
    res = run(ctx, [dict(A=A, row0=1, ldx=1)], **opts)
    monkeypatch.delenv("DM_DEBUG")
    err = capfd.readouterr().err
    print("\n".join(ln for ln in err.splitlines() if "preconditioner level" in ln or "[jacobi_rows] sweep " in ln))
    assert res[4] == 0 and "[jacobi_rows] sweep " not in err      # placed by a level, not swept
    report("vii cut %g" % cut, check_all([A], res, opts), res[4])
    sigma = res[3][0, :300]
    assert int((sigma > cut * sigma[0]).sum()) == k
    YG = jc.region(res[1], res[2][0])[:, :320]
    up, lo = np.linalg.svd(YG[:k], compute_uv=False), np.linalg.svd(YG[k:], compute_uv=False)
    m = 3.2e5 if margin is None else margin
    e_up = np.abs(up - s_np[:k]).max() / (1e-12 * s_np[0])
    e_lo = np.abs(lo - s_np[k:]).max() / ((1e-12 * m * cut + 1e-16) * s_np[0])
    print("[contract] vii cut %g: upper side %.3g, lower side %.3g of the bound" % (cut, e_up, e_lo))
    assert e_up <= 1.0 and e_lo <= 1.0


def test_subspace_cut_too_few_rows_for_a_level(ctx):
    """60 rows: no level of its own below the first, the sweeps do the work — and then the full contract holds."""
    A = jc.gapped(60, 80, 1e-4, 2)
    opts = dict(unconverged=True, subspace_cut=1e-4, subspace_margin=100.0)
    res = run(ctx, [dict(A=A, row0=1, ldx=1)], **opts)
    assert res[4] > 0
    report("vii 60 rows, swept", check_all([A], res, opts, exact=[jc.exact_sigma("gapped", (60, 80, 1e-4, 2))]), res[4])
    assert int((res[3][0, :60] > 1e-4 * res[3][0, 0]).sum()) == 30
