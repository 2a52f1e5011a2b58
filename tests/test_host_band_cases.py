"""CPU-only checks of the band-power case tables (tests/band_cases.py): the tables reach the kernel paths they claim,
the float64 restatements stay within a tenth of every bound against the long-double references, every mutant leaves its
bound on its named case, and the long-double references reproduce the unmodified reference's recorded products
(tests/golden/qestimator.npz, psmc.npz) as the float64 ones do."""
import os

import numpy as np
import pytest

import band_cases as bc
from test_host_psmc import alt_fisher, alt_vecs, golden_products
from test_host_qestimator import golden_modes, q_estimate, sky_to_svd

pytestmark = pytest.mark.skipif(not bc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")


# ---- the tables -----------------------------------------------------------------------------------------------------
def test_tables_reach_the_paths_they_claim():
    names = [c["name"] for c in bc.CASES]
    assert len(set(names)) == len(names) and {c["group"] for c in bc.CASES} == set(bc.GROUPS)
    assert len(bc.QCALLS) == 10 == len(set(bc.QCALLS))
    assert {(y, n) for y, n, _, _ in bc.QCALLS} == {(False, False), (False, True), (True, False), (True, True)}
    assert {(cp, zm) for _, n, cp, zm in bc.QCALLS if n} == {(a, b) for a in (False, True) for b in (False, True)}
    by = bc.BY_NAME
    for c in bc.CASES:      # the tables are not symmetric in (f, f'), unless F = 1 leaves no choice
        cl = bc.inputs(c["name"])["cl"]
        assert c["F"] == 1 or not np.allclose(cl, cl.transpose(0, 1, 3, 2))
        d = bc.inputs(c["name"])
        assert all(n <= nd for n, nd, a in zip(d["nmodes"], d["ndof"], bc.active(c)) if a)
    pol = by["pol"]
    assert (pol["F"], pol["K"], pol["P"], pol["L"], pol["nbands"], pol["R"]) == (3, 3, 4, 6, 3, 3)
    assert list(bc.inputs("pol")["l0"]) == [0, 2, 5] and (bc.inputs("pol")["svnum"][1] == 0).any()
    # modes: the strided walk of the noise term
    assert list(bc.inputs("modes")["nmodes"]) == [1, 255, 256, 257] and list(bc.inputs("modes600")["nmodes"]) == [600]
    assert by["modes"]["K"] == 128 and by["modes"]["F"] == 5 and by["modes"]["L"] == 5 and by["modes"]["R"] == 3
    assert bc.inputs("modes")["ndof"].max() < 512      # solo and batched launches pick the same GEMM variant
    # gram: 1, 1, 2 and 2 chunks, 256 x 8 fills one exactly
    assert bc.gram_chunks(by["gram"]) == [1, 1, 2, 2] and 256 * by["gram"]["R"] == bc.BG_CHUNK
    assert bc.gram_chunks(by["modes600"]) == [1] and by["gram"]["L"] == bc.LC
    assert by["bands1"]["nbands"] == 1 and by["bands17"]["nbands"] ** 2 > 256
    # freqs: the staged row chunks of the band product
    assert bc.row_chunks(1) == (16, 1) and bc.row_chunks(129) == (16, 9) and bc.row_chunks(256) == (16, 16)
    assert bc.row_chunks(80) == (48, 2) and bc.row_chunks(17) == (32, 1)      # what test_gpu_band_edges.py says of them
    assert 129 - 8 * 16 == 1 and bc.REFUSED_F == 257
    assert [by["freqs_F%d" % F]["F"] for F in (1, 129, 256)] == [1, 129, 256]
    assert (bc.inputs("freqs_F129")["svnum"][0] == 0).sum() == 1
    # ells
    for L, l0 in ((1, (0, -3, 0)), (4, (3, -3, 0)), (5, (4, -3, 0))):
        assert list(bc.inputs("ells_L%d" % L)["l0"]) == list(l0) and l0[0] == L - 1
    # idle: which blocks have nothing to do, and what they hand to the device
    assert bc.active(by["idle"]) == [True, False, True, False, False]
    assert bc.active(by["idle_rev"]) == [False, False, True, False, True]
    d = bc.inputs("idle")
    assert list(d["nmodes"][[1, 3, 4]]) == [0, 4, 4] and d["ndof"][3] == 0 and d["l0"][4] == by["idle"]["L"] and d["ndof"][1] > 0
    lay = bc.layout("idle")
    for b in (3, 4):
        assert np.isnan(lay.evals[lay.evals_off[b]: lay.evals_off[b] + 4]).all()
        assert np.isnan(lay.x[lay.x_off[b]: lay.x_off[b] + 4 * 3]).all()
    assert np.isnan(lay.evecs[lay.evecs_off[4]: lay.evecs_off[4] + 4 * d["ndof"][4]]).all() and d["ndof"][4] > 0
    assert np.isnan(lay.x[: bc.GAP]).all() and np.isnan(lay.evals[-bc.GAP:]).all()
    assert np.isfinite(lay.x[lay.x_off[0]: lay.x_off[0] + d["nmodes"][0] * 3]).all()
    # draws and moments
    big = bc.DRAW_BY_NAME["big_normal_p1"]
    assert big["nmodes"][0] * big["R"] == 1100000 > bc.DRAW_CAP == 1048576
    assert {(c["kind"], c["power"]) for c in bc.DRAW_CASES if c["name"].startswith("big")} == {(0, 1), (0, 0), (1, -1)}
    w = bc.DRAW_BY_NAME["wrap_normal"]
    assert w["s0"] < 2 ** 31 < w["s0"] + w["R"] and (w["nmodes"], w["R"]) == ((5,), 8)
    assert bc.MOMENT_NQ == (1, 2, 18) and bc.MOMENT_NS == (2, 3, 255, 256, 257, 1000) and bc.MOMENT_NBLK == 3
    q0, q1 = bc.moment_data(2, 1000, False), bc.moment_data(2, 1000, True)
    assert np.abs(q1.mean(axis=-1) / q1.std(axis=-1)).min() > 0.99e6 and np.abs(q0.mean(axis=-1)).max() < 0.5
    assert set(bc.MUTANT_CASE) == set(bc.MUTANTS)


# ---- the float64 restatements stay within a tenth of every bound ----------------------------------------------------
@pytest.mark.parametrize("group", bc.GROUPS)
def test_float64_restatements_are_a_tenth_inside_the_pin(group):
    wq, wv, wf = 0.0, 0.0, 0.0
    for c in bc.group_cases(group):
        for call in bc.QCALLS:
            got = bc.f64_q(c, call)
            fails, r = bc.check_q(c, call, got)
            assert not fails, fails
            wq = max(wq, r)
            for b, a in enumerate(bc.active(c)):
                assert a or not got[b].any()
        vecs, fisher = bc.f64_alt(c)
        fails, rv, rf = bc.check_alt(c, vecs, fisher)
        assert not fails, fails
        assert bc.check_alt(c, None, fisher)[0] == []
        wv, wf = max(wv, rv), max(wf, rf)
    print("%s: float64 restatement, worst err / (1e-12 max|ref|): q %.4f, band vectors %.4f, Fisher %.4f" % (group, wq, wv, wf))
    assert 0.0 < max(wq, wv, wf) <= 0.1


def test_float64_moments_are_a_tenth_inside_the_bounds():
    wm, wc = 0.0, 0.0
    for nq in bc.MOMENT_NQ:
        for ns in bc.MOMENT_NS:
            for shifted in (False, True):
                q = bc.moment_data(nq, ns, shifted)
                mean = q.mean(axis=-1)
                cov = np.stack([np.cov(qb).reshape(nq, nq) for qb in q])
                fails, rm, rc = bc.check_moments(q, mean, cov)
                assert not fails, (nq, ns, shifted, fails)
                wm, wc = max(wm, rm), max(wc, rc)
    print("moments: float64 np.mean / np.cov, worst err / bound: mean %.4f, covariance %.4f" % (wm, wc))
    assert 0.0 < wm <= 0.1 and 0.0 < wc <= 0.1


def test_draw_references_and_layout():
    c = bc.DRAW_BY_NAME["wrap_rademacher"]
    buf, xoff, ev, eoff = bc.draw_layout(c)
    assert xoff[0] == bc.GAP and buf.size == 5 * 8 + 2 * bc.GAP and np.isnan(buf).all()
    good = buf.copy()
    good[xoff[0]: xoff[0] + 40] = bc.ref_draw(c, 0).ravel()
    assert bc.check_draw(c, good) == ([], 0.0)
    bad = good.copy()
    bad[xoff[0] + 7] *= -1.0
    assert bc.check_draw(c, bad)[0]
    bad = good.copy()
    bad[1] = 0.0
    assert any("between the blocks" in f for f in bc.check_draw(c, bad)[0])
    # sample numbers beyond 2^31 are the continuation of the stream: column r of the draw is sample s0 + r
    from test_host_psmc import draws

    ref = bc.ref_draw(c, 0)
    for r in (3, 4, 7):
        one = draws(bc.DRAW_SEED, 3, 5, 1, 2, kind=1, power=-1, evals=bc.draw_evals(c["name"])[0], start=c["s0"] + r)
        assert np.array_equal(one[:, 0], ref[:, r])


# ---- every mutant leaves its bound on its named case ----------------------------------------------------------------
@pytest.mark.parametrize("mutant", bc.MUTANTS)
def test_every_mutant_is_caught(mutant):
    kind, where, call = bc.MUTANT_CASE[mutant]
    if kind == "q":
        c = bc.BY_NAME[where]
        good = np.stack([bc.ref_q(c, b, call).astype(np.float64) for b in range(len(c["blocks"]))])
        assert bc.check_q(c, call, good)[0] == []
        fails, ratio = bc.check_q(c, call, good, mutant)
        print("mutant %s on %s %s: err / pin %.3g" % (mutant, where, call, ratio))
        assert fails and ratio >= 10.0
        if mutant == "table_T":      # invisible without y, as it must be: Re x^H C x = Re x^H C^T x
            auto = (False,) + call[1:]
            good = np.stack([bc.ref_q(c, b, auto).astype(np.float64) for b in range(len(c["blocks"]))])
            assert bc.check_q(c, auto, good, mutant)[0] == []
        if mutant == "noise_256":    # blocks of at most 256 modes cannot show it, the band rows neither
            assert all("noise row" in f and ("block 3" in f) for f in fails)
        if mutant in bc.ALT_MUTANT_CASE:
            c = bc.BY_NAME[bc.ALT_MUTANT_CASE[mutant]]
            vecs, fisher = _alt_good(c)
            f2, rv, rf = bc.check_alt(c, vecs, fisher, mutant)
            print("mutant %s on dm_psmc_alt %s: band vectors %.3g, Fisher %.3g" % (mutant, c["name"], rv, rf))
            assert f2 and rv >= 10.0 and rf >= 10.0
    elif kind == "alt":
        c = bc.BY_NAME[where]
        vecs, fisher = _alt_good(c)
        assert bc.check_alt(c, vecs, fisher)[0] == []
        fails, rv, rf = bc.check_alt(c, vecs, fisher, mutant)
        print("mutant %s on %s: band vectors %.3g, Fisher %.3g" % (mutant, where, rv, rf))
        assert fails and rf >= 10.0 and rv <= 1.0     # both are mistakes of the Gram stage
        if mutant == "gram_2048":    # blocks with one chunk cannot show it
            assert not any("block 0" in f or "block 1" in f for f in fails)
            assert any("block 2" in f for f in fails) and any("block 3" in f for f in fails)
    elif kind == "moments":
        q = bc.moment_data(*where)
        mean, cov, _, _ = bc.ref_moments(q)
        mean, cov = mean.astype(np.float64), cov.astype(np.float64)
        cov = np.maximum(cov, cov.transpose(0, 2, 1))      # the rounding of a symmetric matrix is symmetric already
        assert bc.check_moments(q, mean, cov)[0] == []
        fails, rm, rc = bc.check_moments(q, mean, cov, mutant)
        print("mutant %s on nq, ns, shifted = %s: mean err / bound %.3g, covariance %.3g" % (mutant, where, rm, rc))
        assert fails and rc >= 10.0 and (mutant == "cov_ns" or rm >= 10.0)
        if mutant == "moments_256":
            small = bc.moment_data(2, 256, True)
            m2, c2, _, _ = bc.ref_moments(small)
            assert bc.check_moments(small, m2.astype(np.float64), c2.astype(np.float64), mutant)[0] == []
    else:
        c = bc.DRAW_BY_NAME[where]
        buf, xoff, _, _ = bc.draw_layout(c)
        good = buf.copy()
        for b, n in enumerate(c["nmodes"]):
            good[xoff[b]: xoff[b] + n * c["R"]] = bc.ref_draw(c, b).ravel()
        assert bc.check_draw(c, good) == ([], 0.0)
        fails, ratio = bc.check_draw(c, good, mutant)
        print("mutant %s on %s: %s" % (mutant, where, fails))
        assert len(fails) == 1 and "block 0" in fails[0] and "element %d" % bc.DRAW_CAP in fails[0] and ratio >= 10.0


def _alt_good(c):
    parts = [bc.ref_alt(c, b) for b in range(len(c["blocks"]))]
    vecs = np.concatenate([v.reshape(c["nbands"], -1) for v, _ in parts], axis=1).astype(np.complex128)
    return vecs, np.stack([f for _, f in parts]).astype(np.complex128)


# ---- the long-double references against the unmodified reference ----------------------------------------------------
def test_long_double_references_reproduce_the_golden_products(golden_dir):
    g = np.load(os.path.join(golden_dir, "svdkl_unpol.npz"))
    cl = np.load(os.path.join(golden_dir, "psfisher.npz"))["clarray"]
    q = np.load(os.path.join(golden_dir, "qestimator.npz"))
    kw = dict(dtype=bc.CLD)
    for mi in [int(m) for m in q["mlist"]]:
        ev, E = golden_modes(g, mi)
        bs, sv = g["m%d_beam_svd" % mi], g["m%d_svnum" % mi]
        v = E @ sky_to_svd(bs, sv, q["m%d_a" % mi])
        scale = np.abs(q["m%d_q" % mi]).max()
        got = q_estimate(ev, E, bs, sv, cl, v, **kw)
        assert got.dtype == bc.LD
        assert np.abs(got - q["m%d_q" % mi]).max() <= 1e-12 * scale
        assert np.abs(got - q_estimate(ev, E, bs, sv, cl, v)).max() <= 1e-13 * scale
        for cp in (0, 1):
            for zm in (0, 1):
                ref = q["m%d_qn_%d%d" % (mi, cp, zm)]
                got = q_estimate(ev, E, bs, sv, cl, v, noise=True, crosspower=bool(cp), zero_mean=bool(zm), **kw)
                assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        w = v[:, ::-1].copy()
        assert np.abs(q_estimate(ev, E, bs, sv, cl, v, w, **kw) - q_estimate(ev, E, bs, sv, cl, w, v, **kw)).max() <= 1e-15 * scale
    p = np.load(os.path.join(golden_dir, "psmc.npz"))
    ns = int(p["nsamples"])
    for mi in p["mlist"]:
        if int(p["m%d_nmodes" % mi]) == 0:
            continue
        ev, E, bs, sv = golden_products(p, mi)
        qa = q_estimate(ev, E, bs, sv, cl, p["m%d_x" % mi], **kw)
        mean, cov, _, _ = bc.ref_moments(qa[None].astype(np.float64))
        f, b = p["m%d_mc_fisher" % mi], p["m%d_mc_bias" % mi]
        assert np.abs(cov[0] - f).max() <= 1e-12 * np.abs(f).max() and np.abs(mean[0] - b).max() <= 1e-12 * np.abs(b).max()
        vecs = alt_vecs(ev, E, bs, sv, cl, p["m%d_signs" % mi], **kw)
        fa = alt_fisher(vecs, ns, **kw)
        ref = p["m%d_alt_fisher" % mi]
        assert fa.dtype == bc.CLD and np.abs(fa - ref).max() <= 1e-12 * np.abs(ref).max(), mi
