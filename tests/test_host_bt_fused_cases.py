"""CPU only: the case table of tests/bt_fused_cases.py against the library's own choice of ring-transform kernels
(`dm_bt_ring_plan_info`, the function the launch goes through), and the reference and bound that test_gpu_bt_fused.py
holds the device to.

Plan coverage: every row of `bt_dft_rows` and `bt_fft_rows` (dm_btgen.hip) is named by some case with real beams and by
some case with complex beams; no pair is unselectable, so none is excepted.

Accuracy of the reference: its float64 ring sums are redone in long double with exactly reduced phases on six rings
(first, last, nside - 1, the equator, a cap ring, a belt ring) for m in (0, 8, 23), its Legendre sums for the same m over
all rings.  With rho = max |G_ld - G| / S over the sampled ring sums, the reference error of an element is estimated as
rho A + |c_ld - c| and has to stay below 1/8 of the element's bound.  Measured over the 48 problems: rho <= 1.6e-15 (the
FFT of numpy against the long-double sum, as a fraction of sum |f|), worst ratio to the bound 0.0072 (nside 2, four maps);
the slab evaluation lies within 0.0039 of the bound of the oracle's functions on whole maps; the bound is at most 3.2e-12 of
a column's largest coefficient; the three nside-1024 references take 6, 8 and 9 s.

Mutants: five kernel mistakes restated on the reference (`bt_fused_cases.MUTANTS`) leave the bound by factors of 1e7 and
more on the named cases.
"""
import numpy as np
import pytest

import bt_fused_cases as bc
from gemm_cases import LD, LD_OK
from oracle import btgen as ob

CLD = np.clongdouble
PI_LD = LD("3.14159265358979323846264338327950288")
DFT_ROWS = [(True, 4, 2, 1), (False, 4, 2, 2), (False, 4, 1, 4), (True, 1, 2, 4), (False, 1, 4, 4), (False, 1, 1, 8)]
FFT_ROWS = [(4, 1), (4, 2), (4, 4), (4, 8), (1, 1), (1, 2), (1, 4), (1, 8), (1, 16)]
# rows that no input can select, with the reason: none — every (row, real / complex) pair is reached by some case
NOT_COVERED = {}

PROBLEMS = []
for _c in bc.CASES:
    if bc.pkey(_c) not in [bc.pkey(BC) for BC in PROBLEMS]:
        PROBLEMS.append(_c)


def _plan(case):
    from driftscan_amd import _lib

    m_lo, m_hi = case["m_range"]
    return _lib.bt_ring_plan_info(case["nside"], case["P"] == 4, m_lo, m_hi, case["lmax"], case["cplx"], case["ncol"])


def test_case_rows_are_what_the_library_picks():
    for case in bc.CASES:
        pl = _plan(case)
        assert pl["use_fft"] == (case["fft"] is not None), (case["name"], pl)
        assert pl["fft_npt"] == (case["fft"] or 0), (case["name"], pl)
        assert pl["dft_row"] == case["dft"], (case["name"], pl)
        nring = 4 * case["nside"] - 1
        assert pl["nring_dft"] == (2 * case["nside"] - 2 if pl["use_fft"] else nring), (case["name"], pl)
        if pl["use_fft"]:
            assert 4 <= pl["fft_cpw"] <= 32


def test_plan_names_every_row():
    seen = set()
    for case in bc.CASES:
        pl = _plan(case)
        seen.add(("dft", pl["dft_row"], case["cplx"]))
        if pl["use_fft"]:
            seen.add(("fft", (case["P"], pl["fft_npt"]), case["cplx"]))
    want = {("dft", r, cb) for r in DFT_ROWS for cb in (False, True)} | {("fft", r, cb) for r in FFT_ROWS for cb in (False, True)}
    missing = want - seen
    print("rows named: %d of %d; not covered: %s" % (len(want & seen), len(want), sorted(missing)))
    assert missing == set(NOT_COVERED), sorted(missing)
    # the belt in matrix form on long rings, and the wide polarised call without FFT
    assert any(c["fft"] is None and c["m_range"] in bc.WIDE and c["nside"] == 1024 and c["P"] == 4 for c in bc.CASES)
    assert any(c["fft"] is None and c["m_range"] in bc.WIDE and c["nside"] == 48 for c in bc.CASES)


def test_plan_of_an_empty_call():
    from driftscan_amd import _lib

    assert _lib.bt_ring_plan_info(8, True, 30, 40, 23, False, 5) == dict(use_fft=False, fft_npt=0, fft_cpw=0, nring_dft=0, dft_row=None)
    assert _lib.bt_ring_plan_info(8, True, 0, 23, 23, False, 0)["nring_dft"] == 0
    # m above the group's band limit does not count: 20 .. 40 at lmax 23 is four m-values
    assert _lib.bt_ring_plan_info(8, True, 20, 40, 23, False, 5)["dft_row"] == (False, 4, 2, 2)
    with pytest.raises(_lib.DriftMIError):
        _lib.bt_ring_plan_info(0, True, 0, 23, 23, False, 5)


@pytest.mark.parametrize("name", [c["name"] for c in PROBLEMS if c["nside"] <= 64])
def test_slab_reference_is_the_oracle(name):
    """The slab evaluation against `construct_pol_*` / `transfer_single(fft=True)` / `fold_to_m` on whole maps."""
    prob = bc.problem(bc.BY_NAME[name])
    nside, P, lmax, lside = prob.nside, prob.P, prob.lmax, prob.lside
    ap = ob.ang_positions(nside)
    hz = ob.horizon(ap, prob.zenith).astype(np.float64)
    beams = prob.beams.reshape(bc.NBEAM, ap.shape[0], -1)
    worst = 0.0
    for c in range(prob.ncol):
        bi, bj = beams[prob.bi[c]], beams[prob.bj[c]]
        fr = ob.fringe(ap, prob.zenith, prob.uv[c])
        if P == 4:
            maps = (ob.construct_pol_complex if prob.cplx else ob.construct_pol_real)(bi, bj, fr, hz)
        else:
            px = 4.0 * np.pi / ap.shape[0]
            om_i, om_j = np.sum(np.abs(bi[:, 0]) ** 2 * hz) * px, np.sum(np.abs(bj[:, 0]) ** 2 * hz) * px
            maps = hz * fr * bi[:, 0] * bj[:, 0].conjugate() / np.sqrt(om_i * om_j)
        cl = int(prob.col_lmax[c])
        if prob.ring_w is None:
            t = ob.transfer_single(maps, nside, lmax, lside, P == 4, fft=True)
        else:
            t = ob.transfer_single(maps, nside, lmax, lside, P == 4, niter=0, ring_w=prob.ring_w, fft=True)
        for m, blk in enumerate(ob.fold_to_m(t[None], lmax)):
            full = np.zeros((2, P, lside + 1), dtype=np.complex128)
            full[:, :, m:] = blk[0]
            full[:, :, cl + 1 :] = 0.0          # the column's own band limit (telescope.py:792-802)
            r, ok = bc.worst_ratio(prob.ref[m, :, c], full, prob.bound[m, None, c] / 8.0)
            assert ok, (name, c, m, r)
            worst = max(worst, r / 8.0)
    print("%s: slab evaluation within %.3g of the bound of the oracle on whole maps" % (name, worst))


def _cis_ld(mm, n, k0):
    """exp(i mm phi_j) in long double from the exactly reduced phase pi (mm (k0 + 2 j) mod 2 n) / n."""
    q = (int(mm) * (k0 + 2 * np.arange(n, dtype=np.int64))) % (2 * n)
    a = PI_LD * q.astype(LD) / LD(n)
    return np.cos(a) + CLD(1j) * np.sin(a)


@pytest.mark.skipif(not LD_OK, reason="np.longdouble has no 64-bit mantissa here")
@pytest.mark.parametrize("name", [c["name"] for c in PROBLEMS])
def test_problem(name):
    """Horizon precondition, non-vacuity, tightness of the bound and accuracy of the reference of one Problem."""
    case = bc.BY_NAME[name]
    prob = bc.problem(case)
    nside, P, lmax, ncol = prob.nside, prob.P, prob.lmax, prob.ncol
    nring = 4 * nside - 1
    assert prob.horizon_margin >= bc.HORIZON_MIN, prob.horizon_margin
    assert np.isfinite(prob.ref.view(np.float64)).all() and np.isfinite(prob.bound).all()
    # exact zeros of the layout
    l = np.arange(prob.lside + 1)
    for m in range(lmax + 1):
        assert not prob.ref[m][..., l < m].any() and not prob.bound[m][..., l < m].any()
    assert not prob.ref[0, 1].any() and not prob.ref[..., lmax + 1 :].any()
    # non-vacuity: a coefficient above 100 x its bound in every m-block (m <= col_lmax) of every column
    ratio = np.abs(prob.ref) / np.where(prob.bound > 0, prob.bound, np.inf)[:, None]       # (m, 2, ncol, P, L)
    best = ratio.max(axis=(1, 3, 4))                                                       # (m, ncol)
    need = np.arange(lmax + 1)[:, None] <= prob.col_lmax[None, :]
    assert (best[need] > 100.0).all(), (name, best[need].min())
    # at least ten times tighter than the 1e-10 pin of test_gpu_btgen
    big = np.abs(prob.ref).max(axis=(0, 1, 3, 4))
    tight = prob.bound.max(axis=(0, 2, 3)) / big
    assert (tight <= 1e-11).all(), (name, tight.max())
    # accuracy of the reference
    rings = sorted({0, nring - 1, nside - 1, 2 * nside - 1, max(nside // 2 - 1, 0), min(nside + nside // 2, nring - 1)})
    msamp = [m for m in (0, 8, 23) if m <= lmax]
    k0 = (prob.phi0 != 0.0).astype(np.int64)
    assert np.array_equal(prob.phi0, k0 * (np.pi / prob.nphi))
    rho = 0.0
    for r in rings:
        f = prob.slab_maps([r])[:, :, 0, :].astype(CLD)                                    # (ncol, P, n)
        n = f.shape[-1]
        for m in msamp:
            gp = (f * _cis_ld(m, n, int(k0[r]))).sum(axis=-1)
            gn = np.conj((f * _cis_ld(-m, n, int(k0[r]))).sum(axis=-1))
            S = prob.S[r]
            pos = S > 0          # (a ring below the horizon; V of a real beam with itself: exact zeros)
            for s, g in ((0, gp), (1, gn)):
                assert not prob.G[s, m, r][~pos].any()
                if pos.any():
                    rho = max(rho, float((np.abs(g - prob.G[s, m, r].astype(CLD))[pos] / S[pos].astype(LD)).max()))
    worst = 0.0
    for m in msamp:
        lam, W, X = prob.tables(m)
        for s in range(2):
            if m == 0 and s == 1:
                continue
            g = (prob.G[s, m] * prob.wr[:, None, None]).astype(CLD)                        # (nring, ncol, P)
            n_l = lmax + 1 - m
            c = np.zeros((ncol, P, n_l), dtype=CLD)
            lamL = lam.astype(LD)
            if P == 1:
                c[:, 0] = np.einsum("lr,rc->cl", lamL, g[:, :, 0])
            else:
                WL, XL = W.astype(LD), X.astype(LD)
                c[:, 0] = np.einsum("lr,rc->cl", lamL, g[:, :, 0])
                c[:, 3] = np.einsum("lr,rc->cl", lamL, g[:, :, 3])
                c[:, 1] = np.einsum("lr,rc->cl", WL, g[:, :, 1]) - CLD(1j) * np.einsum("lr,rc->cl", XL, g[:, :, 2])
                c[:, 2] = np.einsum("lr,rc->cl", WL, g[:, :, 2]) + CLD(1j) * np.einsum("lr,rc->cl", XL, g[:, :, 1])
            keep = (np.arange(m, lmax + 1)[None, :] <= prob.col_lmax[:, None])[:, None, :]
            d = (c - prob.ref[m, s, :, :, m : lmax + 1].astype(CLD)) * keep
            est = rho * prob.A[m, :, :, m : lmax + 1] + np.maximum(np.abs(d.real), np.abs(d.imag)).astype(np.float64)
            b = prob.bound[m, :, :, m : lmax + 1]
            assert (est <= b / 8.0).all(), (name, m, s, float((est / np.where(b > 0, b, np.inf)).max()))
            worst = max(worst, float((est / np.where(b > 0, b, np.inf)).max()))
    print("%s: reference %.1f s, horizon margin %.2e, bound <= %.2e of the largest coefficient, ring sums %.2e of sum|f| from "
          "long double, reference error / bound <= %.4f" % (name, prob.seconds, prob.horizon_margin, tight.max(), rho, worst))
    assert worst <= 0.125


@pytest.mark.parametrize("name,mutant,seen", [
    ("long-n64-P4-c-c5-m0_23", "lastpixel", True), ("depth-n2-P1-r-c17-m0_23", "wrap", True), ("depth-n4-P4-r-c17-m0_23", "wrap", True),
    ("depth-n8-P4-r-c17-m0_23", "wrap", False), ("ringw-n128-P4-r-c5-m0_23", "ringw", True), ("ringw-n8-P4-r-c5-m0_23", "ringw", True),
    ("long-n64-P1-c-c5-m0_23", "conj", True), ("long-n64-P4-c-c5-m0_23", "conj", True), ("long-n64-P4-r-c5-m0_23", "vsign", True)])
def test_bound_sees_mutants(name, mutant, seen):
    """Reference-level restatements of kernel mistakes (bt_fused_cases.MUTANTS) leave the bound on the named case — the
    wrap of m on the belt only where m reaches N = 4 nside, which is what the nside 2 and 4 cases are for."""
    prob = bc.problem(bc.BY_NAME[name])
    ratio, ok = bc.worst_ratio(prob.coefficients(prob.ring_sums(mutant=mutant)[0]), prob.ref, prob.bound[:, None])
    print("%s, mutant %s: worst |mutant - ref| / bound = %.3g" % (name, mutant, ratio))
    assert ok != seen and (ratio > 1e3) == seen
    assert set(bc.MUTANTS) >= {mutant}
