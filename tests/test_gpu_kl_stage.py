"""GPU: the KL covariance stage element by element — `project_cov` on every route of its driver, `project_diag`,
`regularise`, `fisher` — against the long-double references and derived bounds of tests/kl_cases.py, and the host-side
bookkeeping of `eigh_gen` (holes in the list of solved blocks, offsets with gaps, the zero shortcut and the
non-positive-definite rescue under a cut) and of the one-call drivers `kl_m` / `doublekl_m` against the same steps
composed from the single entry points.  The modes buffer of `eigh_gen` is allocated by the wrapper: the test dirties the
allocator's cache with NaN first, so its gaps and its unformed rows are checked against poison like those of A and B."""
import os

import numpy as np
import pytest
import scipy.linalg as la

import kl_cases as kc
from parity_util import assert_spectrum, pencil_tol, relerr

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not kc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")]


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 30)
    yield c
    c.close()


def _cov_group(ctx, route, env_full=False):
    cases = [c for c in kc.COV_CASES if kc.cov_route(c) == route and c["env_full"] == env_full]
    assert cases
    fails, worst = [], {}
    for c in cases:
        f, r = kc.check_cov(c, kc.run_cov(ctx, c))
        fails += f
        worst[c["name"]] = r
    name = max(worst, key=worst.get)
    print("project_cov %s%s: %d launches, worst err / bound %.3f (%s)"
          % (route, " under DM_COV_FULL" if env_full else "", len(cases), worst[name], name))
    assert not fails, "\n".join(fails)


def test_project_cov_full_route(ctx):
    _cov_group(ctx, "full")


def test_project_cov_mirror_route(ctx):
    _cov_group(ctx, "mirror")


def test_project_cov_fallback_route(ctx):
    _cov_group(ctx, "fallback")


def test_project_cov_accumulate_route(ctx):
    _cov_group(ctx, "accumulate")


def test_project_cov_full_switch(ctx, monkeypatch):
    monkeypatch.setenv("DM_COV_FULL", "1")
    _cov_group(ctx, "full", env_full=True)


def test_project_diag(ctx):
    fails, worst = [], {}
    for c in kc.DIAG_CASES:
        f, r = kc.check_diag(c, kc.run_diag(ctx, c))
        fails += f
        worst[c["name"]] = r
    name = max(worst, key=worst.get)
    print("project_diag: %d launches, worst err / bound %.3f (%s)" % (len(kc.DIAG_CASES), worst[name], name))
    assert not fails, "\n".join(fails)


def test_regularise(ctx):
    fails = []
    for c in kc.REG_CASES:
        fails += kc.check_reg(c, kc.run_reg(ctx, c))
    print("regularise: %d launches, %d failures (the check is exact)" % (len(kc.REG_CASES), len(fails)))
    assert not fails, "\n".join(fails)


def test_fisher(ctx):
    for sym in (False, True):
        got = kc.run_fisher(ctx, sym)
        again = kc.run_fisher(ctx, sym)
        fails, worst = kc.check_fisher(got)
        print("fisher cl_symmetric=%d: worst err / (1e-12 max|F|) %.4f" % (sym, worst))
        assert not fails, "\n".join(fails)
        assert kc.same_bits(got, again)


# ---- eigh_gen: bookkeeping ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [None, "upper", "lower"])
def test_eigh_gen_bookkeeping(ctx, golden_dir, cut):
    g = np.load(os.path.join(golden_dir, "eigh_gen.npz"))
    mats, lay, bufA, bufB = kc.eigh_batch(g)
    dA, dB = ctx.to_device(bufA), ctx.to_device(bufB)
    # The wrapper allocates the eigenvalues and the modes itself.  Several NaN tensors of exactly those sizes are made and
    # released first, so that the caching allocator hands one of them back: zero rows and the gaps of the modes buffer
    # are then checked against NaN, not against whatever a fresh allocation holds.
    dirty = [ctx.to_device(np.full(bufA.size, kc.POISON, dtype=np.complex128)) for _ in range(8)]
    dirty += [ctx.to_device(np.full(max(sum(lay.n), 1), np.nan)) for _ in range(8)]
    ctx.sync()
    del dirty
    evals, evoff, evecs, ac, _ = ctx.eigh_gen(dA, dB, lay.n, lay.off, cut=None if cut is None else (cut, kc.EIGH_CUT))
    nkeep = ctx.last_nkeep
    ev, E = evals.cpu().numpy(), evecs.cpu().numpy()
    # A and B are destroyed inside their blocks only
    assert kc.outside_changed(bufA, dA.cpu().numpy(), lay.in_view) == 0
    assert kc.outside_changed(bufB, dB.cpu().numpy(), lay.in_view) == 0
    assert E.shape == bufA.shape
    assert np.isnan(E[~lay.in_view].real).all() and np.isnan(E[~lay.in_view].imag).all()    # the gaps kept their poison
    npd = len(mats) - 1
    assert all(ac[b] == 0.0 for b in range(npd)) and np.isclose(ac[npd], float(g["npd_ac"]), rtol=1e-5)
    worst = 0.0
    for b, (A, B) in enumerate(mats):
        n = lay.n[b]
        if n == 0:
            assert nkeep[b] == 0
            continue
        evb = ev[evoff[b]: evoff[b] + n]
        Eb = kc.view(lay, E, b)
        Bc = B + ac[b] * np.eye(n)
        zero = b == kc.EIGH_ZERO
        if zero:
            ref, eref = np.zeros(n), np.eye(n)
            assert not evb.any()                            # exactly 0
        else:
            ref, V = la.eigh(A, Bc)
            eref = V.T.conj()
            tol = pencil_tol(Bc)
            assert_spectrum(evb, ref, tol, "block %d" % b)
            worst = max(worst, np.abs(evb - ref).max() / np.abs(ref).max() / tol)
        i_ev = int(np.searchsorted(ref, kc.EIGH_CUT))
        rows = {None: slice(0, n), "upper": slice(i_ev, n), "lower": slice(0, i_ev)}[cut]
        formed = np.zeros(n, dtype=bool)
        formed[rows] = True
        assert nkeep[b] == formed.sum(), (b, nkeep[b], formed.sum())
        assert not Eb[~formed].real.any() and not Eb[~formed].imag.any() and not np.isnan(Eb[~formed]).any()
        if zero:    # include/driftmi.h: kept rows are rows of the identity, the others are zero
            assert np.array_equal(Eb[formed], np.eye(n, dtype=np.complex128)[formed])
            assert 0 < i_ev == n    # every eigenvalue lies below the cut: 'upper' keeps nothing, 'lower' everything
            continue
        Ek, erk, k = Eb[formed], eref[formed], int(formed.sum())
        rn_ref = relerr(erk @ Bc @ erk.T.conj(), np.eye(k), 1.0)
        rs_ref = relerr(erk @ A @ erk.T.conj(), np.diag(ref[formed]), np.abs(ref).max())
        assert relerr(Ek @ Bc @ Ek.T.conj(), np.eye(k), 1.0) <= max(10 * rn_ref, 10 * tol, 1e-8)
        assert relerr(Ek @ A @ Ek.T.conj(), np.diag(evb[formed]), np.abs(ref).max()) <= max(10 * rs_ref, 10 * tol, 1e-8)
    print("eigh_gen cut=%s: nkeep %s, worst eigenvalue err / pencil_tol %.3g" % (cut, [int(k) for k in nkeep], worst))


# ---- the one-call drivers against the composed steps ----------------------------------------------------------------
def _covariances(ctx, d, dev, noise_scale):
    """S and N of kltransform.py:258-308 from the single entry points, dense offsets."""
    from driftscan_amd._lib import block_offsets

    ndofs = d["svnum"].sum(axis=1)
    off, tot = block_offsets(ndofs)
    S, N = ctx.empty((max(tot, 1),), np.complex128), ctx.empty((max(tot, 1),), np.complex128)
    ctx.project_cov(dev["beam"], d["svnum"], dev["cl_sg"], S, off, l0=d["l0"], zero_first=True, symmetric=True)
    ctx.project_cov(dev["beam"], d["svnum"], dev["cl_fg"], N, off, l0=d["l0"], zero_first=True, symmetric=True)
    ctx.regularise(N, ndofs, off, kc.DRV["regulariser"])
    ctx.project_diag(dev["ut"], d["svnum"], dev["npower"], N, off, alpha=noise_scale, accumulate=True)
    ctx.sync()
    return S, N, ndofs, off


def _blocks(buf, ndofs, off):
    h = buf.cpu().numpy()
    return [h[off[b]: off[b] + n * n].reshape(n, n) for b, n in enumerate(int(x) for x in ndofs)]


def _spectra(Ss, Ns):
    return [la.eigh(S, N, eigvals_only=True) if S.shape[0] else np.zeros(0) for S, N in zip(Ss, Ns)]


def _device_inputs(ctx, d):
    return {k: ctx.to_device(np.array(d[k])) for k in ("beam", "ut", "cl_sg", "cl_fg", "npower")}


def test_kl_m_matches_the_composed_steps(ctx):
    d = kc.driver_inputs()
    dev = _device_inputs(ctx, d)
    S, N, ndofs, off = _covariances(ctx, d, dev, 1.0)
    Sh, Nh = _blocks(S, ndofs, off), _blocks(N, ndofs, off)
    assert not Sh[2].any() and Sh[0].any()          # l0 >= L: the zero shortcut
    spectra = _spectra(Sh, Nh)
    thr = kc.safe_cut([s for s in spectra if s.size and s.any()])
    for cut in (None, ("upper", thr), ("lower", thr)):
        Sc, Nc = S.clone(), N.clone()
        ev_c, evoff_c, E_c, ac_c, _ = ctx.eigh_gen(Sc, Nc, ndofs, off, cut=cut)
        nkeep_c = ctx.last_nkeep
        ev, evoff, E, off_k, ac, nkeep = ctx.kl_m(dev["beam"], dev["ut"], d["svnum"], d["l0"], dev["cl_sg"], None, True,
                                                   dev["cl_fg"], None, True, dev["npower"], 1.0, kc.DRV["regulariser"], cut=cut)
        assert np.array_equal(nkeep, nkeep_c) and np.array_equal(ac, ac_c) and np.array_equal(off_k, off)
        ev, ev_c, Eh = ev.cpu().numpy(), ev_c.cpu().numpy(), E.cpu().numpy()
        for b, n in enumerate(int(x) for x in ndofs):
            if n == 0:
                assert nkeep[b] == 0
                continue
            tol = pencil_tol(Nh[b])
            assert_spectrum(ev[evoff[b]: evoff[b] + n], ev_c[evoff_c[b]: evoff_c[b] + n], tol, "kl_m block %d" % b)
            assert_spectrum(ev[evoff[b]: evoff[b] + n], spectra[b], tol, "kl_m block %d against LAPACK" % b)
            i_ev = int(np.searchsorted(spectra[b], thr))
            assert nkeep[b] == (n if cut is None else n - i_ev if cut[0] == "upper" else i_ev)
            formed = np.zeros(n, dtype=bool)
            formed[{None: slice(0, n), "upper": slice(i_ev, n), "lower": slice(0, i_ev)}[cut and cut[0]]] = True
            Eb = Eh[off[b]: off[b] + n * n].reshape(n, n)
            assert not Eb[~formed].real.any() and not Eb[~formed].imag.any()
            Ek = Eb[formed]
            if not Sh[b].any():     # the zero shortcut: rows of the identity, eigenvalues exactly 0
                assert np.array_equal(Ek, np.eye(n, dtype=np.complex128)[formed]) and not ev[evoff[b]: evoff[b] + n].any()
                continue
            assert relerr(Ek @ Nh[b] @ Ek.T.conj(), np.eye(int(formed.sum())), 1.0) <= max(10 * tol, 1e-8)
        print("kl_m cut=%s: nkeep %s" % (cut and cut[0], [int(k) for k in nkeep]))


@pytest.mark.parametrize("fg", ["gap", "all"])
def test_doublekl_m_matches_the_composed_steps(ctx, fg):
    """fg = 'gap': the foreground threshold sits in a gap of the stage-1 spectra, the S = 0 block keeps nothing.
    fg = 'all': the threshold is -1, every mode of every block passes stage 1 — the S = 0 block takes the zero shortcut
    under an 'upper' cut that keeps all of its rows (the identity), and takes it again in stage 2, where its modes are
    the identity times those rows."""
    from driftscan_amd._lib import block_offsets

    d = kc.driver_inputs()
    dev = _device_inputs(ctx, d)
    floor = kc.DRV["floor_scale"]
    S, N, ndofs, off = _covariances(ctx, d, dev, floor)
    N2 = N.clone()
    ctx.project_diag(dev["ut"], d["svnum"], dev["npower"], N2, off, alpha=1.0 - floor, accumulate=True)
    ctx.sync()
    Sh, Nh, N2h = _blocks(S, ndofs, off), _blocks(N, ndofs, off), _blocks(N2, ndofs, off)
    spectra1 = _spectra(Sh, Nh)
    fg_thr = kc.safe_cut([s for s in spectra1 if s.size and s.any()]) if fg == "gap" else -1.0
    # ---- stage 1 composed
    ev1, evoff1, E1, ac1, _ = ctx.eigh_gen(S.clone(), N.clone(), ndofs, off, cut=("upper", float(np.nextafter(fg_thr, np.inf))))
    keep = ctx.last_nkeep.copy()
    if fg == "gap":
        assert 0 < keep[0] < ndofs[0] and keep[1] == 0 and keep[2] == 0 and 0 < keep[3] < ndofs[3]
    else:
        assert np.array_equal(keep, ndofs) and keep[2] > 0
    assert [int(k) for k in keep] == [int((s > fg_thr).sum()) for s in spectra1]
    ev1, E1h = ev1.cpu().numpy(), E1.cpu().numpy()
    # ---- stage 2 composed: the pencils restricted to the kept rows (doublekl.py:70-80), formed on the host
    off2, tot2 = block_offsets(keep)
    cs, cn = np.zeros(max(tot2, 1), dtype=np.complex128), np.zeros(max(tot2, 1), dtype=np.complex128)
    cnb = []
    for b, (n, r) in enumerate(zip((int(x) for x in ndofs), (int(x) for x in keep))):
        Ek = E1h[off[b]: off[b] + n * n].reshape(n, n)[n - r:]
        cs[off2[b]: off2[b] + r * r] = (Ek @ Sh[b] @ Ek.T.conj()).ravel()
        cnb.append(Ek @ N2h[b] @ Ek.T.conj())
        cn[off2[b]: off2[b] + r * r] = cnb[b].ravel()
    spectra2 = [la.eigh(cs[off2[b]: off2[b] + r * r].reshape(r, r), cnb[b], eigvals_only=True) if r else np.zeros(0)
                for b, r in enumerate(int(x) for x in keep)]
    thr2 = kc.safe_cut([s for s in spectra2 if s.size and s.any()])
    assert thr2 > 0.0
    for cut in (None, ("upper", thr2)):
        ev2, evoff2, E2, ac2, _ = ctx.eigh_gen(ctx.to_device(cs), ctx.to_device(cn), keep, off2, cut=cut)
        nk2 = ctx.last_nkeep
        f_ev, evs, evoff, modes, off_d, nmodes, nkeep, ac = ctx.doublekl_m(
            dev["beam"], dev["ut"], d["svnum"], d["l0"], dev["cl_sg"], None, True, dev["cl_fg"], None, True, dev["npower"],
            floor, kc.DRV["regulariser"], fg_thr, cut=cut)
        assert np.array_equal(nmodes, keep) and np.array_equal(nkeep, nk2) and np.array_equal(ac, ac1)
        f_ev, evs, ev2, modes = f_ev.cpu().numpy(), evs.cpu().numpy(), ev2.cpu().numpy(), modes.cpu().numpy()
        if fg == "all":     # the zero shortcut in both stages: zero eigenvalues, identity modes where the cut keeps them
            n = int(ndofs[2])
            assert nmodes[2] == n and nkeep[2] == (n if cut is None else 0)
            assert not f_ev[evoff[2]: evoff[2] + n].any() and not evs[evoff[2]: evoff[2] + n].any()
            want = np.eye(n, dtype=np.complex128) if cut is None else np.zeros((n, n), dtype=np.complex128)
            assert np.array_equal(modes[off_d[2]: off_d[2] + n * n].reshape(n, n), want)
        for b, (n, r) in enumerate(zip((int(x) for x in ndofs), (int(x) for x in keep))):
            if n == 0:
                continue
            assert_spectrum(f_ev[evoff[b]: evoff[b] + n], ev1[evoff1[b]: evoff1[b] + n], pencil_tol(Nh[b]), "stage 1, block %d" % b)
            if r:
                assert_spectrum(evs[evoff[b]: evoff[b] + r], ev2[evoff2[b]: evoff2[b] + r], pencil_tol(cnb[b]),
                                "stage 2, block %d" % b)
                assert_spectrum(evs[evoff[b]: evoff[b] + r], spectra2[b], pencil_tol(cnb[b]), "stage 2 against LAPACK, block %d" % b)
                if cut is not None:
                    assert nkeep[b] == r - int(np.searchsorted(spectra2[b], thr2))
        print("doublekl_m fg=%s cut=%s: nmodes %s, nkeep %s" % (fg, cut and cut[0], [int(k) for k in nmodes], [int(k) for k in nkeep]))
