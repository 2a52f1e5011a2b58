"""CPU: the quadratic-estimator API exists with the reference's signatures (psestimation.py:582, timestream.py:463-523,
:570), and a numpy restatement of q — used by the GPU tests as well — agrees with the unmodified reference's
q_estimator (tests/golden/qestimator.npz, from tests/gen_golden_qestimator.py)."""
import inspect
import os

import numpy as np
import pytest


def _as(dtype, cplx, real=()):
    """The arrays `cplx` in the complex `dtype` and `real` in its real type (None stays None); untouched for complex128,
    so that the float64 statement is exactly what it was."""
    if np.dtype(dtype) == np.complex128:
        return list(cplx) + list(real)
    rd = np.zeros(0, dtype=dtype).real.dtype
    return ([None if v is None else np.asarray(v, dtype=dtype) for v in cplx]
            + [np.asarray(v, dtype=rd) for v in real])


def sky_to_svd(beam_svd, svnum, a, dtype=np.complex128):
    """(F, P, L, ...) sky vector -> SVD basis (temperature only): x[f-range] = B_f[:, 0, :] a[f, 0].  `dtype`: the
    complex type of the arithmetic (np.clongdouble for an extended-precision reference)."""
    beam_svd, a = _as(dtype, (beam_svd, a))
    bounds = np.concatenate([[0], np.cumsum(svnum)])
    out = np.zeros((bounds[-1],) + a.shape[3:], dtype=dtype)
    for f in range(len(svnum)):
        out[bounds[f] : bounds[f + 1]] = np.tensordot(beam_svd[f, : svnum[f], 0, :], a[f, 0], axes=(1, 0))
    return out


def svd_to_sky(beam_svd, svnum, x, dtype=np.complex128):
    """SVD basis -> (F, L, ...) sky vector through B^H (temperature only)."""
    beam_svd, x = _as(dtype, (beam_svd, x))
    bounds = np.concatenate([[0], np.cumsum(svnum)])
    F, L = beam_svd.shape[0], beam_svd.shape[-1]
    out = np.zeros((F, L) + x.shape[1:], dtype=dtype)
    for f in range(F):
        out[f] = np.tensordot(beam_svd[f, : svnum[f], 0, :].conj(), x[bounds[f] : bounds[f + 1]], axes=(0, 0))
    return out


def q_estimate(evals, evecs, beam_svd, svnum, clarray, x, y=None, noise=False, crosspower=False, zero_mean=True,
               dtype=np.complex128):
    """q (nbands [+1], ...) of KL data x (and y); evecs (nmodes, ndof) rows = modes, clarray (nbands, L, F, F)."""
    evecs, beam_svd, x, y, evals, clarray = _as(dtype, (evecs, beam_svd, x, y), (evals, clarray))
    w = 1.0 / (evals + 1.0)
    x0 = (x.T * w).T
    x2 = svd_to_sky(beam_svd, svnum, evecs.conj().T @ x0, dtype=dtype)
    if y is None:
        y0, y2 = x0, x2
    else:
        y0 = (y.T * w).T
        y2 = svd_to_sky(beam_svd, svnum, evecs.conj().T @ y0, dtype=dtype)
    nb = clarray.shape[0]
    q = np.zeros((nb + (1 if noise else 0),) + x.shape[1:], dtype=np.zeros(0, dtype=dtype).real.dtype)
    for a in range(nb):
        # sum over l, f, f' of conj(y2[f, l]) C[a, l, f, f'] x2[f', l]
        q[a] = np.einsum("fl...,lfg,gl...->...", y2.conj(), clarray[a], x2).real
    if noise:
        wn = (0.0 if crosspower else 1.0) + (evals if zero_mean else 0.0)
        q[-1] = np.sum((x0 * y0.conj()).T.real * wn, axis=-1)
    return q


# ---- the API ---------------------------------------------------------------------------------------------------------
def _params(f):
    return list(inspect.signature(f).parameters)


def test_api_signatures():
    from driftscan_amd import psestimation, timestream

    assert _params(psestimation.PSEstimation.q_estimator) == ["self", "mi", "vec1", "vec2", "noise"]
    sig = inspect.signature(psestimation.PSEstimation.q_estimator)
    assert sig.parameters["vec2"].default is None and sig.parameters["noise"].default is False
    assert _params(psestimation.PSEstimation.q_estimator_batch) == ["self", "ms", "vecs1", "vecs2", "noise"]
    assert _params(timestream.Timestream.set_psestimator) == ["self", "psname"]
    assert _params(timestream.Timestream.powerspectrum) == ["self"]
    assert _params(timestream.cross_powerspectrum) == ["timestreams", "psname", "psfile"]
    ts = timestream.Timestream("/nonexistent/ts", None)
    ts.set_psestimator("ps1")
    assert ts.psname == "ps1"
    assert ts._psfile == os.path.abspath("/nonexistent/ts") + "/ps_ps1.hdf5"


def test_nosvd_refused():
    from driftscan_amd import beamtransfer, psestimation

    class _KL(object):
        pass

    kl = _KL()
    kl.beamtransfer = beamtransfer.BeamTransferNoSVD.__new__(beamtransfer.BeamTransferNoSVD)
    ps = psestimation.PSExact.__new__(psestimation.PSExact)
    ps.kltrans = kl
    with pytest.raises(NotImplementedError):
        ps.q_estimator_batch([0], [np.zeros(3)])


# ---- the restatement against the reference ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden(golden_dir):
    return (np.load(os.path.join(golden_dir, "svdkl_unpol.npz")), np.load(os.path.join(golden_dir, "psfisher.npz")),
            np.load(os.path.join(golden_dir, "qestimator.npz")))


def golden_modes(g, mi):
    """The reference's KL modes of m (the file keeps the nkept largest, rows = modes)."""
    nk = int(g["m%d_kl_nkept" % mi])
    return g["m%d_kl_evals" % mi][-nk:], g["m%d_kl_evecs" % mi][-nk:]


def test_restatement_against_reference(golden):
    g, p, q = golden
    cl = p["clarray"]
    for mi in [int(m) for m in q["mlist"]]:
        ev, E = golden_modes(g, mi)
        assert ev.size == int(q["m%d_nmodes" % mi])
        bs, sv = g["m%d_beam_svd" % mi], g["m%d_svnum" % mi]
        v = E @ sky_to_svd(bs, sv, q["m%d_a" % mi])
        scale = np.abs(q["m%d_q" % mi]).max()
        assert np.abs(q_estimate(ev, E, bs, sv, cl, v) - q["m%d_q" % mi]).max() <= 1e-12 * scale
        assert np.abs(q_estimate(ev, E, bs, sv, cl, v[:, 0]) - q["m%d_q1" % mi]).max() <= 1e-12 * scale
        for cp in (0, 1):
            for zm in (0, 1):
                ref = q["m%d_qn_%d%d" % (mi, cp, zm)]
                got = q_estimate(ev, E, bs, sv, cl, v, noise=True, crosspower=bool(cp), zero_mean=bool(zm))
                assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()
        # the cross estimate of a vector with itself is the auto estimate; q(x, y) = q(y, x)
        w = v[:, ::-1].copy()
        assert np.allclose(q_estimate(ev, E, bs, sv, cl, v, v), q["m%d_q" % mi], rtol=0, atol=1e-12 * scale)
        assert np.allclose(q_estimate(ev, E, bs, sv, cl, v, w), q_estimate(ev, E, bs, sv, cl, w, v), rtol=0,
                           atol=1e-12 * scale)
