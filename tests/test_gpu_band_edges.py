"""GPU: the band products and sky projections shared by dm_qestimate and dm_psmc_alt (dm_band.hip) at the frequency
counts the golden products never reach, on synthetic device tensors against the numpy restatements
(test_host_qestimator.q_estimate, test_host_psmc.alt_vecs / alt_fisher):

  F = 3    K of the MFMA padded to 4, one partial 16-row tile
  F = 17   two 16-row tiles, the second ragged; K padded 17 -> 20; one frequency without modes (the zero fill of x2)
  F = 80   the table tile staged in two row chunks (48 + 32)
  R = 130  N = nblk R = 260 complex columns: three workgroups along the columns, the last one partly masked

L = 6 is two chunks of multipoles, the second partial; l0 = (0, 5) masks block 1 in all but the last multipole.  The
device gets beams that are NOT zero below l0, the restatement (which has no mask) the same beams zeroed there, so the
mask itself is under test.  Bounds: 1e-12 of the largest reference value per block, the project's pin for these
estimators; the float64 restatements differ from themselves in extended precision (numpy longdouble, same inputs) by at
most 7e-15 of it for q (F = 80, with y), 1.2e-15 for the band vectors and 3e-16 for the Fisher matrices, so the
references are more than two orders inside the bound."""
import functools

import numpy as np
import pytest

from test_host_psmc import alt_fisher, alt_vecs
from test_host_qestimator import q_estimate

pytestmark = pytest.mark.gpu

NBLK, K, P, L, NBANDS = 2, 2, 1, 6, 3
L0 = (0, 5)
NSAMPLES = 7   # the divisor of the Fisher sums
CASES = [(3, 3), (17, 3), (80, 3), (3, 130)]   # (F, R)


def crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


@functools.lru_cache(maxsize=None)
def case(F, R):
    """Inputs of one batch and the references of every test on it (computed once, not modified)."""
    rng = np.random.default_rng(1000 * F + R)
    svnum = rng.integers(1, K + 1, size=(NBLK, F))
    if F == 17:
        svnum[0, 5] = svnum[1, 11] = 0
    beam = crandn(rng, NBLK, F, K, P, L)
    cl = rng.standard_normal((NBANDS, L, F, F))
    cl = cl + cl.transpose(0, 1, 3, 2)
    ndof = svnum.sum(axis=1)
    nmodes = np.array([ndof[0] // 2 + 1, ndof[1]])
    blocks = []
    for b in range(NBLK):
        E = np.linalg.qr(crandn(rng, ndof[b], nmodes[b]))[0].T.copy()   # orthonormal rows = modes
        ev = 0.1 + 5.0 * rng.random(nmodes[b])
        x, y = crandn(rng, nmodes[b], R), crandn(rng, nmodes[b], R)
        masked = beam[b].copy()
        masked[..., : L0[b]] = 0.0
        ref = dict(q=q_estimate(ev, E, masked, svnum[b], cl, x, noise=True, crosspower=False, zero_mean=True),
                   qxy=q_estimate(ev, E, masked, svnum[b], cl, x, y, noise=True, crosspower=False, zero_mean=True))
        # the library takes the draws with their (lam + 1)^-1/2 weight, the restatement applies it
        ref["vecs"] = alt_vecs(ev, E, masked, svnum[b], cl, x)
        ref["fisher"] = alt_fisher(ref["vecs"], NSAMPLES)
        blocks.append(dict(E=E, ev=ev, x=x, y=y, xw=x * ((ev + 1.0) ** -0.5)[:, np.newaxis], ref=ref))
    return dict(F=F, R=R, svnum=svnum, beam=beam, cl=cl, nmodes=nmodes, ndof=ndof, blocks=blocks)


def device_args(ctx, c):
    """The arguments Context.qestimate and Context.psmc_alt share, on the device, and the column offsets."""
    off = lambda n: np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64)   # noqa: E731
    cat = lambda key: ctx.to_device(np.concatenate([blk[key].ravel() for blk in c["blocks"]]))   # noqa: E731
    cl = ctx.to_device(np.ascontiguousarray(c["cl"].transpose(0, 2, 3, 1)))   # (nbands, F, F, L)
    args = (ctx.to_device(c["beam"]), c["svnum"], np.array(L0), cl, cat("E"), off(c["nmodes"] * c["ndof"]), c["nmodes"],
            cat("ev"), off(c["nmodes"]), c["R"])
    return args, cat, off(c["nmodes"]) * c["R"]


@pytest.mark.parametrize("cross", [False, True])
@pytest.mark.parametrize("F, R", CASES)
def test_qestimate(F, R, cross):
    from driftscan_amd import device

    ctx = device.get_context()
    c = case(F, R)
    args, cat, xoff = device_args(ctx, c)
    x, y = cat("x"), (cat("y") if cross else None)
    got = ctx.qestimate(*args, x, xoff, y=y, noise=True, crosspower=False, zero_mean=True).cpu().numpy()
    again = ctx.qestimate(*args, x, xoff, y=y, noise=True, crosspower=False, zero_mean=True).cpu().numpy()
    assert got.shape == (NBLK, NBANDS + 1, R)
    for b, blk in enumerate(c["blocks"]):
        ref = blk["ref"]["qxy" if cross else "q"]
        err, scale = np.abs(got[b] - ref).max(), np.abs(ref).max()
        print("qestimate F=%d R=%d cross=%d block %d: err / max|ref| = %.2e" % (F, R, cross, b, err / scale))
        assert err <= 1e-12 * scale, (b, err / scale)
    assert np.array_equal(got, again)


@pytest.mark.parametrize("F, R", CASES)
def test_psmc_alt(F, R):
    from driftscan_amd import device

    ctx = device.get_context()
    c = case(F, R)
    args, cat, xoff = device_args(ctx, c)
    xw = cat("xw")
    fisher, vecs = (t.cpu().numpy() for t in ctx.psmc_alt(*args, xw, xoff, NSAMPLES, want_vecs=True))
    fisher2, vecs2 = (t.cpu().numpy() for t in ctx.psmc_alt(*args, xw, xoff, NSAMPLES, want_vecs=True))
    assert fisher.shape == (NBLK, NBANDS, NBANDS) and vecs.shape == (NBANDS, int(c["nmodes"].sum()) * R)
    for b, blk in enumerate(c["blocks"]):
        ref = blk["ref"]
        n = int(c["nmodes"][b])
        v = vecs[:, xoff[b] : xoff[b] + n * R].reshape(NBANDS, n, R)
        verr, vscale = np.abs(v - np.stack(ref["vecs"])).max(), np.abs(np.stack(ref["vecs"])).max()
        ferr, fscale = np.abs(fisher[b] - ref["fisher"]).max(), np.abs(ref["fisher"]).max()
        print("psmc_alt F=%d R=%d block %d: vectors %.2e of max|v|, Fisher %.2e of max|F|"
              % (F, R, b, verr / vscale, ferr / fscale))
        assert verr <= 1e-12 * vscale, (b, verr / vscale)
        assert ferr <= 1e-12 * fscale, (b, ferr / fscale)
    assert np.array_equal(fisher, fisher2) and np.array_equal(vecs, vecs2)
