"""The pair solver `jac_inner` with Q in registers and two workgroups per CU (dm_jacobi.hip).

Three things are held: the two-sided route at the block counts where the pair items change shape, the one-sided route
on a launch of several rounds per CU, and that a result depends neither on what shares the CU nor on where in the launch
its item sits (bit-identical to the same matrix solved alone)."""
import numpy as np
import pytest

import jacobi_cases as jc

pytestmark = pytest.mark.gpu

NDISTINCT = 40


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 30)
    yield c
    c.close()


def graded_herm(rng, nb, n):
    """Hermitian matrices with spectra graded over 12 decades (as test_gpu_primitives.py::test_jacobi_herm)."""
    X = jc.crand(rng, nb, n, n)
    lam = 10.0 ** rng.uniform(-12, 0, (nb, n))
    Qm = np.linalg.qr(X)[0]
    C = (Qm * lam[:, None, :]) @ Qm.conj().transpose(0, 2, 1)
    return 0.5 * (C + C.conj().transpose(0, 2, 1))


def herm(ctx, C):
    nb, n = C.shape[0], C.shape[1]
    ev, W, sweeps = ctx.jacobi_herm(ctx.to_device(C), n, n, strideC=n * n, batch=nb)
    return ev.cpu().numpy()[:, :n], W.cpu().numpy(), sweeps


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def placement(n, ndistinct, seed):
    """Which distinct matrix sits at each of n positions: every one at least once, the copies scattered."""
    rng = np.random.default_rng(seed)
    src = np.concatenate([np.arange(ndistinct), rng.integers(0, ndistinct, n - ndistinct)])
    return rng.permutation(src)


# n = 64 is one pair item per matrix; 32, 33 and 63 are a single block, a one-row and a short second block; 65 and 96 are
# three blocks: rounds with a bye
@pytest.mark.parametrize("n", [32, 33, 63, 64, 65, 96])
def test_two_sided_graded(ctx, n):
    rng = np.random.default_rng(1000 + n)
    nb = 3
    C = graded_herm(rng, nb, n)
    ev, W, sweeps = herm(ctx, C)
    for b in range(nb):
        ref = np.linalg.eigvalsh(C[b])
        lmax = np.abs(ref).max()
        e_ev = np.abs(np.sort(ev[b]) - ref).max() / lmax
        e_un = np.abs(W[b] @ W[b].conj().T - np.eye(n)).max()
        e_dg = np.abs(W[b] @ C[b] @ W[b].conj().T - np.diag(ev[b])).max() / lmax
        print("[jac_inner] n %3d matrix %d sweeps %2d: eigenvalues %.3g lmax, |W W^H - I| %.3g, |W C W^H - diag| %.3g lmax"
              % (n, b, sweeps, e_ev, e_un, e_dg))
        assert e_ev <= 2e-12, sweeps
        assert e_un < 1e-12
        assert e_dg <= 2e-12
    assert sweeps < 30


def test_two_sided_position_independent(ctx):
    """640 matrices of n = 64: more than two pair items per CU and a partial last round; 40 are distinct, the others
    copies at other positions.  Every position carries the bits of its original solved alone."""
    n, nb = 64, 640
    D = graded_herm(np.random.default_rng(64640), NDISTINCT, n)
    src = placement(nb, NDISTINCT, 1)
    ev, W, _ = herm(ctx, D[src])
    alone = [herm(ctx, D[k:k + 1]) for k in range(NDISTINCT)]
    bad = [j for j in range(nb) if not (same_bits(W[j], alone[src[j]][1][0]) and same_bits(ev[j], alone[src[j]][0][0]))]
    assert not bad, "%d of %d positions differ from their matrix solved alone, the first at %d" % (len(bad), nb, bad[0])


def test_one_sided_resident_batch(ctx):
    """600 problems of 64 rows x 80 columns graded over 8 decades (one pair item each, several rounds per CU), held to
    conditions a to f; 40 are distinct and every position carries the bits of its original solved alone."""
    rows, cols, nprob = 64, 80, 600
    opts = dict(unconverged=True)
    mats = [jc.graded(rows, cols, 8, seed) for seed in range(NDISTINCT)]
    src = placement(nprob, NDISTINCT, 2)
    Zin, probs = jc.pack([dict(A=mats[k]) for k in src])
    dZ = ctx.to_device(Zin)
    sigma, sweeps = ctx.jacobi_rows_problems(dZ, probs, **opts)
    Zout, sigma = dZ.cpu().numpy(), sigma.cpu().numpy()
    worst = dict.fromkeys("abcde", 0.0)
    for j, p in enumerate(probs):
        # f once, for the whole buffer: `others` of the first problem are all the rest
        r = jc.check_rows_result(mats[src[j]], Zin, Zout, sigma[j], p, sweeps, opts, others=probs[1:] if j == 0 else (),
                                 parts="abcdef" if j == 0 else "abcde")
        worst = {k: max(worst[k], r[k]) for k in worst}
    print("[jac_inner] one-sided, %d problems, sweeps %d: " % (nprob, sweeps)
          + "  ".join("%s %.3g" % (k, worst[k]) for k in "abcde") + " of the bound")
    assert sweeps < 30
    bad = []
    for k in range(NDISTINCT):
        Zi, pk = jc.pack([dict(A=mats[k])])
        dz = ctx.to_device(Zi)
        sk, _ = ctx.jacobi_rows_problems(dz, pk, **opts)
        Yk, sk = jc.region(dz.cpu().numpy(), pk[0]), sk.cpu().numpy()[0, :rows]
        bad += [j for j in np.flatnonzero(src == k)
                if not (same_bits(jc.region(Zout, probs[j]), Yk) and same_bits(sigma[j, :rows], sk))]
    assert not bad, "%d of %d positions differ from their problem solved alone, the first at %d" % (
        len(bad), nprob, min(bad))
