"""`dm_blockvec_grouped` (ragged block-apply for a few vectors) and the device time -> m transform
(`dm_mmode_twiddle` + the strided-batched ZGEMM) against extended-precision references.

Bound of the block-apply, per output element and derived, not tuned: |y - y_ref| <= 4 (K + 2) eps (|A| |x|) with
eps = 2^-53 — above the forward error sqrt(2) gamma_{K+2} (|A| |x|) of a length-K complex fp64 inner product in any
order of summation, with or without FMA.  The reference is the same product in `np.clongdouble`."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
SENTINEL = complex(1234.5, -6789.25)
MS = (0, 1, 3, 64, 65, 1000)
KS = (0, 1, 5, 63, 64, 257, 4096)


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd import device

    device.reset_context()
    return device.get_context()


def _crandn(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


class Batch(object):
    """Problems laid out in three flat host buffers with non-trivial leading dimensions: A along K (`contig` "K": rows of
    K + 3 elements) or along M ("M": columns of M + 2), x in rows of R + 1, y in rows of R + 2 with one guard row before
    and behind every block — the guards and the columns beyond R must keep the sentinel."""

    def __init__(self, rng, specs, R):
        from driftscan_amd import _lib

        self.R, self.specs = R, list(specs)
        self.ldx, self.ldc = R + 1, R + 2
        a0, x0, y0, cols = 0, 0, 0, []
        for (M, K, contig, conjA, conjB) in self.specs:
            lda = K + 3 if contig == "K" else M + 2
            cols.append(dict(a0=a0, x0=x0, y0=y0 + self.ldc, M=M, K=K, rsA=lda if contig == "K" else 1,
                             csA=1 if contig == "K" else lda, rsB=self.ldx, csB=1, ldc=self.ldc, conjA=int(conjA),
                             conjB=int(conjB)))
            a0 += (M if contig == "K" else K) * lda
            x0 += K * self.ldx
            y0 += (M + 2) * self.ldc
        self.A = _crandn(rng, max(a0, 1))
        self.x = _crandn(rng, max(x0, 1))
        self.ny = max(y0, 1)
        self.table = _lib.blockvec_table(**{k: np.array([c[k] for c in cols], dtype=np.int64) for k in _lib.BLOCKVEC_FIELDS})

    def operands(self, i):
        """(op(A), op(x)) of problem i as dense complex128 arrays."""
        M, K, contig, conjA, conjB = self.specs[i]
        t = self.table[i]
        lda = K + 3 if contig == "K" else M + 2
        if contig == "K":
            A = self.A[t["a0"] : t["a0"] + M * lda].reshape(M, lda)[:, :K]
        else:
            A = self.A[t["a0"] : t["a0"] + K * lda].reshape(K, lda)[:, :M].T
        x = self.x[t["x0"] : t["x0"] + K * self.ldx].reshape(K, self.ldx)[:, : self.R]
        return (A.conj() if conjA else A), (x.conj() if conjB else x)

    def run(self, ctx, route=None):
        y = ctx.to_device(np.full((self.ny,), SENTINEL))
        ctx.blockvec_grouped(ctx.to_device(self.A), ctx.to_device(self.x), y, self.table, self.R, route=route)
        ctx.sync()
        return y.cpu().numpy()

    def block(self, y, i):
        """The (M + 2, ldc) region of problem i in an output buffer, guards included."""
        M = self.specs[i][0]
        y0 = int(self.table[i]["y0"]) - self.ldc
        return y[y0 : y0 + (M + 2) * self.ldc].reshape(M + 2, self.ldc)


def _all_specs():
    specs = []
    for M in MS:
        for K in KS:
            for contig in ("K", "M"):
                for conjA in (False, True):
                    specs.append((M, K, contig, conjA, (M + K) % 3 == 0))
    return specs


@pytest.mark.parametrize("R", [1, 2, 3, 8])
def test_blockvec_ragged_batches(ctx, R):
    rng = np.random.default_rng(100 + R)
    specs = _all_specs()
    order = rng.permutation(len(specs))
    b = Batch(rng, [specs[i] for i in order], R)
    y = b.run(ctx, route="blockvec")
    worst = 0.0
    for i, (M, K, contig, conjA, conjB) in enumerate(b.specs):
        blk = b.block(y, i)
        assert np.all(blk[0] == SENTINEL) and np.all(blk[-1] == SENTINEL), ("guard rows", M, K, contig)
        assert np.all(blk[:, R:] == SENTINEL), ("columns beyond R", M, K, contig)
        if M == 0 or K == 0:
            assert np.all(blk == SENTINEL), ("skipped problem written", M, K, contig)
            continue
        A, x = b.operands(i)
        Al, xl = A.astype(np.clongdouble), x.astype(np.clongdouble)
        ref = Al @ xl
        bound = 4.0 * (K + 2) * EPS * (np.abs(Al) @ np.abs(xl))
        err = np.abs(blk[1:-1, :R].astype(np.clongdouble) - ref)
        worst = max(worst, float((err / bound).max()))
        assert np.all(err <= bound), (M, K, contig, conjA, conjB, float((err / bound).max()))
    print("R = %d: largest error / bound = %.3g over %d problems" % (R, worst, len(b.specs)))


@pytest.mark.parametrize("R", [1, 4, 8])
def test_blockvec_batch_invariance(ctx, R):
    """A problem run alone and inside a batch of forty others gives bit-identical output."""
    rng = np.random.default_rng(7)
    probes = [(65, 257, "K", False, False), (1000, 4096, "K", True, False), (65, 257, "M", False, True), (1000, 63, "M", True, False)]
    others = [(int(rng.integers(0, 300)), int(rng.integers(0, 700)), "KM"[int(rng.integers(0, 2))], bool(rng.integers(0, 2)), False)
              for _ in range(40)]
    for probe in probes:
        alone = Batch(np.random.default_rng(1), [probe], R)
        y1 = alone.block(alone.run(ctx, route="blockvec"), 0).copy()
        specs = others[:17] + [probe] + others[17:]
        full = Batch(np.random.default_rng(2), specs, R)
        # the probe's data in the batch's buffers
        t, t1 = full.table[17], alone.table[0]
        na = (probe[0] if probe[2] == "K" else probe[1]) * (probe[1] + 3 if probe[2] == "K" else probe[0] + 2)
        full.A[t["a0"] : t["a0"] + na] = alone.A[t1["a0"] : t1["a0"] + na]
        nx = probe[1] * full.ldx
        full.x[t["x0"] : t["x0"] + nx] = alone.x[t1["x0"] : t1["x0"] + nx]
        y2 = full.block(full.run(ctx, route="blockvec"), 17)
        assert y1.tobytes() == y2.tobytes(), probe


def test_blockvec_wide_calls_go_to_the_zgemm(ctx):
    """R above the kernel's register budget: the Python side sends the same table to the grouped ZGEMM."""
    from driftscan_amd import _lib

    R = _lib.BLOCKVEC_MAX_R + 4
    b = Batch(np.random.default_rng(5), [(65, 257, "K", False, False), (64, 63, "M", True, False), (0, 5, "K", False, False)], R)
    y = b.run(ctx)
    for i in (0, 1):
        A, x = b.operands(i)
        ref = A.astype(np.clongdouble) @ x.astype(np.clongdouble)
        bound = 4.0 * (b.specs[i][1] + 2) * EPS * (np.abs(A) @ np.abs(x))
        assert np.all(np.abs(b.block(y, i)[1:-1, :R] - ref) <= bound)
    with pytest.raises(ValueError):
        b.run(ctx, route="blockvec")
    # 7 or 8 right-hand sides: whichever kernel `blockvec_route` picks (short rows: the ZGEMM, long rows: the kernel)
    for specs in ([(65, 92, "K", False, False), (64, 216, "K", True, False)], [(65, 1472, "K", False, False), (300, 700, "M", True, False)]):
        b = Batch(np.random.default_rng(6), specs, 8)
        y = b.run(ctx)
        for i in range(len(specs)):
            A, x = b.operands(i)
            ref = A.astype(np.clongdouble) @ x.astype(np.clongdouble)
            assert np.all(np.abs(b.block(y, i)[1:-1, :8] - ref) <= 4.0 * (specs[i][1] + 2) * EPS * (np.abs(A) @ np.abs(x)))
            assert np.all(b.block(y, i)[:, 8:] == SENTINEL) and np.all(b.block(y, i)[0] == SENTINEL)


def test_blockvec_rejects_out_of_range_problems(ctx):
    from driftscan_amd import _lib

    A, x, y = (ctx.zeros((64,), np.complex128) for _ in range(3))
    tab = _lib.blockvec_table(a0=0, x0=0, y0=0, M=9, K=8, rsA=8, csA=1, rsB=1, csB=1, ldc=1)   # 72 elements of A
    with pytest.raises(ValueError):
        ctx.blockvec_grouped(A, x, y, tab, 1)


@pytest.mark.parametrize("ntime", [17, 21, 256, 1025])
def test_mmode_transform_against_fft(ctx, ntime):
    """`dm_mmode_twiddle` + ZGEMM against np.fft.fft(x) / ntime for every mmax from 1 to (ntime - 1) // 2:
    |X_m - ref| <= 4 (ntime + 2) eps sum_t |x_t| / ntime."""
    rng = np.random.default_rng(ntime)
    nf, npairs = 2, 3
    x = _crandn(rng, nf, npairs, ntime)
    ref = np.fft.fft(x, axis=-1) / ntime
    bound = 4.0 * (ntime + 2) * EPS * np.abs(x).sum(axis=-1) / ntime          # (nf, npairs)
    X = ctx.to_device(x)
    W = ctx.mmode_twiddle(ntime, (ntime - 1) // 2).cpu().numpy()
    t, m = np.meshgrid(np.arange(ntime), np.arange((ntime - 1) // 2 + 1), indexing="ij")
    pi = 4 * np.arctan(np.longdouble(1))
    arg = 2 * pi * ((t * m) % ntime).astype(np.longdouble) / ntime
    assert np.abs(W - (np.cos(arg) - 1j * np.sin(arg)) / ntime).max() <= 4.0 * EPS / ntime     # a few ulp of 1 / ntime
    worst = 0.0
    for mmax in range(1, (ntime - 1) // 2 + 1):
        out = ctx.mmode_transform(X, mmax)
        ctx.sync()
        got = out.cpu().numpy()
        assert got.shape == (mmax + 1, nf, 2, npairs)
        want = np.zeros_like(got)
        want[:, :, 0, :] = np.moveaxis(ref[..., : mmax + 1], -1, 0)
        want[1:, :, 1, :] = np.moveaxis(ref[..., : -mmax - 1 : -1].conj(), -1, 0)
        err = np.abs(got - want)
        assert np.all(got[0, :, 1, :] == 0)
        assert np.all(err <= bound[None, :, None, :]), (ntime, mmax, float((err / bound[None, :, None, :]).max()))
        worst = max(worst, float((err / bound[None, :, None, :]).max()))
    print("ntime = %d: largest error / bound = %.3g" % (ntime, worst))
