"""Case tables, long-double references, bounds and mutants for the band-power estimators: the 13 kernels of dm_band.hip,
dm_qest.hip and dm_psmc.hip behind `dm_qestimate`, `dm_psmc_alt`, `dm_psmc_draw` and `dm_psmc_moments`.

Nothing here needs a GPU.  `CASES` lists the batches of the two estimators, `QCALLS` the ten flag settings of
`dm_qestimate`; `inputs` draws a batch (seeded, cached, write-protected) and `layout` lays it out as the device receives
it; `ref_q`, `ref_alt`, `ref_moments` and `ref_draw` are the references, each with a `mutant=` argument; `check_q`,
`check_alt`, `check_moments` and `check_draw` hold a result against them.  test_host_band_cases.py checks the tables,
the float64 restatements and the mutants on the CPU, test_gpu_band_cases.py runs the launches.

References.  np.longdouble / np.clongdouble throughout: `q_estimate` (test_host_qestimator.py), `alt_vecs` and
`alt_fisher` (test_host_psmc.py) with dtype=np.clongdouble, a two-pass mean and ddof = 1 covariance for the moments.
`draws` (test_host_psmc.py) is integer arithmetic followed by float64 and stays as it is.

Inputs.  The device gets beams that are random in every polarisation, in every row >= svnum and below l0, and band
tables that are NOT symmetric in (f, f').  The references see polarisation 0 alone, zeroed below max(l0, 0).  A block
that has nothing to do (nmodes = 0; every svnum = 0; l0 >= L) gets NaN eigenvectors, eigenvalues and data columns
wherever those have a length; its outputs have to be exactly 0.0.  Modes, eigenvalues and data columns lie at offsets
with GAP NaN elements in front of every block.

Which case reaches which line (the numbers are the rows of the table of untested paths this file was written from):
see the comments in `CASES`, `DRAW_CASES` and `MOMENT_NS`.

Bounds.

  q, band vectors, Fisher matrices of dm_psmc_alt:   |got - ref| <= PIN max|ref|,  PIN = 1e-12,
      the project's pin for these estimators (test_gpu_band_edges.py), per block and per output: the band rows of q, the
      noise row of q (another kernel, another scale), the band vectors, the Fisher matrix.  A componentwise bound through
      absolute values is of no use here (y2^H C x2 with a random C cancels), so the pin is only meaningful where float64
      arithmetic itself sits well inside it: test_host_band_cases.py measures the float64 restatements against the
      long-double values on every case and demands <= 1e-13 max|ref|, a tenth of the pin.  Measured worst
      err / (PIN max|ref|) per group, q over the ten calls / band vectors / Fisher matrices:
                   float64 restatement (numpy)      MI355X
          pol      0.0004 / 0.0003 / 0.0003         0.0007 / 0.0003 / 0.0003
          modes    0.0018 / 0.0010 / 0.0005         0.0018 / 0.0022 / 0.0004
          gram     0.0012 / 0.0007 / 0.0004         0.0021 / 0.0020 / 0.0003
          bands    0.0006 / 0.0004 / 0.0005         0.0004 / 0.0003 / 0.0006
          freqs    0.0323 / 0.0010 / 0.0002         0.0012 / 0.0017 / 0.0003
          ells     0.0006 / 0.0004 / 0.0005         0.0004 / 0.0003 / 0.0004
          idle     0.0007 / 0.0004 / 0.0005         0.0005 / 0.0003 / 0.0002
      (freqs: numpy's einsum sums the 2 x 256 x 256 terms of F = 256 one after the other.)

  moments, u = 2^-53, ns samples, d the exact deviation from the exact mean:
      mean:        |got - ref| <= (ns + 8) u mean_s |q_a|                                            =: delta_a
      covariance:  |got - ref| <= (ns + 16) u [ sum_s |d_a| |d_c| + ns delta_a delta_c ] / (ns - 1)
      The mean is a sum of ns terms (any order: at most ns - 1 additions touch a term) and a division; the covariance
      sums ns products of two rounded differences and divides; the device's mean is off by at most delta, which enters
      the sum of products in second order only, sum_s d = 0.  ns is kept in the factor, the tree depth is not
      substituted.  The covariance equals its transpose bit for bit and its diagonal is >= 0.  Measured worst
      err / bound over the 18 shapes, mean / covariance: np.mean and np.cov 0.011 / 0.044; MI355X 0.0011 / 0.0097 on the
      samples of order one, 0.0090 / 0.0078 on the shifted ones.

  draws:  Rademacher draws compare bit for bit; normal draws within 1e-14 max|ref| per block, the bound of
      test_gpu_psmc.py::test_draws_match_restatement (log, sqrt and sincos of the device against numpy's).  Measured on
      an MI355X: at most 0.024 of that bound (big_normal_p1).

  exact zeros:  an element that is exactly zero in exact arithmetic has to be exactly zero: every output of a block
      with nothing to do, and the noise row under crosspower without zero_mean (every weight is 0).  The mirrored
      triangle of a Fisher matrix is the conjugate of the other with no rounding between them.  (The imaginary part of
      the diagonal of a Fisher matrix is under the pin only: numpy's own v conj(v) leaves a rounding there where the
      product is fused.)

Mutants.  `MUTANTS` are restatements with one planted error; `MUTANT_CASE` names the case (and call) on which
test_host_band_cases.py shows that each of them leaves its bound by a factor of ten or more.
"""
import functools
import zlib

import numpy as np

from gemm_cases import LD, LD_OK, U  # noqa: F401  (LD_OK is re-exported for the test modules)
from test_host_psmc import alt_fisher, alt_vecs, draws
from test_host_qestimator import q_estimate

CLD = np.clongdouble
GAP = 5
POISON = complex(np.nan, np.nan)
PIN = 1e-12
LC = 4                  # DM_BAND_LC: multipoles per band-product workgroup
BG_CHUNK = 2048         # complex elements per partial sum of band_gram_kernel
DRAW_CAP = 4096 * 256   # threads of the largest grid of psmc_draw_kernel
FR_ROWS = 4096          # doubles of the staged table tile of band_product_kernel
NSAMPLES = 7            # the divisor of the Fisher sums of dm_psmc_alt
IDLE_NMODES = 4

MUTANTS = ("pol1", "table_T", "mask_gt", "no_l0", "noise_256", "flags_swapped", "last_lchunk", "gram_2048",
           "lower_noconj", "moments_256", "cov_ns", "draw_cap")


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _frozen(a):
    a.setflags(write=False)
    return a


# ---- the batches of dm_qestimate and dm_psmc_alt --------------------------------------------------------------------
def blk(l0=0, nmodes=None, kind="active", svnum=None):
    """One block.  kind: 'active', or one of the three ways of having nothing to do: 'nmodes0', 'sv0' (every svnum = 0,
    nmodes = 4) and 'l0L' (l0 = L, nmodes = 4).  nmodes None: ndof // 2 + 1 for an even block number, ndof for an odd."""
    return dict(l0=l0, nmodes=nmodes, kind=kind, svnum=svnum)


def case(name, group, F, K, P, L, nbands, R, blocks):
    return dict(name=name, group=group, F=F, K=K, P=P, L=L, nbands=nbands, R=R, blocks=blocks)


def _sv_for(nmodes, F, K):
    """svnum with ndof >= nmodes, a little above it (and below 512)."""
    base = -(-nmodes // F)
    return tuple(min(K, base + (f % 2)) for f in range(F))


POL = dict(F=3, K=3, P=4, L=6, nbands=3, R=3)


def _pol_blocks(l0=(0, 2, 5)):
    # block 1 has a frequency without modes: the zero fill of x2 in dm_band_proj::to_sky
    return [blk(l0[0]), blk(l0[1], svnum=(2, 0, 3)), blk(l0[2])]


CASES = [
    # (1) P = 4: the beam row stride P L and the polarisation-0 offset of dm_band_proj::to_sky and of the back-projection
    #     of dm_psmc_alt.  (2) the tables are not symmetric in (f, f') (every case): band_table_transpose_kernel and the
    #     A operand of band_product_kernel, visible in the calls with y and in dm_psmc_alt.  (8) l0 = L - 1 in block 2.
    case("pol", "pol", blocks=_pol_blocks(), **POL),
    # (3) nmodes = 255, 256, 257 and 600: the first trip of the strided walk of qest_noise_kernel exactly full, its second
    #     trip with one mode, its third.  (4) every flag setting at these shapes (QCALLS).  600 x 3 elements: one Gram
    #     chunk; L = 5 is a full chunk of multipoles and one more.
    case("modes", "modes", 5, 128, 1, 5, 2, 3,
         [blk(l0, n, svnum=_sv_for(n, 5, 128)) for n, l0 in zip((1, 255, 256, 257), (0, 1, 0, 2))]),
    case("modes600", "modes", 5, 128, 1, 5, 2, 3, [blk(1, 600, svnum=_sv_for(600, 5, 128))]),
    # (5) nmodes R = 296, 2048, 2056, 2400: 1, 1, 2 and 2 chunks of band_gram_kernel in one launch, 256 x 8 fills one
    #     exactly; band_gram_reduce_kernel walks nchunks[b] of the nchunk = 2 slots.  (8) L = 4 is exactly one chunk.
    case("gram", "gram", 3, 128, 1, 4, 2, 8,
         [blk(l0, n, svnum=_sv_for(n, 3, 128)) for n, l0 in zip((37, 256, 257, 300), (0, 0, 1, 3))]),
    # (6) nbands = 1; nbands = 17: 289 pairs give band_gram_reduce_kernel a second workgroup, 17 z-slices go through
    #     band_table_transpose_kernel.  (4) without noise nq = nbands = 1 is the smallest output stride of
    #     qest_reduce_kernel.
    case("bands1", "bands", blocks=_pol_blocks(), **dict(POL, nbands=1)),
    case("bands17", "bands", blocks=_pol_blocks(), **dict(POL, nbands=17)),
    # (7) F = 1 (Fk = 4, one row); F = 129: Fk = 132, FR = 16, nine staged row chunks, the last with one row; F = 256:
    #     sixteen full chunks.  F = 257 is refused (REFUSED_F).  One frequency of block 0 has no modes where F > 1.
    case("freqs_F1", "freqs", 1, 1, 2, 2, 2, 2, [blk(0), blk(1)]),
    case("freqs_F129", "freqs", 129, 1, 2, 2, 2, 2, [blk(0), blk(1)]),
    case("freqs_F256", "freqs", 256, 1, 2, 2, 2, 2, [blk(0), blk(1)]),
    # (8) L = 1, L = 4 (exactly one chunk of multipoles), L = 5 (a chunk and one more); l0 = L - 1, l0 < 0, l0 = 0
    case("ells_L1", "ells", blocks=_pol_blocks(l0=(0, -3, 0)), **dict(POL, L=1)),
    case("ells_L4", "ells", blocks=_pol_blocks(l0=(3, -3, 0)), **dict(POL, L=4)),
    case("ells_L5", "ells", blocks=_pol_blocks(l0=(4, -3, 0)), **dict(POL, L=5)),
    # (9) blocks with nothing to do of all three kinds in the middle and last, and (reversed) first: dm_band_proj::init,
    #     the active table of qest_reduce_kernel, the zero fill of the noise row, the Gram descriptors with nm = 0
    case("idle", "idle", blocks=[blk(0), blk(1, kind="nmodes0"), blk(2), blk(0, kind="sv0"), blk(6, kind="l0L")], **POL),
    case("idle_rev", "idle", blocks=[blk(6, kind="l0L"), blk(0, kind="sv0"), blk(2), blk(1, kind="nmodes0"), blk(0)], **POL),
]
BY_NAME = {c["name"]: c for c in CASES}
GROUPS = ("pol", "modes", "gram", "bands", "freqs", "ells", "idle")
REFUSED_F = 257     # (7) DM_ARG(F <= 256) of dm_band_proj::init: a non-zero status, the outputs untouched

# (4) y or no y; no noise row, or a noise row under the four settings of crosspower and zero_mean: ten calls per case
QCALLS = [(y, noise, cp, zm) for y in (False, True)
          for noise, cp, zm in ((False, False, False), (True, False, False), (True, False, True), (True, True, False),
                                (True, True, True))]


def group_cases(group):
    return [c for c in CASES if c["group"] == group]


def row_chunks(F):
    """(rows per staged chunk, number of chunks) of band_product_kernel."""
    Fk = (F + 3) & ~3
    FR = max(16, min((F + 15) & ~15, (FR_ROWS // Fk) & ~15))
    return FR, -(-F // FR)


def gram_chunks(c):
    return [-(-(int(n) * c["R"]) // BG_CHUNK) if a else 0 for n, a in zip(inputs(c["name"])["nmodes"], active(c))]


def active(c):
    return [b["kind"] == "active" for b in c["blocks"]]


@functools.lru_cache(maxsize=None)
def _inputs(name, F=None):
    c = BY_NAME[name]
    F = c["F"] if F is None else F          # (the refused launch is freqs_F256 drawn again with F = 257)
    K, P, L, nb, R = (c[k] for k in ("K", "P", "L", "nbands", "R"))
    rng = _rng("band", name, F)
    nblk = len(c["blocks"])
    d = dict(beam=_frozen(_crand(rng, nblk, F, K, P, L)), cl=_frozen(rng.standard_normal((nb, L, F, F))),
             svnum=np.zeros((nblk, F), dtype=np.int64), nmodes=np.zeros(nblk, dtype=np.int64),
             l0=np.array([b["l0"] for b in c["blocks"]], dtype=np.int64), blocks=[])
    for b, spec in enumerate(c["blocks"]):
        sv = np.array(spec["svnum"]) if spec["svnum"] is not None else rng.integers(1, K + 1, size=F)
        if c["group"] == "freqs" and F > 1 and b == 0:
            sv[F // 2] = 0
        if spec["kind"] == "sv0":
            sv[:] = 0
        ndof = int(sv.sum())
        if spec["kind"] == "active":
            n = spec["nmodes"] if spec["nmodes"] is not None else (ndof // 2 + 1 if b % 2 == 0 else ndof)
            assert 0 < n <= ndof and spec["l0"] < L
            E = np.linalg.qr(_crand(rng, ndof, n))[0].T.copy()      # orthonormal rows = modes
            ev = 0.1 + 5.0 * rng.random(n)
            x, y, xw = (_crand(rng, n, R) for _ in range(3))
        else:
            n = 0 if spec["kind"] == "nmodes0" else IDLE_NMODES
            assert spec["kind"] != "l0L" or spec["l0"] >= L
            E = np.full((n, ndof), POISON)
            ev = np.full(n, np.nan)
            x, y, xw = (np.full((n, R), POISON) for _ in range(3))
        d["svnum"][b], d["nmodes"][b] = sv, n
        d["blocks"].append({k: _frozen(v) for k, v in dict(E=E, ev=ev, x=x, y=y, xw=xw).items()})
    d["ndof"] = d["svnum"].sum(axis=1)
    return d


def inputs(name):
    """The batch of a case: beam (nblk, F, K, P, L), cl (nbands, L, F, F), svnum, l0, nmodes, ndof and per block E
    (nmodes, ndof), ev, x, y and xw (the weighted draws dm_psmc_alt takes).  Computed once, read-only."""
    return _inputs(name)


class Layout(object):
    """The batch as the device receives it: flat evecs / evals / x / y / xw buffers with GAP NaN elements in front of
    every block and after the last, their offsets, and cl as (nbands, F, F, L)."""


def _gapped(parts, dtype):
    off, at = [], 0
    for p in parts:
        at += GAP
        off.append(at)
        at += p.size
    buf = np.full(at + GAP, np.nan, dtype=dtype) if dtype == np.float64 else np.full(at + GAP, POISON, dtype=dtype)
    for o, p in zip(off, parts):
        buf[o: o + p.size] = p.ravel()
    return buf, np.array(off, dtype=np.int64)


def layout(name, F=None):
    d = _inputs(name, F)
    lay = Layout()
    lay.beam, lay.svnum, lay.l0, lay.nmodes = d["beam"], d["svnum"], d["l0"], d["nmodes"]
    lay.cl = np.ascontiguousarray(d["cl"].transpose(0, 2, 3, 1))
    lay.evecs, lay.evecs_off = _gapped([b["E"] for b in d["blocks"]], np.complex128)
    lay.evals, lay.evals_off = _gapped([b["ev"] for b in d["blocks"]], np.float64)
    lay.x, lay.x_off = _gapped([b["x"] for b in d["blocks"]], np.complex128)
    lay.y = _gapped([b["y"] for b in d["blocks"]], np.complex128)[0]
    lay.xw = _gapped([b["xw"] for b in d["blocks"]], np.complex128)[0]
    return lay


def v_offsets(c):
    """Offsets of the blocks in one band of the vectors of dm_psmc_alt (dense: the library lays them out), and T."""
    n = inputs(c["name"])["nmodes"] * c["R"]
    return np.concatenate([[0], np.cumsum(n)[:-1]]).astype(np.int64), int(n.sum())


# ---- references -----------------------------------------------------------------------------------------------------
def ref_beam(c, b, mutant=None):
    """(F, K, 1, L): what the estimators see of the beam of block b — polarisation 0, zero below max(l0, 0)."""
    d = inputs(c["name"])
    p = 1 if mutant == "pol1" else 0
    bm = d["beam"][b][:, :, p: p + 1, :].copy()
    lo = max(int(d["l0"][b]), 0)
    if mutant == "mask_gt":
        lo += 1
    if mutant == "no_l0":
        lo = 0
    bm[..., :lo] = 0.0
    if mutant == "last_lchunk":
        bm[..., LC * ((c["L"] - 1) // LC):] = 0.0
    return bm


def _q(c, b, y, noise, cp, zm, mutant, dtype):
    d = inputs(c["name"])
    blkd = d["blocks"][b]
    nq = c["nbands"] + (1 if noise else 0)
    rd = LD if dtype is CLD else np.float64
    if not active(c)[b]:
        return np.zeros((nq, c["R"]), dtype=rd)
    cl = d["cl"].transpose(0, 1, 3, 2) if mutant == "table_T" else d["cl"]
    if mutant == "flags_swapped":
        cp, zm = zm, cp
    yy = blkd["y"] if y else None
    q = q_estimate(blkd["ev"], blkd["E"], ref_beam(c, b, mutant), d["svnum"][b], cl, blkd["x"], yy, noise=noise,
                   crosspower=cp, zero_mean=zm, dtype=dtype)
    if mutant == "noise_256" and noise:
        k = 256
        q[-1] = q_estimate(blkd["ev"][:k], blkd["E"][:k], ref_beam(c, b), d["svnum"][b], cl, blkd["x"][:k],
                           None if yy is None else yy[:k], noise=True, crosspower=cp, zero_mean=zm, dtype=dtype)[-1]
    return q


@functools.lru_cache(maxsize=None)
def _ref_q(name, b, y, cp, zm, mutant):
    return _frozen(_q(BY_NAME[name], b, y, True, cp, zm, mutant, CLD))


def ref_q(c, b, call, mutant=None):
    """q (nq, R) of block b in np.longdouble for call = (y, noise, crosspower, zero_mean); computed once."""
    y, noise, cp, zm = call
    q = _ref_q(c["name"], b, y, cp, zm, mutant)
    return q if noise else q[:-1]


def f64_q(c, call):
    """The float64 restatement of one call, (nblk, nq, R): what a correct device may return."""
    return np.stack([_q(c, b, *call, None, np.complex128) for b in range(len(c["blocks"]))])


def _alt(c, b, mutant, dtype):
    d = inputs(c["name"])
    blkd = d["blocks"][b]
    nb, n, R = c["nbands"], int(d["nmodes"][b]), c["R"]
    if not active(c)[b]:
        return np.zeros((nb, n, R), dtype=dtype), np.zeros((nb, nb), dtype=dtype)
    rd = LD if dtype is CLD else np.float64
    cl = d["cl"].transpose(0, 1, 3, 2) if mutant == "table_T" else d["cl"]
    # alt_vecs applies the weight (lam + 1)^-1/2 to its draws, the library takes them weighted: undo it here
    cf = (blkd["ev"].astype(rd) + 1) ** rd(-0.5)
    signs = blkd["xw"].astype(dtype) / cf[:, None]
    vecs = np.stack(alt_vecs(blkd["ev"], blkd["E"], ref_beam(c, b, mutant), d["svnum"][b], cl, signs, dtype=dtype))
    gv = vecs.reshape(nb, -1)[:, :BG_CHUNK] if mutant == "gram_2048" else vecs
    fisher = alt_fisher(list(gv), NSAMPLES, dtype=dtype)
    if mutant == "lower_noconj":
        fisher = np.where(np.triu(np.ones((nb, nb), dtype=bool), 1), fisher.T, fisher)
    return vecs, fisher


@functools.lru_cache(maxsize=None)
def _ref_alt(name, b, mutant):
    v, f = _alt(BY_NAME[name], b, mutant, CLD)
    return _frozen(v), _frozen(f)


def ref_alt(c, b, mutant=None):
    """(band vectors (nbands, nmodes, R), Fisher matrix (nbands, nbands)) of block b in np.clongdouble; computed once."""
    return _ref_alt(c["name"], b, mutant)


def f64_alt(c):
    """The float64 restatement: (vecs (nbands, T), fisher (nblk, nbands, nbands))."""
    parts = [_alt(c, b, None, np.complex128) for b in range(len(c["blocks"]))]
    vecs = np.concatenate([v.reshape(c["nbands"], -1) for v, _ in parts], axis=1)
    return vecs, np.stack([f for _, f in parts])


# ---- checks ---------------------------------------------------------------------------------------------------------
def _pin(got, ref, what, fails):
    """err / (PIN max|ref|) of one output of one block; where the reference is exactly 0 the result has to be."""
    if got.size == 0:
        return 0.0
    if not (np.isfinite(got.real).all() and np.isfinite(got.imag).all()):
        fails.append("%s: not finite (unwritten, or NaN read from a block with nothing to do)" % what)
        return np.inf
    err = float(np.abs(got.astype(ref.dtype) - ref).max())
    scale = float(np.abs(ref).max())
    if scale == 0.0:
        if err != 0.0:
            fails.append("%s: exactly 0 in exact arithmetic, got up to %.3e" % (what, err))
            return np.inf
        return 0.0
    ratio = err / (PIN * scale)
    if not ratio <= 1.0:
        fails.append("%s: err %.3e of max|ref|, pin %.0e" % (what, err / scale, PIN))
    return ratio


def check_q(c, call, got, mutant=None):
    """(failures, worst err / (PIN max|ref|)) of the (nblk, nq, R) result of one call.  `mutant` turns the check round
    for the host test: `got` is then held against a wrong reference."""
    nb, nq = c["nbands"], c["nbands"] + (1 if call[1] else 0)
    if got.shape != (len(c["blocks"]), nq, c["R"]):
        return ["shape %s" % (got.shape,)], np.inf
    fails, worst = [], 0.0
    for b in range(len(c["blocks"])):
        ref = ref_q(c, b, call, mutant)
        what = "%s %s block %d" % (c["name"], call, b)
        worst = max(worst, _pin(got[b, :nb], ref[:nb], what + " bands", fails))
        if call[1]:
            worst = max(worst, _pin(got[b, nb:], ref[nb:], what + " noise row", fails))
    return fails, worst


def _cbits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_cbits(a), _cbits(b))


def check_alt(c, vecs, fisher, mutant=None):
    """(failures, worst ratio of the band vectors, of the Fisher matrices); vecs (nbands, T) or None."""
    nb, nblk = c["nbands"], len(c["blocks"])
    voff, T = v_offsets(c)
    fails, wv, wf = [], 0.0, 0.0
    if fisher.shape != (nblk, nb, nb) or (vecs is not None and vecs.shape != (nb, T)):
        return ["shape"], np.inf, np.inf
    for b in range(nblk):
        vref, fref = ref_alt(c, b, mutant)
        what = "%s block %d" % (c["name"], b)
        if vecs is not None:
            n = vref.shape[1] * vref.shape[2]
            wv = max(wv, _pin(vecs[:, voff[b]: voff[b] + n], vref.reshape(nb, n), what + " band vectors", fails))
        wf = max(wf, _pin(fisher[b], fref, what + " Fisher", fails))
        if not np.array_equal(np.triu(fisher[b], 1), np.triu(np.conj(fisher[b].T), 1)):     # (-0.0 == 0.0, NaN != NaN)
            fails.append("%s: the mirrored triangle of the Fisher matrix is not the conjugate of the other" % what)
    return fails, wv, wf


# ---- mutants: the case (and call) that has to catch each ------------------------------------------------------------
# kind 'q': (case, call) of dm_qestimate; 'alt': a case of dm_psmc_alt; 'moments': (nq, ns, shifted); 'draw': a draw case
MUTANT_CASE = dict(
    pol1=("q", "pol", (False, False, False, False)),
    table_T=("q", "pol", (True, False, False, False)),
    mask_gt=("q", "ells_L5", (False, False, False, False)),
    no_l0=("q", "pol", (True, True, False, True)),
    noise_256=("q", "modes", (False, True, False, True)),
    flags_swapped=("q", "modes600", (True, True, True, False)),
    last_lchunk=("q", "ells_L5", (True, False, False, False)),
    gram_2048=("alt", "gram", None),
    lower_noconj=("alt", "pol", None),
    moments_256=("moments", (2, 257, True), None),
    cov_ns=("moments", (18, 1000, False), None),
    draw_cap=("draw", "big_normal_p1", None),
)
# the transposed table shows in dm_psmc_alt as well, the masks and the dropped chunk too
ALT_MUTANT_CASE = dict(pol1="pol", table_T="pol", mask_gt="pol", no_l0="pol", last_lchunk="pol")


# ---- moments --------------------------------------------------------------------------------------------------------
MOMENT_NBLK = 3
MOMENT_NQ = (1, 2, 18)      # (12) one row; 18: 324 workgroups of psmc_cov_kernel, 153 of them above the diagonal
# (12) ns = 2, 3: the smallest divisors; 255, 256, 257: the strided walk of psmc_mean_kernel / psmc_cov_kernel one
#      short of full, full, and with a second trip of one sample; 1000: four trips, the last ragged
MOMENT_NS = (2, 3, 255, 256, 257, 1000)
MOMENT_GRID_NS = 16
MOMENT_SHIFT = 1e6         # (12) the second data set: a mean of 1e6 times the spread of every row


@functools.lru_cache(maxsize=None)
def moment_data(nq, ns, shifted):
    """q (3, nq, ns) float64: correlated samples of order one; `shifted`: plus 1e6 times the spread of its row.

    At ns = 2 and 3 the bounds are 10 and 11 u (mean), 18 and 19 u (covariance), and a float64 two-pass statement spends
    up to 3 and 6 roundings itself: a tenth of the bound is less than what float64 arithmetic on arbitrary data can keep
    (np.mean / np.cov reach 0.18 and 0.15 of the bounds there, whatever the seed).  So below MOMENT_GRID_NS samples the
    data lie on a grid of 2^-10 with a row sum that ns divides: mean, deviations and products are then exact in float64
    in any order, what is left is the one rounding of the last division, and every error of logic (a dropped sample, the
    divisor, a one-pass variance, which squares 2^30 grid units) shows as it does on arbitrary data."""
    rng = _rng("moments", nq, ns)
    mix = np.eye(nq) + 0.5 * rng.standard_normal((MOMENT_NBLK, nq, nq))
    q = mix @ rng.standard_normal((MOMENT_NBLK, nq, ns))
    sign = np.where(rng.random((MOMENT_NBLK, nq, 1)) < 0.5, -1.0, 1.0)
    shift = MOMENT_SHIFT * sign * q.std(axis=-1, keepdims=True)
    if ns < MOMENT_GRID_NS:
        k = np.rint(q * 1024.0).astype(np.int64)
        k[..., -1] -= k.sum(axis=-1) % ns
        assert not (k.sum(axis=-1) % ns).any()
        q, shift = k / 1024.0, np.rint(shift * 1024.0) / 1024.0
    if shifted:
        q = q + shift
    return _frozen(np.ascontiguousarray(q))


def ref_moments(q, mutant=None):
    """(mean, cov, mean bound, cov bound) in np.longdouble of q (nblk, nq, ns): two passes, ddof = 1."""
    ns = q.shape[-1]
    qq = q.astype(LD)
    mean = qq.sum(axis=-1) / ns
    d = qq - mean[..., None]
    cov = np.einsum("bas,bcs->bac", d, d) / (ns - 1)
    bm = (ns + 8) * LD(U) * np.abs(qq).sum(axis=-1) / ns
    bc = (ns + 16) * LD(U) * (np.einsum("bas,bcs->bac", np.abs(d), np.abs(d)) + ns * bm[:, :, None] * bm[:, None, :]) / (ns - 1)
    if mutant == "moments_256":
        mean = qq[..., :256].sum(axis=-1) / ns
        dm = qq[..., :256] - mean[..., None]
        cov = np.einsum("bas,bcs->bac", dm, dm) / (ns - 1)
    if mutant == "cov_ns":
        cov = cov * (ns - 1) / ns
    return mean, cov, bm, bc


def check_moments(q, mean, cov, mutant=None):
    """(failures, worst mean err / bound, worst covariance err / bound)."""
    nblk, nq, ns = q.shape
    rmean, rcov, bm, bc = ref_moments(q, mutant)
    fails = []
    if mean.shape != (nblk, nq) or cov.shape != (nblk, nq, nq):
        return ["shape"], np.inf, np.inf
    em, ec = np.abs(mean.astype(LD) - rmean), np.abs(cov.astype(LD) - rcov)
    if not (em <= bm).all():
        fails.append("mean: %d of %d elements outside the bound, worst err / bound %.3g"
                     % ((~(em <= bm)).sum(), em.size, float(np.nanmax(em / bm))))
    if not (ec <= bc).all():
        fails.append("covariance: %d of %d elements outside the bound, worst err / bound %.3g"
                     % ((~(ec <= bc)).sum(), ec.size, float(np.nanmax(ec / bc))))
    if not same_bits(cov, np.ascontiguousarray(cov.transpose(0, 2, 1))):
        fails.append("covariance: not equal to its transpose bit for bit")
    if not (np.diagonal(cov, axis1=1, axis2=2) >= 0).all():
        fails.append("covariance: a diagonal element is negative or NaN")
    wm, wc = float(np.max(em / bm)), float(np.max(ec / bc))
    return fails, (wm if np.isfinite(wm) else np.inf), (wc if np.isfinite(wc) else np.inf)


# ---- draws ----------------------------------------------------------------------------------------------------------
DRAW_TOL = 1e-14
DRAW_SEED = 0x123456789AB


def draw_case(name, ms, nmodes, R, s0, kind, power, stream):
    return dict(name=name, ms=ms, nmodes=nmodes, R=R, s0=s0, kind=kind, power=power, stream=stream)


DRAW_CASES = [
    # (10) 1100 x 1000 = 1.1 M elements, more than the 4096 x 256 threads of the capped grid: the stride loop of
    #      psmc_draw_kernel makes a second trip for the elements from 1 048 576 on; beside a block of 18 elements, whose
    #      workgroups beyond the first have nothing to do.  Both kinds; normal draws with power 1 and 0, Rademacher -1.
    draw_case("big_normal_p1", (17, 4), (1100, 6), 1000, 5, 0, 1, 0),
    draw_case("big_normal_p0", (17, 4), (1100, 6), 1000, 5, 0, 0, 1),
    draw_case("big_rademacher", (17, 4), (1100, 6), 1000, 5, 1, -1, 2),
    # (11) sample numbers 2^31 - 4 ... 2^31 + 3: the counter word s0 + r is formed in uint32_t
    draw_case("wrap_normal", (3,), (5,), 8, 2 ** 31 - 4, 0, 1, 0),
    draw_case("wrap_rademacher", (3,), (5,), 8, 2 ** 31 - 4, 1, -1, 2),
]
DRAW_BY_NAME = {c["name"]: c for c in DRAW_CASES}


@functools.lru_cache(maxsize=None)
def draw_evals(name):
    c = DRAW_BY_NAME[name]
    rng = _rng("draw evals", c["nmodes"])
    return [_frozen(5.0 * rng.random(n)) for n in c["nmodes"]]


def draw_layout(c):
    """(NaN buffer, x_off, evals buffer, evals_off): GAP elements in front of every block and after the last."""
    buf, xoff = _gapped([np.empty(n * c["R"], dtype=np.complex128) for n in c["nmodes"]], np.complex128)
    buf[:] = POISON
    ev, eoff = _gapped(draw_evals(c["name"]), np.float64)
    return buf, xoff, ev, eoff


@functools.lru_cache(maxsize=None)
def _ref_draw(name, b):
    c = DRAW_BY_NAME[name]
    return _frozen(draws(DRAW_SEED, c["ms"][b], c["nmodes"][b], c["R"], c["stream"], kind=c["kind"], power=c["power"],
                         evals=draw_evals(name)[b], start=c["s0"]))


def ref_draw(c, b, mutant=None):
    """The (nmodes, R) draws of block b; computed once."""
    ref = _ref_draw(c["name"], b)
    if mutant == "draw_cap" and ref.size > DRAW_CAP:
        ref = ref.copy()
        ref.reshape(-1)[DRAW_CAP:] = POISON
    return ref


def check_draw(c, buf, mutant=None):
    """(failures, worst err / (1e-14 max|ref|) of the normal draws) of a result buffer laid out by draw_layout."""
    start, xoff, _, _ = draw_layout(c)
    if buf.shape != start.shape:
        return ["buffer shape changed"], np.inf
    fails, worst = [], 0.0
    inside = np.zeros(buf.size, dtype=bool)
    for b, n in enumerate(c["nmodes"]):
        sl = slice(xoff[b], xoff[b] + n * c["R"])
        inside[sl] = True
        got, ref = buf[sl].reshape(n, c["R"]), ref_draw(c, b, mutant)
        if c["kind"] == 1:
            if not same_bits(got, ref):
                fails.append("%s block %d: Rademacher draws differ in %d elements"
                             % (c["name"], b, (_cbits(got) != _cbits(ref)).reshape(n, c["R"], 2).any(axis=2).sum()))
        else:
            err = np.abs(got - ref)
            bad = ~(err <= DRAW_TOL * np.abs(_ref_draw(c["name"], b)).max())
            ratio = float(np.nanmax(err)) / (DRAW_TOL * float(np.abs(_ref_draw(c["name"], b)).max()))
            worst = np.inf if bad.any() and not np.isfinite(err).all() else max(worst, ratio)
            if bad.any():
                fails.append("%s block %d: %d normal draws outside 1e-14 max|ref|, the first at element %d"
                             % (c["name"], b, bad.sum(), int(np.flatnonzero(bad.reshape(-1))[0])))
    moved = ((_cbits(buf).reshape(-1, 2) != _cbits(start).reshape(-1, 2)).any(axis=1) & ~inside).sum()
    if moved:
        fails.append("%s: %d elements between the blocks were written" % (c["name"], moved))
    return fails, worst
