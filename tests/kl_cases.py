"""Case tables, long-double references and bounds for the KL covariance stage: `dm_project_cov`, `dm_project_diag`,
`dm_regularise` (driftscan_amd/csrc/dm_kl.hip) and `dm_fisher` (dm_fisher.hip), plus the pencils and the batch of the
`dm_eigh_gen` bookkeeping and driver tests.

Nothing here needs a GPU.  `COV_CASES`, `DIAG_CASES`, `REG_CASES` and `FISHER` list the launches; `cov_layout` /
`diag_layout` / `reg_layout` lay one out in a poisoned host buffer; `ref_project_cov`, `ref_project_diag`,
`ref_regularise` and `ref_fisher` are the references; `check_cov` / `check_diag` / `check_reg` / `check_fisher` compare
a result with them; `run_*` send a launch through the `Context` wrappers.

Layout.  Every output buffer holds its blocks at offsets with GAP = 5 poisoned (NaN) elements in front of each one.  A
view that the call overwrites starts as NaN and must come back finite, a view that it accumulates onto starts as a
random, non-Hermitian C0; everything outside the views keeps its bits.

Beams and the l0 mask.  The device gets beams that are NOT zero below l0; the references mask the multipoles below
clamp(l0, 0, L) themselves, so the mask and its clamp are under test.

Bounds (derived, nothing measured), for the real and the imaginary part of every element separately:

    project_cov:   |got - ref| <= npairs (2 Kc + 8) 2^-53 ( sum_pairs (|B| |C_l| |B|^H)_ij + |C0_ij| ),  Kc = L - l0
    project_diag:  |got - ref| <= (2 T + 8) 2^-53 ( |alpha| (|U| |d| |U|^H)_ij + |C0_ij| )

the (2K + 8) 2^-53 bound of gemm_cases.py applied once per accumulated pol pair: every partial sum is bounded by the
total of the moduli.  An element whose bound is 0 (a block with l0 >= L, every pair masked, an off-diagonal frequency
block of project_diag) has to be exact; where the call accumulates onto such an element it keeps its bits.  On the
mirror route the frequency blocks f != f' also satisfy out[j, i] == conj(out[i, j]) bit for bit.

    regularise:    each part of a diagonal element is fl(v + fl(reg m)) or the single rounding fma(reg, m, v) — the
                   compiler may contract — with m numpy's lexicographic complex max; every other element keeps its bits.
                   (NaN inputs are out of scope: numpy propagates them, the kernel does not.)

    fisher:        |got - ref| <= 1e-12 max|F_ref| per block, the project's pin for the estimators
                   (test_gpu_band_edges.py).  A componentwise bound through the abs matrices is of no use here, E S E^H
                   cancels heavily: it comes to 3e-6 of |F|.  The float64 restatement oracle.psfisher.fisher_m lies at
                   4.4e-16 max|F_ref| from the long-double value on this batch (test_host_kl_cases.py asserts <= 1e-13
                   and prints it).

`MUTANTS` are reference-level mistakes; test_host_kl_cases.py shows that each one leaves a bound or the pin on a
named case.
"""
import functools
import zlib
from fractions import Fraction

import numpy as np

from gemm_cases import LD, LD_OK, U  # noqa: F401  (LD_OK is re-exported for the test modules)

CLD = np.clongdouble
GAP = 5
POISON = complex(np.nan, np.nan)
CHUNK = 16384          # contraction chunk of the Gram product of dm_fisher
FISHER_PIN = 1e-12
MUTANTS = ("l0", "lastl", "mirror", "weight_ff", "polswap", "svoffset", "lexmax_re", "lastchunk", "sqrtw")

SHAPES = dict(small=dict(F=3, K=4, L=6, P=1), tiles=dict(F=5, K=30, L=7, P=1), pol=dict(F=3, K=12, L=6, P=4))
# kept modes per (block, frequency).  "tiles": ndof = 64, 65, 129, 150 and 0; a frequency without modes first (block 0),
# in the middle and last (block 1; 129 and 150 cannot have one with K = 30)
SVNUM = dict(
    small=((4, 3, 0), (0, 4, 2), (1, 0, 4), (4, 4, 4)),
    tiles=((0, 20, 20, 20, 4), (30, 30, 0, 5, 0), (30, 30, 30, 30, 9), (30, 30, 30, 30, 30), (0, 0, 0, 0, 0)),
    pol=((12, 7, 0), (0, 12, 5), (3, 0, 12), (12, 12, 12), (0, 0, 0)),
)


def l0_pool(L):
    return (0, L - 1, L, -3, L + 2, 3)


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _crand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def _frozen(a):
    a.setflags(write=False)
    return a


def _dev(ctx, a):
    return ctx.to_device(np.array(a))     # a writable copy: the tables themselves are read-only


def svnum_of(shape):
    return np.array(SVNUM[shape], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def beams(shape):
    """(nblk, F, K, P, L) complex, not zero anywhere."""
    s = SHAPES[shape]
    return _frozen(_crand(_rng("beam", shape), len(SVNUM[shape]), s["F"], s["K"], s["P"], s["L"]))


@functools.lru_cache(maxsize=None)
def cl_table(shape, sym):
    """(P, P, F, F, L) real.  `sym`: symmetric in the two frequencies for every pol pair (and still different for (p, q)
    and (q, p)); else asymmetric in the frequencies too."""
    s = SHAPES[shape]
    cl = _rng("cl", shape).standard_normal((s["P"], s["P"], s["F"], s["F"], s["L"]))
    if sym:
        cl = cl + cl.transpose(0, 1, 3, 2, 4)   # exactly symmetric: the two sums commute
    return _frozen(np.ascontiguousarray(cl))


# ---- layouts --------------------------------------------------------------------------------------------------------
class Layout(object):
    """buf: the poisoned host buffer as the device receives it; off / n: element offset and size of every block; in_view:
    True inside the block views."""


def block_layout(ns, key, start):
    """start: 'nan' (views NaN) or 'c0' (views random and non-Hermitian)."""
    lay = Layout()
    lay.n = [int(n) for n in ns]
    lay.off, at = [], 0
    for n in lay.n:
        at += GAP
        lay.off.append(at)
        at += n * n
    total = at + GAP
    lay.buf = np.full(total, POISON, dtype=np.complex128)
    lay.in_view = np.zeros(total, dtype=bool)
    rng = _rng("c0", key)
    for n, off in zip(lay.n, lay.off):
        lay.in_view[off: off + n * n] = True
        if start == "c0":
            lay.buf[off: off + n * n] = _crand(rng, n * n)
    lay.off = np.array(lay.off, dtype=np.int64)
    return lay


def view(lay, buf, b):
    n = lay.n[b]
    return buf[lay.off[b]: lay.off[b] + n * n].reshape(n, n)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64).reshape(-1, 2)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def outside_changed(before, after, in_view):
    """Number of elements outside every view whose bits changed."""
    return int(((_bits(before) != _bits(after)).any(axis=1) & ~in_view).sum())


def _within(got, ref, bound, what):
    """(failures, worst ratio) of got against the long-double ref with the bound on each part."""
    if got.size == 0:
        return [], 0.0
    er = np.abs(got.real.astype(LD) - ref.real)
    ei = np.abs(got.imag.astype(LD) - ref.imag)
    err = np.maximum(er, ei)
    bad = ~(er <= bound) | ~(ei <= bound)    # a NaN fails
    pos = bound > 0
    ratio = float(np.max(np.where(pos, err / np.where(pos, bound, 1), 0)))
    if not np.isfinite(ratio):
        ratio = np.inf
    fails = []
    if bad.any():
        i, j = (int(x[0]) for x in np.nonzero(bad))
        fails.append("%s: %d of %d elements outside the bound, first (%d, %d): err %.3e, bound %.3e"
                     % (what, bad.sum(), bad.size, i, j, float(err[i, j]), float(bound[i, j])))
    return fails, ratio


# ---- project_cov ----------------------------------------------------------------------------------------------------
def cov_case(name, shape, rot, sym_cl, symmetric, zero_first=True, npol=None, mask=None, env_full=False):
    """mask: None, 'diag', 'tq' (the diagonal plus (T,Q) and (Q,T)), 'none' (every pair masked) or 'tt' ((T,T) alone).
    Block b gets l0 = l0_pool(L)[(b + rot) % 6].  A caller may only say `symmetric` for a table that is."""
    assert sym_cl or not symmetric
    return dict(name=name, shape=shape, rot=rot, sym_cl=sym_cl, symmetric=symmetric, zero_first=zero_first, npol=npol,
                mask=mask, env_full=env_full)


COV_CASES = [
    cov_case("small_full", "small", 0, False, False),
    cov_case("small_mirror", "small", 3, True, True),
    cov_case("tiles_full", "tiles", 3, False, False),
    cov_case("tiles_full_rot0", "tiles", 0, False, False),
    cov_case("tiles_mirror", "tiles", 3, True, True),
    cov_case("tiles_mirror_rot1", "tiles", 1, True, True),
    cov_case("tiles_mirror_rot4", "tiles", 4, True, True),
    cov_case("pol_mirror_diag", "pol", 3, True, True, mask="diag"),
    cov_case("pol_fallback_tq", "pol", 3, True, True, mask="tq"),
    cov_case("tiles_sym_accumulate", "tiles", 5, True, True, zero_first=False),
    cov_case("pol_sym_accumulate", "pol", 2, True, True, zero_first=False, mask="diag"),
    cov_case("pol_npol1_nomask", "pol", 3, True, True, npol=1),
    cov_case("pol_npol1_mask", "pol", 0, False, False, npol=1, mask="tt"),
    cov_case("pol_dense_nomask", "pol", 3, False, False),
    cov_case("pol_dense_nomask_sym", "pol", 5, True, True),
    cov_case("tiles_allmasked_zero", "tiles", 3, False, False, mask="none"),
    cov_case("tiles_allmasked_keep", "tiles", 3, False, False, zero_first=False, mask="none"),
    cov_case("pol_allmasked_zero", "pol", 3, True, True, mask="none"),
    cov_case("pol_allmasked_keep", "pol", 3, True, True, zero_first=False, mask="none"),
    cov_case("tiles_envfull", "tiles", 3, True, True, env_full=True),
    cov_case("pol_envfull_diag", "pol", 3, True, True, mask="diag", env_full=True),
]
COV_BY_NAME = {c["name"]: c for c in COV_CASES}


def cov_mask(c):
    """The (P, P) int mask handed to the library, or None."""
    P = SHAPES[c["shape"]]["P"]
    if c["mask"] is None:
        return None
    m = np.zeros((P, P), dtype=np.int32)
    if c["mask"] in ("diag", "tq"):
        m[np.arange(P), np.arange(P)] = 1
    if c["mask"] == "tq":
        m[0, 1] = m[1, 0] = 1
    if c["mask"] == "tt":
        m[0, 0] = 1
        m[1:, :] = 1      # rows beyond npol are not to be looked at
    return m


def cov_pairs(c):
    P = SHAPES[c["shape"]]["P"]
    npol = P if c["npol"] is None else c["npol"]
    m = cov_mask(c)
    return [(pi, pj) for pi in range(npol) for pj in range(npol) if m is None or m[pi, pj]]


def cov_l0(c):
    pool = l0_pool(SHAPES[c["shape"]]["L"])
    return np.array([pool[(b + c["rot"]) % len(pool)] for b in range(len(SVNUM[c["shape"]]))], dtype=np.int64)


def cov_route(c):
    """The route rule of dm_project_cov restated: 'accumulate' without the clear bit; with it 'mirror' when the caller
    vouches for the frequency symmetry, DM_COV_FULL is unset and no unmasked pair is off the diagonal — 'fallback' when
    only such a pair prevents it — and 'full' otherwise."""
    if not c["zero_first"]:
        return "accumulate"
    if not c["symmetric"] or c["env_full"]:
        return "full"
    return "fallback" if any(pi != pj for pi, pj in cov_pairs(c)) else "mirror"


def ref_project_cov(beam, svnum, cl, l0, pairs, C0=None, mutant=None):
    """One block in np.clongdouble: (value, bound).  beam (F, K, P, L) unmasked, cl (P, P, F, F, L), l0 any int."""
    F, K, P, L = beam.shape
    svnum = [int(x) for x in svnum]
    n = sum(svnum)
    l0c = min(max(int(l0), 0), L)
    lo, hi = l0c, L
    if mutant == "l0":
        lo = l0c - 1 if l0c > 0 else 1
    if mutant == "lastl":
        hi = L - 1
    Kc = L - l0c
    fr = np.repeat(np.arange(F), svnum)           # frequency of every row
    shifted = next((f for f in range(F) if svnum[f] > 0), None) if mutant == "svoffset" else None

    def rows(p):
        parts = []
        for f in range(F):
            src = np.roll(beam[f, :, p, :], -1, axis=0) if f == shifted else beam[f, :, p, :]
            parts.append(src[: svnum[f], lo:hi])
        return np.concatenate(parts, axis=0).astype(CLD) if n else np.zeros((0, max(hi - lo, 0)), dtype=CLD)

    out = np.zeros((n, n), dtype=CLD)
    ab = np.zeros((n, n), dtype=LD)
    if n and hi > lo:
        for pi, pj in pairs:
            Ri, Rj = (rows(pj), rows(pi)) if mutant == "polswap" else (rows(pi), rows(pj))
            W = cl[pi, pj][fr[:, None], fr[None, :], lo:hi].astype(LD)
            if mutant == "weight_ff":
                W = W.transpose(1, 0, 2)
            for k in range(hi - lo):
                out += (Ri[:, k, None] * W[:, :, k]) * Rj[:, k].conj()[None, :]
                ab += (np.abs(Ri[:, k, None]) * np.abs(W[:, :, k])) * np.abs(Rj[:, k])[None, :]
        if mutant == "mirror":
            low = fr[:, None] > fr[None, :]
            out = np.where(low, out.T, out)
    c0 = np.zeros((n, n), dtype=CLD) if C0 is None else C0.astype(CLD)
    bound = len(pairs) * (2 * Kc + 8) * LD(U) * (ab + np.abs(c0))
    return out + c0, bound


def cov_layout(c):
    ndof = svnum_of(c["shape"]).sum(axis=1)
    return block_layout(ndof, ("cov", c["name"]), "nan" if c["zero_first"] else "c0")


@functools.lru_cache(maxsize=None)
def _cov_refs(name, mutant=None):
    c = COV_BY_NAME[name]
    lay = cov_layout(c)
    beam, cl, sv, l0 = beams(c["shape"]), cl_table(c["shape"], c["sym_cl"]), svnum_of(c["shape"]), cov_l0(c)
    return [ref_project_cov(beam[b], sv[b], cl, l0[b], cov_pairs(c), None if c["zero_first"] else view(lay, lay.buf, b),
                            mutant) for b in range(len(sv))]


def cov_refs(c, mutant=None):
    """[(value, bound)] per block, computed once."""
    return _cov_refs(c["name"], mutant)


def cov_refs_as_buffer(c, mutant=None):
    """The float64 rounding of the (mutated) reference laid out like a device result."""
    lay = cov_layout(c)
    out = lay.buf.copy()
    for b, (ref, _) in enumerate(cov_refs(c, mutant)):
        view(lay, out, b)[...] = ref.astype(np.complex128)
    return out


def check_cov(c, out):
    """(failures, worst err / bound) of the result buffer of a project_cov launch."""
    lay = cov_layout(c)
    if out.shape != lay.buf.shape:
        return ["buffer shape changed"], np.inf
    fails, worst = [], 0.0
    moved = outside_changed(lay.buf, out, lay.in_view)
    if moved:
        fails.append("%d elements outside the views changed" % moved)
    sv, l0, L = svnum_of(c["shape"]), cov_l0(c), SHAPES[c["shape"]]["L"]
    route = cov_route(c)
    for b, (ref, bound) in enumerate(cov_refs(c)):
        got = view(lay, out, b)
        f, r = _within(got, ref, bound, "%s block %d" % (c["name"], b))
        fails += f
        worst = max(worst, r)
        if not c["zero_first"] and (not cov_pairs(c) or l0[b] >= L) and not same_bits(got, view(lay, lay.buf, b)):
            fails.append("%s block %d: nothing to add, yet the bits of C0 changed" % (c["name"], b))
        if route == "mirror" and got.size and cov_pairs(c) and l0[b] < L:   # (a zero fill is +0 on both sides)
            fr = np.repeat(np.arange(len(sv[b])), sv[b])
            off = fr[:, None] != fr[None, :]
            ne = (_bits(got) != _bits(np.conj(got.T))).any(axis=1).reshape(got.shape) & off
            if ne.any():
                fails.append("%s block %d: %d mirrored elements are not the bitwise conjugate" % (c["name"], b, ne.sum()))
    return fails, worst


def run_cov(ctx, c):
    """One `project_cov` call on a fresh device copy of the layout; the result buffer on the host.  DM_COV_FULL is the
    caller's to set (monkeypatch) for the cases with env_full."""
    lay = cov_layout(c)
    out = ctx.to_device(lay.buf)
    beam = _dev(ctx, beams(c["shape"]))
    cl = _dev(ctx, cl_table(c["shape"], c["sym_cl"]))
    ctx.project_cov(beam, svnum_of(c["shape"]), cl, out, lay.off, npol=c["npol"], polmask=cov_mask(c), l0=cov_l0(c),
                    zero_first=c["zero_first"], symmetric=c["symmetric"])
    ctx.sync()
    return out.cpu().numpy()


# ---- project_diag ---------------------------------------------------------------------------------------------------
DIAG_T = (1, 20, 67)
DIAG_ALPHA = (1.0, 0.37)
DIAG_CASES = [dict(name="diag_T%d_a%g_%s" % (T, a, "acc" if acc else "set"), T=T, alpha=a, accumulate=acc)
              for T in DIAG_T for a in DIAG_ALPHA for acc in (False, True)]


@functools.lru_cache(maxsize=None)
def diag_inputs(T):
    """beam_ut (nblk, F, K, T) and dmat (F, T) of the "tiles" shape; row 1 of dmat is all zero, the signs are mixed."""
    s = SHAPES["tiles"]
    rng = _rng("diag", T)
    ut = _crand(rng, len(SVNUM["tiles"]), s["F"], s["K"], T)
    d = rng.uniform(0.5, 2.0, (s["F"], T)) * np.where(rng.random((s["F"], T)) < 0.25, -1.0, 1.0)
    d[1] = 0.0
    return _frozen(ut), _frozen(d)


def ref_project_diag(ut, svnum, dmat, alpha, C0=None):
    """One block in np.clongdouble: (value, bound).  ut (F, K, T), dmat (F, T)."""
    F, K, T = ut.shape
    svnum = [int(x) for x in svnum]
    n = sum(svnum)
    out = np.zeros((n, n), dtype=CLD)
    ab = np.zeros((n, n), dtype=LD)
    at = 0
    for f in range(F):
        m = svnum[f]
        u = ut[f, :m].astype(CLD)
        d = dmat[f].astype(LD)
        for k in range(T if m else 0):
            out[at: at + m, at: at + m] += (u[:, k, None] * d[k]) * u[:, k].conj()[None, :]
            ab[at: at + m, at: at + m] += (np.abs(u[:, k, None]) * abs(d[k])) * np.abs(u[:, k])[None, :]
        at += m
    c0 = np.zeros((n, n), dtype=CLD) if C0 is None else C0.astype(CLD)
    bound = (2 * T + 8) * LD(U) * (abs(LD(alpha)) * ab + np.abs(c0))
    return LD(alpha) * out + c0, bound


def diag_layout(c):
    return block_layout(svnum_of("tiles").sum(axis=1), ("diag", c["name"]), "c0" if c["accumulate"] else "nan")


@functools.lru_cache(maxsize=None)
def _diag_refs(name):
    c = next(x for x in DIAG_CASES if x["name"] == name)
    lay = diag_layout(c)
    ut, d = diag_inputs(c["T"])
    sv = svnum_of("tiles")
    return [ref_project_diag(ut[b], sv[b], d, c["alpha"], view(lay, lay.buf, b) if c["accumulate"] else None)
            for b in range(len(sv))]


def diag_refs(c):
    return _diag_refs(c["name"])


def check_diag(c, out):
    lay = diag_layout(c)
    if out.shape != lay.buf.shape:
        return ["buffer shape changed"], np.inf
    fails, worst = [], 0.0
    moved = outside_changed(lay.buf, out, lay.in_view)
    if moved:
        fails.append("%d elements outside the views changed" % moved)
    sv = svnum_of("tiles")
    for b, (ref, bound) in enumerate(diag_refs(c)):
        got = view(lay, out, b)
        f, r = _within(got, ref, bound, "%s block %d" % (c["name"], b))
        fails += f
        worst = max(worst, r)
        if got.size:
            fr = np.repeat(np.arange(len(sv[b])), sv[b])
            off = fr[:, None] != fr[None, :]
            if c["accumulate"]:
                moved = ((_bits(got) != _bits(view(lay, lay.buf, b))).any(axis=1).reshape(got.shape) & off).sum()
                if moved:
                    fails.append("%s block %d: %d elements of off-diagonal frequency blocks changed" % (c["name"], b, moved))
            elif (got[off] != 0).any():
                fails.append("%s block %d: off-diagonal frequency blocks are not exactly 0" % (c["name"], b))
    return fails, worst


def run_diag(ctx, c):
    lay = diag_layout(c)
    ut, d = diag_inputs(c["T"])
    out = ctx.to_device(lay.buf)
    ctx.project_diag(_dev(ctx, ut), svnum_of("tiles"), _dev(ctx, d), out, lay.off, alpha=c["alpha"],
                     accumulate=c["accumulate"])
    ctx.sync()
    return out.cpu().numpy()


# ---- regularise -----------------------------------------------------------------------------------------------------
REG_N = (1, 2, 255, 0, 256, 257, 300)       # one call; the empty block sits in the middle
REG_VALUES = (1e-14, 0.5)
REG_DESIGNS = ("unique", "tie_early", "tie_late", "negative", "last")
REG_CASES = [dict(name="reg_%s_%g" % (d, r), design=d, reg=r) for d in REG_DESIGNS for r in REG_VALUES]
TIE_SPLIT = 4096   # 16 workgroups of 256: flat indices below belong to the first stride pass, those from it to the second


def tie_positions(n):
    """Flat indices of the two tied entries: on either side of 4096 where the matrix is that large (workgroup 15 in the
    first pass, workgroup 0 in the second), else the second and the last but one element."""
    if n * n > 4200:
        return 4000, 4200
    return (1, n * n - 2) if n * n >= 4 else None


@functools.lru_cache(maxsize=None)
def reg_matrix(design, n):
    """Non-Hermitian complex, parts in (-1, 1), with the designed maximum."""
    rng = _rng("reg", design, n)
    A = rng.uniform(-1, 1, (n, n)) + 1j * rng.uniform(-1, 1, (n, n))
    flat = A.reshape(-1)
    if n == 0:
        return _frozen(A)
    if design == "unique" and n > 1:
        flat[n * n - n] = 2.5 + 0.3j           # (n - 1, 0): off the diagonal
    elif design in ("tie_early", "tie_late") and tie_positions(n):
        p, q = tie_positions(n)
        hi, lo = 2.5 + 0.9j, 2.5 + 0.1j
        flat[p], flat[q] = (hi, lo) if design == "tie_early" else (lo, hi)
    elif design == "negative":
        A.real[...] = -np.abs(A.real) - 0.1
    elif design == "last":
        flat[n * n - 1] = 2.5 + 0.3j
    return _frozen(A)


def lexmax(A, mutant=None):
    """numpy's complex max, lexicographic in (re, im); the mutant breaks ties on the real part by position."""
    flat = A.reshape(-1)
    if mutant == "lexmax_re":
        return flat[int(np.argmax(flat.real))]
    cand = flat[flat.real == flat.real.max()]
    return cand[int(np.argmax(cand.imag))]


def _fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))    # Fraction -> float rounds correctly, once


def ref_regularise(A, reg, mutant=None):
    """(two-rounding diagonal, fma diagonal) as complex128 vectors; every other element is A's."""
    n = A.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.complex128), np.zeros(0, dtype=np.complex128)
    m = lexmax(A, mutant)
    d = A.diagonal()
    two = (d.real + reg * m.real) + 1j * (d.imag + reg * m.imag)
    one = np.array([complex(_fma(reg, m.real, v.real), _fma(reg, m.imag, v.imag)) for v in d])
    return two, one


def reg_layout(c):
    lay = block_layout(REG_N, ("reg", c["name"]), "nan")
    for b, n in enumerate(REG_N):
        view(lay, lay.buf, b)[...] = reg_matrix(c["design"], n)
    return lay


def reg_expected(c, mutant=None):
    """The two-rounding result as a device buffer would hold it."""
    lay = reg_layout(c)
    out = lay.buf.copy()
    for b, n in enumerate(REG_N):
        two, _ = ref_regularise(reg_matrix(c["design"], n), c["reg"], mutant)
        v = view(lay, out, b)
        v[np.arange(n), np.arange(n)] = two
    return out


def check_reg(c, out):
    """failures of the result buffer of a regularise launch."""
    lay = reg_layout(c)
    if out.shape != lay.buf.shape:
        return ["buffer shape changed"]
    fails = []
    moved = outside_changed(lay.buf, out, lay.in_view)
    if moved:
        fails.append("%d elements outside the views changed" % moved)
    for b, n in enumerate(REG_N):
        if n == 0:
            continue
        A = reg_matrix(c["design"], n)
        got = view(lay, out, b)
        offd = ~np.eye(n, dtype=bool)
        moved = ((_bits(got) != _bits(A)).any(axis=1).reshape(n, n) & offd).sum()
        if moved:
            fails.append("%s n=%d: %d off-diagonal elements changed" % (c["name"], n, moved))
        two, one = ref_regularise(A, c["reg"])
        d = got.diagonal()
        ok = ((d.real == two.real) | (d.real == one.real)) & ((d.imag == two.imag) | (d.imag == one.imag))
        if not ok.all():
            i = int(np.nonzero(~ok)[0][0])
            fails.append("%s n=%d: %d diagonal elements are neither fl(v + fl(reg m)) nor fma(reg, m, v), first %d: got %r, "
                         "expected %r" % (c["name"], n, (~ok).sum(), i, d[i], two[i]))
    return fails


def run_reg(ctx, c):
    lay = reg_layout(c)
    out = ctx.to_device(lay.buf)
    ctx.regularise(out, np.array(REG_N), lay.off, c["reg"])
    ctx.sync()
    return out.cpu().numpy()


# ---- fisher ---------------------------------------------------------------------------------------------------------
FISHER = dict(nbands=3, order=(3, 2, 1, 0, 4), nmodes=(140, 129, 1, 0, 0))
# blocks of the "tiles" shape reordered to ndof = (150, 129, 65, 64, 0); l0 = (0, 3, L - 1, 0, 0)


def fisher_chunks():
    return [-(-(m * m) // CHUNK) for m in FISHER["nmodes"]]


@functools.lru_cache(maxsize=None)
def fisher_inputs():
    s = SHAPES["tiles"]
    order = list(FISHER["order"])
    rng = _rng("fisher")
    d = dict(beam=np.ascontiguousarray(beams("tiles")[order]), svnum=svnum_of("tiles")[order],
             l0=np.array([0, 3, s["L"] - 1, 0, 0], dtype=np.int64), nmodes=np.array(FISHER["nmodes"], dtype=np.int64))
    cl = rng.standard_normal((FISHER["nbands"], s["L"], s["F"], s["F"]))
    d["cl"] = cl + cl.transpose(0, 1, 3, 2)            # (nbands, L, F, F), symmetric in the frequencies
    d["ndof"] = d["svnum"].sum(axis=1)
    d["E"], d["lam"] = [], []
    for n, m in zip(d["ndof"], d["nmodes"]):
        q = np.linalg.qr(_crand(rng, int(n), int(m)))[0] if m else np.zeros((int(n), 0), dtype=np.complex128)
        d["E"].append(np.ascontiguousarray(q.T))        # orthonormal rows = modes
        d["lam"].append(0.1 + 5.0 * rng.random(int(m)))
    # device layout of the modes and eigenvalues: NaN gaps in front of every block, which nothing may read
    eoff, voff, ea, va = [], [], 0, 0
    for n, m in zip(d["ndof"], d["nmodes"]):
        ea += GAP
        va += GAP
        eoff.append(ea)
        voff.append(va)
        ea += int(n) * int(m)
        va += int(m)
    d["evecs_buf"] = np.full(ea + GAP, POISON, dtype=np.complex128)
    d["evals_buf"] = np.full(va + GAP, np.nan, dtype=np.float64)
    for b, (E, lam) in enumerate(zip(d["E"], d["lam"])):
        d["evecs_buf"][eoff[b]: eoff[b] + E.size] = E.ravel()
        d["evals_buf"][voff[b]: voff[b] + lam.size] = lam
    d["evecs_off"], d["evals_off"] = np.array(eoff, dtype=np.int64), np.array(voff, dtype=np.int64)
    return d


def _cmatmul(A, B):
    """A @ B for np.clongdouble through four real products (numpy's long-double matmul has no complex fast path)."""
    ar, ai, br, bi = A.real, A.imag, B.real, B.imag
    out = np.empty((A.shape[0], B.shape[1]), dtype=CLD)
    out.real = ar @ br - ai @ bi
    out.imag = ar @ bi + ai @ br
    return out


@functools.lru_cache(maxsize=None)
def _fisher_bands(b):
    """D_a = Et S_a Et^H of block b for every band, unweighted (Et = E here; the weights are applied afterwards)."""
    d = fisher_inputs()
    E = d["E"][b].astype(CLD)
    out = []
    for a in range(FISHER["nbands"]):
        cl = np.ascontiguousarray(d["cl"][a].transpose(1, 2, 0))[None, None]     # (1, 1, F, F, L)
        S, _ = ref_project_cov(d["beam"][b], d["svnum"][b], cl, d["l0"][b], [(0, 0)])
        out.append(_cmatmul(_cmatmul(E, S), E.conj().T))
    return out


def ref_fisher(b, mutant=None):
    """F_ab = sum_ij D_a[i, j] conj(D_b[i, j]) of block b in long double, D_a = Et S_a Et^H, Et = diag((lam + 1)^-1/2) E."""
    d = fisher_inputs()
    nb, m = FISHER["nbands"], int(d["nmodes"][b])
    w = (d["lam"][b].astype(LD) + 1) ** (LD(-1) if mutant == "sqrtw" else LD(-0.5))
    D = [(Da * w[:, None] * w[None, :]).reshape(-1) for Da in _fisher_bands(b)]
    if mutant == "lastchunk":
        D = [x[:CHUNK] for x in D]
    F = np.zeros((nb, nb), dtype=CLD)
    for a in range(nb):
        for c in range(nb):
            F[a, c] = np.sum(D[a] * D[c].conj()) if m else 0
    return F


def check_fisher(got, mutant=None):
    """(failures, worst err / (1e-12 max|F_ref|)) of a (nblk, nbands, nbands) result against the (mutated) reference —
    the mutant argument turns the check round for the host test: `got` is then held against a wrong reference."""
    d = fisher_inputs()
    fails, worst = [], 0.0
    for b in range(len(d["ndof"])):
        ref = ref_fisher(b, mutant)
        scale = float(np.abs(ref).max())
        if not np.isfinite(got[b].real).all() or not np.isfinite(got[b].imag).all():
            fails.append("fisher block %d is not finite" % b)
            continue
        err = float(np.abs(got[b].astype(CLD) - ref).max())
        if scale == 0.0:
            if err != 0.0:
                fails.append("fisher block %d has no modes and is not exactly 0" % b)
            continue
        worst = max(worst, err / (FISHER_PIN * scale))
        if not err <= FISHER_PIN * scale:
            fails.append("fisher block %d: err %.3e of max|F|, pin %.0e" % (b, err / scale, FISHER_PIN))
    return fails, worst


def run_fisher(ctx, cl_symmetric):
    d = fisher_inputs()
    cl = ctx.to_device(np.ascontiguousarray(d["cl"].transpose(0, 2, 3, 1)))     # (nbands, F, F, L)
    out = ctx.fisher(ctx.to_device(d["beam"]), d["svnum"], d["l0"], cl, ctx.to_device(d["evecs_buf"]), d["evecs_off"],
                     d["nmodes"], ctx.to_device(d["evals_buf"]), d["evals_off"], cl_symmetric=cl_symmetric)
    return out.cpu().numpy()


# ---- eigh_gen: pencils with a known spectrum ------------------------------------------------------------------------
EIGH_NS = (33, 20, 0, 65, 7)       # the second one gets A = 0; the 'npd' pencil of tests/golden/eigh_gen.npz follows
EIGH_ZERO = 1
EIGH_CUT = 1e9
# The golden 'npd' pencil has its eigenvalues at 1.5e-3 ... 39.5 and 2.2e10 ... 7.5e10: the cut sits in that gap, 1e9 from
# the one side and 2e10 from the other, more than 1e-3 lambda_max — a round value inside the gap that the golden spectrum
# fixes, not its midpoint; the margin is what counts.  The designed spectra keep the same distance
# (test_host_kl_cases.py asserts it for every pencil of the batch).


def eigh_spectrum(n):
    """n ascending eigenvalues with gaps: the lower two thirds in [0.1, 1e7], the others in [1e10, 1e11]."""
    k = n - n // 3
    return np.concatenate([np.logspace(-1, 7, k), np.logspace(10, 11, n - k)])


@functools.lru_cache(maxsize=None)
def pencil(n, zero=False):
    """(A, B, lambda): B = L L^H with a well-conditioned L, A = L Q diag(lambda) Q^H L^H, both exactly Hermitian."""
    rng = _rng("pencil", n)
    if n == 0:
        z = np.zeros((0, 0), dtype=np.complex128)
        return z, z, np.zeros(0)
    Lm = np.tril(_crand(rng, n, n), -1) / np.sqrt(2.0 * n)
    Lm[np.arange(n), np.arange(n)] = rng.uniform(1.0, 2.0, n)
    Q = np.linalg.qr(_crand(rng, n, n))[0]
    lam = np.zeros(n) if zero else eigh_spectrum(n)
    herm = lambda M: 0.5 * (M + M.conj().T)   # noqa: E731
    B = herm(Lm @ Lm.conj().T)
    A = herm(Lm @ (Q * lam) @ Q.conj().T @ Lm.conj().T)
    if zero:
        A = np.zeros_like(A)
    return _frozen(A), _frozen(B), lam


def eigh_batch(golden_npz):
    """[(A, B)] of the batch and its layout with gaps (shared by A, B and the modes)."""
    mats = [pencil(n, zero=(i == EIGH_ZERO))[:2] for i, n in enumerate(EIGH_NS)]
    mats.append((golden_npz["npd_A"], golden_npz["npd_B"]))
    lay = block_layout([A.shape[0] for A, _ in mats], "eigh", "nan")
    bufA, bufB = lay.buf.copy(), lay.buf.copy()
    for b, (A, B) in enumerate(mats):
        view(lay, bufA, b)[...] = A
        view(lay, bufB, b)[...] = B
    return mats, lay, bufA, bufB


# ---- drivers --------------------------------------------------------------------------------------------------------
DRV = dict(F=3, K=6, P=1, L=8, T=14, svnum=((6, 5, 4), (0, 0, 0), (6, 6, 6), (5, 0, 6)), l0=(1, 0, 9, 2),
           regulariser=1e-14, floor_scale=1e-3)
# blocks: a normal one, ndof = 0, l0 >= L (S = 0: the zero shortcut), a frequency without modes


@functools.lru_cache(maxsize=None)
def driver_inputs():
    """Positive semi-definite signal and foreground tables (a_l > 0 times a Gaussian frequency correlation) and a
    positive noise power, so that N is positive definite and the spectra of S against N are positive."""
    F, K, P, L, T = (DRV[k] for k in "FKPLT")
    rng = _rng("driver")
    nblk = len(DRV["svnum"])
    df = np.arange(F)[:, None] - np.arange(F)[None, :]
    sg = rng.uniform(0.5, 2.0, L)[None, None, :] * np.exp(-0.5 * (df / 0.7) ** 2)[:, :, None]
    fg = 30.0 * rng.uniform(0.5, 2.0, L)[None, None, :] * np.exp(-0.5 * (df / 4.0) ** 2)[:, :, None]
    return dict(beam=_frozen(_crand(rng, nblk, F, K, P, L)), ut=_frozen(_crand(rng, nblk, F, K, T)),
                svnum=np.array(DRV["svnum"], dtype=np.int64), l0=np.array(DRV["l0"], dtype=np.int64),
                cl_sg=_frozen(np.ascontiguousarray(sg[None, None])), cl_fg=_frozen(np.ascontiguousarray(fg[None, None])),
                npower=_frozen(rng.uniform(0.5, 2.0, (F, T))))


def safe_cut(spectra, margin=1e-3):
    """A threshold at a gap midpoint that keeps `margin` lambda_max (of its own block) from every eigenvalue of every
    block — three orders above what the solvers resolve, so that searchsorted is not in doubt.  Among those the one that
    leaves the most modes on the smaller side of the cut in every block, then the one with the widest margin."""
    spectra = [np.sort(np.asarray(s, dtype=np.float64)) for s in spectra if len(s)]
    best, cut = None, None
    for ev in spectra:
        for lo, hi in zip(ev[:-1], ev[1:]):
            mid = 0.5 * (lo + hi)
            dist = min(np.min(np.abs(s - mid)) / max(np.abs(s).max(), 1e-300) for s in spectra)
            if dist < margin:
                continue
            key = (min(min(int((s > mid).sum()), int((s < mid).sum())) for s in spectra), dist)
            if best is None or key > best:
                best, cut = key, mid
    assert cut is not None, "no gap keeps the margin"
    return float(cut)
