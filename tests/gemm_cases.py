"""Case table, long-double reference and derived error bound for the grouped GEMM (driftscan_amd/csrc/dm_gemm.hip).

Nothing here needs a GPU.  `CASES` lists the problems, `materialise` lays one out in poisoned host buffers,
`reference` forms the product in np.longdouble (or, for the host checks, as numpy would) together with the
per-element bound, `check` compares a result buffer with it, and `run` is the glue that sends cases through
`Context.zgemm_grouped_ex`.

Bound (derived, nothing measured), for the real and the imaginary part of every element separately:

    |got - ref| <= (2K + 8) 2^-53 ( hypot(alpha, alpha_im) (|A| diag|s| |B|)_ij + |beta| |C0_ij| )

with (K + 4) in place of (2K + 8) for the all-real class: each part of an output is a sum of at most 2K fma-rounded
products (K for real data) taken in some order, so its error is at most 2K u times the sum of the moduli of the terms,
which |A| |s| |B| bounds (|ar br| + |ai bi| <= |a| |b|); the scaling by s, by alpha and the beta C0 term add a constant
number of roundings.

Poisoning: every view is smaller than its buffer; A, B and kscale are NaN outside their views; C holds a sentinel
outside its view (and between its columns for csc > 1) that must come back bit for bit; with beta = 0 the view of C
starts as NaN and must come back finite; elements outside the tile set of a triangular product keep their bits.
"""
import zlib

import numpy as np

from driftscan_amd._lib import (ZGEMM_ALL_REAL, ZGEMM_B_GATHER, ZGEMM_B_REAL, ZGEMM_CONJ_A, ZGEMM_CONJ_B, ZGEMM_LOWER,
                                ZGEMM_UPPER, ZGEMM_UPPER128)

U = 2.0 ** -53
LD = np.longdouble
LD_OK = np.finfo(np.longdouble).eps < 2e-19   # 64-bit mantissa; the tests skip where long double is only a double
CLASS_FLAG = dict(complex=0, real_b=ZGEMM_B_REAL, all_real=ZGEMM_ALL_REAL, gathered=ZGEMM_B_GATHER)
MUTANTS = ("lastk", "conj", "alpha_im", "kscale", "block", "gather")
PAD = 3


def case(name, cls, M, N, K, groups, a_kfast=True, b_kfast=True, conjA=False, conjB=False, alpha=1.0, alpha_im=0.0,
         beta=0.0, csc=1, kscale=False, tri=0, gather=None, nb=1, solo=True):
    """One row of the table.  gather = dict(cols, wcols, rs1): run of B and weight run of every column, and whether
    the runs are contiguous (rsB = 1).  `inert` names the mutants that cannot change this case's result; the host
    test checks both directions (an inert mutant reproduces the product exactly, every other one leaves the bound)."""
    c = dict(name=name, cls=cls, M=M, N=N, K=K, groups=tuple(groups), a_kfast=a_kfast, b_kfast=b_kfast, conjA=conjA,
             conjB=conjB, alpha=alpha, alpha_im=alpha_im, beta=beta, csc=csc, kscale=kscale or cls == "gathered",
             tri=tri, gather=gather, nb=nb, solo=solo)
    assert (cls == "gathered") == (gather is not None)
    empty = M == 0 or N == 0
    inert = set()
    if empty or K == 0:
        inert |= {"lastk", "conj", "alpha_im", "kscale", "gather"}
    if not (conjA or conjB):
        inert.add("conj")
    if alpha_im == 0.0:
        inert.add("alpha_im")
    if not c["kscale"]:
        inert.add("kscale")
    if cls != "gathered" or N < 2:
        inert.add("gather")
    if empty or (K == 0 and beta == 1.0):   # C = 1 * C0 exactly: a block left alone cannot show
        inert.add("block")
    c["inert"] = frozenset(inert)
    return c


def _build_cases():
    out = []
    E = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 96, 97, 127, 128, 129]
    NW = [159, 160, 255, 256, 257, 513]
    KS = [0, 1, 3, 4, 5, 15, 16, 17, 64, 129]
    TRI = {"lower": ZGEMM_LOWER, "upper": ZGEMM_UPPER, "upper128": ZGEMM_UPPER | ZGEMM_UPPER128}

    # ---- complex class: M and N edges against the K list, layouts, conj flags and beta rotating -----------------
    for i, m in enumerate(E):
        n, k = E[(7 * i + 3) % len(E)], KS[i % len(KS)]
        out.append(case("c_edge_%dx%dx%d" % (m, n, k), "complex", m, n, k, ["complex"], a_kfast=i % 2 == 0,
                        b_kfast=i % 3 == 0, conjA=i % 4 == 1, conjB=i % 4 == 2, beta=[0.0, 1.0, -2.0][i % 3]))
    for i, n in enumerate(NW):
        m, k = [33, 64, 17, 96, 65, 32][i], KS[(i + 3) % len(KS)]
        out.append(case("c_wide_%dx%dx%d" % (m, n, k), "complex", m, n, k, ["complex"], a_kfast=i % 2 == 1,
                        b_kfast=i % 2 == 0, conjB=i % 3 == 0, beta=[0.0, 1.0][i % 2]))
    out += [
        case("c_k0_beta0", "complex", 33, 17, 0, ["complex"]),
        case("c_k0_beta1", "complex", 64, 64, 0, ["complex"], beta=1.0),
        case("c_k0_beta-2", "complex", 17, 65, 0, ["complex"], beta=-2.0, alpha_im=0.5),
        case("c_aim_only", "complex", 64, 64, 16, ["complex"], alpha=0.0, alpha_im=1.5),
        case("c_aim_both_csc3", "complex", 64, 64, 16, ["complex"], alpha=0.7, alpha_im=-1.3, beta=1.0, csc=3),
        case("c_aim_ragged_csc3", "complex", 33, 65, 17, ["complex"], alpha=-1.0, alpha_im=0.5, beta=-2.0, csc=3),
        case("c_flat_int_rmw", "complex", 32, 128, 5, ["complex"], beta=-2.0),
        case("c_flat_int_ow", "complex", 32, 128, 64, ["complex"]),
        case("c_csc3_cc", "complex", 97, 130, 129, ["complex"], conjA=True, conjB=True, csc=3),
        case("c_ks_interior", "complex", 64, 64, 16, ["complex"], kscale=True),
        case("c_ks_interior_rmw", "complex", 128, 128, 64, ["complex"], kscale=True, beta=1.0, b_kfast=False),
        case("c_ks_ragged", "complex", 50, 40, 129, ["complex"], kscale=True, conjB=True, a_kfast=False),
    ]
    for i, (ca, cb) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        for j, (ak, bk) in enumerate([(True, True), (False, False), (True, False), (False, True)]):
            out.append(case("c_lay_%d%d_%d%d" % (ca, cb, ak, bk), "complex", 65, 33, 17, ["complex"], a_kfast=ak,
                            b_kfast=bk, conjA=ca, conjB=cb, beta=float(j % 2)))
    # ---- triangular tile flags (complex class only) ------------------------------------------------------------
    for i, n in enumerate([64, 65, 129, 200]):
        out.append(case("c_lower_%d" % n, "complex", n, n, [5, 16, 17, 64][i], ["complex"], tri=TRI["lower"],
                        beta=float(i % 2), conjB=True, b_kfast=i % 2 == 0))
    for key in ("upper", "upper128"):
        for i, n in enumerate([65, 129, 193, 257]):
            out.append(case("c_%s_%d" % (key, n), "complex", n, n, [17, 4, 16, 15][i], ["complex"], tri=TRI[key],
                            beta=float((i + 1) % 2), conjA=i % 2 == 1, a_kfast=i % 2 == 0))
    # ---- deep class: every complex problem of the launch has K >= 512 (also run in the mixed-K launch) ----------
    for i, k in enumerate([512, 516, 520, 513, 518, 523]):
        out.append(case("d_int_%d" % k, "complex", 64, [64, 128][i % 2], k, ["deep", "complex"], beta=float(i % 2),
                        a_kfast=i % 2 == 0, b_kfast=i % 3 != 0, conjA=i == 4))
        out.append(case("d_rag_%d" % k, "complex", 97, 130, k, ["deep", "complex"], beta=float((i + 1) % 2),
                        a_kfast=i % 2 == 1, b_kfast=i % 3 == 0, conjB=i == 1))
    out += [
        case("d_flat_int_512", "complex", 32, 128, 512, ["deep"]),
        case("d_flat_int_516_rmw", "complex", 32, 128, 516, ["deep"], beta=1.0),
        case("d_flat_rag_523", "complex", 17, 33, 523, ["deep"], beta=-2.0, alpha_im=0.25),
        case("d_flat_rag_520", "complex", 65, 100, 520, ["deep"]),
    ]
    # ---- real B: a launch where narrow problems dominate and one where wide ones do ---------------------------
    for i, m in enumerate(E):
        n, k = E[(4 * i + 6) % len(E)], KS[(i + 4) % len(KS)]
        out.append(case("r_edge_%dx%dx%d" % (m, n, k), "real_b", m, n, k, ["real_narrow"], a_kfast=i % 2 == 1,
                        b_kfast=i % 3 == 1, conjA=i % 4 == 0, beta=[0.0, 1.0, -2.0][(i + 1) % 3]))
    out += [
        case("r_int_ow", "real_b", 64, 64, 16, ["real_narrow"]),
        case("r_int_rmw_aim", "real_b", 128, 64, 17, ["real_narrow"], beta=1.0, alpha=0.5, alpha_im=2.0),
        case("r_flat_int_ow", "real_b", 32, 128, 16, ["real_narrow"]),
        case("r_flat_int_rmw", "real_b", 32, 128, 5, ["real_narrow"], beta=1.0, csc=3),
        case("r_ks", "real_b", 64, 64, 64, ["real_narrow"], kscale=True),
        case("r_nw_16x160", "real_b", 16, 160, 4, ["real_narrow"]),
        case("r_nw_33x257", "real_b", 33, 257, 5, ["real_narrow"], beta=1.0, b_kfast=False),
        case("r_nw_17x513", "real_b", 17, 513, 16, ["real_narrow"], a_kfast=False),
        case("r_w_64x256", "real_b", 64, 256, 64, ["real_wide"]),
        case("r_w_128x128_rmw", "real_b", 128, 128, 16, ["real_wide"], beta=1.0),
        case("r_w_65x257", "real_b", 65, 257, 17, ["real_wide"], beta=-2.0, conjA=True, b_kfast=False),
        case("r_w_32x160", "real_b", 32, 160, 16, ["real_wide"], a_kfast=False),
        case("r_w_32x256_flat_ow", "real_b", 32, 256, 15, ["real_wide"]),
        case("r_w_32x256_flat_rmw", "real_b", 32, 256, 4, ["real_wide"], beta=1.0),
        case("r_w_97x513", "real_b", 97, 513, 64, ["real_wide"], alpha_im=-0.5, csc=3),
        case("r_w_128x255", "real_b", 128, 255, 15, ["real_wide"], beta=1.0, kscale=True),
        case("r_w_129x159", "real_b", 129, 159, 129, ["real_wide"]),
        case("r_wn_64x17", "real_b", 64, 17, 16, ["real_wide"], beta=1.0),
        case("r_wn_33x129", "real_b", 33, 129, 5, ["real_wide"]),
        case("r_wn_17x129_flat", "real_b", 17, 129, 3, ["real_wide"], beta=-2.0),
    ]
    # ---- gathered B -------------------------------------------------------------------------------------------
    def gat(n, nruns, nw, rs1, permute=False, seed=0):
        r = np.random.default_rng(seed)
        cols = r.permutation(n) % nruns if permute else np.arange(n) % nruns
        return dict(cols=[int(x) for x in cols], wcols=[int(x) for x in (np.arange(n) * 3 + 1) % nw], rs1=rs1)
    out += [
        case("g_shared", "gathered", 65, 33, 17, ["gathered"], gather=gat(33, 5, 33, False)),
        case("g_permuted", "gathered", 64, 64, 16, ["gathered"], gather=gat(64, 64, 7, False, permute=True, seed=1)),
        case("g_conjb_rmw", "gathered", 97, 130, 129, ["gathered"], conjB=True, beta=1.0,
             gather=gat(130, 40, 130, False, permute=True, seed=2)),
        case("g_rs1", "gathered", 33, 17, 64, ["gathered"], gather=gat(17, 6, 4, True), a_kfast=False),
        case("g_rs1_rmw", "gathered", 128, 128, 5, ["gathered"], beta=-2.0, conjA=True, gather=gat(128, 9, 11, True)),
        case("g_1x1x1", "gathered", 1, 1, 1, ["gathered"], gather=gat(1, 1, 1, True)),
        case("g_129x257", "gathered", 129, 257, 5, ["gathered"], gather=gat(257, 31, 257, False, permute=True, seed=3),
             alpha_im=0.75, csc=3),
        case("g_k0", "gathered", 17, 31, 0, ["gathered"], beta=1.0, gather=gat(31, 3, 2, True)),
        case("g_flat", "gathered", 17, 100, 15, ["gathered"], gather=gat(100, 100, 100, False, permute=True, seed=4)),
        case("g_flat_rmw", "gathered", 96, 63, 4, ["gathered"], beta=1.0, gather=gat(63, 2, 63, True)),
    ]
    # ---- all real -----------------------------------------------------------------------------------------------
    for i, m in enumerate(E):
        n, k = E[(11 * i + 5) % len(E)], KS[(i + 7) % len(KS)]
        out.append(case("a_edge_%dx%dx%d" % (m, n, k), "all_real", m, n, k, ["all_real"], a_kfast=i % 2 == 0,
                        b_kfast=i % 2 == 1 if i % 4 < 2 else i % 2 == 0, beta=float(i % 2)))
    out += [
        case("a_int_ow", "all_real", 64, 128, 16, ["all_real"], b_kfast=False),
        case("a_int_rmw", "all_real", 128, 64, 64, ["all_real"], beta=1.0, a_kfast=False),
        case("a_17x257", "all_real", 17, 257, 16, ["all_real"], alpha=-0.5),
        case("a_64x513", "all_real", 64, 513, 4, ["all_real"], beta=1.0, b_kfast=False),
    ]
    # ---- one launch with all four classes, empty problems in between, K rising so that the sort reorders ------
    out += [
        case("m_c5", "complex", 70, 40, 5, ["mixed"], beta=1.0),
        case("m_empty_m", "complex", 0, 40, 5, ["mixed"]),
        case("m_r17", "real_b", 33, 65, 17, ["mixed"]),
        case("m_empty_n", "real_b", 33, 0, 17, ["mixed"]),
        case("m_a16", "all_real", 65, 66, 16, ["mixed"]),
        case("m_g3", "gathered", 40, 70, 3, ["mixed"], gather=gat(70, 8, 9, False)),
        case("m_empty_a", "all_real", 0, 0, 4, ["mixed"]),
        case("m_c129", "complex", 130, 65, 129, ["mixed"], conjA=True),
        case("m_r64", "real_b", 64, 200, 64, ["mixed"], beta=1.0),
        case("m_empty_g", "gathered", 0, 5, 4, ["mixed"], gather=gat(5, 2, 2, False)),
        case("m_g64", "gathered", 65, 33, 64, ["mixed"], beta=1.0, gather=gat(33, 33, 33, True)),
        case("m_a70", "all_real", 129, 17, 70, ["mixed"], beta=1.0),
    ]
    # ---- chunked tile remap: more tiles than one round of chunks (8 x 256 complex, 8 x 64 for the others) ------
    out += [
        case("x_complex", "complex", 8, 8, 4, ["chunk"], nb=2050, solo=False, conjB=True),
        case("x_real", "real_b", 8, 8, 4, ["chunk"], nb=520, solo=False, beta=1.0),
        case("x_allreal", "all_real", 8, 8, 4, ["chunk"], nb=520, solo=False),
        case("x_gathered", "gathered", 8, 8, 4, ["chunk"], nb=520, solo=False, gather=gat(8, 3, 8, False)),
    ]
    names = [c["name"] for c in out]
    assert len(set(names)) == len(names)
    return out


CASES = _build_cases()
# three dependent products for one call: launch 1 reads the C of launch 0 as its A, launch 2 that of launch 1
CHAIN = [case("chain_0", "complex", 65, 33, 17, [], conjB=True),
         case("chain_1", "complex", 65, 70, 33, [], b_kfast=False, alpha_im=0.5),
         case("chain_2", "complex", 65, 20, 70, [], beta=1.0, alpha=-1.0)]


def refused_problems():
    """(label, problem without tensors) for every flag combination the planner refuses."""
    base = dict(M=8, N=8, K=4, rsA=4, csA=1, rsB=8, csB=1, ldc=8)
    g = np.zeros((8, 2), dtype=np.int32)
    AR, BR, BG = ZGEMM_ALL_REAL, ZGEMM_B_REAL, ZGEMM_B_GATHER
    return [
        ("all_real+kscale", dict(base, flags=AR, has_kscale=True)),
        ("all_real+csc", dict(base, flags=AR, csc=2, ldc=16)),
        ("all_real+alpha_im", dict(base, flags=AR, alpha_im=1.0)),
        ("all_real+conjA", dict(base, flags=AR | ZGEMM_CONJ_A)),
        ("all_real+conjB", dict(base, flags=AR | ZGEMM_CONJ_B)),
        ("all_real+b_real", dict(base, flags=AR | BR)),
        ("all_real+b_gather", dict(base, flags=AR | BG, has_kscale=True, bgather=g)),
        ("b_real+b_gather", dict(base, flags=BR | BG, has_kscale=True, bgather=g)),
        ("b_gather-no-bgather", dict(base, flags=BG, has_kscale=True)),
        ("b_gather-no-kscale", dict(base, flags=BG, bgather=g)),
        ("b_real+lower", dict(base, flags=BR | ZGEMM_LOWER)),
    ]
BY_NAME = {c["name"]: c for c in CASES}
GROUPS = ("complex", "deep", "real_narrow", "real_wide", "gathered", "all_real", "mixed", "chunk")


def group_cases(group):
    return [c for c in CASES if group in c["groups"]]


def flags_of(c):
    return (CLASS_FLAG[c["cls"]] | (ZGEMM_CONJ_A if c["conjA"] else 0) | (ZGEMM_CONJ_B if c["conjB"] else 0) | c["tri"])


class Data(object):
    """Host buffers of one case and integer index arrays of its views (batch first): A_buf[iA] is (nb, M, K),
    B_buf[iB] is (nb, K, N) (through the gather where there is one), ks_buf[iks] is (nb, K) or, gathered, (nb, K, N)."""


def materialise(c, A_values=None):
    rng = np.random.default_rng(zlib.crc32(c["name"].encode()))
    M, N, K, nb, cls = c["M"], c["N"], c["K"], c["nb"], c["cls"]
    d = Data()
    d.case = c
    cplx = cls != "all_real"
    bb = np.arange(nb)[:, None, None]

    def rnd(shape, is_c):
        v = rng.standard_normal(shape)
        return v + 1j * rng.standard_normal(shape) if is_c else v

    def buf(n, is_c):
        return np.full(n, complex(np.nan, np.nan) if is_c else np.nan, dtype=np.complex128 if is_c else np.float64)

    # A: (M x K), rows spread over six decades so that an error in a small row cannot hide behind a large one
    d.rsA, d.csA = (K + PAD, 1) if c["a_kfast"] else (1, M + PAD)
    d.a_off = PAD
    d.a_slab = max(M - 1, 0) * d.rsA + max(K - 1, 0) * d.csA + 1 + PAD
    d.A_buf = buf(d.a_off + nb * d.a_slab, cplx)
    d.iA = d.a_off + bb * d.a_slab + np.arange(M)[None, :, None] * d.rsA + np.arange(K)[None, None, :] * d.csA
    d.row_scale = 10.0 ** rng.uniform(-3, 3, size=(nb, M, 1))
    vals = d.row_scale * rnd((nb, M, K), cplx)   # drawn either way: B and C do not depend on A_values
    d.A_buf[d.iA] = vals if A_values is None else A_values
    # B: (K x N)
    b_c = cls in ("complex", "gathered")
    d.b_off = PAD + 1
    d.bgather = None
    kk, nn = np.arange(K)[None, :, None], np.arange(N)[None, None, :]
    if cls == "gathered":
        g = c["gather"]
        cols, wcols = np.asarray(g["cols"], dtype=np.int64), np.asarray(g["wcols"], dtype=np.int64)
        nruns, nw = int(cols.max()) + 1 if N else 1, int(wcols.max()) + 1 if N else 1
        if g["rs1"]:
            d.rsB, x = 1, np.arange(nruns) * (K + PAD)
        else:
            d.rsB, x = nruns + PAD, np.arange(nruns)
        d.csB = 0
        d.b_slab = int(x.max()) + max(K - 1, 0) * d.rsB + 1 + PAD
        d.B_buf = buf(d.b_off + nb * d.b_slab, True)
        runs = d.b_off + bb * d.b_slab + kk * d.rsB + x[None, None, :]
        d.B_buf[runs] = rnd((nb, K, nruns), True)
        d.iB = runs[:, :, cols] if N else runs[:, :, :0]
        y = np.arange(nw) * (K + PAD)
        d.ks_off = PAD + 2
        d.ks_slab = int(y.max()) + K + PAD
        d.ks_buf = buf(d.ks_off + nb * d.ks_slab, False)
        wruns = d.ks_off + bb * d.ks_slab + kk + y[None, None, :]
        d.ks_buf[wruns] = 10.0 ** rng.uniform(-1, 1, size=(nb, K, nw)) * rng.choice([-1.0, 1.0], size=(nb, K, nw))
        d.iks = wruns[:, :, wcols] if N else wruns[:, :, :0]
        d.bgather = np.stack([x[cols], y[wcols]], axis=1).astype(np.int32) if N else np.zeros((0, 2), np.int32)
    else:
        d.rsB, d.csB = (1, K + PAD) if c["b_kfast"] else (N + PAD, 1)
        d.b_slab = max(K - 1, 0) * d.rsB + max(N - 1, 0) * d.csB + 1 + PAD
        d.B_buf = buf(d.b_off + nb * d.b_slab, b_c)
        d.iB = d.b_off + bb * d.b_slab + kk * d.rsB + nn * d.csB
        d.B_buf[d.iB] = rnd((nb, K, N), b_c)
        d.ks_off, d.ks_slab, d.ks_buf, d.iks = PAD + 2, K + PAD, None, None
        if c["kscale"]:
            d.ks_buf = buf(d.ks_off + nb * d.ks_slab, False)
            d.iks = d.ks_off + np.arange(nb)[:, None] * d.ks_slab + np.arange(K)[None, :]
            d.ks_buf[d.iks] = 10.0 ** rng.uniform(-1, 1, size=(nb, K)) * rng.choice([-1.0, 1.0], size=(nb, K))
    # C: sentinel everywhere, then the view (NaN where beta = 0 says it is not read)
    d.csc = c["csc"]
    d.ldc = N * d.csc + PAD
    d.c_off = PAD + 4
    d.c_slab = M * d.ldc + PAD
    n = d.c_off + nb * d.c_slab
    d.C_buf = (1000.0 + np.arange(n)) - 1j * (np.arange(n) + 0.5) if cplx else 1000.0 + np.arange(n)
    d.C_buf = d.C_buf.astype(np.complex128 if cplx else np.float64)
    d.iC = d.c_off + bb * d.c_slab + np.arange(M)[None, :, None] * d.ldc + nn * d.csc
    d.C_buf[d.iC] = d.row_scale * rnd((nb, M, N), cplx) if c["beta"] != 0.0 else np.nan * (1 + 1j if cplx else 1)
    d.in_view = np.zeros(n, dtype=bool)
    d.in_view[d.iC] = True
    return d


def problems(d, launch=0):
    """The problem dicts of `_lib.zgemm_plan_info` / `Context.zgemm_grouped_ex` (the latter wants the tensors added)."""
    c = d.case
    return [dict(M=c["M"], N=c["N"], K=c["K"], rsA=d.rsA, csA=d.csA, rsB=d.rsB, csB=d.csB, ldc=d.ldc, csc=d.csc,
                 flags=flags_of(c), alpha=c["alpha"], alpha_im=c["alpha_im"], beta=c["beta"], launch=launch,
                 a_off=d.a_off + b * d.a_slab, b_off=d.b_off + b * d.b_slab, c_off=d.c_off + b * d.c_slab,
                 ks_off=d.ks_off + b * d.ks_slab, has_kscale=d.ks_buf is not None, bgather=d.bgather)
            for b in range(c["nb"])]


def tile_set(c):
    """(M, N) mask of the elements a triangular product computes: whole 64 x 64 tiles on or below (LOWER) / on or above
    (UPPER) the block diagonal, with UPPER128 also the tile left of an odd diagonal tile."""
    a, b = np.arange(c["M"])[:, None] // 64, np.arange(c["N"])[None, :] // 64
    m = np.ones((c["M"], c["N"]), dtype=bool)
    if c["tri"] & ZGEMM_LOWER:
        m &= b <= a
    if c["tri"] & ZGEMM_UPPER:
        m &= b >= ((a & ~1) if c["tri"] & ZGEMM_UPPER128 else a)
    return m


def reference(d, dtype=LD, mutant=None, want_bound=True):
    """(re, im, bound) of the expected view of C, each (nb, M, N); im is None for the all-real class.  dtype = LD: four
    real products in long double.  dtype = np.float64: the product as numpy forms it (complex128 matmul), the
    stand-in for a correct kernel in the host tests; `mutant` then plants one of MUTANTS."""
    c = d.case
    K, cls, cplx = c["K"], c["cls"], c["cls"] != "all_real"
    assert mutant is None or mutant in MUTANTS
    A, B, C0 = d.A_buf[d.iA], d.B_buf[d.iB], d.C_buf[d.iC]
    iks = d.iks
    if mutant == "gather" and "gather" not in c["inert"]:
        g = c["gather"]
        n1 = 0
        n2 = next(n for n in range(1, c["N"]) if g["cols"][n] != g["cols"][0])
        perm = np.arange(c["N"])
        perm[[n1, n2]] = [n2, n1]
        B = d.B_buf[d.iB[:, :, perm]]
    ks = d.ks_buf[iks] if iks is not None else None
    if mutant == "lastk" and K > 0:
        A, B = A[:, :, :K - 1], B[:, :K - 1, :]
        ks = ks[:, :K - 1] if ks is not None else None
    ar, ai = (A.real, A.imag) if cplx else (A, np.zeros_like(A))
    br, bi = (B.real, B.imag) if np.iscomplexobj(B) else (B, np.zeros_like(B))
    if mutant != "conj":
        ai = -ai if c["conjA"] else ai
        bi = -bi if c["conjB"] else bi
    absA, absB = np.hypot(ar, ai), np.hypot(br, bi)
    ar, ai, br, bi = (x.astype(dtype) for x in (ar, ai, br, bi))
    if ks is not None:
        absks = np.abs(ks)
        if cls == "gathered":
            absB = absB * absks
        else:
            absA = absA * absks[:, None, :]
        if mutant != "kscale":
            s = ks.astype(dtype)
            if cls == "gathered":
                br, bi = br * s, bi * s
            else:
                ar, ai = ar * s[:, None, :], ai * s[:, None, :]
    if dtype is LD or not cplx:
        pr = np.matmul(ar, br)
        pi = None
        if cplx:
            pr = pr - np.matmul(ai, bi)
            pi = np.matmul(ar, bi) + np.matmul(ai, br)
    else:
        p = np.matmul(ar + 1j * ai, br + 1j * bi)
        pr, pi = p.real, p.imag
    al, aim, beta = dtype(c["alpha"]), dtype(-c["alpha_im"] if mutant == "alpha_im" else c["alpha_im"]), dtype(c["beta"])
    c0r, c0i = (C0.real.astype(dtype), C0.imag.astype(dtype)) if cplx else (C0.astype(dtype), None)
    if cplx:
        re, im = al * pr - aim * pi, al * pi + aim * pr
    else:
        re, im = al * pr, None
    if c["beta"] != 0.0:
        re = re + beta * c0r
        im = im + beta * c0i if cplx else None
    mask = tile_set(c)[None]
    re = np.where(mask, re, c0r)
    im = np.where(mask, im, c0i) if cplx else None
    if mutant == "block":
        re[:, :16, :16] = c0r[:, :16, :16]
        if cplx:
            im[:, :16, :16] = c0i[:, :16, :16]
    bound = None
    if want_bound:
        fac = (2 * K + 8) if cplx else (K + 4)
        bound = np.hypot(c["alpha"], c["alpha_im"]) * np.matmul(absA, absB)
        if c["beta"] != 0.0:
            bound = bound + abs(c["beta"]) * np.abs(C0)
        bound = np.where(mask, fac * U * bound, 0.0)
    return re, im, bound


_CACHE = {}


def save_cache(path, names):
    """The materialised cases and their references for a child process (long double survives pickling)."""
    import pickle

    with open(path, "wb") as f:
        pickle.dump({n: cached(n) for n in names}, f, protocol=4)


def load_cache(path):
    import pickle

    with open(path, "rb") as f:
        _CACHE.update(pickle.load(f))


def cached(name):
    """(Data, (re, im, bound)) of a case, materialised and referenced once per process and never written to."""
    if name not in _CACHE:
        d = materialise(BY_NAME[name])
        _CACHE[name] = (d, reference(d))
    return _CACHE[name]


def outside(d, ref, re, im):
    """Per-element test of a candidate view (re, im as (nb, M, N)) against a reference triple: True where an element
    is outside the bound (NaN counts as outside)."""
    rre, rim, bound = ref
    bad = ~(np.abs(re.astype(LD) - rre) <= bound)
    if rim is not None:
        bad |= ~(np.abs(im.astype(LD) - rim) <= bound)
    return bad


def check(d, ref, C_out):
    """Failures (strings) of a result buffer: sentinel bits outside the view, bound and tile set inside."""
    c = d.case
    fails = []
    w = 2 if c["cls"] != "all_real" else 1
    got_bits = np.ascontiguousarray(C_out).view(np.uint64).reshape(-1, w)
    old_bits = d.C_buf.view(np.uint64).reshape(-1, w)
    if C_out.shape != d.C_buf.shape:
        return ["%s: buffer shape changed" % c["name"]]
    moved = (got_bits != old_bits).any(axis=1) & ~d.in_view
    if moved.any():
        fails.append("%s: %d elements outside the view of C changed, first at %d" % (c["name"], moved.sum(),
                                                                                      int(np.flatnonzero(moved)[0])))
    mask = np.broadcast_to(tile_set(c)[None], d.iC.shape)
    keep = (got_bits[d.iC] != old_bits[d.iC]).any(axis=-1) & ~mask
    if keep.any():
        fails.append("%s: %d elements outside the tile set changed" % (c["name"], keep.sum()))
    V = C_out[d.iC]
    re, im = (V.real, V.imag) if w == 2 else (V, None)
    bad = outside(d, ref, re, im) & mask
    if bad.any():
        b, i, j = (int(x[0]) for x in np.nonzero(bad))
        err = abs(complex(V[b, i, j]) - complex(ref[0][b, i, j], ref[1][b, i, j] if w == 2 else 0.0))
        fails.append("%s: %d of %d elements outside the bound, first (%d, %d, %d): got %r, |err| %.3e, bound %.3e"
                     % (c["name"], bad.sum(), mask.sum(), b, i, j, V[b, i, j], err, float(ref[2][b, i, j])))
    return fails


# ---- device glue ---------------------------------------------------------------------------------------------------
def upload(ctx, d):
    """Fresh device copies of a case's buffers: (A, B, C, kscale)."""
    return (ctx.to_device(d.A_buf), ctx.to_device(d.B_buf), ctx.to_device(d.C_buf),
            ctx.to_device(d.ks_buf) if d.ks_buf is not None else None)


def run(ctx, items):
    """items: (Data, launch id) pairs.  One `zgemm_grouped_ex` call for all of them on fresh device copies; returns
    the result buffers of C on the host, one per item."""
    probs, tens = [], []
    for d, launch in items:
        t = upload(ctx, d)
        tens.append(t)
        for p in problems(d, launch):
            p.update(A=t[0], B=t[1], C=t[2], kscale=t[3])
            probs.append(p)
    ctx.zgemm_grouped_ex(probs)
    ctx.sync()
    return [t[2].cpu().numpy() for t in tens]


def run_and_check(ctx, names, solo):
    """Every named case in a launch of its own (solo) or all in one launch; the list of failures."""
    items = [(cached(n)[0], i if solo else 0) for i, n in enumerate(names)]
    outs = run(ctx, items)
    fails = []
    for n, o in zip(names, outs):
        d, ref = cached(n)
        fails += check(d, ref, o)
    return fails


def child_names():
    return [c["name"] for c in CASES if c["cls"] != "all_real" and "mixed" not in c["groups"]]


def child_main(cache=None):
    """Body of the DM_GEMM4=0 child process: the complex, real-B and gathered cases, each in a launch of its own and
    in its class's launch, and the chunk-remap launch, on the LDS-staged kernels.  Returns the exit status."""
    from driftscan_amd import _lib

    if cache:
        load_cache(cache)
    names = [n for n in child_names() if BY_NAME[n]["solo"]]
    ctx = _lib.Context(0, workspace_bytes=1 << 28)   # first: it imports torch before the library is loaded
    info = _lib.zgemm_plan_info(problems(cached(names[0])[0]))
    if info[0]["use4"]:
        print("the planner still chose the register-only kernels")
        return 2
    fails = run_and_check(ctx, names, solo=True)
    for g in ("complex", "deep", "real_narrow", "real_wide", "gathered", "chunk"):
        fails += run_and_check(ctx, [c["name"] for c in group_cases(g) if c["cls"] != "all_real"], solo=False)
    for f in fails[:40]:
        print(f)
    print("lds fallback: %d cases, %d failures" % (len(names), len(fails)))
    return 1 if fails else 0
