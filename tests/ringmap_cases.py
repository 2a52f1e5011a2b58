"""The cases of the ring-map tests, their long-double reference and the checker.

A case is one launch: nf frequencies, several groups of unequal size (group 0 lists scattered rows, and every later
group begins with the first row of group 0, so that row is shared), v of either sign with v = 0 and one spacing per
group (a non-commensurate cylinder), |tau| up to a few hundred turns, row amplitudes graded over six decades, a
non-uniform sinza with both ends, weights with zeros, negatives and NaN, whole samples at D = 0, and NaN in vis wherever
the sample is not kept.  The shapes sit at the edges of the 16 x 16 x 4 MFMA tile and of the 128 x 128 workgroup tile."""
import numpy as np

from driftscan_amd.timestream import ringmap_host

U = 2.0 ** -53

# name: (nf, nt, nel, group sizes)
CASES = {
    "edges": (2, 37, 17, (1, 3, 4, 5, 17)),
    "wide": (1, 130, 33, (67, 5, 17)),
    "one": (3, 1, 1, (1, 4)),
    "fifteen": (1, 15, 15, (3, 67)),
    "sixteen": (2, 17, 16, (4, 5, 1)),
    "blocks": (1, 130, 129, (5, 17)),   # two elevation blocks and two sample blocks of a workgroup
}
SCALES = (2.1, 6.3, 10.7)   # 1 / m: with |v| up to 27 m, |tau| up to 290 turns


def make(name, w_none=False, taper_none=False):
    nf, nt, nel, sizes = CASES[name]
    rng = np.random.default_rng(sum(ord(ch) for ch in name))
    nmem = int(sum(sizes))
    nrow = nmem + 3
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    members = rng.permutation(nrow)[:nmem].astype(np.int32)   # scattered rows, some rows unused
    for g in range(1, len(sizes)):
        members[off[g]] = members[0]                           # a row that the groups share
    v = np.concatenate([(np.arange(n) - n // 3) * 0.31 * (1.0 + 1.0 / (g + 2)) for g, n in enumerate(sizes)])
    taper = None if taper_none else rng.uniform(0.5, 3.0, nmem)
    scale = np.array(SCALES[:nf])
    sinza = np.sort(rng.uniform(-1.0, 1.0, nel))
    if nel >= 2:
        sinza[0], sinza[-1] = -1.0, 1.0
    amp = 10.0 ** (-6.0 * np.arange(nrow) / max(nrow - 1, 1))
    vis = (rng.standard_normal((nf, nrow, nt)) + 1j * rng.standard_normal((nf, nrow, nt))) * amp[None, :, None]
    w = None
    if not w_none:
        w = rng.uniform(0.5, 2.0, (nf, nrow, nt))
        drop = rng.random((nf, nrow, nt))
        w[drop < 0.2] = 0.0
        w[(drop >= 0.2) & (drop < 0.25)] = -1.0
        w[(drop >= 0.25) & (drop < 0.3)] = np.nan
        if nt > 1:
            w[:, :, [0, nt // 2]] = 0.0     # whole samples with nothing kept: D = 0
            w[0, :, 0] = np.nan
        vis[~(w > 0)] = np.nan              # a sample that is not kept reaches nothing
    return dict(name=name, nf=nf, nrow=nrow, nt=nt, nel=nel, group_off=off, members=members, v=v, taper=taper, scale=scale,
                sinza=sinza, vis=vis, w=w)


def reference(c, parts=2):
    """`ringmap_host` in long double: (map, D, D2)."""
    return ringmap_host(c["vis"], c["w"], c["group_off"], c["members"], c["v"], c["scale"], c["sinza"], taper=c["taper"],
                        parts=parts, dtype=np.longdouble)


def bound(c):
    """(nf, ngroup, nt) long double: 2^-53 (6 pi max|tau| + 8 + 2 nb_g) sum_b x_b |V_b| / D, 0 where D = 0; and nb_g."""
    off, mem = c["group_off"], c["members"]
    ngroup = off.shape[0] - 1
    ld = np.longdouble
    out = np.zeros((c["nf"], ngroup, c["nt"]), dtype=ld)
    smax = np.abs(c["sinza"]).max()
    for f in range(c["nf"]):
        for g in range(ngroup):
            sl = slice(off[g], off[g + 1])
            rows = mem[sl]
            nb = rows.size
            if nb == 0:
                continue
            T = np.ones(nb, dtype=ld) if c["taper"] is None else c["taper"][sl].astype(ld)
            kept = np.ones((nb, c["nt"]), dtype=bool) if c["w"] is None else c["w"][f, rows] > 0
            wg = np.ones((nb, c["nt"]), dtype=ld) if c["w"] is None else np.where(kept, c["w"][f, rows], 0.0).astype(ld)
            x = T[:, None] * wg
            absv = np.where(kept, np.abs(np.where(kept, c["vis"][f, rows], 0.0)), 0.0).astype(ld)
            d = x.sum(axis=0)
            taumax = ld(c["scale"][f]) * np.abs(c["v"][sl]).max() * smax
            fac = ld(U) * (6 * np.pi * taumax + 8 + 2 * nb)
            out[f, g] = np.where(d != 0, fac * (x * absv).sum(axis=0) / np.where(d != 0, d, 1), 0)
    return out, np.diff(off)


def check(c, got, ref):
    """Every element of got = (map, D, D2) (D, D2 may be None) against ref = (map, D, D2) in long double: the map under
    `bound`, D and D2 to (nb_g + 2) 2^-53 relative, the exact zeros (D = 0) exactly.  Planes of the reference beyond
    those of `got` are ignored.  Returns (complaints, the worst map error in units of its bound)."""
    bad = []
    bnd, nb = bound(c)
    gm = np.asarray(got[0])
    rm = ref[0][:, :, : gm.shape[2]]
    if gm.shape != rm.shape:
        return ["map has shape %s, not %s" % (gm.shape, rm.shape)], np.inf
    err = np.abs(gm.astype(np.longdouble) - rm)
    lim = bnd[:, :, None, None, :]
    over = ~(err <= lim)
    if over.any():
        i = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err - lim)), err.shape)
        bad.append("map: %d elements over the bound, first (f, g, p, e, t) = %s: error %.3g, bound %.3g"
                   % (over.sum(), i, err[i], np.broadcast_to(lim, err.shape)[i]))
    zero = ref[1] == 0
    if np.any(gm[np.broadcast_to(zero[:, :, None, None, :], gm.shape)] != 0):
        bad.append("map is not exactly 0 where D = 0")
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0))) if err.size else 0.0
    for name, g, r in (("D", got[1], ref[1]), ("D2", got[2], ref[2])):
        if g is None:
            continue
        g = np.asarray(g)
        if g.shape != r.shape:
            bad.append("%s has shape %s, not %s" % (name, g.shape, r.shape))
            continue
        tol = (nb[None, :, None] + 2) * np.longdouble(U) * np.abs(r)
        if np.any(~(np.abs(g.astype(np.longdouble) - r) <= tol)):
            bad.append("%s is outside (nb + 2) 2^-53 relative" % name)
        if np.any(g[zero] != 0):
            bad.append("%s is not exactly 0 where D = 0" % name)
    return bad, worst
