"""The cases of the formed-beam tests, their long-double reference and the checker.

A case is one launch.  Its groups: sizes 1, 3, 64, 65 and 130 on a (u, v) grid (at most 7 distinct u: the factorised path;
the sizes sit on the 64 members a wave takes of a chunk), one with only u = 0 and one with only u != 0, an irregular one
(every member its own u and v: the direct path) and, in "main", one of 300 members over the 160 rows (two chunks of 256).
Rows are scattered and shared between groups, amplitudes graded over six decades, |tau| up to a few hundred turns, weights
with zeros, negatives and NaN, NaN in vis wherever the sample is not kept, env = 0 and env > 0 in one call.  Its sources:
H = 0, H = 1, 2 H + 1 = nt, windows that wrap through sample 0 from both sides, duplicates, a dropped source (H = -1)
between kept ones, a source whose every sample is flagged, one half a sample off the grid, one within 1e-3 of the zenith
declination, the rest at random.  The kernel takes no horizon decision, so H is free."""
import numpy as np

from driftscan_amd.timestream import formed_beam_host, formedbeam_tables

U = 2.0 ** -53
KPHI = 18.0          # |tau_hat - tau| <= 17.2 u Tmax


def K0(env):
    return 24.0 + 61.0 * env


def K1(env):
    return 6.0 + 61.0 * env


THETA_Z = np.pi / 4 + 0.1
SCALES = (2.1, 6.3, 10.7, 4.4, 8.8)     # 1 / m
ENVS = (0.0, 5.0, 0.7, 0.0, 40.0)

# name: (nf, nt, nsrc, group sizes on the grid, size of the irregular group, size of the two-chunk group)
CASES = {
    "main": (3, 97, 65, (1, 3, 64, 65, 130), 20, 300),
    "single": (2, 16, 1, (3, 5), 9, 0),
    "ragged": (1, 256, 130, (3, 65), 12, 0),
    "five": (5, 31, 7, (1, 64), 10, 0),
}


def make(name, w_none=False, taper_none=False):
    nf, nt, nsrc, sizes, nirr, nbig = CASES[name]
    rng = np.random.default_rng(sum(ord(ch) for ch in name))
    nrow = 160 if name == "main" else 70
    ugrid = np.array([-6.0, -4.0, -2.0, 0.0, 2.0, 4.0, 6.0])
    us, vs, off = [], [], [0]
    for g, n in enumerate(sizes):
        if g == 1:                                     # only u = 0
            uu, vv = np.zeros(n), (np.arange(n) + 1) * 0.31
        elif g == 0:                                   # only u != 0
            uu, vv = np.full(n, 2.0), np.zeros(n)
        else:                                          # the grid, by (v, u)
            j = np.arange(n)
            uu, vv = ugrid[j % 7], (j // 7 - (n // 7) // 3) * 0.31 * (1.0 + 1.0 / (g + 2))
        us.append(uu)
        vs.append(vv)
        off.append(off[-1] + n)
    if nirr:
        us.append(rng.uniform(-20.0, 20.0, nirr))
        vs.append(rng.uniform(-27.0, 27.0, nirr))
        off.append(off[-1] + nirr)
    if nbig:
        j = np.arange(nbig)
        us.append(ugrid[j % 5])
        vs.append((j // 5 - 20) * 0.45)
        off.append(off[-1] + nbig)
    u, v = np.concatenate(us), np.concatenate(vs)
    nmem = u.size
    off = np.asarray(off, dtype=np.int32)
    members = rng.integers(0, nrow, nmem).astype(np.int32)
    members[off[:-1]] = members[0]                     # a row that the groups share
    uvals, iu = np.unique(u, return_inverse=True)
    vvals, iv = np.unique(v, return_inverse=True)
    taper = None if taper_none else rng.uniform(0.5, 3.0, nmem)
    scale, env = np.array(SCALES[:nf]), np.array(ENVS[:nf])
    # the sources
    theta = THETA_Z + rng.uniform(-0.9, 0.6, nsrc)
    k0 = rng.integers(0, nt, nsrc)
    frac = rng.uniform(-0.5, 0.5, nsrc)
    half = rng.integers(0, min(12, (nt - 1) // 2) + 1, nsrc)
    flagged = None
    if nsrc >= 13:
        half[0], half[1] = 0, 1
        half[2] = (nt - 1) // 2 if nt % 2 else nt // 2 - 1
        k0[3], half[3] = 1, min(5, (nt - 1) // 2)      # wraps below sample 0
        k0[4], half[4] = nt - 2, min(5, (nt - 1) // 2)  # wraps past sample nt - 1
        theta[6], k0[6], frac[6], half[6] = theta[5], k0[5], frac[5], half[5]   # duplicates, and one far away in the list
        theta[nsrc - 1], k0[nsrc - 1], frac[nsrc - 1], half[nsrc - 1] = theta[5], k0[5], frac[5], half[5]
        half[7] = -1                                    # dropped, between kept ones
        flagged = 12
        k0[12], half[12] = nt // 2, 1                     # every sample of it is flagged below
        frac[9] = 0.5 - 1e-9                            # half a sample off the grid
        theta[10] = THETA_Z + 5e-4                      # y cancels
        frac[10], half[10] = 0.01, 2
        theta[11], frac[11], half[11] = THETA_Z - 1e-3, 0.0, 0
    elif nsrc == 1:
        half[0] = 3
    turn = ((k0 + frac) / nt) % 1.0
    turn = np.where(turn >= 1.0, 0.0, turn)
    k0 = (np.rint(turn.astype(np.longdouble) * nt).astype(np.int64) % nt).astype(np.int32)
    tabs = formedbeam_tables(THETA_Z, theta)
    amp = 10.0 ** (-6.0 * np.arange(nrow) / max(nrow - 1, 1))
    vis = (rng.standard_normal((nf, nrow, nt)) + 1j * rng.standard_normal((nf, nrow, nt))) * amp[None, :, None]
    w = None
    if not w_none:
        w = rng.uniform(0.5, 2.0, (nf, nrow, nt))
        drop = rng.random((nf, nrow, nt))
        w[drop < 0.2] = 0.0
        w[(drop >= 0.2) & (drop < 0.25)] = -1.0
        w[(drop >= 0.25) & (drop < 0.3)] = np.nan
        if flagged is not None:
            ks = (k0[flagged] + np.arange(-1, 2)) % nt
            w[:, :, ks] = 0.0
            w[0, :, ks[0]] = np.nan
        vis[~(w > 0)] = np.nan                          # a sample that is not kept reaches nothing
    return dict(name=name, nf=nf, nrow=nrow, nt=nt, nsrc=nsrc, group_off=off, members=members, u=u, v=v, uvals=uvals,
                vvals=vvals, iu=np.asarray(iu).reshape(-1).astype(np.int32), iv=np.asarray(iv).reshape(-1).astype(np.int32),
                taper=taper, scale=scale, env=env, k0=k0, half=half.astype(np.int32), turn=turn, sinth=tabs["sinth"],
                yc0=tabs["yc0"], yc1=tabs["yc1"], vis=vis, w=w, flagged=flagged)


def host(c, parts=2, dtype=np.float64, **over):
    a = dict(c, **over)
    return formed_beam_host(a["vis"], a["w"], a["group_off"], a["members"], a["u"], a["v"], a["scale"], a["env"], a["k0"],
                            a["half"], a["turn"], a["sinth"], a["yc0"], a["yc1"], taper=a["taper"], parts=parts, dtype=dtype)


def reference(c, parts=2):
    """`formed_beam_host` in long double: (beam, D, D2), and sum A x_b |V_b| / D (nf, ngroup, nsrc) for the bound: the
    statement on |V| with every baseline at 0."""
    ref = host(c, parts, np.longdouble)
    absv = np.abs(c["vis"]).astype(np.complex128)      # NaN stays NaN: such samples are not kept
    zero = np.zeros_like(c["u"])
    mag = host(c, 1, np.longdouble, vis=absv, u=zero, v=zero)[0][:, :, 0]
    return ref + (mag,)


def bound(c, ref):
    """(nf, ngroup, nsrc) long double: 2^-53 (KPHI 2 pi Tmax + K0 + 2 nterms) sum A x_b |V_b| / D, and nterms (ngroup, nsrc)."""
    off = c["group_off"]
    ngroup = off.shape[0] - 1
    ld = np.longdouble
    nb = np.diff(off)
    nterms = nb[:, None] * np.where(c["half"] >= 0, 2 * c["half"] + 1, 0)[None, :]
    out = np.zeros((c["nf"], ngroup, c["nsrc"]), dtype=ld)
    for f in range(c["nf"]):
        for p in range(ngroup):
            if nb[p] == 0:
                continue
            sl = slice(off[p], off[p + 1])
            tmax = ld(c["scale"][f]) * (np.abs(c["u"][sl]) + np.abs(c["v"][sl])).max()
            out[f, p] = ld(U) * (KPHI * 2 * np.pi * tmax + K0(c["env"][f]) + 2 * nterms[p]) * ref[3][f, p]
    return out, nterms


def check(c, got, ref):
    """Every element of got = (beam, D, D2) (D, D2 may be None) against ref = `reference`: the beam under `bound`, D and D2
    to (nterms + K1) 2^-53 relative, the exact zeros (D = 0) exactly.  Planes of the reference beyond those of `got` are
    ignored.  Returns (complaints, the worst beam error in units of its bound)."""
    bad = []
    bnd, nterms = bound(c, ref)
    gb = np.asarray(got[0])
    rb = ref[0][:, :, : gb.shape[2]]
    if gb.shape != rb.shape:
        return ["beam has shape %s, not %s" % (gb.shape, rb.shape)], np.inf
    err = np.abs(gb.astype(np.longdouble) - rb)
    lim = bnd[:, :, None, :]
    over = ~(err <= lim)
    if over.any():
        i = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err - lim)), err.shape)
        bad.append("beam: %d elements over the bound, first (f, p, part, s) = %s: error %.3g, bound %.3g"
                   % (over.sum(), i, err[i], np.broadcast_to(lim, err.shape)[i]))
    zero = ref[1] == 0
    if np.any(gb[np.broadcast_to(zero[:, :, None, :], gb.shape)] != 0):
        bad.append("beam is not exactly 0 where D = 0")
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.max(np.where(lim > 0, err / np.where(lim > 0, lim, 1), 0))) if err.size else 0.0
    k1 = np.array([K1(e) for e in c["env"]])
    for name, g, r in (("D", got[1], ref[1]), ("D2", got[2], ref[2])):
        if g is None:
            continue
        g = np.asarray(g)
        if g.shape != r.shape:
            bad.append("%s has shape %s, not %s" % (name, g.shape, r.shape))
            continue
        tol = (nterms[None, :, :] + k1[:, None, None]) * np.longdouble(U) * np.abs(r)
        if np.any(~(np.abs(g.astype(np.longdouble) - r) <= tol)):
            bad.append("%s is outside (nterms + K1) 2^-53 relative" % name)
        if np.any(g[zero] != 0):
            bad.append("%s is not exactly 0 where D = 0" % name)
    return bad, worst
