"""GPU: the band-power estimators element by element — `dm_qestimate`, `dm_psmc_alt`, `dm_psmc_draw` and
`dm_psmc_moments` through their C entry points, on the case tables of tests/band_cases.py against its long-double
references, bounds and exact zeros.  Every output sits in a NaN-filled buffer with guard elements around it: every
element has to be written (or be exactly zero for a block with nothing to do), every guard has to keep its bits, a
second call has to give the same bits, and a block solved alone the bits it has inside its batch."""
import ctypes

import numpy as np
import pytest

import band_cases as bc

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not bc.LD_OK, reason="np.longdouble has no 64-bit mantissa here")]

G = 64      # guard elements in front of and behind every output


@pytest.fixture(scope="module")
def ctx():
    from driftscan_amd._lib import Context

    c = Context(0, workspace_bytes=1 << 30)
    yield c
    c.close()


class Guarded(object):
    """A NaN-filled device buffer of n elements between two guards of G."""

    def __init__(self, ctx, n, dtype):
        self.n = int(n)
        fill = bc.POISON if dtype == np.complex128 else np.nan
        self.start = np.full(self.n + 2 * G, fill, dtype=dtype)
        self.dev = ctx.to_device(self.start)
        self.ptr = ctx.ptr(self.dev[G:])

    def host(self, what):
        """The n elements on the host; the guards are checked."""
        h = self.dev.cpu().numpy()
        assert bc.same_bits(h[:G], self.start[:G]) and bc.same_bits(h[G + self.n:], self.start[G + self.n:]), \
            "guard elements around %s were written" % what
        return h[G: G + self.n]


def _i32(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))


def _i64(a):
    a = np.ascontiguousarray(a, dtype=np.int64)
    return a, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))


class Batch(object):
    """The device copy of a layout, and the argument lists of the two estimators for all of its blocks or for one."""

    def __init__(self, ctx, c, lay):
        self.ctx, self.c, self.lay = ctx, c, lay
        self.F, self.K, self.P, self.L = (int(v) for v in lay.beam.shape[1:])
        for k in ("beam", "cl", "evecs", "evals", "x", "y", "xw"):
            setattr(self, k, ctx.to_device(np.array(getattr(lay, k))))

    def common(self, blocks):
        """(arguments from nblk to evals_off_host, x_off pointer, the host arrays to keep alive)."""
        lay, ctx = self.lay, self.ctx
        b0, nblk = blocks.start, blocks.stop - blocks.start
        sv, svp = _i32(lay.svnum[blocks])
        l0, l0p = _i32(lay.l0[blocks])
        nm, nmp = _i32(lay.nmodes[blocks])
        eo, eop = _i64(lay.evecs_off[blocks])
        vo, vop = _i64(lay.evals_off[blocks])
        xo, xop = _i64(lay.x_off[blocks])
        args = (nblk, self.F, self.K, self.P, self.L, ctx.ptr(self.beam[b0:]), svp, l0p, self.c["nbands"], ctx.ptr(self.cl),
                ctx.ptr(self.evecs), eop, nmp, ctx.ptr(self.evals), vop)
        return args, xop, (sv, l0, nm, eo, vo, xo)

    def qestimate(self, call, blocks=None):
        """(status, q (nblk, nq, R) on the host) of one call of dm_qestimate on a poisoned, guarded output."""
        ctx, c = self.ctx, self.c
        blocks = blocks or slice(0, len(c["blocks"]))
        y, noise, cp, zm = call
        args, xop, keep = self.common(blocks)
        nblk, nq = args[0], c["nbands"] + (1 if noise else 0)
        out = Guarded(ctx, nblk * nq * c["R"], np.float64)
        flags = (1 if noise else 0) | (2 if cp else 0) | (4 if zm else 0)
        rc = ctx.lib.dm_qestimate(ctx.h, *args, c["R"], ctx.ptr(self.x), ctx.ptr(self.y) if y else None, xop, flags, out.ptr)
        ctx.sync()
        return rc, out.host("q").reshape(nblk, nq, c["R"])

    def psmc_alt(self, want_vecs, blocks=None):
        """(status, vecs (nbands, T) or None, fisher (nblk, nbands, nbands)) of one call of dm_psmc_alt."""
        ctx, c = self.ctx, self.c
        blocks = blocks or slice(0, len(c["blocks"]))
        args, xop, keep = self.common(blocks)
        nblk, nb = args[0], c["nbands"]
        T = int((self.lay.nmodes[blocks] * c["R"]).sum())
        fisher = Guarded(ctx, nblk * nb * nb, np.complex128)
        vecs = Guarded(ctx, nb * T, np.complex128) if want_vecs else None
        rc = ctx.lib.dm_psmc_alt(ctx.h, *args, c["R"], ctx.ptr(self.xw), xop, bc.NSAMPLES, vecs.ptr if want_vecs else None,
                                 fisher.ptr)
        ctx.sync()
        return rc, (vecs.host("the band vectors").reshape(nb, T) if want_vecs else None), \
            fisher.host("the Fisher matrices").reshape(nblk, nb, nb)


def _run_case(ctx, c):
    """Every call of both estimators on one case: (failures, worst q ratio, worst vector ratio, worst Fisher ratio)."""
    bt = Batch(ctx, c, bc.layout(c["name"]))
    nblk, R = len(c["blocks"]), c["R"]
    fails, wq, wv, wf = [], 0.0, 0.0, 0.0
    for call in bc.QCALLS:
        rc, q = bt.qestimate(call)
        assert rc == 0, (c["name"], call, rc)
        f, r = bc.check_q(c, call, q)
        fails += f
        wq = max(wq, r)
        rc, again = bt.qestimate(call)
        if rc != 0 or not bc.same_bits(q, again):
            fails.append("%s %s: a second call gives other bits" % (c["name"], call))
        for b in range(nblk if nblk > 1 else 0):
            rc, solo = bt.qestimate(call, slice(b, b + 1))
            if rc != 0 or not bc.same_bits(solo[0], q[b]):
                fails.append("%s %s: block %d alone gives other bits than in its batch" % (c["name"], call, b))
    voff = bc.v_offsets(c)[0]
    for want in (True, False):
        rc, vecs, fisher = bt.psmc_alt(want)
        assert rc == 0, (c["name"], want, rc)
        f, rv, rf = bc.check_alt(c, vecs, fisher)
        fails += f
        wv, wf = max(wv, rv), max(wf, rf)
        rc, vecs2, fisher2 = bt.psmc_alt(want)
        if rc != 0 or not bc.same_bits(fisher, fisher2) or (want and not bc.same_bits(vecs, vecs2)):
            fails.append("%s want_vecs=%d: a second call gives other bits" % (c["name"], want))
        if want:
            with_vecs = fisher
            # (a block without modes alone has T = 0: its vector buffer is the two guards and nothing between them)
            for b in range(nblk if nblk > 1 else 0):
                rc, sv, sf = bt.psmc_alt(True, slice(b, b + 1))
                n = int(bt.lay.nmodes[b]) * R
                inside = np.ascontiguousarray(vecs[:, voff[b]: voff[b] + n])
                if rc != 0 or not bc.same_bits(sf[0], fisher[b]) or not bc.same_bits(sv, inside):
                    fails.append("%s: block %d alone gives other bits than in its batch" % (c["name"], b))
        elif not bc.same_bits(fisher, with_vecs):
            fails.append("%s: the Fisher matrices depend on want_vecs" % c["name"])
    return fails, wq, wv, wf


@pytest.mark.parametrize("group", bc.GROUPS)
def test_estimators(ctx, group):
    fails, wq, wv, wf = [], 0.0, 0.0, 0.0
    for c in bc.group_cases(group):
        f, q, v, fi = _run_case(ctx, c)
        fails += f
        wq, wv, wf = max(wq, q), max(wv, v), max(wf, fi)
    print("%s: worst err / (1e-12 max|ref|): q %.4f, band vectors %.4f, Fisher %.4f" % (group, wq, wv, wf))
    assert not fails, "\n".join(fails[:20])


def test_F_257_is_refused_and_nothing_is_written(ctx):
    c = dict(bc.BY_NAME["freqs_F256"], F=bc.REFUSED_F)
    bt = Batch(ctx, c, bc.layout("freqs_F256", F=bc.REFUSED_F))
    assert bt.F == 257
    for call in (bc.QCALLS[0], bc.QCALLS[-1]):
        rc, q = bt.qestimate(call)
        assert rc != 0 and np.isnan(q).all()
    rc, vecs, fisher = bt.psmc_alt(True)
    assert rc != 0 and np.isnan(vecs).all() and np.isnan(fisher).all()


# ---- draws ----------------------------------------------------------------------------------------------------------
def _draw(ctx, c, blocks=None):
    """The result buffer (laid out by bc.draw_layout, guards around it) of one dm_psmc_draw call for all blocks or one."""
    start, xoff, ev, eoff = bc.draw_layout(c)
    blocks = blocks or slice(0, len(c["nmodes"]))
    out = Guarded(ctx, start.size, np.complex128)
    mm, mmp = _i32(c["ms"][blocks])
    nm, nmp = _i32(c["nmodes"][blocks])
    xo, xop = _i64(xoff[blocks])
    vo, vop = _i64(eoff[blocks])
    evd = ctx.to_device(ev)
    rc = ctx.lib.dm_psmc_draw(ctx.h, len(mm), mmp, nmp, ctx.ptr(evd) if c["power"] else None, vop if c["power"] else None,
                              bc.DRAW_SEED, c["stream"], c["kind"], c["power"], c["s0"], c["R"], out.ptr, xop)
    assert rc == 0, (c["name"], rc)
    ctx.sync()
    return out.host("the draws"), xoff


@pytest.mark.parametrize("name", [c["name"] for c in bc.DRAW_CASES])
def test_draws(ctx, name):
    c = bc.DRAW_BY_NAME[name]
    buf, xoff = _draw(ctx, c)
    fails, worst = bc.check_draw(c, buf)
    print("%s: worst err / (1e-14 max|ref|) %.4f" % (name, worst))
    assert not fails, "\n".join(fails)
    assert bc.same_bits(buf, _draw(ctx, c)[0]), "a second call gives other bits"
    for b, n in enumerate(c["nmodes"] if len(c["nmodes"]) > 1 else ()):
        solo, _ = _draw(ctx, c, slice(b, b + 1))
        sl = slice(xoff[b], xoff[b] + n * c["R"])
        assert bc.same_bits(solo[sl], buf[sl]), "block %d alone gives other bits than in its batch" % b
        rest = np.ones(buf.size, dtype=bool)
        rest[sl] = False
        assert np.isnan(solo[rest]).all()


# ---- moments --------------------------------------------------------------------------------------------------------
def _moments(ctx, q):
    nblk, nq, ns = q.shape
    mean, cov = Guarded(ctx, nblk * nq, np.float64), Guarded(ctx, nblk * nq * nq, np.float64)
    qd = ctx.to_device(np.array(q))     # a writable copy: the tables themselves are read-only
    rc = ctx.lib.dm_psmc_moments(ctx.h, nblk, nq, ns, ctx.ptr(qd), mean.ptr, cov.ptr)
    assert rc == 0
    ctx.sync()
    return mean.host("the mean").reshape(nblk, nq), cov.host("the covariance").reshape(nblk, nq, nq)


@pytest.mark.parametrize("shifted", [False, True])
def test_moments(ctx, shifted):
    fails, wm, wc = [], 0.0, 0.0
    for nq in bc.MOMENT_NQ:
        for ns in bc.MOMENT_NS:
            q = bc.moment_data(nq, ns, shifted)
            mean, cov = _moments(ctx, q)
            f, rm, rc = bc.check_moments(q, mean, cov)
            fails += ["nq %d ns %d: %s" % (nq, ns, x) for x in f]
            wm, wc = max(wm, rm), max(wc, rc)
            mean2, cov2 = _moments(ctx, q)
            if not (bc.same_bits(mean, mean2) and bc.same_bits(cov, cov2)):
                fails.append("nq %d ns %d: a second call gives other bits" % (nq, ns))
            for b in range(bc.MOMENT_NBLK):
                m1, c1 = _moments(ctx, np.ascontiguousarray(q[b: b + 1]))
                if not (bc.same_bits(m1[0], mean[b]) and bc.same_bits(c1[0], cov[b])):
                    fails.append("nq %d ns %d: block %d alone gives other bits than in its batch" % (nq, ns, b))
    print("moments shifted=%d: worst err / bound: mean %.4f, covariance %.4f" % (shifted, wm, wc))
    assert not fails, "\n".join(fails[:20])
