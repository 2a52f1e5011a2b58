"""Figures of DESIGN.md section 4.21, one step per process so that each runs under a time limit of its own:

    for s in 4x8x128 1x2x512; do for L in 64 1 0; do
        timeout -k 10 300 python scratch/modelcal_measure.py $s $L || break 2
    done; done                                   # -> $MODELCAL_OUT/modelcal_measure.json (default: profiles/)

The class tables of cylinder telescopes of 2 x 64 and 4 x 128 feeds (8128 and 130 816 members), ntime = 1025, nreal x nf =
4 x 8 and 1 x 2 (4.3 GB of visibilities each, 6.4 GB with weights), the shapes of scratch/redcal_measure.py.  The data are
a random model spread over the pairs with gains 5 % and 0.05 rad off one, constant over each solution interval, plus noise
at 1 % of the rms visibility.  Medians of 7 after a warm-up, the device idle around every call.  Per iteration: (time of
24 iterations - time of 8) / 16 with tol = 0, which leaves out the tables and the closing pass; an iteration reads vis and
w twice (each member sits in the lists of two feeds).  To convergence: the defaults (damping 0.5, tol 1e-10) with maxiter =
2000.  Interval 0 measures the iteration of `redcal_solve` on the same data instead, for comparison."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from benchlib.common import CFG2
from driftscan_amd import cylinder, device

SHAPES = {"4x8x128": (4, 8, 2, 64, 1025), "1x2x512": (1, 2, 4, 128, 1025)}
name, L = sys.argv[1], int(sys.argv[2])
nreal, nf, ncyl, nfeeds, ntime = SHAPES[name]
ctx = device.get_context()
torch = ctx.torch


def timed(fn):
    ctx.sync(); torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); ctx.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def median(fn, reps=7):
    fn()
    ts = sorted(timed(fn) for _ in range(reps))
    return ts[len(ts) // 2], ts


tel = cylinder.UnpolarisedCylinderTelescope.from_config(dict(CFG2, num_cylinders=ncyl, num_feeds=nfeeds))
off, mem = tel.redundant_pairs()
nfeed, npairs, nmem = int(tel.nfeed), int(tel.npairs), int(mem.shape[0])
Lg = max(L, 1)
nint = -(-ntime // Lg)
torch.manual_seed(1)
gq = 1 + 0.05 * ctx.empty((nreal, nf, nfeed, nint), np.complex128).normal_()
gt = gq[..., torch.arange(ntime, device=gq.device) // Lg].contiguous()
model = ctx.empty((1, nf, npairs, ntime), np.complex128).normal_()
vis = ctx.vis_expand(model.expand(nreal, nf, npairs, ntime).contiguous(), off, mem, g=gt)
vis += 0.01 * torch.empty_like(vis).normal_()
w = 0.5 + torch.rand((nreal, nf, nmem, ntime), dtype=torch.float64, device=vis.device)
rec = dict(nfeed=nfeed, npairs=npairs, members=nmem, interval=L, nint=nint, vis_bytes=vis.numel() * 16, w_bytes=w.numel() * 8)
if L == 0:
    solve = lambda ww, **kw: ctx.redcal_solve(vis, off, mem, w=ww, **kw)
    reads = 3
else:
    out = dict(g=ctx.empty((nreal, nf, nfeed, nint), np.complex128), iters=ctx.empty((nreal, nf, nint), np.int32),
               step=ctx.empty((nreal, nf, nint), np.float64), chi2=ctx.empty((nreal, nf, nint), np.float64),
               gweight=ctx.empty((nreal, nf, nfeed, nint), np.float64))
    solve = lambda ww, **kw: ctx.modelcal_solve(vis, model, off, mem, L, w=ww, out=out, **kw)
    reads = 2
for key, ww in (("weights", w), ("plain", None)):
    few = median(lambda: solve(ww, tol=0.0, maxiter=8))
    many = median(lambda: solve(ww, tol=0.0, maxiter=24))
    per = (many[0] - few[0]) / 16
    nbytes = reads * (rec["vis_bytes"] + (rec["w_bytes"] if ww is not None else 0))
    rec["iteration_" + key] = dict(maxiter8_s=few, maxiter24_s=many, per_iteration_s=per, bytes_read=nbytes,
                                   read_GBps=nbytes / per / 1e9)
if L:
    full = median(lambda: solve(w, maxiter=2000), reps=3)
    iters, step = ctx.to_host(out["iters"]), ctx.to_host(out["step"])
    turn = (out["g"] * gq.conj()).sum(dim=2, keepdim=True)
    gerr = float((out["g"] * (turn.conj() / turn.abs()) - gq).abs().max())
    rec["to_convergence"] = dict(total_s=full, iterations_min=int(iters.min()), iterations_median=int(np.median(iters)),
                                 iterations_max=int(iters.max()), not_converged=int((~(step < 1e-10)).sum()),
                                 intervals=int(iters.size), s_per_frequency=full[0] / (nreal * nf), max_gain_error=gerr)
print(name, L, json.dumps(rec))
path = os.path.join(os.environ.get("MODELCAL_OUT", os.path.join(ROOT, "profiles")), "modelcal_measure.json")
res = json.load(open(path)) if os.path.exists(path) else {}
res["%s, %s" % (name, "redcal iteration" if L == 0 else "interval %d" % L)] = rec
open(path, "w").write(json.dumps(res, indent=1))
