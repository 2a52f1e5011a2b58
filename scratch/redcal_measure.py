"""Figures of DESIGN.md section 4.18.

    python scratch/redcal_measure.py            # -> $REDCAL_OUT/redcal_measure.json (default: .)

The class tables of cylinder telescopes of 2 x 64 and 4 x 128 feeds (8128 and 130 816 members), ntime = 1025, nreal x nf =
4 x 8 and 1 x 2 (4.3 GB of visibilities each, 6.4 GB with weights), as scratch/stack_measure.py.  The data are a random sky
spread over the pairs with gains 5 % and 0.05 rad off one (independent per sample: every sample is a problem of its own, so
the time correlation of a GainModel would change nothing) plus noise at 1 % of the rms visibility.  Medians of 7 after a
warm-up, the device idle around every call.  Per iteration: (time of 24 iterations - time of 8) / 16 with tol = 0, which
leaves out the tables and the chi^2 pass; beside `vis_stack` with weights and gains and a device copy of vis and w.  To
convergence: the defaults (damping 0.4, tol 1e-10) with maxiter = 2000."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib.common import CFG2
from driftscan_amd import cylinder, device

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


res = {}
for name, (nreal, nf, ncyl, nfeeds, ntime) in (("4x8x128x1025", (4, 8, 2, 64, 1025)), ("1x2x512x1025", (1, 2, 4, 128, 1025))):
    tel = cylinder.UnpolarisedCylinderTelescope.from_config(dict(CFG2, num_cylinders=ncyl, num_feeds=nfeeds))
    off, mem = tel.redundant_pairs()
    nfeed, npairs, nmem = int(tel.nfeed), int(tel.npairs), int(mem.shape[0])
    torch.manual_seed(1)
    gt = 1 + 0.05 * ctx.empty((nreal, nf, nfeed, ntime), np.complex128).normal_()
    sky = ctx.empty((nreal, nf, npairs, ntime), np.complex128).normal_()
    vis = ctx.vis_expand(sky, off, mem, g=gt)
    vis += 0.01 * torch.empty_like(vis).normal_()
    w = 0.5 + torch.rand((nreal, nf, nmem, ntime), dtype=torch.float64, device=vis.device)
    out = dict(g=ctx.empty((nreal, nf, nfeed, ntime), np.complex128), y=ctx.empty((nreal, nf, npairs, ntime), np.complex128),
               iters=ctx.empty((nreal, nf, ntime), np.int32), step=ctx.empty((nreal, nf, ntime), np.float64),
               chi2=ctx.empty((nreal, nf, ntime), np.float64))
    o, wo = ctx.empty((nreal, nf, npairs, ntime), np.complex128), ctx.empty((nreal, nf, npairs, ntime), np.float64)
    dstv, dstw = torch.empty_like(vis), torch.empty_like(w)
    rec = dict(nfeed=nfeed, npairs=npairs, members=nmem, max_class=int(np.diff(off).max()),
               tile=int(ctx.lib.dm_ts_gain_tile(nfeed)), vis_bytes=vis.numel() * 16, w_bytes=w.numel() * 8)
    rec["copy_vis_and_w_s"] = median(lambda: (dstv.copy_(vis), dstw.copy_(w), None)[2])
    del dstv, dstw
    rec["vis_stack_weights_gains_s"] = median(lambda: ctx.vis_stack(vis, off, mem, w=w, g=gt, out=o, wout=wo))
    for key, ww in (("weights", w), ("plain", None)):
        few = median(lambda: ctx.redcal_solve(vis, off, mem, w=ww, tol=0.0, maxiter=8, out=out))
        many = median(lambda: ctx.redcal_solve(vis, off, mem, w=ww, tol=0.0, maxiter=24, out=out))
        per = (many[0] - few[0]) / 16
        nbytes = 3 * (rec["vis_bytes"] + (rec["w_bytes"] if ww is not None else 0))
        rec["iteration_" + key] = dict(maxiter8_s=few, maxiter24_s=many, per_iteration_s=per, bytes_read=nbytes,
                                       read_GBps=nbytes / per / 1e9)
    rec["copy_GBps"] = 2 * (rec["vis_bytes"] + rec["w_bytes"]) / rec["copy_vis_and_w_s"][0] / 1e9
    full = median(lambda: ctx.redcal_solve(vis, off, mem, w=w, maxiter=2000, out=out), reps=3)
    iters, step = ctx.to_host(out["iters"]), ctx.to_host(out["step"])
    gerr = None
    if name.startswith("1x2"):
        from driftscan_amd import timestream

        gfix, _ = timestream.fix_degeneracies(ctx.to_host(out["g"])[0, :1, :, :64], ctx.to_host(out["y"])[0, :1, :, :64], off, mem,
                                              ref=ctx.to_host(gt)[0, :1, :, :64])
        gerr = float(np.abs(gfix - ctx.to_host(gt)[0, :1, :, :64]).max())
    rec["to_convergence"] = dict(total_s=full, iterations_min=int(iters.min()), iterations_median=int(np.median(iters)),
                                 iterations_max=int(iters.max()), not_converged=int((~(step < 1e-10)).sum()),
                                 samples=int(iters.size), s_per_frequency=full[0] / (nreal * nf),
                                 max_gain_error_after_fix_64_samples=gerr)
    res[name] = rec
    print(name, json.dumps(rec))
    del vis, w, gt, sky, out, o, wo
open(os.path.join(os.environ.get("REDCAL_OUT", "."), "redcal_measure.json"), "w").write(json.dumps(res, indent=1))
