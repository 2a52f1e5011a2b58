"""Figures of DESIGN.md section 4.17.

    python scratch/stack_measure.py stack -             # vis_stack / vis_expand alone against a device copy
    python scratch/stack_measure.py one VARIANT         # one variant of the larger table, for a counter run of its own
    python scratch/stack_measure.py products DIR        # the products of BASELINE configs[1] into DIR (beams only)
    python scratch/stack_measure.py none DIR            # simulate_visibilities(8 realisations), stacked: runs on the parent too
    python scratch/stack_measure.py files DIR           # one unstacked realisation written, then stack_baselines with its log

`stack`: the class tables of cylinder telescopes of 2 x 64 and 4 x 128 feeds (8128 and 130 816 members), ntime = 1025,
nreal x nf = 4 x 8 and 1 x 2 (4.3 GB of visibilities each, 6.4 GB with weights); variants with weights and gains, weights
only, neither, and vis_expand with gains; medians of 7 after a warm-up, the device idle around every call, beside a
device-to-device copy of as many bytes as the kernel reads (the copy also writes them).  The JSON goes to $STACK_OUT
(default: .) as stack_<mode>_<tag>.json, tag = $STACK_TAG."""
import json
import os
import sys
import time

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib.common import CFG2
from driftscan_amd import cylinder, device, manager, timestream

what, d = sys.argv[1], sys.argv[2]
ctx = device.get_context()
torch = ctx.torch
res = {}


def timed(fn):
    ctx.sync(); torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); ctx.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def median(fn, reps=7):
    fn()
    ts = sorted(timed(fn) for _ in range(reps))
    return ts[len(ts) // 2], ts


def stack_figures(only=None):
    out = {}
    cases = (("4x8x128x1025", (4, 8, 2, 64, 1025)), ("1x2x512x1025", (1, 2, 4, 128, 1025)))
    for name, (nreal, nf, ncyl, nfeeds, ntime) in cases[1:] if only else cases:
        tel = cylinder.UnpolarisedCylinderTelescope.from_config(dict(CFG2, num_cylinders=ncyl, num_feeds=nfeeds))
        off, mem = tel.redundant_pairs()
        nfeed, npairs, nmem = int(tel.nfeed), int(tel.npairs), int(mem.shape[0])
        vis = ctx.empty((nreal, nf, nmem, ntime), np.complex128).normal_()
        w = torch.rand((nreal, nf, nmem, ntime), dtype=torch.float64, device=vis.device)
        g = ctx.empty((nreal, nf, nfeed, ntime), np.complex128).normal_()
        sky = ctx.empty((nreal, nf, npairs, ntime), np.complex128).normal_()
        o, wo = ctx.empty((nreal, nf, npairs, ntime), np.complex128), ctx.empty((nreal, nf, npairs, ntime), np.float64)
        dstv, dstw = torch.empty_like(vis), torch.empty_like(w)
        variants = dict(weights_gains=lambda: ctx.vis_stack(vis, off, mem, w=w, g=g, out=o, wout=wo),
                        weights=lambda: ctx.vis_stack(vis, off, mem, w=w, out=o, wout=wo),
                        plain=lambda: ctx.vis_stack(vis, off, mem, out=o, wout=wo),
                        gains=lambda: ctx.vis_stack(vis, off, mem, g=g, out=o, wout=wo),
                        expand_gains=lambda: ctx.vis_expand(sky, off, mem, g=g, out=vis),
                        expand_plain=lambda: ctx.vis_expand(sky, off, mem, out=vis))
        rec = dict(nfeed=nfeed, npairs=npairs, members=nmem, max_class=int(np.diff(off).max()),
                   tile=int(ctx.lib.dm_ts_gain_tile(nfeed)), vis_bytes=vis.numel() * 16, w_bytes=w.numel() * 8,
                   g_bytes=g.numel() * 16, out_bytes=o.numel() * 24)
        if only:
            rec[only + "_s"] = median(variants[only], reps=5)
        else:
            copy_vw = median(lambda: (dstv.copy_(vis), dstw.copy_(w), None)[2])
            copy_v = median(lambda: (dstv.copy_(vis), None)[1])
            rec.update(copy_vis_and_w_s=copy_vw, copy_vis_s=copy_v)
            for key in ("plain", "weights", "gains", "weights_gains"):
                rec[key + "_s"] = median(variants[key])
            rec["expand_plain_s"] = median(variants["expand_plain"])
            rec["expand_gains_s"] = median(variants["expand_gains"])
            rec["ratio_to_copy"] = dict(plain=rec["plain_s"][0] / copy_v[0], weights=rec["weights_s"][0] / copy_vw[0],
                                        gains=rec["gains_s"][0] / copy_v[0],
                                        weights_gains=rec["weights_gains_s"][0] / copy_vw[0],
                                        expand_plain=rec["expand_plain_s"][0] / copy_v[0],
                                        expand_gains=rec["expand_gains_s"][0] / copy_v[0])
            rec["read_GBps"] = dict(plain=rec["vis_bytes"] / rec["plain_s"][0] / 1e9,
                                    weights=(rec["vis_bytes"] + rec["w_bytes"]) / rec["weights_s"][0] / 1e9,
                                    weights_gains=(rec["vis_bytes"] + rec["w_bytes"]) / rec["weights_gains_s"][0] / 1e9,
                                    copy=2 * rec["vis_bytes"] / copy_v[0] / 1e9)
        out[name] = rec
        del vis, w, g, sky, o, wo, dstv, dstw
    return out


if what in ("stack", "one"):
    res["stack"] = stack_figures(only=d if what == "one" else None)
else:
    conf = dict(config=dict(beamtransfers=True, kltransform=False, psfisher=False, output_directory=d + "/prod", truncate=False),
                telescope=dict(type="UnpolarisedCylinder", **CFG2))
    if what == "products":
        os.makedirs(d, exist_ok=True)
        open(d + "/params.yaml", "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(d + "/params.yaml")
    tel = pm.telescope
    if what == "products":
        pm.generate()
    elif what == "none":
        kw = dict(skymodels=("signal",), ndays=10, seed=5, sky_seed=2)
        fn = lambda: timestream.simulate_visibilities(pm, 8, **kw)
        res.update(nfreq=tel.nfreq, nfeed=tel.nfeed, npairs=tel.npairs, ntime=2 * tel.mmax + 1,
                   simulate_visibilities_s=median(fn, reps=5))
    elif what == "files":
        kw = dict(skymodels=("signal",), ndays=10, seed=5, sky_seed=2, gains=dict(sigma_amp=0.01, sigma_phase=0.01,
                                                                                 corr_time=600.0, seed=1))
        t0 = time.perf_counter()
        uns = timestream.simulate_ensemble(pm, d + "/uns", 1, unstacked=True, **kw)[0]
        res["simulate_ensemble_unstacked_s"] = time.perf_counter() - t0
        runs = []
        for k in range(5):
            timestream.sim_log = {}
            t0 = time.perf_counter()
            timestream.stack_baselines(pm, uns.directory, d + "/stacked_%d" % k, calibrate="file")
            runs.append(dict(timestream.sim_log, total=time.perf_counter() - t0))
            timestream.sim_log = None
        off, mem = tel.redundant_pairs()
        res.update(nfreq=tel.nfreq, nfeed=tel.nfeed, npairs=tel.npairs, members=int(mem.shape[0]), ntime=2 * tel.mmax + 1,
                   stack_baselines_runs=runs)
print(json.dumps(res))
name = "stack_%s_%s.json" % (what, os.environ.get("STACK_TAG", "run"))
open(os.path.join(os.environ.get("STACK_OUT", "."), name), "w").write(json.dumps(res, indent=1))
