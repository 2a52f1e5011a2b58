"""Figures of DESIGN.md section 4.15.

    python scratch/gains_measure.py products DIR        # the products of BASELINE configs[1] into DIR (beams only)
    python scratch/gains_measure.py none DIR            # simulate_visibilities(8 realisations) without gains
    python scratch/gains_measure.py all DIR             # ... alternating with a GainModel, the log, and ts_gain_apply alone
    python scratch/gains_measure.py apply -             # ts_gain_apply alone (for a counter run of its own)

`none` uses nothing this feature added, so the same file runs from a checkout of the parent commit (its own package on the
path) for the comparison of gains=None across the two: run the two in turns, several times each.  After one warm-up of
every case, three repeats of the wall time (device idle before and after); with `all` the two cases alternate, then one
more call with gains and the opt-in log (`timestream.sim_log`, which waits for the device at every step).  Then
`ts_gain_apply` alone at (R, nf, nfeed, ntime) = (8, 16, 128, 1025) and (8, 8, 512, 1025) on the pair tables of cylinder
telescopes of 2 x 64 and 4 x 128 feeds, best of 5 wall times, beside a device copy of the same sky and out bytes and the
time the LDS reads of the loop need at the aggregate LDS rate (2 x 16 B per member, realisation, frequency and sample).
The JSON goes to $GAINS_OUT (default: .) as gains_<mode>_<tag>.json, tag = $GAINS_TAG."""
import json
import os
import sys
import time

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib.common import CFG2
from driftscan_amd import cylinder, device, manager, timestream

LDS_BYTES_PER_S = 150e12   # aggregate ds_read_b64 / b128 rate with every CU streaming (MI355X, ~2.4 GHz)

what, d = sys.argv[1], sys.argv[2]
ctx = device.get_context()
torch = ctx.torch
res = {}


def timed(fn):
    ctx.sync(); torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); ctx.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def apply_figures(reps=5):
    out = {}
    for name, (nreal, nf, ncyl, nfeeds, ntime) in (("8x16x128x1025", (8, 16, 2, 64, 1025)), ("8x8x512x1025", (8, 8, 4, 128, 1025))):
        tel = cylinder.UnpolarisedCylinderTelescope.from_config(dict(CFG2, num_cylinders=ncyl, num_feeds=nfeeds))
        off, mem = tel.redundant_pairs()
        nfeed, npairs = int(tel.nfeed), int(tel.npairs)
        g = ctx.empty((nreal, nf, nfeed, ntime), np.complex128).normal_()
        sky = ctx.empty((nreal, nf, npairs, ntime), np.complex128).normal_()
        buf = ctx.empty((nreal, nf, npairs, ntime), np.complex128)
        ctx.ts_gain_apply(g, off, mem, sky, out=buf)
        ta = [timed(lambda: ctx.ts_gain_apply(g, off, mem, sky, out=buf)) for _ in range(reps)]
        tc = [timed(lambda: (buf.copy_(sky), None)[1]) for _ in range(reps)]
        lds = 32.0 * mem.shape[0] * nreal * nf * ntime
        out[name] = dict(nfeed=nfeed, npairs=npairs, members=int(mem.shape[0]), max_class=int(np.diff(off).max()),
                         tile=int(ctx.lib.dm_ts_gain_tile(nfeed)), ts_gain_apply_wall_s=ta, copy_wall_s=tc,
                         copy_bytes=2 * buf.numel() * 16, g_bytes=g.numel() * 16, lds_read_bytes=lds,
                         lds_read_estimate_s=lds / LDS_BYTES_PER_S)
        del g, sky, buf
    return out


if what == "apply":
    res["apply"] = apply_figures()
    print(json.dumps(res))
    sys.exit(0)
conf = dict(config=dict(beamtransfers=True, kltransform=False, psfisher=False, output_directory=d + "/prod", truncate=False),
            telescope=dict(type="UnpolarisedCylinder", **CFG2))
if what == "products":
    os.makedirs(d, exist_ok=True)
    open(d + "/params.yaml", "w").write(yaml.dump(conf))
pm = manager.ProductManager.from_config(d + "/params.yaml")
if what == "products":
    pm.generate()
else:
    bt, tel = pm.beamtransfer, pm.telescope
    kw = dict(skymodels=("signal",), ndays=10, seed=5, sky_seed=2)
    cases = [("none", lambda: timestream.simulate_visibilities(pm, 8, **kw))]
    if what == "all":
        gains = dict(sigma_amp=0.01, sigma_phase=0.01, corr_time=600.0, seed=1)
        cases.append(("gains", lambda: timestream.simulate_visibilities(pm, 8, gains=gains, **kw)))
    for name, fn in cases:   # warm-up
        timed(fn)
    times = {name: [] for name, _ in cases}
    for _ in range(3):
        for name, fn in cases:
            times[name].append(timed(fn))
    res.update(nm=tel.mmax + 1, nfreq=tel.nfreq, nfeed=tel.nfeed, npairs=tel.npairs, ntime=2 * tel.mmax + 1, wall_s=times)
    if what == "all":
        timestream.sim_log = {}
        total = timed(cases[1][1])
        res["gains_split_s"] = dict(timestream.sim_log, total=total)
        timestream.sim_log = None
        res["ratio_gains_over_none"] = [a / b for a, b in zip(times["gains"], times["none"])]
        res["apply"] = apply_figures()
print(json.dumps(res))
name = "gains_%s_%s.json" % (what, os.environ.get("GAINS_TAG", "run"))
open(os.path.join(os.environ.get("GAINS_OUT", "."), name), "w").write(json.dumps(res, indent=1))
