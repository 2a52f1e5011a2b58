"""Figures of DESIGN.md section 4.13.

    python scratch/tsim_measure.py all
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o tsim -- python scratch/tsim_measure.py noise

`all`: the products of BASELINE configs[1] (129 m, 16 frequencies) are generated into a temporary directory; after one
warm-up of every case, three alternating repeats of the wall time (device idle before and after, file writing included
where there are files) of `simulate` (one sky model, ndays = 10), of `simulate_ensemble` for 1 and 8 realisations with the
same arguments and of `simulate_visibilities` for the same two; then one more `simulate_ensemble` of 8 with the opt-in
log (`timestream.sim_log`), which waits for the device at every step.  Then `ts_noise` against a device fill of the same
bytes at (8, 16, npairs, 257) and at one 4 GiB chunk of the configs[2] axes (8, 64, 512, 1025), best of 5 wall times.
`noise`: five `ts_noise` calls and five fills at each of the two shapes only, for the kernel trace.
The JSON goes to $TSIM_OUT (default: .)."""
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib.common import CFG2
from driftscan_amd import device, manager, timestream

what = sys.argv[1] if len(sys.argv) > 1 else "all"
ctx = device.get_context()
torch = ctx.torch
res = {}


def timed(fn):
    ctx.sync(); torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); ctx.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def noise_cases(npairs):
    return (("configs1_8x16x%dx257" % npairs, (8, 16, npairs, 257)), ("chunk_8x64x512x1025", (8, 64, 512, 1025)))


def noise_figures(npairs, reps=5):
    out = {}
    for name, (nreal, nf, npr, ntime) in noise_cases(npairs):
        sigma = ctx.to_device(np.ones((nf, npr)))
        buf = ctx.empty((nreal, nf, npr, ntime), np.complex128)
        fg = np.arange(nf)
        ctx.ts_noise(sigma, fg, ntime, nreal, 1, out=buf)
        buf.zero_()
        tn = [timed(lambda: ctx.ts_noise(sigma, fg, ntime, nreal, 1, out=buf)) for _ in range(reps)]
        tf = [timed(lambda: (buf.zero_(), None)[1]) for _ in range(reps)]
        out[name] = dict(bytes=buf.numel() * 16, ts_noise_wall_s=tn, fill_wall_s=tf)
        del buf, sigma
    return out


if what == "noise":
    res["noise"] = noise_figures(46)
else:
    d = tempfile.mkdtemp(prefix="tsim_")
    try:
        conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=False, output_directory=d + "/prod", truncate=False),
                    telescope=dict(type="UnpolarisedCylinder", **CFG2),
                    kltransform=[dict(type="KLTransform", name="kl", threshold=0.1, use_foregrounds=False)])
        open(d + "/params.yaml", "w").write(yaml.dump(conf))
        pm = manager.ProductManager.from_config(d + "/params.yaml")
        pm.generate()
        bt, tel = pm.beamtransfer, pm.telescope
        bt._dev.clear()
        bt.__dict__.pop("_stack_memo", None)
        kw = dict(skymodels=("signal",), ndays=10, seed=5, sky_seed=2)
        count = [0]

        def fresh():
            count[0] += 1
            return "%s/ts_%03d" % (d, count[0])

        cases = (
            ("simulate", lambda: timestream.simulate(pm, fresh(), **kw)),
            ("ensemble_1", lambda: timestream.simulate_ensemble(pm, fresh(), 1, **kw)),
            ("ensemble_8", lambda: timestream.simulate_ensemble(pm, fresh(), 8, **kw)),
            ("visibilities_1", lambda: timestream.simulate_visibilities(pm, 1, **kw)),
            ("visibilities_8", lambda: timestream.simulate_visibilities(pm, 8, **kw)),
        )
        for name, fn in cases:   # warm-up
            timed(fn)
        times = {name: [] for name, _ in cases}
        for _ in range(3):
            for name, fn in cases:
                times[name].append(timed(fn))
        timestream.sim_log = {}
        total = timed(cases[2][1])
        split = dict(timestream.sim_log, total=total)
        timestream.sim_log = None
        res.update(nm=tel.mmax + 1, nfreq=tel.nfreq, npairs=tel.npairs, ntel=bt.ntel, nsky=bt.nsky, ntime=2 * tel.mmax + 1,
                   wall_s=times, ensemble_8_split_s=split,
                   ratio_ensemble_8_over_simulate=[a / b for a, b in zip(times["ensemble_8"], times["simulate"])],
                   ratio_ensemble_1_over_simulate=[a / b for a, b in zip(times["ensemble_1"], times["simulate"])])
        res["noise"] = noise_figures(int(tel.npairs))
    finally:
        shutil.rmtree(d, ignore_errors=True)
print(json.dumps(res))
name = "tsim_configs1.json" if what == "all" else "tsim_noise_walls.json"
open(os.path.join(os.environ.get("TSIM_OUT", "."), name), "w").write(json.dumps(res, indent=1))
