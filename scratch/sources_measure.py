"""Figures of DESIGN.md section 4.14: `skysim.source_alm` at 4096 polarised sources, lmax 512, 64 frequencies (a warm-up,
then the median of 5 wall times, the device idle before and after; the split into tables, phases and products from the
profiling classes of one more call) beside `healpix.sphtrans_sky` of a 64-frequency polarised nside-512 map to the same
lmax, the route it replaces (a warm-up, then 3 calls, 1 if one takes more than 20 s).

    python scratch/sources_measure.py [OUTDIR]

writes OUTDIR/sources_lmax512.json (default: the current directory)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device, healpix, skysim  # noqa: E402

out = {}
OUT = os.path.join(sys.argv[1] if len(sys.argv) > 1 else ".", "sources_lmax512.json")
ctx = device.get_context(workspace_bytes=1 << 30)
lmax, nf, nsrc = 512, 64, 4096
cat = skysim.random_catalogue(nsrc, 1, pol_frac=0.1)
nu = np.linspace(400.0, 800.0, nf)
flux = skysim.source_spectra(cat, nu)
arrs = (cat["theta"], cat["phi"], flux)


def timed(fn, n):
    ts = []
    for _ in range(n):
        ctx.sync()
        t0 = time.perf_counter()
        r = fn()
        ctx.sync()
        ts.append(time.perf_counter() - t0)
        del r
    return ts


call = lambda: skysim.source_alm(arrs, lmax, to_host=False)
timed(call, 1)
ts = timed(call, 5)
out["source_alm"] = dict(nsrc=nsrc, lmax=lmax, nf=nf, npol=4, seconds=ts, median_s=float(np.median(ts)))
print("source_alm", ts, flush=True)
ctx.prof_reset(2)
timed(call, 1)
rep = ctx.prof_report()
ctx.prof_reset(False)
out["source_alm_split_ms"] = {k: dict(ms=v["ms"], launches=v["launches"]) for k, v in rep.items()}
print(rep, flush=True)
a = ctx.to_host(skysim.source_alm(arrs, lmax, m_range=(0, 7), to_host=False))
out["finite"] = bool(np.isfinite(a.view(np.float64)).all())
del a
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)

# the route this replaces: a pixelised map through the ring analysis
nside = 512
mp = np.zeros((nf, 4, 12 * nside * nside))
mp[:, :, ::9973] = 1.0
t0 = time.perf_counter()
r = healpix.sphtrans_sky(mp, lmax)
ctx.sync()
warm = time.perf_counter() - t0
del r
print("sphtrans_sky warm-up", warm, flush=True)
n = 3 if warm < 20.0 else 1
ts = []
for _ in range(n):
    t0 = time.perf_counter()
    r = healpix.sphtrans_sky(mp, lmax)
    ctx.sync()
    ts.append(time.perf_counter() - t0)
    del r
    print("sphtrans_sky", ts[-1], flush=True)
out["sphtrans_sky"] = dict(nside=nside, lmax=lmax, nf=nf, npol=4, map_bytes=int(mp.nbytes), warmup_s=warm, seconds=ts,
                           median_s=float(np.median(ts)))
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
