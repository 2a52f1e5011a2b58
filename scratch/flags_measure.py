"""Figures of DESIGN.md section 4.16.

    python scratch/flags_measure.py solve -             # toeplitz_solve at four shapes, the dense route at the first
    python scratch/flags_measure.py products DIR        # products of BASELINE configs[1] (beams only) into DIR, and two
                                                        # simulated timestreams of 640 samples: DIR/ts_w (20 % flagged in
                                                        # bursts of 3, with a `weight` dataset) and DIR/ts_c (complete)
    python scratch/flags_measure.py mmodes DIR NAME     # `_generate_mmodes_device` on DIR/NAME, five repeats

`mmodes` on ts_c uses nothing this feature added, so the same file runs from a checkout of the parent commit (its own
package on the path) on the same files: run the processes in turns.  Method: device idle before and after every timed
call, one warm-up, then repeats (wall seconds; the median is what DESIGN.md quotes).  `solve` times `Context.toeplitz_solve`
(which clones b) and, at (n, batch, nrhs) = (257, 736, 1), the dense route through the kernels the parent commit has:
assemble A (torch indexing), `zpotrf`, two `ztrsm`.  The JSON goes to $FLAGS_OUT (default: .) as
flags_<mode>_<tag>.json, tag = $FLAGS_TAG."""
import json
import os
import sys
import time

import numpy as np
import yaml

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchlib.common import CFG2
from driftscan_amd import device, manager, timestream

what, d = sys.argv[1], sys.argv[2]
ctx = device.get_context()
torch = ctx.torch
res = {}


def timed(fn):
    ctx.sync(); torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); ctx.sync(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    del out
    return dt


def flagged_columns(n, batch, seed):
    """First columns of `batch` systems of order n: 25 % of ceil(2.5 n) samples flagged at random."""
    rng = np.random.default_rng(seed)
    ntime = int(np.ceil(2.5 * n))
    w = (rng.random((batch, ntime)) > 0.25).astype(np.float64)
    wd = ctx.to_device(w).to(torch.complex128)
    W = ctx.mmode_twiddle(ntime, n - 1)
    col = ctx.empty((batch, n), np.complex128)
    ctx.zgemm(wd, W, col, batch, n, ntime, rsA=ntime, csA=1, rsB=n, csB=1, ldc=n)
    return col


def solve_figures(reps=7):
    out = {}
    for n, batch, nrhs in ((257, 736, 1), (257, 128, 8), (1025, 2048, 1), (2049, 1024, 1)):
        col = flagged_columns(n, batch, n + nrhs)
        b = ctx.empty((batch, nrhs, n), np.complex128).normal_()
        x, info = ctx.toeplitz_solve(col, b)
        assert not bool(info.any())
        rec = dict(levinson_wall_s=[timed(lambda: ctx.toeplitz_solve(col, b)) for _ in range(reps)],
                   clone_wall_s=[timed(lambda: b.clone()) for _ in range(reps)],
                   lds_bytes=(2 + nrhs) * n * 16 + 80 * (1 + nrhs), flops=8.0 * (1 + nrhs) * n * n * batch)
        if (n, batch, nrhs) == (257, 736, 1):
            k = torch.arange(n, device=col.device)
            dd = k[:, None] - k[None, :]

            def dense():
                A = torch.where(dd[None] >= 0, col[:, dd.abs()], col[:, dd.abs()].conj()).contiguous()
                y = b.transpose(1, 2).clone(memory_format=torch.contiguous_format)  # (batch, n, nrhs): a copy, solved in place
                info = ctx.zpotrf(A, n, n, stride=n * n, batch=batch)
                ctx.ztrsm(A, y, n, nrhs, n, nrhs, conjtrans=False, strideL=n * n, strideB=n * nrhs, batch=batch)
                ctx.ztrsm(A, y, n, nrhs, n, nrhs, conjtrans=True, strideL=n * n, strideB=n * nrhs, batch=batch)
                return y, info

            y, dinfo = dense()
            assert not dinfo.any()
            rec["dense_wall_s"] = [timed(dense) for _ in range(reps)]
            rec["dense_bytes"] = batch * n * n * 16
            rec["dense_vs_levinson_max_rel_diff"] = float((y[:, :, 0] - x[:, 0]).abs().max() / x.abs().max())
        out["%dx%dx%d" % (n, batch, nrhs)] = rec
        del col, b, x
    return out


if what == "solve":
    res["solve"] = solve_figures()
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
        kw = dict(skymodels=(), maps=(), ndays=10, seed=5, resolution=86400.0 / 640)
        timestream.simulate_ensemble(pm, d + "/ens_w", 1, weights=dict(fraction=0.2, burst=3, seed=5), **kw)
        timestream.simulate_ensemble(pm, d + "/ens_c", 1, **kw)
        os.rename(d + "/ens_w/real_0000", d + "/ts_w")
        os.rename(d + "/ens_c/real_0000", d + "/ts_c")
    else:
        name = sys.argv[3]
        ts = timestream.Timestream(d + "/" + name, pm)
        tag = os.environ.get("FLAGS_TAG", "run")
        times = []
        for i in range(6):   # the first is the warm-up
            ts.output_directory = "%s/out_%s_%s_%d" % (d, name, tag, i)
            times.append(timed(lambda: ts._generate_mmodes_device(4.0)))
        res.update(name=name, nfreq=tel.nfreq, npairs=tel.npairs, mmax=tel.mmax, ntime=ts.ntime, warmup_wall_s=times[0],
                   wall_s=times[1:])
print(json.dumps(res))
name = "flags_%s_%s.json" % (what + ("_" + sys.argv[3] if what == "mmodes" else ""), os.environ.get("FLAGS_TAG", "run"))
open(os.path.join(os.environ.get("FLAGS_OUT", "."), name), "w").write(json.dumps(res, indent=1))
