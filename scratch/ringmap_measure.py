"""Figures of DESIGN.md section 4.25: dm_ringmap against a device copy of the bytes it reads and against the route a user
has without it, on the same card — a complex phase table made with torch, the weighted copy of the visibilities,
torch.matmul (batched over the groups of a frequency), the real part (and the imaginary part with parts = 2) and the
division.

    python scratch/ringmap_measure.py [REPS]

Two shapes: 4 frequencies x 16 groups x 511 members x 4096 samples x 1024 elevations (256 feeds per cylinder), and a small
array of 64 members x 256 elevations (4 x 16 groups, 4096 samples); each with and without weights (10 % of the samples
flagged) and with parts 1 and 2.  Medians of HIP events over REPS (default 10) timed calls after 3 warm-up calls; the
kernel and the torch route are measured three times in turn.  flops = 4 parts nf nmem nel nt (the real product the
kernel computes; the torch route computes 8 nf nmem nel nt whatever parts is).  The JSON goes to $RINGMAP_OUT
(default: .) as ringmap_measure.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 10
ctx = device.get_context()
torch = ctx.torch


def median_ms(fn, reps=reps, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def torch_route(x, w, v, taper, scale, sinza, ngroup, nb, parts):
    """map (nf, ngroup, parts, nel, nt) for groups of nb consecutive rows each."""
    nf, nrow, nt = x.shape
    out = torch.empty((nf, ngroup, parts, sinza.shape[0], nt), dtype=torch.float64, device=x.device)
    vg, tg = v.reshape(ngroup, nb), taper.reshape(ngroup, nb)
    for f in range(nf):
        tau = scale[f] * vg[:, None, :] * sinza[None, :, None]                     # (ngroup, nel, nb)
        table = torch.polar(torch.ones_like(tau), -2.0 * np.pi * (tau - torch.round(tau)))
        xw = tg[:, :, None] * (w[f].reshape(ngroup, nb, nt) if w is not None else 1.0)
        xw = xw.expand(ngroup, nb, nt)
        prod = torch.matmul(table, xw * x[f].reshape(ngroup, nb, nt))               # the weighted copy, the complex product
        d = xw.sum(dim=1)[:, None, :]
        out[f, :, 0] = prod.real / d
        if parts == 2:
            out[f, :, 1] = prod.imag / d
    return out


res = dict(reps=reps, cases=[])
for label, nf, ngroup, nb, nt, nel in (("small", 4, 16, 64, 4096, 256), ("large", 4, 16, 511, 4096, 1024)):
    gen = torch.Generator(device="cuda").manual_seed(nb)
    nrow = ngroup * nb
    x = ctx.empty((nf, nrow, nt), np.complex128)
    torch.view_as_real(x).normal_(generator=gen)
    w_all = torch.rand((nf, nrow, nt), dtype=torch.float64, device=x.device, generator=gen).add_(0.5)
    w_all.masked_fill_(torch.rand((nf, nrow, nt), dtype=torch.float32, device=x.device, generator=gen) < 0.1, 0.0)
    dx, dw = torch.empty_like(x), torch.empty_like(w_all)
    off = np.arange(ngroup + 1, dtype=np.int32) * nb
    members = np.arange(nrow, dtype=np.int32)
    v = ctx.to_device(np.tile((np.arange(nb) - nb // 2) * 0.3048, ngroup))
    taper = ctx.to_device(np.tile(np.hanning(nb + 2)[1:-1] + 0.1, ngroup))
    scale = ctx.to_device(np.linspace(400.0, 800.0, nf) / 299.792458)
    sinza = ctx.to_device(np.linspace(-1.0, 1.0, nel))
    for weighted in (False, True):
        w = w_all if weighted else None
        for parts in (1, 2):
            out = (ctx.empty((nf, ngroup, parts, nel, nt), np.float64), ctx.empty((nf, ngroup, nt), np.float64),
                   ctx.empty((nf, ngroup, nt), np.float64))

            def kernel():
                ctx.ringmap(x, off, members, v, scale, sinza, w=w, taper=taper, parts=parts, out=out[0], norm=out[1], norm2=out[2])

            def route():
                return torch_route(x, w, v, taper, scale, sinza, ngroup, nb, parts)

            def copy():
                dx.copy_(x)
                if weighted:
                    dw.copy_(w)

            runs = [(median_ms(kernel), median_ms(route, reps=max(3, reps // 3), warm=1)) for _ in range(3)]
            kernel()
            ref = route()
            ctx.sync()
            agree = float((out[0] - ref).abs().max() / ref.abs().max())
            del ref
            t_copy = median_ms(copy)
            flops = 4.0 * parts * nf * nrow * nel * nt
            t_k = float(np.median([a for a, _ in runs]))
            case = dict(shape=label, nf=nf, ngroup=ngroup, members=nb, nt=nt, nel=nel, weighted=weighted, parts=parts,
                        kernel_ms=[a for a, _ in runs], torch_route_ms=[b for _, b in runs], copy_ms=t_copy, flops=flops,
                        kernel_tflops=flops / t_k * 1e-9, map_against_torch=agree,
                        kernel_over_torch=t_k / float(np.median([b for _, b in runs])), kernel_over_copy=t_k / t_copy)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del out
            torch.cuda.empty_cache()
    del x, w_all, dx, dw
    torch.cuda.empty_cache()
open(os.path.join(os.environ.get("RINGMAP_OUT", "."), "ringmap_measure.json"), "w").write(json.dumps(res, indent=1))
