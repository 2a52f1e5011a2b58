"""Figures of DESIGN.md section 4.27: dm_delay_spectrum against a device copy of the bytes it reads and against the route a
user has without it, on the same card — a masked, tapered copy of the data, a complex phase table made with torch,
torch.matmul, abs()^2 and a sum per bin, and the same again for the window.

    python scratch/delayspec_measure.py [REPS]

Three shapes (nf, nd, nrow, nt) = (64, 64, 96, 2049), (256, 256, 24, 2049) and (1024, 1024, 8, 2049), each with 0 % and
30 % of the samples flagged and with one bin and 32 bins.  Medians of HIP events over REPS (default 10) timed calls after
3 warm-up calls; the kernel and the torch route are measured three times in turn.  flops = 12 nf nd nrow nt (the two real
products the kernels compute: 8 for q, 4 for h; the torch route computes 8 + 8 complex-product flops for the same).  The
MFMA fraction is the kernel's rate over the 78.6 TFLOP/s fp64 matrix peak of the card.  The JSON goes to $DELAYSPEC_OUT
(default: .) as delayspec_measure.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device

PEAK_TFLOPS = 78.6
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


def torch_route(x, w, taper, step, nd, a0, off):
    """(q, h) (nrow, nbin, nd) with the mask weighting and min_valid = 1."""
    nf, nrow, nt = x.shape
    y = taper[:, None, None] * ((w > 0).to(torch.float64) if w is not None else torch.ones_like(x.real))
    yx = (y * x).permute(1, 0, 2)                                    # the masked, tapered copy (nrow, nf, nt)
    out = []
    for k0, rhs in ((a0, yx), (0, y.permute(1, 0, 2).to(torch.complex128))):
        phi = step[None, :] * (torch.arange(nd, device=x.device, dtype=torch.float64) - k0)[:, None]
        table = torch.polar(torch.ones_like(phi), 2.0 * np.pi * (phi - torch.round(phi)))   # (nd, nf)
        cube = torch.matmul(table, rhs)                               # the transformed cube (nrow, nd, nt)
        p = cube.real ** 2 + cube.imag ** 2
        out.append(torch.stack([p[:, :, int(o0) : int(o1)].sum(dim=2) for o0, o1 in zip(off[:-1], off[1:])], dim=1))
    return out


res = dict(reps=reps, peak_tflops=PEAK_TFLOPS, cases=[])
for nf, nd, nrow, nt in ((64, 64, 96, 2049), (256, 256, 24, 2049), (1024, 1024, 8, 2049)):
    gen = torch.Generator(device="cuda").manual_seed(nf)
    x = ctx.empty((nf, nrow, nt), np.complex128)
    torch.view_as_real(x).normal_(generator=gen)
    w_all = torch.ones((nf, nrow, nt), dtype=torch.float64, device=x.device)
    w_all.masked_fill_(torch.rand((nf, nrow, nt), dtype=torch.float32, device=x.device, generator=gen) < 0.3, 0.0)
    dx, dw = torch.empty_like(x), torch.empty_like(w_all)
    step = ctx.to_device((np.arange(nf) - 0.5 * (nf - 1)) / nf)
    taper = ctx.to_device(np.blackman(nf + 2)[1:-1])
    a0 = nd // 2
    for flagged in (False, True):
        w = w_all if flagged else None
        for nbin in (1, 32):
            per = -(-nt // nbin)
            off = np.append(np.arange(0, nt, per), nt).astype(np.int32)
            nb = off.size - 1
            out = tuple(ctx.empty(s, d) for s, d in (((nrow, nb, nd), np.float64), ((nrow, nb, nd), np.float64),
                                                     ((nrow, nb), np.float64), ((nrow, nb), np.float64), ((nrow, nb), np.int32)))

            def kernel():
                ctx.delay_spectrum(x, w=w, taper=taper, step=step, nd=nd, a0=a0, bins=off, out=out)

            def route():
                return torch_route(x, w, taper, step, nd, a0, off)

            def copy():
                dx.copy_(x)
                if flagged:
                    dw.copy_(w)

            runs = [(median_ms(kernel), median_ms(route, reps=max(3, reps // 3), warm=1)) for _ in range(3)]
            kernel()
            ref = route()
            ctx.sync()
            agree = [float((o - r).abs().max() / r.abs().max()) for o, r in zip(out[:2], ref)]
            del ref
            t_copy = median_ms(copy)
            flops = 12.0 * nf * nd * nrow * nt
            t_k = float(np.median([a for a, _ in runs]))
            rate = flops / t_k * 1e-9
            case = dict(nf=nf, nd=nd, nrow=nrow, nt=nt, flagged=0.3 if flagged else 0.0, nbin=nb, kernel_ms=[a for a, _ in runs],
                        torch_route_ms=[b for _, b in runs], copy_ms=t_copy, flops=flops, kernel_tflops=rate,
                        mfma_fraction=rate / PEAK_TFLOPS, q_h_against_torch=agree,
                        kernel_over_torch=t_k / float(np.median([b for _, b in runs])), kernel_over_copy=t_k / t_copy)
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del out
            torch.cuda.empty_cache()
    del x, w_all, dx, dw
    torch.cuda.empty_cache()
open(os.path.join(os.environ.get("DELAYSPEC_OUT", "."), "delayspec_measure.json"), "w").write(json.dumps(res, indent=1))
