"""Figures of DESIGN.md section 4.22: dm_rfi_flag_freq against the route there was before it — transpose to
(nt, nrow, nf), dm_rfi_flag, transpose back — and against a device copy of the same bytes; dm_rfi_dilate on both axes
against a device copy of w.

    python scratch/rfi2d_measure.py [NT [REPS]]

Stacked days cut to what fits: (nf, nrow) = (1024, 24) with segments of 1024 (tiles of 4 series) and of 512 (tiles of
8), (2048, 12) with one segment (tiles of 2) and (64, 384) (tiles of 8), each with NT (default 8616, a sidereal day at a
10 s cadence) samples of unit complex noise, a carrier of 20 sigma in 1 % of the channels, broadband bursts of 20 sigma
over 4 samples in 0.5 % of the samples, and 2 % of the samples flagged.  Medians of HIP events over REPS (default 20)
timed calls after 3 warm-up calls; the kernel and the transposing route are measured three times in turn.  The JSON goes
to $RFI2D_OUT (default: .) as rfi2d_measure.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device, timestream

nt = int(sys.argv[1]) if len(sys.argv) > 1 else 8616
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
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


def data(nf, nrow):
    gen = torch.Generator(device="cuda").manual_seed(nf + nrow)
    x = ctx.empty((nf, nrow, nt), np.complex128)
    torch.view_as_real(x).normal_(generator=gen).mul_(np.sqrt(0.5))
    rng = np.random.default_rng(nf)
    for f in np.nonzero(rng.random(nf) < 0.01)[0]:
        x[int(f)] += 20.0
    for s in np.nonzero(rng.random(nt) < 0.00125)[0]:
        x[:, :, int(s) : int(s) + 4] += 20.0
    w = torch.rand((nf, nrow, nt), dtype=torch.float64, device=x.device, generator=gen).add_(0.5)
    w.masked_fill_(torch.rand((nf, nrow, nt), dtype=torch.float32, device=x.device, generator=gen) < 0.02, 0.0)
    return x, w


res = dict(nt=nt, reps=reps, cases=[])
for nf, nrow, segment in ((1024, 24, 1024), (1024, 24, 512), (2048, 12, 2048), (64, 384, 1024)):
    P = timestream.rfi_params(dict(segment=segment))
    x, w = data(nf, nrow)
    nseg = -(-nf // segment)
    tile = ctx.lib.dm_rfi_freq_tile(-(-nf // nseg))
    out = (ctx.empty((nf, nrow, nt), np.float64), ctx.empty((nseg, nrow, nt), np.float64), ctx.empty((nrow, nt), np.int32),
           ctx.empty((nf, nt), np.int32))
    back = [torch.empty_like(o) for o in out]
    dx, dw, dw2 = torch.empty_like(x), torch.empty_like(w), torch.empty_like(w)

    def kernel():
        ctx.rfi_flag_freq(x, w=w, out=out, **P)

    def transposing():
        xt, wt = x.permute(2, 1, 0).contiguous(), w.permute(2, 1, 0).contiguous()
        o = ctx.rfi_flag(xt, w=wt, **P)
        for b, t in zip(back, o):
            b.copy_(t.permute(*range(t.dim() - 1, -1, -1)))

    def flag_only(xt, wt, o):
        ctx.rfi_flag(xt, w=wt, out=o, **P)

    def copy():
        dx.copy_(x), dw.copy_(w), dw2.copy_(w)

    runs = [(median_ms(kernel), median_ms(transposing)) for _ in range(3)]
    kernel()
    transposing()
    ctx.sync()
    equal = all(bool(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a,
                                 b.view(torch.int64) if b.dtype == torch.float64 else b)) for a, b in zip(out, back))
    xt, wt = x.permute(2, 1, 0).contiguous(), w.permute(2, 1, 0).contiguous()
    o_t = ctx.rfi_flag(xt, w=wt, **P)
    t_flag = median_ms(lambda: flag_only(xt, wt, o_t))
    del xt, wt, o_t
    t_copy = median_ms(copy)
    case = dict(nf=nf, nrow=nrow, segment=segment, tile=tile, samples=nf * nrow * nt, kernel_ms=[r[0] for r in runs],
                transposing_route_ms=[r[1] for r in runs], time_kernel_on_transposed_ms=t_flag, copy_ms=t_copy,
                bit_equal=equal, flagged_share=float((out[0] == 0).double().mean()),
                kernel_over_route=float(np.median([r[0] for r in runs]) / np.median([r[1] for r in runs])),
                kernel_over_copy=float(np.median([r[0] for r in runs]) / t_copy))
    # dilation of the flags of the pass, against a copy of w
    wf = out[0].clone()
    t_w = median_ms(lambda: dw.copy_(wf))
    for axis in ("time", "freq"):
        nadd = ctx.empty((nf, nrow) if axis == "time" else (nrow, nt), np.int32)
        for ref, tag in ((None, "no_ref"), (w, "ref")):
            t = median_ms(lambda: ctx.rfi_dilate(wf, 0.2, axis=axis, ref=ref, out=(dw, nadd)))
            case["dilate_%s_%s_ms" % (axis, tag)] = t
            case["dilate_%s_%s_over_copy" % (axis, tag)] = t / t_w
            case["dilate_%s_%s_added_share" % (axis, tag)] = float(nadd.sum().item()) / (nf * nrow * nt)
    case["copy_w_ms"] = t_w
    res["cases"].append(case)
    print(json.dumps(case), flush=True)
    del x, w, out, back, dx, dw, dw2, wf
    torch.cuda.empty_cache()
open(os.path.join(os.environ.get("RFI2D_OUT", "."), "rfi2d_measure.json"), "w").write(json.dumps(res, indent=1))
