"""Figures of DESIGN.md section 4.19: dm_sidereal_regrid for one day against a device copy of the same input bytes and
against a plain torch formulation (gather plus masked sums) on the same tensors.

    python scratch/sidereal_measure.py [NFEED [NTIME [REPS]]]

One day of 2 frequencies, the NFEED (NFEED + 1) / 2 feed-pair rows of NFEED feeds (default 512: 131 328 rows) and the
8616 samples of a sidereal day at a 10 s cadence, onto NTIME (default 2049) grid samples with a = 3, with and without
weights (2 % of the samples flagged).  Medians of HIP events over REPS (default 20) timed calls after 3 warm-up calls.
The torch formulation goes in chunks of rows so that its gathered tensor fits beside the data; it does not compensate
its tap sum.  The JSON goes to $SIDEREAL_OUT (default: .) as sidereal_measure.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device, timestream

nfeed = int(sys.argv[1]) if len(sys.argv) > 1 else 512
ntime = int(sys.argv[2]) if len(sys.argv) > 2 else 2049
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ctx = device.get_context()
torch = ctx.torch
nf, nrow, a = 2, nfeed * (nfeed + 1) // 2, 3
dphi = 2 * np.pi * 10.0 / timestream.T_SIDEREAL_DAY
nt_in = int(2 * np.pi / dphi)
phi0 = 1.0


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
    return ts[len(ts) // 2], ts


x = ctx.empty((nf, nrow, nt_in), np.complex128).normal_()
w = torch.rand((nf, nrow, nt_in), dtype=torch.float64, device=x.device).add_(0.5)
w.masked_fill_(torch.rand((nf, nrow, nt_in), dtype=torch.float32, device=x.device) < 0.02, 0.0)
dx, dw = torch.empty_like(x), torch.empty_like(w)
shape = (nf, nrow, ntime)
acc = (ctx.empty(shape, np.complex128), ctx.empty(shape, np.float64), ctx.empty(shape, np.float64),
       torch.empty(shape, dtype=torch.int32, device=x.device))
res = dict(nf=nf, nfeed=nfeed, rows=nrow, nt_in=nt_in, ntime=ntime, a=a, x_bytes=x.numel() * 16, w_bytes=w.numel() * 8,
           out_bytes=acc[0].numel() * 36, reps=reps)

taps = timestream.sidereal_taps_host(nt_in, ntime, a, phi0, dphi)
T = max(len(c) for _, c in taps)
res["taps"] = T
first = np.array([f for f, _ in taps])
coef = np.zeros((ntime, T))
for k, (_, c) in enumerate(taps):
    coef[k, : len(c)] = c.astype(np.float64)
j = first[:, None] + np.arange(T)[None, :]
inr = (j >= 0) & (j < nt_in) & (coef != 0)
idx_d = ctx.to_device(np.clip(j, 0, nt_in - 1).astype(np.int64))
inr_d, coef_d = ctx.to_device(inr), ctx.to_device(np.where(inr, coef, 0.0))
ntap_d = ctx.to_device((coef != 0).sum(axis=1))
chunk = max(1, int(6e9 // (nf * ntime * T * 16)))


def torch_regrid(weighted):
    for r0 in range(0, nrow, chunk):
        xg = x[:, r0 : r0 + chunk][..., idx_d]                                      # (nf, R, ntime, T)
        if weighted:
            wg = w[:, r0 : r0 + chunk][..., idx_d]
            ok = (wg > 0) & inr_d
            c = torch.where(ok, coef_d, 0.0)
            sv = (c * c / torch.where(ok, wg, 1.0)).sum(-1)
            xg = torch.where(ok[..., None], torch.view_as_real(xg), 0.0)
        else:
            ok, c = inr_d.expand(xg.shape), coef_d.expand(xg.shape)
            sv = (c * c).sum(-1)
            xg = torch.view_as_real(xg)
        S, nu = c.sum(-1), ok.sum(-1)
        valid = (nu == ntap_d) & (nu > 0)
        Ss = torch.where(valid, S, 1.0)
        xh = (c[..., None] * xg).sum(-2) / Ss[..., None]
        W = torch.where(valid, Ss * Ss / torch.where(valid, sv, 1.0), 0.0)
        sl = slice(r0, r0 + chunk)
        torch.view_as_real(acc[0])[:, sl] = W[..., None] * xh
        acc[1][:, sl] = W
        acc[2][:, sl] = W * (xh * xh).sum(-1)
        acc[3][:, sl] = valid


def write_call(wd):
    ctx.check(ctx.lib.dm_sidereal_regrid(ctx.h, nf, nrow, nt_in, ntime, a, phi0, dphi, 1.0, ctx.ptr(x), ctx.ptr(wd),
                                         *(ctx.ptr(t) for t in acc), 0), "dm_sidereal_regrid")


for weighted in (False, True):
    tag = "weights" if weighted else "plain"
    wd = w if weighted else None
    kern = median_ms(lambda: write_call(wd))                                      # accumulate = 0: every output written
    mine = [ctx.to_host(t[:, :64]) for t in acc]
    kacc = median_ms(lambda: ctx.sidereal_regrid(x, phi0, dphi, ntime, w=wd, a=a, acc=acc))   # adds to the accumulators
    copy = median_ms((lambda: (dx.copy_(x), dw.copy_(w))) if weighted else (lambda: dx.copy_(x)))
    tor = median_ms(lambda: torch_regrid(weighted), reps=max(3, reps // 4), warm=1)
    theirs = [ctx.to_host(t[:, :64]) for t in acc]
    rd = res["x_bytes"] + (res["w_bytes"] if weighted else 0)
    res[tag] = dict(kernel_ms=kern, kernel_accumulate_ms=kacc, copy_ms=copy, torch_ms=tor,
                    kernel_over_copy=kern[0] / copy[0], kernel_over_torch=kern[0] / tor[0],
                    read_GBps=rd / kern[0] / 1e6, copy_GBps=2 * rd / copy[0] / 1e6,
                    torch_agrees=bool(np.array_equal(mine[3], theirs[3])
                                      and np.abs(mine[1] - theirs[1]).max() <= 1e-12 * np.abs(mine[1]).max()
                                      and np.abs(mine[0] - theirs[0]).max() <= 1e-12 * np.abs(mine[0]).max()))
print(json.dumps(res))
open(os.path.join(os.environ.get("SIDEREAL_OUT", "."), "sidereal_measure.json"), "w").write(json.dumps(res, indent=1))
