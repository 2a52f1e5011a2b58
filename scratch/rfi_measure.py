"""Figures of DESIGN.md section 4.20: dm_rfi_flag for one day against a device copy of the bytes it reads and writes and
against a torch formulation of the same method on the same tensors.

    python scratch/rfi_measure.py [NFEED [NT [REPS]]]

One day of 2 frequencies, the NFEED (NFEED + 1) / 2 feed-pair rows of NFEED feeds (default 512: 131 328 rows) and NT
(default 8616, a sidereal day at a 10 s cadence) samples of unit complex noise with bursts of 20 sigma over 4 samples in
0.5 % of the samples, default parameters (9 segments of 957 or 958 samples), with and without weights (2 % of the
samples flagged).  Medians of HIP events over REPS (default 20) timed calls after 3 warm-up calls.  The copy moves x
(and w) to another buffer and w to w_out: the bytes the kernel reads, and more than it writes.  The torch formulation
goes in chunks of rows and segment by segment (sort for the median, shifted adds for the background and the windows).
The JSON goes to $RFI_OUT (default: .) as rfi_measure.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device, timestream

nfeed = int(sys.argv[1]) if len(sys.argv) > 1 else 512
nt = int(sys.argv[2]) if len(sys.argv) > 2 else 8616
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 20
ctx = device.get_context()
torch = ctx.torch
nf, nrow = 2, nfeed * (nfeed + 1) // 2
P = timestream.rfi_params()
g_h, t_h = timestream.rfi_tables_host(P["kernel_sigma"], P["windows"], P["chi1"], P["rho"], P["niter"], P["base"])
H = g_h.shape[0] - 1
segs = timestream.rfi_segments(nt, P["segment"])


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


x = ctx.empty((nf, nrow, nt), np.complex128).normal_()
for f in range(nf):   # bursts: the same samples in every row of a frequency
    start = np.nonzero(np.random.default_rng(f).random(nt) < 0.00125)[0]
    for s in start:
        x[f, :, s : s + 4] += 20.0
w = torch.rand((nf, nrow, nt), dtype=torch.float64, device=x.device).add_(0.5)
w.masked_fill_(torch.rand((nf, nrow, nt), dtype=torch.float32, device=x.device) < 0.02, 0.0)
dx, dw = torch.empty_like(x), torch.empty_like(w)
out = (ctx.empty((nf, nrow, nt), np.float64), ctx.empty((nf, nrow, len(segs)), np.float64), ctx.empty((nf, nrow), np.int32),
       ctx.empty((nf, nt), np.int32))
tw = torch.empty_like(out[0])
res = dict(nf=nf, nfeed=nfeed, rows=nrow, nt=nt, segments=len(segs), params={k: list(v) if isinstance(v, tuple) else v
                                                                              for k, v in P.items()},
           x_bytes=x.numel() * 16, w_bytes=w.numel() * 8, out_bytes=out[0].numel() * 8, reps=reps)
chunk = 8192


def torch_flag(weighted):
    """The method of section 4.20 in torch (row_share = 1), flags into tw."""
    for r0 in range(0, nrow, chunk):
        for j0, j1 in segs:
            n = j1 - j0
            X = x[:, r0 : r0 + chunk, j0:j1].reshape(-1, n)
            if weighted:
                Wv = w[:, r0 : r0 + chunk, j0:j1].reshape(-1, n)
                I = ~(Wv > 0)
                X = X.masked_fill(I, 0.0)
            else:
                Wv = torch.ones(X.shape, dtype=torch.float64, device=X.device)
                I = torch.zeros(X.shape, dtype=torch.bool, device=X.device)
            B = I.clone()
            whole = torch.zeros(X.shape[0], dtype=torch.bool, device=X.device)
            for it in range(P["niter"]):
                cnt = (~B).sum(1)
                whole |= cnt < P["min_good"]
                sx, sg = torch.zeros_like(X), torch.zeros(X.shape, dtype=torch.float64, device=X.device)
                for d in range(-H, H + 1):
                    lo, hi = max(0, -d), min(n, n - d)
                    ok = ~B[:, lo + d : hi + d]
                    sx[:, lo:hi] += (float(g_h[abs(d)]) * X[:, lo + d : hi + d]) * ok
                    sg[:, lo:hi] += float(g_h[abs(d)]) * ok
                unj = ~I & (sg == 0)
                a = torch.where(I | unj, 0.0, (X - sx / torch.where(sg > 0, sg, 1.0)).abs())
                srt = torch.sort(torch.where(B, float("inf"), a), dim=1).values
                med = srt.gather(1, (torch.clamp(cnt - 1, min=0) // 2)[:, None])
                D = I | unj
                for i, M in enumerate(P["windows"]):
                    if M > n:
                        break
                    nst = n - M + 1
                    notD = ~D
                    c = torch.zeros((X.shape[0], nst), dtype=torch.float64, device=X.device)
                    S = torch.zeros_like(c)
                    for k in range(M):
                        c += notD[:, k : k + nst]
                        S += torch.where(notD[:, k : k + nst], a[:, k : k + nst], 0.0)
                    hit = (c >= 1) & (S > c * (med * float(t_h[it, i])))
                    D = D.clone()
                    for k in range(M):
                        D[:, k : k + nst] |= hit
                B = D
            fl = B | whole[:, None]
            tw[:, r0 : r0 + chunk, j0:j1] = torch.where(fl, 0.0, Wv).reshape(nf, -1, n)


for weighted in (False, True):
    tag = "weights" if weighted else "plain"
    wd = w if weighted else None
    kern = median_ms(lambda: ctx.rfi_flag(x, w=wd, out=out, **P))
    occ = median_ms(lambda: ctx.rfi_flag(x, w=wd, out=out, **dict(P, row_share=0.5)))
    ctx.rfi_flag(x, w=wd, out=out, **P)
    share = float((out[0] == 0).double().mean())
    copy = median_ms((lambda: (dx.copy_(x), dw.copy_(w), tw.copy_(w))) if weighted else (lambda: (dx.copy_(x), tw.copy_(w))))
    tor = median_ms(lambda: torch_flag(weighted), reps=3, warm=1)
    differ = float(((out[0] == 0) != (tw == 0)).double().mean())
    rd = res["x_bytes"] + (res["w_bytes"] if weighted else 0)
    moved = 2 * rd + 2 * res["out_bytes"]
    res[tag] = dict(kernel_ms=kern, kernel_row_share_half_ms=occ, copy_ms=copy, torch_ms=tor, flagged_share=share,
                    torch_differs_share=differ, kernel_over_copy=kern[0] / copy[0], torch_over_kernel=tor[0] / kern[0],
                    kernel_GBps=(rd + res["out_bytes"]) / kern[0] / 1e6, copy_GBps=moved / copy[0] / 1e6)
print(json.dumps(res))
open(os.path.join(os.environ.get("RFI_OUT", "."), "rfi_measure.json"), "w").write(json.dumps(res, indent=1))
