"""Figures of DESIGN.md section 4.23: dm_delay_fit against a device copy of the same bytes and against the route a user
has without it — batched torch.einsum for G and b, torch.linalg.cholesky and cholesky_solve, on the same card.

    python scratch/delay_measure.py [NT [REPS]]

(nf, nrow) = (64, 96) and (256, 24): a few frequencies' worth of rows of a stacked day, NT (default 2049) samples each;
ranks 8, 16, 32 and 64 (random orthonormal bases: the cost does not depend on the numbers), 0, 5 and 30 % of the samples
flagged, in inpaint mode (the one with the fill weights).  Medians of HIP events on the context's stream over REPS
(default 10) timed calls after 3 warm-up calls; the kernel and the torch route are measured three times in turn.  The
torch route computes model and fill weights only (no mode logic), in chunks of samples that bound its (samples, r, r)
workspace; it factors with `cholesky_ex`, and the batch elements whose factorisation it reports as failed are counted
(`torch_failed`) and left out of the comparison of the fills.  The JSON goes to $DELAY_OUT (default: .) as delay_measure.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device

nt = int(sys.argv[1]) if len(sys.argv) > 1 else 2049
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 10
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


def torch_route(x, w, A, chunk=None):
    """model (nf, nrow, nt), fill weights and the failed factorisations for one class: G = A^T diag(w) A and b per sample,
    Cholesky, solves."""
    nf, nrow, n = x.shape
    chunk = chunk or (8192 if A.shape[1] * nf < 64 * 256 else 2048)   # the batched triangular solve copies (chunk, r, nf)
    xs, wsm = x.reshape(nf, -1), w.reshape(nf, -1)
    model, fill = torch.empty_like(xs), torch.empty_like(wsm)
    Ac = A.to(x.dtype)
    failed = torch.zeros(xs.shape[1], dtype=torch.bool, device=x.device)
    for s0 in range(0, xs.shape[1], chunk):
        om = wsm[:, s0 : s0 + chunk]
        G = torch.einsum("fi,fs,fj->sij", A, om, A)
        b = torch.einsum("fi,fs->si", Ac, om * xs[:, s0 : s0 + chunk])
        L, bad = torch.linalg.cholesky_ex(G)
        failed[s0 : s0 + chunk] = bad != 0
        c = torch.cholesky_solve(b.unsqueeze(-1), L.to(x.dtype)).squeeze(-1)
        model[:, s0 : s0 + chunk] = torch.einsum("fi,si->fs", Ac, c)
        Y = torch.linalg.solve_triangular(L, A.T.unsqueeze(0).expand(L.shape[0], -1, -1), upper=False)
        fill[:, s0 : s0 + chunk] = (1.0 / (Y * Y).sum(dim=1)).T
    return model.reshape(x.shape), fill.reshape(w.shape), failed.reshape(x.shape[1:])


res = dict(nt=nt, reps=reps, cases=[])
for nf, nrow in ((64, 96), (256, 24)):
    gen = torch.Generator(device="cuda").manual_seed(nf + nrow)
    x = ctx.empty((nf, nrow, nt), np.complex128)
    torch.view_as_real(x).normal_(generator=gen).mul_(np.sqrt(0.5))
    dx, dw = torch.empty_like(x), ctx.empty((nf, nrow, nt), np.float64)
    out = (torch.empty_like(x), ctx.empty((nf, nrow, nt), np.float64), ctx.empty((nrow, nt), np.int32))
    of = ctx.to_device(np.zeros(nrow, dtype=np.int32))
    for r in (8, 16, 32, 64):
        if r > nf:
            continue
        A = np.linalg.qr(np.random.default_rng(r).standard_normal((nf, r)))[0]
        table, ranks = ctx.delay_pack([A])
        A_d = ctx.to_device(np.ascontiguousarray(A))
        tile = ctx.lib.dm_delay_tile(nf, r)
        for share in (0.0, 0.05, 0.3):
            w = torch.rand((nf, nrow, nt), dtype=torch.float64, device=x.device, generator=gen).add_(0.5)
            if share > 0:
                w.masked_fill_(torch.rand((nf, nrow, nt), dtype=torch.float32, device=x.device, generator=gen) < share, 0.0)

            def kernel():
                ctx.delay_fit(x, w=w, basis=(table, ranks), basis_of=of, mode="inpaint", out=out)

            def copy():
                dx.copy_(x), dw.copy_(w)

            try:   # on some shapes the batched solves of the torch route fail to allocate: the script would stop there
                runs = [(median_ms(kernel), median_ms(lambda: torch_route(x, w, A_d), reps=max(3, reps // 3), warm=1))
                        for _ in range(3)]
            except RuntimeError as e:
                print(json.dumps(dict(nf=nf, nrow=nrow, rank=r, flagged_share=share, torch_route_error=str(e)[:200])), flush=True)
                break
            kernel()
            model, fill, failed = torch_route(x, w, A_d)
            ctx.sync()
            flagged = w == 0
            solved = (out[2] == 0)[None].expand_as(flagged)
            sel = flagged & solved & ~failed[None].expand_as(flagged)
            agree = float((out[0] - model)[sel].abs().max() / model[sel].abs().max()) if bool(sel.any()) else 0.0
            t_copy = median_ms(copy)
            case = dict(nf=nf, nrow=nrow, rank=r, tile=tile, flagged_share=share, samples=nf * nrow * nt, series=nrow * nt,
                        kernel_ms=[a for a, _ in runs], torch_route_ms=[b for _, b in runs], copy_ms=t_copy,
                        unsolved=int((out[2] != 0).sum().item()), torch_failed=int(failed.sum().item()), fill_against_torch=agree,
                        kernel_over_torch=float(np.median([a for a, _ in runs]) / np.median([b for _, b in runs])),
                        kernel_over_copy=float(np.median([a for a, _ in runs]) / t_copy))
            res["cases"].append(case)
            print(json.dumps(case), flush=True)
            del w, model, fill
        del table, A_d
    del x, dx, dw, out
    torch.cuda.empty_cache()
open(os.path.join(os.environ.get("DELAY_OUT", "."), "delay_measure.json"), "w").write(json.dumps(res, indent=1))
