"""Figures of DESIGN.md section 4.26: dm_formed_beam against a device copy of the bytes it reads and against the route a
user has without it, on the same card — per chunk of sources torch gathers the window columns, builds the complex phase
tensor (members x sources x samples), multiplies and reduces.

    python scratch/formedbeam_measure.py [REPS] [SOURCES ...]

Shape: 4 frequencies x one class pair of 7 x 511 members (a 4-cylinder, 256-feed array, ordered by (v, u)) x 4096 samples,
with 4096 and 65 536 sources (random positions) at H = 32; each with and without weights (10 % of the samples flagged) and
the envelope.  Medians of HIP events over REPS (default 5) timed calls after 2 warm-up calls; the kernel and the torch
route (fewer calls: it takes seconds) are measured three times in turn.  flops = 10 nf nmem sum_s (2 H_s + 1): the complex
multiply (6) and the real multiply-add (4) of a term, cos / sin not counted; they are given per output instead.  The
JSON goes to $FORMEDBEAM_OUT (default: .) as formedbeam_measure.json."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
counts = [int(a) for a in sys.argv[2:]] or [4096, 65536]
ctx = device.get_context()
torch = ctx.torch
FP64_VECTOR_PEAK = 78.6e12


def median_ms(fn, reps=reps, warm=2):
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


def torch_route(x, w, taper, u, v, scale, env, k0, H, turn, sinth, yc0, yc1, chunk=128):
    """beam (nf, nsrc) of one group whose members are the rows of x in order, every window of half width H."""
    nf, nb, nt = x.shape
    nsrc = k0.shape[0]
    out = torch.empty((nf, nsrc), dtype=torch.float64, device=x.device)
    j = torch.arange(-H, H + 1, device=x.device)
    for c0 in range(0, nsrc, chunk):
        sl = slice(c0, min(c0 + chunk, nsrc))
        ks = (k0[sl, None] + j[None, :]) % nt                                   # (S, K)
        d = turn[sl, None] - ks.to(torch.float64) / nt
        d = d - torch.round(d)
        xg = sinth[sl, None] * torch.sin(2 * np.pi * d)
        yg = yc0[sl, None] - yc1[sl, None] * torch.cos(2 * np.pi * d)
        for f in range(nf):
            A = torch.exp(-env[f] * xg * xg)
            tau = scale[f] * (u[:, None, None] * xg[None] + v[:, None, None] * yg[None])      # (B, S, K)
            ph = torch.polar(torch.ones_like(tau), -2.0 * np.pi * (tau - torch.round(tau)))
            xb = taper[:, None, None].expand(nb, ks.shape[0], ks.shape[1])
            if w is not None:
                xb = xb * w[f][:, ks]
            num = ((x[f][:, ks] * ph).real * xb * A[None]).sum(dim=(0, 2))
            out[f, sl] = num / (xb * A[None]).sum(dim=(0, 2))
    return out


nf, nu, nv, nt, H = 4, 7, 511, 4096, 32
nb = nu * nv
iv, iu = np.divmod(np.arange(nb), nu)                                           # ordered by (v, u)
uvals = (np.arange(nu) - nu // 2) * 22.0
vvals = (np.arange(nv) - nv // 2) * 0.3048
off, members = np.array([0, nb], dtype=np.int32), np.arange(nb, dtype=np.int32)
runs = 0                                                                        # runs of equal v in the 64 members a wave takes
for c0 in range(0, nb, 256):
    for w0 in range(c0, min(c0 + 256, nb), 64):
        runs += len(np.unique(iv[w0 : min(w0 + 64, c0 + 256, nb)]))
gen = torch.Generator(device="cuda").manual_seed(7)
x = ctx.empty((nf, nb, nt), np.complex128)
torch.view_as_real(x).normal_(generator=gen)
w_all = torch.rand((nf, nb, nt), dtype=torch.float64, device=x.device, generator=gen).add_(0.5)
w_all.masked_fill_(torch.rand((nf, nb, nt), dtype=torch.float32, device=x.device, generator=gen) < 0.1, 0.0)
dx, dw = torch.empty_like(x), torch.empty_like(w_all)
taper = 1.1 + np.cos(np.pi * vvals[iv] / (np.abs(vvals).max() + 0.3048))
scale = np.linspace(400.0, 800.0, nf) / 299.792458
dev = {k: ctx.to_device(a) for k, a in dict(uvals=uvals, vvals=vvals, taper=taper, scale=scale, u=uvals[iu], v=vvals[iv]).items()}
res = dict(reps=reps, nf=nf, members=nb, nu=nu, nv=nv, nt=nt, half=H, v_runs_per_sample=runs, fp64_vector_peak=FP64_VECTOR_PEAK, cases=[])
for nsrc in counts:
    rng = np.random.default_rng(nsrc)
    theta = np.pi / 4 + rng.uniform(-0.6, 0.6, nsrc)
    turn = rng.uniform(0.0, 1.0, nsrc)
    k0 = (np.rint(turn * nt).astype(np.int64) % nt).astype(np.int32)
    half = np.full(nsrc, H, dtype=np.int32)
    tz = np.pi / 4
    tabs = dict(turn=turn, sinth=np.sin(theta), yc0=np.sin(tz) * np.cos(theta), yc1=np.cos(tz) * np.sin(theta))
    sd = {k: ctx.to_device(a) for k, a in tabs.items()}
    k0_d = ctx.to_device(k0.astype(np.int64))
    for weighted, fwhm in ((False, None), (True, 0.05)):
        w = w_all if weighted else None
        env = np.zeros(nf) if fwhm is None else 4.0 * np.log(2.0) / (fwhm / scale) ** 2
        env_d = ctx.to_device(env)
        out = (ctx.empty((nf, 1, 1, nsrc), np.float64), ctx.empty((nf, 1, nsrc), np.float64), ctx.empty((nf, 1, nsrc), np.float64))

        def kernel():
            ctx.formed_beam(x, off, members, iu, iv, dev["uvals"], dev["vvals"], dev["scale"], env, k0, half, sd["turn"], sd["sinth"],
                            sd["yc0"], sd["yc1"], w=w, taper=dev["taper"], parts=1, out=out[0], norm=out[1], norm2=out[2])

        def route():
            return torch_route(x, w, dev["taper"], dev["u"], dev["v"], dev["scale"], env_d, k0_d, H, sd["turn"], sd["sinth"], sd["yc0"],
                               sd["yc1"])

        def copy():
            dx.copy_(x)
            if weighted:
                dw.copy_(w)

        rr = 1 if nsrc > 8192 else max(2, reps // 2)
        runs_ms = [(median_ms(kernel), median_ms(route, reps=rr, warm=1 if nsrc <= 8192 else 0)) for _ in range(3)]
        kernel()
        ref = route()
        ctx.sync()
        agree = float((out[0][:, 0, 0] - ref).abs().max() / ref.abs().max())
        del ref
        t_copy = median_ms(copy)
        terms = float(nsrc) * (2 * H + 1)
        flops = 10.0 * nf * nb * terms
        t_k = float(np.median([a for a, _ in runs_ms]))
        case = dict(nsrc=nsrc, weighted=weighted, envelope_fwhm=fwhm, kernel_ms=[a for a, _ in runs_ms],
                    torch_route_ms=[b for _, b in runs_ms], copy_ms=t_copy, bytes_copied=int(x.numel() * 16 + (w.numel() * 8 if weighted else 0)),
                    flops=flops, kernel_tflops=flops / t_k * 1e-9, share_of_fp64_vector_peak=flops / (t_k * 1e-3) / FP64_VECTOR_PEAK,
                    sincospi_per_output=(2 * H + 1) * (1 + nu + runs), beam_against_torch=agree,
                    kernel_over_torch=t_k / float(np.median([b for _, b in runs_ms])), kernel_over_copy=t_k / t_copy)
        res["cases"].append(case)
        print(json.dumps(case), flush=True)
        del out
        torch.cuda.empty_cache()
open(os.path.join(os.environ.get("FORMEDBEAM_OUT", "."), "formedbeam_measure.json"), "w").write(json.dumps(res, indent=1))
