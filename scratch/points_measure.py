"""Figures of DESIGN.md section 4.24: `skysim.alm_at_points` at lmax 512, 64 frequencies, npol 1 and 4, for 4096, 65536
and 10^6 points (a warm-up, then the median of 5 wall times with the result left on the device; 3 where a call takes more
than 5 s), beside the two routes that exist without it:

 (a) `healpix.sphtrans_inv_sky` to nside 512 and the value of the pixel a point falls nearest to (the ring nearest in z,
     the pixel nearest in phi), with its error against the exact evaluation;
 (b) a torch restatement at 4096 points, unpolarised: `healpix.lambda_lm` tables uploaded, one `torch.matmul` per m and
     the phase sum; and the point count at which its tables no longer fit the card, from their size.

    python scratch/points_measure.py [OUTDIR] [--one]

writes OUTDIR/points_measure.json (default: the current directory).  --one makes a single polarised call at 65536 points
after a warm-up at 64, for a kernel trace."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device, healpix, skysim  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
OUT = os.path.join(args[0] if args else ".", "points_measure.json")
out = {}
ctx = device.get_context(workspace_bytes=1 << 30)
torch = ctx.torch
lmax, nf = 512, 64
L = lmax + 1
PEAK_FP64_VECTOR = 78.6e12          # MI355X, flop/s
rows = L * (L + 1) // 2


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


def save():
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1)


def coefficients(npol):
    g = torch.Generator(device="cuda")
    g.manual_seed(npol)
    a = torch.randn((nf, npol, L, L, 2), dtype=torch.float64, device="cuda", generator=g)
    a = torch.view_as_complex(a) * torch.tril(torch.ones((L, L), dtype=torch.float64, device="cuda"))
    a[..., 0] = a[..., 0].real.to(torch.complex128)
    return a.contiguous()


rng = np.random.default_rng(0)
NMAX = 1000000
theta_all, phi_all = np.arccos(rng.uniform(-0.999, 0.999, NMAX)), rng.uniform(0.0, 2.0 * np.pi, NMAX)

if "--one" in sys.argv:
    a = coefficients(4)
    skysim.alm_at_points(a, (theta_all[:64], phi_all[:64]), to_host=False)
    ctx.sync()
    skysim.alm_at_points(a, (theta_all[:65536], phi_all[:65536]), to_host=False)
    ctx.sync()
    print("one call done")
    sys.exit(0)

free, total = torch.cuda.mem_get_info()
out["device_memory_bytes"] = dict(free=int(free), total=int(total))
out["alm_at_points"] = []
for npol in (1, 4):
    a = coefficients(npol)
    skysim.alm_at_points(a, (theta_all[:64], phi_all[:64]), to_host=False)          # warm-up
    for npts in (4096, 65536, NMAX):
        pts = (theta_all[:npts], phi_all[:npts])
        call = lambda: skysim.alm_at_points(a, pts, to_host=False)
        first = timed(call, 1)[0]
        ts = timed(call, 5 if first < 5.0 else 3)
        med = float(np.median(ts))
        flop = float(npts) * rows * nf * (24.0 if npol == 4 else 4.0)               # the products with the coefficients alone
        rec = dict(npts=npts, npol=npol, lmax=lmax, nf=nf, seconds=ts, median_s=med, product_flop=flop,
                   frac_fp64_vector_peak=flop / med / PEAK_FP64_VECTOR)
        out["alm_at_points"].append(rec)
        print(rec, flush=True)
        save()
    del a

# ---- (b) tables + matmul in torch, unpolarised, 4096 points ----------------------------------------------------------------
npts = 4096
a = coefficients(1)
th, ph = theta_all[:npts], phi_all[:npts]
z = np.cos(th)
t0 = time.perf_counter()
tabs = [ctx.to_device(healpix.lambda_lm(lmax, m, z)) for m in range(L)]
ctx.sync()
t_tables = time.perf_counter() - t0
dph = ctx.to_device(ph)


def torch_route():
    acc = torch.zeros((nf, npts), dtype=torch.float64, device="cuda")
    for m in range(L):
        am = a[:, 0, m:, m]
        fr, fi = torch.matmul(am.real, tabs[m]), torch.matmul(am.imag, tabs[m])
        arg = m * dph
        acc += (1.0 if m == 0 else 2.0) * (fr * torch.cos(arg) - fi * torch.sin(arg))
    return acc


timed(torch_route, 1)
ts = timed(torch_route, 5)
want = torch_route().T.cpu().numpy()
got = skysim.alm_at_points(a, (th, ph))[:, 0]
table_bytes_per_point = rows * 8
out["torch_tables"] = dict(npts=npts, npol=1, seconds=ts, median_s=float(np.median(ts)), tables_host_and_upload_s=t_tables,
                           table_bytes=int(table_bytes_per_point * npts),
                           max_abs_difference_to_kernel=float(np.abs(want - got).max()), max_abs_value=float(np.abs(got).max()),
                           points_whose_tables_fill_the_card=dict(npol1=int(total // table_bytes_per_point),
                                                                  npol4=int(total // (3 * table_bytes_per_point))))
print(out["torch_tables"], flush=True)
save()
del tabs, a

# ---- (a) a map at nside 512 and its nearest pixel -----------------------------------------------------------------------------
nside = 512
zr = healpix.ring_z(nside)
nphi, phi0, start = healpix.ring_layout(nside)


def nearest_pixel(theta, phi):
    zz = np.cos(theta)
    k = np.clip(np.searchsorted(-zr, -zz), 1, zr.size - 1)                     # zr descends
    r = np.where(np.abs(zr[k - 1] - zz) <= np.abs(zr[k] - zz), k - 1, k)
    j = np.rint((phi - phi0[r]) / (2.0 * np.pi / nphi[r])).astype(np.int64) % nphi[r]
    return start[r] + j


out["map_route"] = []
for npol, nfm in ((1, 64), (4, 64)):
    a = coefficients(npol)
    npts = 65536
    pix = nearest_pixel(theta_all[:npts], phi_all[:npts])

    def map_route():
        mp = healpix.sphtrans_inv_sky(a[:nfm], nside)                               # (nf, npol, npix) on the host
        return np.ascontiguousarray(mp[:, :, pix].transpose(2, 1, 0))

    first = timed(map_route, 1)[0]
    ts = timed(map_route, 3 if first < 20.0 else 1)
    approx = map_route()
    exact = skysim.alm_at_points(a[:nfm], (theta_all[:npts], phi_all[:npts]))
    rec = dict(npts=npts, npol=npol, nf=nfm, nside=nside, map_bytes=int(nfm * npol * 12 * nside * nside * 8), warmup_s=first,
               seconds=ts, median_s=float(np.median(ts)), max_abs_error_of_nearest_pixel=float(np.abs(approx - exact).max()),
               rms_error_of_nearest_pixel=float(np.sqrt(np.mean((approx - exact) ** 2))), rms_value=float(np.sqrt(np.mean(exact ** 2))))
    out["map_route"].append(rec)
    print(rec, flush=True)
    save()
    del a, approx, exact
print(json.dumps(out))
