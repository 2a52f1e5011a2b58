"""Figures of DESIGN.md section 4.12 at the configs[2] shape (64 channels, npol 4, lmax 512, one realisation).

    python scratch/skysim_measure.py all
    rocprofv3 --kernel-trace --stats -f csv -d DIR -o skysim -- python scratch/skysim_measure.py draw

`all`: wall times (best of 3, device idle before and after) of the roots on the device and with numpy, of draw_alm, of a
device fill of the same bytes, of draw_alm for every second frequency (32 one-row calls per group), of the joint group
of n = 256, of gaussian_sky at nside 512, and of ONE group (n = 64) fused against unfused.  The unfused route does the
same work into the same preallocated [64, L, L] array: zero it, dm_psmc_draw of the n (l + 1) draws of every l to
memory, one grouped ZGEMM of L problems T_l (n x n) times z_l (n x (l + 1)).  The library's ZGEMM has no real-operand
variant, so T_l is cast to complex128 outside the timed region and the product does twice the real-operand flops; the
three parts are therefore timed separately as well: zeroing and drawing alone bound the unfused route from below
whatever the product costs.
`draw`: roots and three draw_alm calls only, for the kernel trace.  The JSON goes to $SKYSIM_OUT (default: .)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from driftscan_amd import device, skymodel, skysim

what = sys.argv[1] if len(sys.argv) > 1 else "all"
ctx = device.get_context()
torch = ctx.torch
freqs = np.linspace(400.0, 500.0, 64)
lmax = 512
cv = skymodel.foreground_model(lmax, freqs, 4)
res = {}


def wall(fn, reps=3):
    best = 1e30
    for _ in range(reps):
        ctx.sync(); torch.cuda.synchronize(); t0 = time.perf_counter(); out = fn(); ctx.sync(); torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
        del out
    return best


roots = skysim.covariance_roots(cv)          # warm-up
res["roots_device_s"] = wall(lambda: skysim.covariance_roots(cv))
a = skysim.draw_alm(cv, roots=roots, to_host=False)
res["alm_bytes"] = a.numel() * 16
del a
res["draw_alm_device_wall_s"] = wall(lambda: skysim.draw_alm(cv, roots=roots, to_host=False))
if what == "all":
    t0 = time.perf_counter(); skysim.covariance_roots(cv, device=False); res["roots_numpy_s"] = time.perf_counter() - t0
    # streaming rate: a device fill of the same array
    buf = ctx.empty((res["alm_bytes"] // 16,), np.complex128)
    buf.zero_()
    res["fill_same_bytes_s"] = wall(lambda: (buf.zero_(), None)[1])
    del buf
    # every second frequency: 32 runs of one row per group, 96 launches
    half = list(range(0, 64, 2))
    skysim.draw_alm(cv, roots=roots, freqs=half, to_host=False)
    res["draw_alm_every_2nd_freq_wall_s"] = wall(lambda: skysim.draw_alm(cv, roots=roots, freqs=half, to_host=False))

    # ---- one group, n = 64: fused against unfused, same output array, same zeros --------------------------------------
    n, L = 64, lmax + 1
    out = ctx.empty((n, L, L), np.complex128)
    jg = np.arange(n)

    def fused():
        ctx.sky_draw(roots[0], jg, jg * L * L, n, 0, n, L, 1, 16, 0, 1, out, (n * L * L, L, 1))

    fused()
    res["one_group_fused_wall_s"] = wall(fused)

    Tc = roots[0].to(torch.complex128).contiguous()
    cols = np.arange(1, L + 1)
    zoff = np.concatenate([[0], np.cumsum(n * cols)])

    def draw_z():
        return ctx.psmc_draw(np.arange(L), n * cols, 1, 1)      # block l: the n (l + 1) draws of multipole l

    def product(z):
        ctx.zgemm_grouped([dict(A=Tc[l], B=z[zoff[l]:zoff[l + 1]], C=out[:, l, :], M=n, N=l + 1, K=n, rsA=n, csA=1,
                                rsB=l + 1, csB=1, ldc=L * L) for l in range(L)])

    def unfused():
        out.zero_()
        product(draw_z())

    unfused()
    z = draw_z()
    res["one_group_unfused_wall_s"] = wall(unfused)
    res["one_group_unfused_zero_s"] = wall(lambda: (out.zero_(), None)[1])
    res["one_group_unfused_draw_s"] = wall(draw_z)
    res["one_group_unfused_zgemm_s"] = wall(lambda: product(z))
    del out, Tc, z

    # the joint-group instantiation (n = 256 > 128: 16 real columns per workgroup)
    cvj = skymodel.foreground_model(lmax, freqs, 4)
    cvj[0, 1] = 0.1 * cvj[1, 1]; cvj[1, 0] = cvj[0, 1].transpose(0, 2, 1)
    rj = skysim.covariance_roots(cvj)
    skysim.draw_alm(cvj, roots=rj, to_host=False)
    res["draw_alm_joint_n256_wall_s"] = wall(lambda: skysim.draw_alm(cvj, roots=rj, to_host=False))
    del rj
    t0 = time.perf_counter(); m = skysim.gaussian_sky(cv, 512, seed=1); res["gaussian_sky_nside512_wall_s"] = time.perf_counter() - t0
    res["gaussian_sky_shape"] = list(m.shape)
print(json.dumps(res))
open(os.environ.get("SKYSIM_OUT", ".") + "/skysim_measure_%s.json" % what, "w").write(json.dumps(res, indent=1))
