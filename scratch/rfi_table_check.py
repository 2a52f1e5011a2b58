"""dm_rfi_table.h against timestream.rfi_tables_host, on the host under ASan and UBSan: H, every
g_d and every threshold bit for bit, and the refusals of the argument check.

    python scratch/rfi_table_check.py"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from driftscan_amd import timestream

exe = os.path.join(ROOT, "scratch", "bin", "rfi_table_check")
os.makedirs(os.path.dirname(exe), exist_ok=True)
subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-I" + os.path.join(ROOT, "driftscan_amd", "csrc"),
                       os.path.join(ROOT, "scratch", "rfi_table_check.cpp"), "-o", exe])


def run(nt=100, segment=1024, kernel_sigma=2.5, chi1=6.0, rho=1.5, niter=3, base=2.0, min_good=16, row_share=1.0,
        windows=(1, 2, 4, 8, 16)):
    args = [str(nt), str(segment), float(kernel_sigma).hex(), float(chi1).hex(), float(rho).hex(), str(niter),
            float(base).hex(), str(min_good), float(row_share).hex()] + [str(M) for M in windows]
    return subprocess.run([exe] + args, capture_output=True, text=True)


sets = [dict(), dict(kernel_sigma=0.4), dict(kernel_sigma=10.6, chi1=4.0, rho=1.2), dict(windows=(1, 2, 4, 8, 16, 32, 64), niter=8),
        dict(windows=(64,), niter=1, base=1.0, rho=1.0), dict(kernel_sigma=1.0 / 3.0), dict(kernel_sigma=32.0 / 3.0),
        dict(chi1=5.5, base=1.7, rho=1.37, windows=(2, 8, 32))]
for p in sets:
    out = run(**p)
    assert out.returncode == 0, (p, out.stdout, out.stderr)
    lines = out.stdout.strip().split("\n")
    q = dict(kernel_sigma=2.5, windows=(1, 2, 4, 8, 16), chi1=6.0, rho=1.5, niter=3, base=2.0)
    q.update(p)
    g, t = timestream.rfi_tables_host(**q)
    assert int(lines[0].split()[1]) == g.shape[0] - 1
    assert np.array_equal(np.array([float.fromhex(v) for v in lines[1].split()[1:]]), g), p
    for it in range(q["niter"]):
        f = lines[2 + it].split()
        assert int(f[1]) == it and np.array_equal(np.array([float.fromhex(v) for v in f[2:]]), t[it]), (p, it)
    print("%s: H %d, %d x %d thresholds: ok" % (p, g.shape[0] - 1, t.shape[0], t.shape[1]))
for p, why in ((dict(nt=-1), "negative"), (dict(segment=0), "segment"), (dict(segment=2049), "segment"),
               (dict(kernel_sigma=0.0), "kernel_sigma"), (dict(kernel_sigma=float("nan")), "kernel_sigma"),
               (dict(kernel_sigma=10.7), "H ="), (dict(windows=()), "windows"), (dict(windows=(3,)), "powers of two"),
               (dict(windows=(2, 1)), "powers of two"), (dict(windows=(128,)), "powers of two"),
               (dict(windows=(1, 2, 4, 8, 16, 32, 64, 64)), "windows"), (dict(chi1=0.0), "chi1"), (dict(rho=0.5), "rho"),
               (dict(niter=0), "niter"), (dict(niter=9), "niter"), (dict(base=0.5), "base"), (dict(min_good=0), "min_good"),
               (dict(row_share=0.0), "row_share"), (dict(row_share=1.1), "row_share")):
    out = run(**p)
    assert out.returncode == 1 and why in out.stdout, (p, out.stdout, out.stderr)
print("all ok")
