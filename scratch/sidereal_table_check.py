"""dm_sidereal_table.h against timestream.sidereal_taps_host, on the host under ASan and UBSan:
first tap, span, tap count and every coefficient bit for bit, A_all and S_all to rounding, and the tiles — they cover the
grid, stay inside the day and the LDS span, and hold every in-range tap of their samples.

    python scratch/sidereal_table_check.py"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sidereal_cases as sc
from driftscan_amd import timestream

exe = os.path.join(ROOT, "scratch", "bin", "sidereal_table_check")
os.makedirs(os.path.dirname(exe), exist_ok=True)
subprocess.check_call(["c++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                       "-I" + os.path.join(ROOT, "driftscan_amd", "csrc"),
                       os.path.join(ROOT, "scratch", "sidereal_table_check.cpp"), "-o", exe])
cases = []
for nt in (37, 64):
    cases += [(sc.equal_cadence(nt), nt, a) for a in (1, 3, 5)] + [(sc.on_grid(nt), nt, 3)]
    cases += [(sc.downsampling(nt), nt, a) for a in (3, 5)]
cases += [(sc.downsampling(150), 150, 3), (sc.partial_arc(), 37, 3)]
cases += [((s, 2 * np.pi / 93, n), 37, 3) for s, n in sc.FOUR_DAYS]
cases += [((1.0, 2 * np.pi * 10 / timestream.T_SIDEREAL_DAY, 8616), 2049, 3), ((-7.3, 2 * np.pi / 1000, 500), 50, 8)]
for (p, d, n), nt, a in cases:
    out = subprocess.run([exe, str(n), str(nt), str(a), float(p).hex(), float(d).hex()], capture_output=True, text=True)
    assert out.returncode == 0, (out.stdout, out.stderr)
    lines = out.stdout.strip().split("\n")
    taps = timestream.sidereal_taps_host(n, nt, a, p, d)
    for k, (first, c) in enumerate(taps):
        f = lines[k].split()
        assert (int(f[0]), int(f[1]), int(f[2])) == (first, len(c), np.count_nonzero(c)), (k, f[:3])
        assert np.array_equal(np.array([float.fromhex(v) for v in f[5:]]), c.astype(np.float64)), k
        A, S = float.fromhex(f[3]), float.fromhex(f[4])
        assert abs(A - float(np.abs(c).sum())) <= 1e-15 * A and abs(S - float(c.sum())) <= 1e-15 * A
    tiles = np.array(lines[nt].split()[1:], dtype=int).reshape(-1, 4)
    assert tiles[:, 1].sum() == nt and np.all(tiles[:, 3] <= 1344) and np.all(tiles[:, 2] >= 0)
    assert np.all(tiles[:, 2] + tiles[:, 3] <= n) and np.all(tiles[:, 1] <= 64)
    for k0, nk, jlo, njs in tiles:
        for k in range(k0, k0 + nk):
            first, c = taps[k]
            lo, hi = max(first, 0), min(first + len(c) - 1, n - 1)
            assert hi < lo or (jlo <= lo and hi < jlo + njs), (k, lo, hi, jlo, njs)
    print("nt_in %d -> ntime %d, a = %d: %s, %d tiles: ok" % (n, nt, a, lines[nt + 1], len(tiles)))
# what the entry point refuses
for args, why in (((36, 37, 0, 0.0, 0.1), "a outside"), ((36, 37, 3, 0.0, -0.1), "dphi"), ((36, 37, 3, 0.0, 1.0), "2 pi"),
                  ((36, 0, 3, 0.0, 0.1), "ntime"), ((36, 1, 8, 0.0, 2 * np.pi / 100), "taps")):
    out = subprocess.run([exe] + [str(v) for v in args[:3]] + [float(v).hex() for v in args[3:]], capture_output=True, text=True)
    assert out.returncode == 1 and why in out.stdout, (args, out.stdout)
print("all ok")
