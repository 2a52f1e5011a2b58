"""Bytes of A per second of dm_blockvec_grouped against dm_zgemm_grouped fed the same descriptors.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o bv -- python scratch/blockvec_rate.py --run DIR/calls.json
    python scratch/blockvec_rate.py --parse DIR --out profiles/blockvec_rates.json

`--run` issues, batch by batch and for R = 1, 2, 4, 6, 8, one warm-up and three timed calls of each route — one kernel dispatch
per call — and writes the list of calls; `--parse` takes the last len(calls) block-apply / grouped-ZGEMM dispatches of the
kernel trace and divides the bytes of A of each call by its kernel time.  Batches: the (m, frequency) blocks of `beam_ut` of
BASELINE configs[1] with the kept-mode counts of real products; its KL eigenvectors (all modes) forwards and, stored
transposed, backwards; and configs[2] block shapes (64 frequencies, ntel and svd_len of the CFG3 telescope, random data)."""
import argparse
import csv
import glob
import json
import os
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

RS = (1, 2, 4, 6, 8)
REPS = 3


def run(path):
    import torch
    import yaml

    from benchlib.common import CFG2, CFG3
    from driftscan_amd import beamtransfer as btmod
    from driftscan_amd import cylinder, device, kltransform as klmod, manager

    ctx = device.get_context()
    d = tempfile.mkdtemp()
    conf = dict(config=dict(beamtransfers=True, kltransform=False, psfisher=False, output_directory=d + "/prod", truncate=False),
                telescope=dict(type="UnpolarisedCylinder", **CFG2))
    open(d + "/params.yaml", "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(d + "/params.yaml")
    pm.generate()
    bt = pm.beamtransfer
    ms = list(range(pm.telescope.mmax + 1))
    svnum1 = bt._svnum_batch(ms)
    ndofs1 = svnum1.sum(axis=1)
    tel3 = cylinder.UnpolarisedCylinderTelescope.from_config(CFG3)
    T3 = 2 * tel3.npairs
    K3 = min(tel3.lmax + 1, T3)
    nb3 = 64
    n3 = tel3.nfreq * K3 // 2

    def randc(n):
        return torch.view_as_complex(torch.randn((int(n), 2), dtype=torch.float64, device="cuda"))

    def batches(R):
        tab, off = btmod.svd_forward_table(svnum1, bt.svd_len, bt.ntel, R)
        yield "configs1 beam_ut (real svnum)", "dot", tab, len(ms) * bt.nfreq * bt.svd_len * bt.ntel, svnum1.size * bt.ntel * R, off[-1] * R
        tab, kloff = klmod.kl_forward_table(ndofs1, ndofs1, np.concatenate([[0], np.cumsum(ndofs1)]), R)
        yield "configs1 KL evecs (all modes)", "dot", tab, (ndofs1 ** 2).sum(), ndofs1.sum() * R, kloff[-1] * R
        tab = klmod.kl_backward_table(ndofs1, ndofs1, kloff, kloff, R)
        yield "configs1 KL evinv (all modes)", "axpy", tab, (ndofs1 ** 2).sum(), ndofs1.sum() * R, kloff[-1] * R
        sv3 = np.full((nb3, tel3.nfreq), K3)
        tab, off = btmod.svd_forward_table(sv3, K3, T3, R)
        yield "configs2 beam_ut shapes, %d m (ntel %d, svd_len %d)" % (nb3, T3, K3), "dot", tab, sv3.size * K3 * T3, sv3.size * T3 * R, off[-1] * R
        tab, kloff = klmod.kl_forward_table([n3], [n3], [0, n3], R)
        yield "configs2 KL evecs shape, one m (ndof %d)" % n3, "dot", tab, n3 * n3, n3 * R, n3 * R
        tab = klmod.kl_backward_table([n3], [n3], [0, n3], [0, n3], R)
        yield "configs2 KL evinv shape, one m (ndof %d)" % n3, "axpy", tab, n3 * n3, n3 * R, n3 * R

    calls = []
    for R in RS:
        for name, form, tab, na, nx, ny in batches(R):
            A, x, y = randc(na), randc(max(nx, 1)), randc(max(ny, 1))
            nbytes = float(16 * (tab["M"] * tab["K"]).sum())
            for route in ("blockvec", "zgemm"):
                for rep in range(REPS + 1):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    ctx.blockvec_grouped(A, x, y, tab, R, route=route)
                    e1.record()
                    ctx.sync()
                    torch.cuda.synchronize()
                    calls.append(dict(batch=name, form=form, R=R, route=route, rep=rep, problems=int(len(tab)), bytes_A=nbytes,
                                      event_ms=float(e0.elapsed_time(e1))))
            del A, x, y
    with open(path, "w") as f:
        json.dump(calls, f)
    print("issued %d calls" % len(calls))


def parse(dirname, out):
    calls = json.load(open(os.path.join(dirname, "calls.json")))
    trace = [p for p in glob.glob(os.path.join(dirname, "**", "*kernel_trace.csv"), recursive=True)]
    rows = []
    for p in trace:
        with open(p) as f:
            for r in csv.DictReader(f):
                if "blockvec_kernel" in r["Kernel_Name"] or ("zgemm" in r["Kernel_Name"] and "grouped" in r["Kernel_Name"]):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    rows = rows[-len(calls):]
    assert len(rows) == len(calls), (len(rows), len(calls))
    table = {}
    for c, (t0, t1, name) in zip(calls, rows):
        assert ("blockvec_kernel" in name) == (c["route"] == "blockvec"), (c, name)
        if c["rep"] == 0:
            continue
        key = (c["batch"], c["form"], c["R"])
        e = table.setdefault(key, dict(batch=c["batch"], form=c["form"], R=c["R"], problems=c["problems"], GB_A=c["bytes_A"] / 1e9))
        e.setdefault(c["route"] + "_us", []).append((t1 - t0) / 1e3)
        e.setdefault(c["route"] + "_event_us", []).append(c["event_ms"] * 1e3)
    res = []
    for e in table.values():
        for route in ("blockvec", "zgemm"):
            best = min(e[route + "_us"])
            e[route + "_TBps"] = e["GB_A"] * 1e9 / (best * 1e-6) / 1e12
        res.append(e)
        print("%-60s %-4s R=%d  blockvec %9.1f us %5.2f TB/s   zgemm %9.1f us %5.2f TB/s" % (
            e["batch"], e["form"], e["R"], min(e["blockvec_us"]), e["blockvec_TBps"], min(e["zgemm_us"]), e["zgemm_TBps"]))
    with open(out, "w") as f:
        json.dump(dict(note="kernel times from a rocprofv3 --kernel-trace run of scratch/blockvec_rate.py (best of 3 after a "
                            "warm-up); TB/s = bytes of A / kernel time; *_event_us: HIP events around the whole call",
                       rows=res), f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--parse")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.run:
        run(a.run)
    else:
        parse(a.parse, a.out)
