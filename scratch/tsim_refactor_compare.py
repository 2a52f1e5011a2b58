"""Two trees of the simulators of timestream.py (DESIGN.md sections 4.13 - 4.20) against each other, bit for bit.

    python scratch/tsim_refactor_compare.py products DIR     # the small products every other mode reads, into DIR/prod
    python scratch/tsim_refactor_compare.py dump DIR [PROD]  # every case below: tensors and files into DIR/dump.npz
    python scratch/tsim_refactor_compare.py trace DIR [PROD] # one case alone, for rocprofv3 --kernel-trace
    python scratch/tsim_refactor_compare.py kernels CSV OUT  # ordered [kernel name, grid] of a kernel-trace CSV as JSON
    python scratch/tsim_refactor_compare.py compare A B [C]  # host only; A, B: two dumps of one tree, C: the other tree's

The package is the one of the tree the file lies in, so a checkout of another commit runs its own copy of this file (or
this one, copied there).  Products: a polarised cylinder of 2 x 3 feeds, 3 frequencies, with one KL transform.  `dump`
keeps every returned tensor and every dataset and attribute of every file written (paths below DIR relative, the
attribute `beamtransfer_path` relative to PROD, the directory of `products`, DIR by default), and beside every case with a sky the sum over m of |c_m| of its
noise-free stacked sky, gains and flags off: the scale of the synthesis bound 4 (2 mmax + 3) eps sum_m |c_m| of
tests/test_gpu_tsim.py.

`compare A B C`: an item that A and B share bit for bit must be in C bit for bit; an item on which A and B differ is
listed and |C - A| must lie within that bound (per member |g|^2 max times the bound of its class when unstacked; an
item that is no `timestream` or has no sky scale fails).  With two dumps only their differences are listed.  The
result is printed as JSON: items compared, bitwise equal, within the bound, the largest ratio to the bound, failures."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

EPS = np.finfo(np.float64).eps


def products(d):
    import yaml

    from driftscan_amd import manager

    conf = dict(config=dict(beamtransfers=True, kltransform=True, psfisher=False, output_directory=d + "/prod", truncate=False),
                telescope=dict(type="PolarisedCylinder", num_freq=3, freq_start=400.0, freq_end=430.0, freq_mode="edge",
                               num_cylinders=2, cylinder_width=2.0, num_feeds=3, feed_spacing=0.4, tsys=1.0),
                kltransform=[dict(type="KLTransform", name="kl", threshold=0.0, inverse=True, use_foregrounds=False)])
    fresh = not os.path.exists(d + "/params.yaml")
    if fresh:
        os.makedirs(d, exist_ok=True)
        open(d + "/params.yaml", "w").write(yaml.dump(conf))
    pm = manager.ProductManager.from_config(d + "/params.yaml")
    if fresh:
        pm.generate()
        from driftscan_amd import healpix, storage

        tel = pm.telescope
        rng = np.random.default_rng(4)
        alm = np.zeros((tel.nfreq, 4, tel.lmax + 1, tel.lmax + 1), dtype=np.complex128)
        for l in range(tel.lmax + 1):
            for m in range(l + 1):
                alm[:, :, l, m] = rng.standard_normal((tel.nfreq, 4)) + (1j * rng.standard_normal((tel.nfreq, 4)) if m else 0)
        alm[:, 1:3, :2] = 0.0
        with storage.File(d + "/sky.hdf5", "w") as f:
            f.create_dataset("map", data=healpix.sphtrans_inv_sky(alm, 32))
    return pm


def cases(pm, d):
    """[(name, function, keywords)]: every branch of the simulators."""
    from driftscan_amd import device, skysim

    ctx = device.get_context()
    tel = pm.telescope
    nf, nfeed, npairs, ntime = int(tel.nfreq), int(tel.nfeed), int(tel.npairs), 2 * int(tel.mmax) + 1
    nmem = int(tel.redundant_pairs()[0][-1])
    rng = np.random.default_rng(23)
    sky = [d + "/sky.hdf5"]
    cat = dict(theta=np.array([0.7, 1.2, 1.9]), phi=np.array([0.3, 2.0, 4.4]), flux=np.array([3.0, 1.5, 0.7]), nu0=410.0,
               index=np.array([-0.7, -0.5, -1.0]))
    model = skysim.GainModel(sigma_amp=0.05, sigma_phase=0.05, corr_time=3600.0, seed=2)
    flags = skysim.FlagModel(fraction=0.05, burst=3, seed=6)

    def crandn(*shape):
        return 1.0 + 0.05 * (rng.standard_normal(shape) + 1j * rng.standard_normal(shape))

    def warr(nfreq, nrow, nt=ntime):
        return (rng.uniform(size=(nfreq, nrow, nt)) > 0.2) * rng.uniform(0.5, 2.0, size=(nfreq, nrow, nt))

    g3, g4 = crandn(nf, nfeed, ntime), crandn(9, nf, nfeed, ntime)
    g2f = crandn(2, nfeed, ntime)
    base = dict(seed=5, sky_seed=3)
    vis = [   # simulate_visibilities and simulate_ensemble, stacked and unstacked each
        ("nothing", dict(nreal=1, ndays=0)),
        ("noise_only", dict(nreal=3, ndays=10)),
        ("maps", dict(nreal=1, maps=sky, ndays=0)),
        ("maps_noise", dict(nreal=3, maps=sky, ndays=10, first=2)),
        ("models", dict(nreal=3, skymodels=("signal", "foreground"), klname="kl", ndays=0)),
        ("model_str_noise", dict(nreal=9, skymodels="signal", ndays=10)),
        ("sources", dict(nreal=1, sources=[cat], ndays=0)),
        ("all_sky_noise", dict(nreal=9, maps=sky, skymodels=("signal",), sources=cat, ndays=10)),
        ("gainmodel", dict(nreal=9, maps=sky, skymodels=("signal",), ndays=10, gains=model)),
        ("gainmodel_no_noise", dict(nreal=3, maps=sky, ndays=0, gains=model)),
        ("gainmodel_no_sky", dict(nreal=3, ndays=10, gains=model)),
        ("gainmodel_small_chunks", dict(nreal=9, maps=sky, skymodels=("signal",), ndays=10, gains=model, chunk_gb=1e-9)),
        ("gains_host_nf", dict(nreal=3, maps=sky, ndays=10, gains=g3)),
        ("gains_host_nreal_nf", dict(nreal=9, maps=sky, ndays=10, gains=g4, chunk_gb=1e-9)),
        ("gains_device_nf", dict(nreal=3, maps=sky, ndays=0, gains="device3")),
        ("gains_device_nreal_nf", dict(nreal=9, skymodels=("signal",), ndays=10, gains="device4")),
        ("gains_freqs", dict(nreal=3, maps=sky, ndays=10, gains=g2f, freqs=[0, 2])),
        ("freqs", dict(nreal=3, maps=sky, skymodels=("signal",), ndays=10, freqs=[0, 2])),
        ("weights_array", dict(nreal=3, maps=sky, ndays=10, weights="array")),
        ("weights_flagmodel", dict(nreal=3, maps=sky, ndays=10, weights=flags)),
        ("weights_small_chunks", dict(nreal=9, maps=sky, ndays=10, weights="array", chunk_gb=1e-9)),
        ("everything", dict(nreal=9, maps=sky, skymodels=("signal",), ndays=10, gains=model, weights="array")),
        ("everything_small_chunks", dict(nreal=9, maps=sky, skymodels=("signal",), ndays=10, gains=model, weights="array",
                                         freqs=[0, 2], chunk_gb=1e-9)),
    ]
    out = []
    for name, kw in vis:
        for unstacked in (False, True):
            kw2 = dict(base, **kw)
            nfk = len(kw2.get("freqs", range(nf)))
            if isinstance(kw2.get("gains"), str):
                kw2["gains"] = ctx.to_device(g3 if kw2["gains"] == "device3" else g4)
            if isinstance(kw2.get("weights"), str):
                kw2["weights"] = warr(nfk, nmem if unstacked else npairs)
            tag = name + ("_unstacked" if unstacked else "")
            out.append(("visibilities_" + tag, "simulate_visibilities", dict(kw2, unstacked=unstacked)))
            out.append(("ensemble_" + tag, "simulate_ensemble", dict(kw2, unstacked=unstacked)))
    one = dict(maps=sky, skymodels=("signal",), ndays=10, sky_seed=3, sky_realisation=1)
    out += [
        ("simulate_noise_gains_weights", "simulate", dict(ndays=10, seed=7, gains=g3, weights=warr(nf, npairs))),
        ("simulate_noise_unseeded", "simulate", dict(ndays=10)),
        ("simulate_sky_gainmodel_weights", "simulate", dict(one, seed=7, gains=model, weights=flags)),
        ("simulate_sky_plain", "simulate", dict(one, seed=9, sources=[cat])),
        ("simulate_unstacked_plain", "simulate_unstacked", dict(one)),
        ("simulate_unstacked_all", "simulate_unstacked", dict(one, seed=4, gains=model, weights=warr(nf, nmem), chunk_gb=1e-9)),
    ]
    days = dict(starts=[0.1, 2.0, 6.0], nsamples=[40, 33, 57], cadence=60.0, maps=sky, skymodels=("signal",), seed=5, sky_seed=3)
    rfi = dict(fraction=0.02, burst=2, amplitude=12.0, seed=3)
    for unstacked in (False, True):
        nrow = nmem if unstacked else npairs
        tag = "_unstacked" if unstacked else ""
        out += [
            ("days_plain" + tag, "simulate_days", dict(days, unstacked=unstacked)),
            ("days_rfi_no_noise" + tag, "simulate_days", dict(days, unstacked=unstacked, ndays=0, rfi=rfi, nsamples=40)),
            ("days_weight_list" + tag, "simulate_days", dict(days, unstacked=unstacked, rfi=rfi, gains=model, first=2,
                                                             weights=[warr(nf, nrow, n) for n in days["nsamples"]])),
            ("days_flagmodel" + tag, "simulate_days", dict(days, unstacked=unstacked, weights=dict(fraction=0.1, burst=2, seed=1),
                                                           freqs=[0, 2], chunk_gb=1e-9)),
            ("days_one_weight" + tag, "simulate_days", dict(days, unstacked=unstacked, nsamples=40, weights=warr(nf, nrow, 40))),
        ]
    return out


def run_case(pm, d, pd, name, fn, kw, items):
    """One call; its tensor, or every dataset and attribute of every file it wrote, into `items`."""
    from driftscan_amd import device, storage, timestream

    ctx = device.get_context()
    kw = dict(kw)
    f = getattr(timestream, fn)
    np.random.seed(1234)   # `simulate` draws from the global stream: with seed=None it goes on from here
    if fn == "simulate_visibilities":
        items[name + "/tensor"] = ctx.to_host(f(pm, kw.pop("nreal"), **kw))
        tss = []
    elif fn == "simulate_ensemble":
        tss = f(pm, "%s/out/%s" % (d, name), kw.pop("nreal"), **kw)
    elif fn == "simulate_days":
        tss = f(pm, ["%s/out/%s/day_%d" % (d, name, k) for k in range(len(kw["starts"]))], kw.pop("starts"), kw.pop("nsamples"),
                kw.pop("cadence"), **kw)
    else:
        tss = [f(pm, "%s/out/%s" % (d, name), **kw)]
    for ts in tss:
        rel = os.path.relpath(ts.directory, "%s/out/%s" % (d, name))
        freqs = kw.get("freqs") or range(pm.telescope.nfreq)
        assert os.path.exists(ts._picklefile), ts.directory
        for fi in freqs:
            with storage.File(ts._ffile(fi), "r") as h:
                key = "%s/%s/f%d/" % (name, rel, fi)
                items[key + "_names"] = np.array(list(h.keys()))          # creation order included
                for dset in h.keys():
                    items[key + dset] = np.asarray(h[dset][:])
                for a in h.attrs.keys():
                    v = h.attrs[a]
                    items[key + "@" + a] = np.array(os.path.relpath(v, pd) if a == "beamtransfer_path" else v)
    # the scale of the synthesis bound
    sky = {k: kw[k] for k in ("maps", "skymodels", "sources", "klname", "sky_seed", "freqs", "first") if k in kw}
    if any(len(sky.get(k, ())) for k in ("maps", "skymodels", "sources")):
        if "sky_realisation" in kw:
            sky["first"] = kw["sky_realisation"]
        nreal = 1 if fn not in ("simulate_visibilities", "simulate_ensemble") else items_nreal(kw, name, items)
        x = timestream.simulate_visibilities(pm, nreal, ndays=0, **sky)
        mmax = int(pm.telescope.mmax)
        items[name + "/_csum"] = np.stack([np.abs(ctx.to_host(ctx.mmode_transform(x[r], mmax))).sum(axis=(0, 2))
                                           for r in range(nreal)])


def items_nreal(kw, name, items):
    t = items.get(name + "/tensor")
    return int(t.shape[0]) if t is not None else len({k.split("/")[1] for k in items if k.startswith(name + "/real_")})


def main():
    what = sys.argv[1]
    if what == "compare":
        return compare(*sys.argv[2:])
    if what == "kernels":
        return kernels(sys.argv[2], sys.argv[3])
    d = os.path.abspath(sys.argv[2])
    pd = os.path.abspath(sys.argv[3]) if len(sys.argv) > 3 else d
    os.makedirs(d, exist_ok=True)
    pm = products(pd)
    if what == "products":
        return
    from driftscan_amd import device

    ctx = device.get_context()
    todo = cases(pm, pd)
    if what == "trace":   # unstacked, with maps, a model, gains, noise and flags, nreal = 9
        todo = [("trace",) + c[1:] for c in todo if c[0] == "visibilities_everything_unstacked"]
    items = {}
    for name, fn, kw in todo:
        run_case(pm, d, pd, name, fn, kw, items)
        ctx.sync()
    tel = pm.telescope
    items["_meta/mmax"] = np.array(int(tel.mmax))
    items["_meta/class_off"] = np.asarray(tel.redundant_pairs()[0])
    if what == "dump":
        np.savez(d + "/dump.npz", **items)
    print("%s: %d cases, %d items" % (what, len(todo), len(items)))


def kernels(csv_name, out):
    import csv

    rows = list(csv.DictReader(open(csv_name)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"] if "Dispatch_Id" in r else r["Start_Timestamp"]))
    names = [[r["Kernel_Name"], [int(r["Grid_Size_X"]), int(r["Grid_Size_Y"]), int(r["Grid_Size_Z"])]] for r in rows]
    json.dump(names, open(out, "w"))
    print("%d dispatches" % len(names))


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and (np.array_equal(a, b) if a.dtype.kind in "US" else
                                                         a.tobytes() == b.tobytes())


def _bound(dump, key):
    """The synthesis bound of item `key`, broadcastable to it, or None."""
    parts = key.split("/")
    csum = dump.get(parts[0] + "/_csum")
    if csum is None or parts[-1] not in ("tensor", "timestream") or parts[0].startswith("days_"):
        return None
    off = dump["_meta/class_off"]
    b = 4 * (2 * int(dump["_meta/mmax"]) + 3) * EPS * csum                      # (nreal, nf, npairs)
    unstacked = "unstacked" in parts[0]
    if unstacked:
        b = np.repeat(b, np.diff(off), axis=-1)
    if parts[-1] == "tensor":
        g2 = 1.0
    else:
        gain = dump.get("/".join(parts[:-1]) + "/gain")
        g2 = 1.0 if gain is None else float(np.abs(gain).max()) ** 2
        reals = sorted({k.split("/")[1] for k in dump if k.startswith(parts[0] + "/") and k.count("/") == 3})
        fdir = sorted({k.split("/")[2] for k in dump if k.startswith(parts[0] + "/" + parts[1] + "/f")})
        b = b[reals.index(parts[1]), fdir.index(parts[2])]
        return g2 * b[:, None]
    return 1.2 * b[..., None]   # gains of 5 per cent in amplitude: |g|^2 < 1.2 to four sigma


def compare(a, b, c=None):
    A, B = (dict(np.load(x + "/dump.npz")) for x in (a, b))
    C = dict(np.load(c + "/dump.npz")) if c else None
    keys = sorted(k for k in A if not k.endswith("/_csum"))
    res = dict(items=len(keys), bitwise_equal=0, within_bound=0, largest_ratio_to_bound=0.0, parent_differs=[], failures=[])
    if set(A) != set(B) or (C is not None and set(A) != set(C)):
        res["failures"].append("the dumps do not hold the same items")
    for k in keys:
        if k not in B or (C is not None and k not in C):
            continue
        stable = _same(A[k], B[k])
        other = B[k] if C is None else C[k]
        if not stable:
            res["parent_differs"].append(k)
        if _same(A[k], other):
            res["bitwise_equal"] += 1
        elif stable and C is not None:
            res["failures"].append(k + ": differs where the first tree reproduces itself")
        else:
            bound = _bound(A, k)
            if bound is None or A[k].shape != other.shape:
                res["failures"].append(k + ": differs and has no bound")
                continue
            ratio = float((np.abs(other - A[k]) / np.maximum(bound, 1e-300)).max())
            res["largest_ratio_to_bound"] = max(res["largest_ratio_to_bound"], ratio)
            if ratio <= 1.0:
                res["within_bound"] += 1
            else:
                res["failures"].append("%s: %.3g times the bound" % (k, ratio))
    res["np_random_path_of_simulate_bitwise"] = all(
        _same(A[k], (B if C is None else C)[k]) for k in keys if k.startswith("simulate_noise_") and k in (B if C is None else C))
    print(json.dumps(res, indent=1))
    return 1 if res["failures"] else 0


if __name__ == "__main__":
    sys.exit(main())
