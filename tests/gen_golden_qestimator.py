#!/usr/bin/env python3
"""Generate tests/golden/qestimator.npz: the unmodified reference's PSExact.q_estimator on the products of
svdkl_unpol.npz with the band tables of psfisher.npz.  Build machine only (needs the reference tree and oracle/_ref):

    make -C oracle ref && python tests/gen_golden_qestimator.py

The inputs are seeded SKY-space vectors a (F, 1, L, 3) per m; the reference projects them into its KL basis and
estimates q from there.  q of v = project_vector_sky_to_kl(m, a) does not depend on the phases of the SVD and KL
vectors, so the device's own modes reproduce it.  Stored per m: a, q of the three columns, q of column 0 as a vector,
and the noise-augmented q under each (crosspower, zero_mean) pair.
TEST INFRASTRUCTURE — never imported by the product."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as gg  # noqa: E402
from oracle import refimport  # noqa: E402


def main():
    ref = refimport.load()
    btmod, klmod, psmod = ref["beamtransfer"], ref["kltransform"], ref["psestimation"]
    g = np.load(os.path.join(gg.OUT, "svdkl_unpol.npz"))
    p = np.load(os.path.join(gg.OUT, "psfisher.npz"))
    F, B, P, lmax = int(g["F"]), int(g["B"]), int(g["P"]), int(g["lmax"])
    L = lmax + 1
    tel = gg.FakeTelescope(F, B, P, lmax, lmax, g["npower"], tsys_flat=1.0)
    tel.frequencies = g["frequencies"]
    bt = btmod.BeamTransfer("/mem/qest/bt", telescope=tel)
    bt.polsvcut, bt.svcut = float(g["polsvcut"]), float(g["svcut"])
    kl = klmod.KLTransform(bt, subdir="kl")
    kl._cvsg, kl._cvfg = g["cv_sg"], g["cv_fg"]
    kl.threshold = float(g["threshold"])
    kl.inverse = False
    import h5py as _h5  # the in-memory stand-in: let the reference's `os.path.exists` checks see its files

    class _OsShim(object):
        def __getattr__(self, name):
            return getattr(os, name)

    class _PathShim(object):
        def __getattr__(self, name):
            return getattr(os.path, name)

        @staticmethod
        def exists(path):
            return _h5.exists(path) or os.path.exists(path)

    shim = _OsShim()
    shim.path = _PathShim()
    klmod.os = shim
    psmod.os = shim
    ps = psmod.PSExact(kl, subdir="ps")
    clarray = p["clarray"]
    nbands = clarray.shape[0]
    ps.clarray = clarray
    ps.k_center = np.arange(nbands, dtype=np.float64)
    ps.bands = list(range(nbands + 1))
    rng = np.random.default_rng(20261015)
    mlist = [int(m) for m in g["mlist"]]
    out = dict(mlist=np.array(mlist), nbands=nbands)
    for mi in mlist:
        gg.write_beam_file(ref, bt, mi, g["m%d_beam_m" % mi])
        bt._generate_svdfile_m(mi)
        kl.transform_save(mi)
        a = rng.standard_normal((F, 1, L, 3)) + 1j * rng.standard_normal((F, 1, L, 3))
        a[:, :, :mi] = 0.0
        v = kl.project_vector_sky_to_kl(mi, a)
        evals, _ = kl.modes_m(mi)
        out["m%d_a" % mi] = a
        out["m%d_nmodes" % mi] = 0 if evals is None else evals.size
        out["m%d_q" % mi] = ps.q_estimator(mi, v)
        out["m%d_q1" % mi] = ps.q_estimator(mi, v[:, 0])
        for cp in (False, True):
            for zm in (False, True):
                ps.crosspower, ps.zero_mean = cp, zm
                out["m%d_qn_%d%d" % (mi, cp, zm)] = ps.q_estimator(mi, v, noise=True)
        ps.crosspower, ps.zero_mean = False, True
        print("qestimator m", mi, "modes", out["m%d_nmodes" % mi], "q[:, 0]", out["m%d_q" % mi][:, 0])
    klmod.os = os
    psmod.os = os
    np.savez_compressed(os.path.join(gg.OUT, "qestimator.npz"), **out)
    print("qestimator.npz")


if __name__ == "__main__":
    main()
