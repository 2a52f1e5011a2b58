#!/usr/bin/env python3
"""Generate tests/golden/psmc.npz: the unmodified reference's PSMonteCarlo._work_fisher_bias_m and
PSMonteCarloAlt._work_fisher_bias_m on the products of svdkl_unpol.npz with the band tables of psfisher.npz, with
recorded draws in place of the random ones.  Build machine only (needs the reference tree and oracle/_ref):

    make -C oracle ref && python tests/gen_golden_psmc.py

PSMonteCarlo.gen_sample is replaced by one returning recorded complex draws, and numpy.random.rand (the Z_2 draws of
PSMonteCarloAlt.gen_vecs) by one returning recorded uniforms.  The draws live in the reference's KL basis, so the
reference's modes are stored too: a test maps the draws into its own basis through U = E_own E_ref^H (a diagonal of
phases).  Stored per m: the reference's SVD products (temperature), modes and eigenvalues, the draws and both
estimators' (Fisher, bias).  The reference's Alt calls numpy.float, gone from numpy 2; this process aliases it.
TEST INFRASTRUCTURE — never imported by the product."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as gg  # noqa: E402
from oracle import refimport  # noqa: E402

NSAMPLES = 48


def main():
    ref = refimport.load()
    btmod, klmod, psmod = ref["beamtransfer"], ref["kltransform"], ref["psestimation"]
    if not hasattr(np, "float"):
        np.float = float   # the reference's psmc.py:124 (this process only)
    from drift.core import psmc

    g = np.load(os.path.join(gg.OUT, "svdkl_unpol.npz"))
    p = np.load(os.path.join(gg.OUT, "psfisher.npz"))
    F, B, P, lmax = int(g["F"]), int(g["B"]), int(g["P"]), int(g["lmax"])
    tel = gg.FakeTelescope(F, B, P, lmax, lmax, g["npower"], tsys_flat=1.0)
    tel.frequencies = g["frequencies"]
    bt = btmod.BeamTransfer("/mem/psmc/bt", telescope=tel)
    bt.polsvcut, bt.svcut = float(g["polsvcut"]), float(g["svcut"])
    kl = klmod.KLTransform(bt, subdir="kl")
    kl._cvsg, kl._cvfg = g["cv_sg"], g["cv_fg"]
    kl.threshold = float(g["threshold"])
    kl.inverse = False
    import h5py as _h5

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
    clarray = p["clarray"]
    nbands = clarray.shape[0]

    def setup(ps, cl):
        ps.clarray = cl
        ps.k_center = np.arange(nbands, dtype=np.float64)
        ps.bands = list(range(nbands + 1))
        ps.nsamples = NSAMPLES
        return ps

    mc = setup(psmc.PSMonteCarlo(kl, subdir="psmc"), clarray)
    alt = setup(psmc.PSMonteCarloAlt(kl, subdir="psalt"), clarray[:, np.newaxis, np.newaxis])   # (nb, 1, 1, L, F, F)
    rng = np.random.default_rng(20261016)
    mlist = [int(m) for m in g["mlist"]]
    out = dict(mlist=np.array(mlist), nbands=nbands, nsamples=NSAMPLES)
    rand0 = np.random.rand
    try:
        for mi in mlist:
            gg.write_beam_file(ref, bt, mi, g["m%d_beam_m" % mi])
            bt._generate_svdfile_m(mi)
            kl.transform_save(mi)
            evals, evecs = kl.modes_m(mi)
            n = 0 if evals is None else evals.size
            out["m%d_nmodes" % mi] = n
            out["m%d_svnum" % mi] = bt._svd_num(mi)[0]
            out["m%d_beam_svd" % mi] = bt.beam_svd(mi)[:, :, 0]   # (F, nsv, L), temperature
            if n == 0:
                continue
            out["m%d_evals" % mi] = evals
            out["m%d_evecs" % mi] = evecs
            x = (rng.standard_normal((n, NSAMPLES)) + 1j * rng.standard_normal((n, NSAMPLES))) / 2**0.5
            x *= ((evals + 1.0) ** 0.5)[:, np.newaxis]
            mc.gen_sample = lambda mi_, nsamples=None, noiseonly=False, x_=x: x_[:, :nsamples]
            f, b = mc._work_fisher_bias_m(mi)
            out["m%d_x" % mi], out["m%d_mc_fisher" % mi], out["m%d_mc_bias" % mi] = x, f, b
            u = rng.random((n, NSAMPLES))
            np.random.rand = lambda *shape, u_=u: u_.reshape(shape)
            f, b = alt._work_fisher_bias_m(mi)
            np.random.rand = rand0
            out["m%d_signs" % mi] = 2.0 * (u <= 0.5) - 1.0
            out["m%d_alt_fisher" % mi], out["m%d_alt_bias" % mi] = f, b
            print("psmc m", mi, "modes", n, "diag F mc", np.diag(out["m%d_mc_fisher" % mi]).real,
                  "alt", np.diag(out["m%d_alt_fisher" % mi]).real)
    finally:
        np.random.rand = rand0
        klmod.os = os
        psmod.os = os
    np.savez_compressed(os.path.join(gg.OUT, "psmc.npz"), **out)
    print("psmc.npz", os.path.getsize(os.path.join(gg.OUT, "psmc.npz")), "bytes")


if __name__ == "__main__":
    main()
