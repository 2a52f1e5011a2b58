"""Timestream simulation, m-mode transform and map-making on top of the GPU-backed operators.

Mirrors ``drift.pipeline.timestream`` (drift/pipeline/timestream.py:15-829): the ``Timestream`` class with the
reference's file layout (``timestream_f/<f>/timestream.hdf5``, ``mmodes/<m>/mode.hdf5``, ``svd.hdf5``,
``klmode_<name>_<thr>.hdf5``, ``klmodes_<name>_<thr>.hdf5``), ``simulate`` and the three map-makers.  These are
CONSUMERS of the per-m operators: every projection goes through
``BeamTransfer`` / ``KLTransform`` (grouped ZGEMMs on the device); the sky-map <-> a_lm transforms
(``cora.util.hputil.sphtrans_sky`` / ``sphtrans_inv_sky`` in the reference, not available here) are the
``healpix`` restatements of this package.  Ranks split frequencies and m as the reference does, but without its two
MPI transposes: timestream files are per frequency and m-mode files per m, so a rank reads the frequencies it needs.
"""
import logging
import os
import pickle
import time
from types import SimpleNamespace

import numpy as np

from . import healpix, parallel, storage, util
from .device import get_context


class Timestream(object):
    directory = None
    output_directory = None
    beamtransfer_dir = None
    no_m_zero = True
    mmode_ridge = 0.0   # Tikhonov term of the weighted m-mode estimate, relative to the mean weight
    flag_noise_bias_correct = False   # powerspectrum() subtracts the noise bias of the flags too (`flag_noise_bias`)

    def __init__(self, tsdir, prodmanager):
        self.directory = os.path.abspath(tsdir)
        self.output_directory = self.directory
        self.manager = prodmanager

    # ---- products this timestream belongs to (timestream.py:41-60) -------------------------------
    @property
    def beamtransfer(self):
        return self.manager.beamtransfer

    @property
    def telescope(self):
        return self.beamtransfer.telescope

    # ---- frequency-ordered files (timestream.py:63-100) ------------------------------------------------
    def _fdir(self, fi):
        return (self.directory + "/timestream_f/" + util.natpattern(self.telescope.nfreq)) % fi

    def _ffile(self, fi):
        return self._fdir(fi) + "/timestream.hdf5"

    @property
    def ntime(self):
        with storage.File(self._ffile(0), "r") as f:
            return int(f.attrs["ntime"])

    def timestream_f(self, fi):
        """[npairs, ntime] visibility timestream of one frequency."""
        with storage.File(self._ffile(fi), "r") as f:
            return f["timestream"][:]

    def weight_f(self, fi):
        """[npairs, ntime] float64 weights of one frequency (flags: 0), or None when the file holds no `weight`."""
        with storage.File(self._ffile(fi), "r") as f:
            return np.asarray(f["weight"][:], dtype=np.float64) if "weight" in f else None

    def is_unstacked(self):
        """Whether the files hold one row per feed pair (the attribute `unstacked`)."""
        with storage.File(self._ffile(0), "r") as f:
            return bool(f.attrs.get("unstacked", 0))

    def _refuse_unstacked(self):
        if os.path.exists(self._ffile(0)) and self.is_unstacked():
            raise ValueError("%s holds unstacked (per-feed-pair) visibilities: stack them first with "
                             "timestream.stack_baselines" % self.directory)

    def _weights_of(self, fs, ntime):
        """(len(fs), npairs, ntime) weights of the frequencies `fs` (ones for a file without the dataset) when the data
        is flagged — the file of frequency 0 holds `weight`, a choice every rank makes alike — else None."""
        if self.weight_f(0) is None:
            return None
        ones = np.ones((self.telescope.npairs, ntime), dtype=np.float64)
        return np.stack([ones if w is None else w for w in (self.weight_f(fi) for fi in fs)]) if len(fs) else \
            np.zeros((0, self.telescope.npairs, ntime), dtype=np.float64)

    def _write_weight_summary(self, local_f, kept, info, infl):
        """Kept-sample counts, solver info and the mean and the largest noise inflation over the 2 mmax + 1 modes of a
        row (all (nfreq, npairs)) of a weighted m-mode estimate, gathered from the ranks' frequencies and written once to
        mmodes/weights.hdf5.  infl: (mmax + 1, len(local_f), 2, npairs)."""
        tel = self.telescope
        per_mode = np.concatenate([infl[:, :, 0], infl[1:, :, 1]], axis=0)      # (2 mmax + 1, len(local_f), npairs)
        parts = parallel.gather_objects((list(local_f), kept, info, per_mode.mean(axis=0), per_mode.max(axis=0)))
        if parallel.rank0():
            nkept = np.zeros((tel.nfreq, tel.npairs), dtype=np.int64)
            infos = np.zeros((tel.nfreq, tel.npairs), dtype=np.int32)
            imean = np.zeros((tel.nfreq, tel.npairs), dtype=np.float64)
            imax = np.zeros((tel.nfreq, tel.npairs), dtype=np.float64)
            for fs, k, i, a, b in parts:
                if len(fs):
                    nkept[fs], infos[fs], imean[fs], imax[fs] = k, i, a, b
            os.makedirs(self.output_directory + "/mmodes", exist_ok=True)
            with storage.File(self.output_directory + "/mmodes/weights.hdf5", "w") as f:
                f.create_dataset("nkept", data=nkept)
                f.create_dataset("info", data=infos)
                f.create_dataset("inflation_mean", data=imean)
                f.create_dataset("inflation_max", data=imax)
                f.attrs["ridge"] = float(self.mmode_ridge)
                f.attrs["ntime"] = int(self.ntime)

    # ---- m-modes (timestream.py:103-185) ------------------------------------------------------------------
    def _mdir(self, mi):
        return (self.output_directory + "/mmodes/" + util.natpattern(self.telescope.mmax)) % abs(mi)

    def _mfile(self, mi):
        return self._mdir(mi) + "/mode.hdf5"

    def mmode(self, mi):
        """[nfreq, 2, npairs] visibility m-mode."""
        with storage.File(self._mfile(mi), "r") as f:
            return f["mmode"][:]

    def _inflfile(self, mi):
        return self._mdir(mi) + "/inflation.hdf5"

    def noise_inflation(self, mi):
        """[nfreq, 2, npairs] float64: the noise variance of every entry of `mmode(mi)` relative to the nominal
        `noisepower` — what the weighted estimate of flagged data wrote next to the mode file,
        ones for data without weights (which writes no such file)."""
        if not os.path.exists(self._inflfile(mi)):
            tel = self.telescope
            return np.ones((tel.nfreq, 2, tel.npairs), dtype=np.float64)
        with storage.File(self._inflfile(mi), "r") as f:
            return f["noise_inflation"][:]

    def _write_inflation(self, infl, m_of, f_of, me, nranks):
        """The noise inflation (mmax + 1, local frequencies, 2, npairs) of this rank's frequencies regrouped by m across
        the ranks exactly as the modes are, one mmodes/<m>/inflation.hdf5 per m of this rank."""
        tel = self.telescope
        got = parallel.exchange([np.ascontiguousarray(infl[m_of[r]]) for r in range(nranks)])
        mine = m_of[me]
        if mine:
            full = np.zeros((len(mine), tel.nfreq, 2, tel.npairs), dtype=np.float64)
            for src, part in enumerate(got):
                if len(f_of[src]):
                    full[:, f_of[src]] = part
            for k, mi in enumerate(mine):
                os.makedirs(self._mdir(mi), exist_ok=True)
                with storage.File(self._inflfile(mi), "w") as f:
                    f.create_dataset("noise_inflation", data=np.ascontiguousarray(full[k]))
                    f.attrs["m"] = mi

    def generate_mmodes(self):
        """FFT the timestreams along time and regroup by m: +m in slot 0, the conjugate of -m in slot 1.  When the files
        hold a dataset `weight` (flags) the modes are the weighted least-squares estimate instead (`mmodes_weighted_host`
        with `mmode_ridge`; counts, solver info and inflation summaries go to mmodes/weights.hdf5, and every m gets the
        per-mode noise inflation of the estimate in mmodes/<m>/inflation.hdf5, `noise_inflation`)."""
        marker = self.output_directory + "/mmodes/COMPLETED_M"
        if os.path.exists(marker):
            return
        self._refuse_unstacked()
        tel = self.telescope
        mmax, nfreq, ntime = tel.mmax, tel.nfreq, self.ntime
        # Each rank transforms ITS frequencies, the result is regrouped by m across ranks (the reference's MPI transpose,
        # timestream.py:150-170): no rank reads every timestream file or holds the full (nfreq, 2, npairs, mmax + 1) array.
        nranks = parallel.size() if parallel._dist() else 1
        all_m = list(range(mmax + 1))
        m_of = [parallel.partition_for(all_m, r, nranks) for r in range(nranks)]
        f_of = [parallel.partition_for(list(range(nfreq)), r, nranks) for r in range(nranks)]
        me = parallel.rank() if parallel._dist() else 0
        local_f = f_of[me]
        pairs = np.zeros((len(local_f), 2, tel.npairs, mmax + 1), dtype=np.complex128)
        weights = self._weights_of(local_f, ntime)
        if weights is not None:
            x = np.stack([self.timestream_f(fi) for fi in local_f]) if local_f else np.zeros((0, tel.npairs, ntime), complex)
            modes, info, infl = mmodes_weighted_host(x, weights, mmax, ridge=self.mmode_ridge, inflation=True)
            pairs[:] = modes.transpose(1, 2, 3, 0)
            self._write_weight_summary(local_f, np.count_nonzero(weights > 0, axis=-1), info, infl)
            self._write_inflation(infl, m_of, f_of, me, nranks)
        else:
            for k, fi in enumerate(local_f):
                row = np.fft.fft(self.timestream_f(fi), axis=-1) / ntime        # (npairs, ntime)
                pairs[k, 0, :, 0] = row[:, 0]
                pairs[k, 0, :, 1:] = row[:, 1 : mmax + 1]
                pairs[k, 1, :, 1:] = row[:, : -mmax - 1 : -1].conj()
        got = parallel.exchange([np.ascontiguousarray(pairs[..., m_of[r]]) for r in range(nranks)])
        mine = m_of[me]
        if mine:
            full = np.zeros((nfreq, 2, tel.npairs, len(mine)), dtype=np.complex128)
            for src, part in enumerate(got):
                if len(f_of[src]):
                    full[f_of[src]] = part
            for k, mi in enumerate(mine):
                os.makedirs(self._mdir(mi), exist_ok=True)
                with storage.File(self._mfile(mi), "w") as f:
                    f.create_dataset("mmode", data=np.ascontiguousarray(full[..., k]))
                    f.attrs["m"] = mi
        parallel.barrier()
        if parallel.rank0():
            open(marker, "a").close()
        parallel.barrier()

    # ---- SVD m-modes (timestream.py:191-231) ----------------------------------------------------------------
    def _svdfile(self, mi):
        return self._mdir(mi) + "/svd.hdf5"

    def mmode_svd(self, mi):
        with storage.File(self._svdfile(mi), "r") as f:
            if f["mmode_svd"].shape[0] == 0:
                return np.zeros((0,), dtype=np.complex128)
            return f["mmode_svd"][:]

    def generate_mmodes_svd(self):
        tel = self.telescope
        for mi in parallel.partition(list(range(tel.mmax + 1))):
            if os.path.exists(self._svdfile(mi)):
                continue
            tm = self.mmode(mi).reshape(tel.nfreq, 2 * tel.npairs)
            svdm = self.beamtransfer.project_vector_telescope_to_svd(mi, tm)
            with storage.File(self._svdfile(mi), "w") as f:
                f.create_dataset("mmode_svd", data=svdm)
                f.attrs["m"] = mi
        parallel.barrier()

    # ---- the batched device route: the same files, one launch per stage and batch of m ----------------------------
    def _generate_mmodes_device(self, chunk_gb):
        """`generate_mmodes` with the time -> m transform on the device (`Context.mmode_transform`: a pruned DFT as two
        strided-batched ZGEMMs against a twiddle table, written in the layout of the mode files); the regrouping across
        ranks and the files are the per-m route's.  Files with a dataset `weight` go through
        `Context.mmode_transform_weighted` and leave mmodes/weights.hdf5 and the per-m
        inflation.hdf5 files of `generate_mmodes`."""
        marker = self.output_directory + "/mmodes/COMPLETED_M"
        if os.path.exists(marker):
            return {}
        self._refuse_unstacked()
        ctx = get_context()
        tel = self.telescope
        mmax, nfreq, ntime, npairs = tel.mmax, tel.nfreq, self.ntime, tel.npairs
        nranks = parallel.size() if parallel._dist() else 1
        all_m = list(range(mmax + 1))
        m_of = [parallel.partition_for(all_m, r, nranks) for r in range(nranks)]
        f_of = [parallel.partition_for(list(range(nfreq)), r, nranks) for r in range(nranks)]
        me = parallel.rank() if parallel._dist() else 0
        local_f = f_of[me]
        pairs = np.zeros((mmax + 1, len(local_f), 2, npairs), dtype=np.complex128)
        per_f = 16 * npairs * (ntime + 2 * (mmax + 1))
        step = max(1, int(chunk_gb * (1 << 30) // max(per_f, 1)))
        weighted = self.weight_f(0) is not None
        kept, infos = [], []
        infl = np.zeros((mmax + 1, len(local_f), 2, npairs), dtype=np.float64) if weighted else None
        if weighted:   # the weights, their product with the data and the right-hand sides share the chunk
            step = max(1, int(chunk_gb * (1 << 30) // max(per_f + 16 * npairs * (2 * ntime + 4 * mmax + 2), 1)))
        for c0 in range(0, len(local_f), step):
            fs = local_f[c0 : c0 + step]
            with self._timed("read"):
                host = np.stack([np.asarray(self.timestream_f(fi), dtype=np.complex128) for fi in fs])
                wts = self._weights_of(fs, ntime) if weighted else None
            with self._timed("upload"):
                X = ctx.to_device(host)
            with self._timed("device"):
                if weighted:
                    out, info, dinf = ctx.mmode_transform_weighted(X, wts, mmax, ridge=self.mmode_ridge, inflation=True)
                    kept.append(np.count_nonzero(wts > 0, axis=-1))
                    infos.append(info.cpu().numpy())
                    infl[:, c0 : c0 + len(fs)] = dinf.cpu().numpy()
                else:
                    out = ctx.mmode_transform(X, mmax)
            with self._timed("download"):
                pairs[:, c0 : c0 + len(fs)] = ctx.to_host(out)
            del X, out
        if weighted:
            self._write_weight_summary(local_f, np.concatenate(kept) if kept else np.zeros((0, npairs), np.int64),
                                       np.concatenate(infos) if infos else np.zeros((0, npairs), np.int32), infl)
            self._write_inflation(infl, m_of, f_of, me, nranks)
        got = parallel.exchange([np.ascontiguousarray(pairs[m_of[r]]) for r in range(nranks)])
        mine = m_of[me]
        if mine:
            full = np.zeros((len(mine), nfreq, 2, npairs), dtype=np.complex128)
            for src, part in enumerate(got):
                if len(f_of[src]):
                    full[:, f_of[src]] = part
            with self._timed("write"):
                for k, mi in enumerate(mine):
                    os.makedirs(self._mdir(mi), exist_ok=True)
                    with storage.File(self._mfile(mi), "w") as f:
                        f.create_dataset("mmode", data=np.ascontiguousarray(full[k]))
                        f.attrs["m"] = mi
        parallel.barrier()
        if parallel.rank0():
            open(marker, "a").close()
        parallel.barrier()
        # what the files of this rank hold, for the SVD stage of the same call (same partition of m)
        return {mi: full[k] for k, mi in enumerate(mine)} if mine else {}

    # Opt-in log of the batched route: a dict set here collects wall seconds per kind of step ("read" product and data
    # files, "upload", "device", "upload+device" for the KL stage, whose eigenvectors go up inside the call, "download",
    # "write"), waiting for the device at every boundary.  None: no waits added.
    mode_log = None

    def _timed(self, what):
        return _StepTimer(self.mode_log, what)

    def _klfile_of(self, mi, klname, threshold):
        return self._mdir(mi) + ("/klmode_%s_%f.hdf5" % (klname, threshold))

    def _kl_entries(self, klnames):
        """[(name, threshold)] of `klnames`: names (threshold of the transform) or (name, threshold) pairs."""
        out = []
        for entry in klnames:
            name, thr = entry if isinstance(entry, (tuple, list)) else (entry, None)
            out.append((name, self.manager.kltransforms[name].threshold if thr is None else thr))
        return out

    def _m_batches(self, ms, per_m_bytes, chunk_gb):
        """`ms` cut into runs whose summed `per_m_bytes(mi)` stays within chunk_gb (at least one m per batch)."""
        return m_batches(ms, per_m_bytes, chunk_gb)

    @staticmethod
    def _write_vector(fname, dset, vec, mi):
        with storage.File(fname, "w") as f:
            f.create_dataset(dset, data=vec)
            f.attrs["m"] = mi

    def generate_modes_batched(self, klnames=(), chunk_gb=4.0):
        """`generate_mmodes`, `generate_mmodes_svd` and, for every entry of `klnames` (a name, or (name, threshold)),
        `generate_mmodes_kl` in one pass: the same files with the same datasets, written where they do not exist yet.

        The per-m methods take every (m, frequency) block through an upload, a launch and a wait of its own.  Here the
        m of this rank go through the device in batches of at most `chunk_gb` of products: `beam_ut` of a batch is
        uploaded once and applied to all its m-modes in ONE launch (`dm_blockvec_grouped`) into the packed `svbounds`
        layout; per KL name the thresholded eigenvectors of the batch are uploaded and applied in one more launch to the
        SVD vectors, which stay on the device in between.  Nothing stays resident after a batch."""
        fresh = self._generate_mmodes_device(chunk_gb)
        ctx = get_context()
        bt, tel = self.beamtransfer, self.telescope
        kls = self._kl_entries(klnames)
        todo = [mi for mi in parallel.partition(list(range(tel.mmax + 1)))
                if not os.path.exists(self._svdfile(mi))
                or any(not os.path.exists(self._klfile_of(mi, n, t)) for n, t in kls)]

        def per_m(mi):
            nd = float(bt.ndof(mi))
            return 16.0 * (tel.nfreq * bt.svd_len * bt.ntel + (nd * nd if kls else 0.0))

        for batch in self._m_batches(todo, per_m, chunk_gb):
            need = [mi for mi in batch if not os.path.exists(self._svdfile(mi))]
            made = {}
            if need:
                with self._timed("read"):
                    tm = np.stack([(fresh[mi] if mi in fresh else self.mmode(mi)).reshape(tel.nfreq, bt.ntel) for mi in need])
                    but = bt._dev_stack(need, "beam_ut") if any(int(bt.ndof(mi)) for mi in need) else None
                with self._timed("upload"):
                    dtm = ctx.to_device(tm[..., None])
                with self._timed("device"):
                    out, off = bt.project_vectors_telescope_to_svd_device(need, dtm, products=but)
                with self._timed("download"):
                    host = ctx.to_host(out)[:, 0] if out.numel() else np.zeros((0,), dtype=np.complex128)
                del out, but, dtm
                with self._timed("write"):
                    for i, mi in enumerate(need):
                        made[mi] = host[off[i] : off[i + 1]].copy()
                        self._write_vector(self._svdfile(mi), "mmode_svd", made[mi], mi)
            svec = None
            for name, thr in kls:
                want = [mi for mi in batch if not os.path.exists(self._klfile_of(mi, name, thr))]
                if not want:
                    continue
                if svec is None:   # the SVD vectors of the batch, packed, for every KL name
                    with self._timed("read"):
                        vecs = [made[mi] if mi in made else self.mmode_svd(mi) for mi in batch]
                    voff = np.concatenate([[0], np.cumsum([v.shape[0] for v in vecs])]).astype(np.int64)
                    with self._timed("upload"):
                        svec = ctx.to_device(np.concatenate(vecs + [np.zeros((1,), dtype=np.complex128)])[:, None])
                idx = [batch.index(mi) for mi in want]
                ndofs = [int(bt.ndof(mi)) for mi in want]
                for i, n in zip(idx, ndofs):
                    if n != voff[i + 1] - voff[i]:
                        raise Exception("Vectors are incompatible.")
                kl = self.manager.kltransforms[name]
                with self._timed("read"):
                    modes = [kl._read_modes(mi, thr)[1] for mi in want]
                with self._timed("upload+device"):   # (the eigenvectors go up inside the call)
                    out, kloff = kl.project_vectors_svd_to_kl_device(want, svec, off=voff[idx], threshold=thr, modes=modes)
                del modes
                with self._timed("download"):
                    host = ctx.to_host(out)[:, 0] if out.numel() else np.zeros((0,), dtype=np.complex128)
                del out
                with self._timed("write"):
                    for i, mi in enumerate(want):
                        self._write_vector(self._klfile_of(mi, name, thr), "mmode_kl", host[kloff[i] : kloff[i + 1]].copy(), mi)
            del svec
        parallel.barrier()

    # ---- map-making (timestream.py:237-300, :400-457) -----------------------------------------------------
    def _alm_to_map(self, make_alm, nside, mapname, mlist=None):
        tel = self.telescope
        mlist = list(range(tel.mmax + 1)) if mlist is None else mlist
        mine = parallel.partition(mlist)
        parts = parallel.gather_objects([(mi, make_alm(mi)) for mi in mine])
        if parallel.rank0():
            alm = np.zeros((tel.nfreq, tel.num_pol_sky, tel.lmax + 1, tel.lmax + 1), dtype=np.complex128)
            for part in parts:
                for mi, a in part:
                    alm[..., mi] = a
            skymap = healpix.sphtrans_inv_sky(alm, nside)
            with storage.File(self.output_directory + "/" + mapname, "w") as f:
                f.create_dataset("map", data=skymap)
        parallel.barrier()

    def mapmake_full(self, nside, mapname):
        self._alm_to_map(lambda mi: self.beamtransfer.project_vector_telescope_to_sky(mi, self.mmode(mi)), nside, mapname)

    def mapmake_svd(self, nside, mapname):
        self.generate_mmodes_svd()
        self._alm_to_map(lambda mi: self.beamtransfer.project_vector_svd_to_sky(mi, self.mmode_svd(mi)), nside, mapname)

    # ---- batched map-making: the a_lm stage of mapmake_svd / mapmake_kl in device batches ----------------------------
    def _alm_batches(self, mlist, vectors, chunk_gb, extra_bytes=None, on_batch=None):
        """[(m, a_lm (nfreq, npol, lmax + 1))] for the m of this rank: `vectors(batch)` gives the packed SVD vectors of a
        batch on the device (rows, 1) and their row offsets; `invbeam_svd` of the batch is uploaded once and applied in
        one launch.  With `on_batch`, every batch is handed on as `on_batch(batch, a_lm)` — the list of its m and the
        device tensor (len(batch), nfreq, npol, lmax + 1, 1) — instead of being brought to the host, and the list that
        comes back is empty."""
        ctx = get_context()
        bt, tel = self.beamtransfer, self.telescope

        def per_m(mi):
            return 16.0 * tel.nfreq * tel.num_pol_sky * (tel.lmax + 1) * bt.svd_len + (extra_bytes(mi) if extra_bytes else 0.0)

        out = []
        for batch in self._m_batches(parallel.partition(mlist), per_m, chunk_gb):
            svec, off = vectors(batch)
            dev = bt.project_vectors_svd_to_sky_device(batch, svec, off=off)
            if on_batch is not None:
                on_batch(list(batch), dev)
                continue
            alm = ctx.to_host(dev)[..., 0]
            out.extend((mi, np.ascontiguousarray(alm[i])) for i, mi in enumerate(batch))
        return out

    def _packed_device(self, vecs):
        """Vectors of a batch back to back on the device as one column, and the row offsets of every m."""
        off = np.concatenate([[0], np.cumsum([v.shape[0] for v in vecs])]).astype(np.int64)
        packed = np.concatenate(list(vecs) + [np.zeros((1,), dtype=np.complex128)])   # (never empty)
        return get_context().to_device(packed[:, None]), off

    def alm_svd_batched(self, mlist=None, chunk_gb=4.0, on_batch=None):
        """The a_lm stage of `mapmake_svd` for this rank's share of `mlist`: [(m, (nfreq, npol, lmax + 1))].  `on_batch`:
        a function (batch, device tensor (len(batch), nfreq, npol, lmax + 1, 1)) that takes every batch on the device
        instead; the list is then empty."""
        mlist = list(range(self.telescope.mmax + 1)) if mlist is None else list(mlist)
        return self._alm_batches(mlist, lambda batch: self._packed_device([self.mmode_svd(mi) for mi in batch]), chunk_gb,
                                 on_batch=on_batch)

    def alm_kl_batched(self, mlist=None, wiener=False, chunk_gb=4.0, on_batch=None):
        """The a_lm stage of `mapmake_kl` for this rank's share of `mlist` (default: all m but m = 0 under `no_m_zero`):
        KL modes, optionally Wiener weighted by lambda / (1 + lambda), through the stored inverse modes back to the SVD
        basis and through `invbeam_svd` to the sky, without leaving the device in between.  `on_batch` as in
        `alm_svd_batched`."""
        kl = self.manager.kltransforms[self.klname]
        thr = self.klthreshold
        bt = self.beamtransfer
        if mlist is None:
            mlist = list(range(1 if self.no_m_zero else 0, self.telescope.mmax + 1))

        def vectors(batch):
            modes = []
            for mi in batch:
                klmode = self.mmode_kl(mi)
                if wiener and klmode.size:
                    evals = kl.evals_m(mi, thr)
                    if evals is not None:
                        klmode = klmode * (evals / (1.0 + evals))
                modes.append(klmode)
            dev, kloff = self._packed_device(modes)
            return kl.project_vectors_kl_to_svd_device(batch, dev, kloff=kloff, threshold=thr)

        def extra(mi):
            return 16.0 * float(bt.ndof(mi)) ** 2

        return self._alm_batches(mlist, vectors, chunk_gb, extra_bytes=extra, on_batch=on_batch)

    # ---- spectra at catalogue positions ---------------------------------------------------------
    def catalogue_spectra(self, cat, source="svd", wiener=False, chunk_gb=4.0, name=None, stack=None):
        """The spectrum of the estimated sky at every position of a catalogue, and the stack of those spectra on each
        object's line: `spectra_<name>.hdf5` in the output directory; returns its path, at once if the file exists.

        The a_lm are those of `mapmake_svd_batched` (``source="svd"``) or `mapmake_kl_batched` (``source="kl"``: the KL
        transform set by `set_kltransform`, which needs `inverse`; ``wiener`` as there; m = 0 left out under
        `no_m_zero`).  Every batch of m stays on the device and goes through `skysim.alm_at_points`' kernel at the
        positions of ``cat`` (`skysim.read_positions`: arrays, a dict or a file) — no map, no nside, a source sits where
        the catalogue puts it.  A rank sums over its own m, batch after batch; the partial sums are added on rank 0 in
        rank order.  Datasets: ``spectra`` (nsrc, npol, nfreq) with polarisations T or T, Q, U, V, ``theta``, ``phi``,
        ``freq`` (MHz), ``ms_used``.  When the catalogue has ``redshift`` or ``stack`` (a dict) is given, also ``stack``
        (npol, 2 K + 1), ``hits``, ``offsets``, ``stack_weight`` and ``channel`` of `skysim.stack_spectra` with
        K = stack["halfwidth"] (default 2), lines at stack["line_mhz"] (default the 21 cm line) / (1 + redshift) and the
        optional stack["source_weight"] and stack["channel_weight"].  ``name`` defaults to the source (and the KL name)."""
        from . import skysim

        if source not in ("svd", "kl"):
            raise ValueError("catalogue_spectra: source is 'svd' or 'kl', got %r" % (source,))
        if name is None:
            name = "svd" if source == "svd" else "kl_%s" % self.klname
        fname = self.output_directory + "/spectra_%s.hdf5" % name
        if os.path.exists(fname):
            return fname
        theta, phi, red = skysim.read_positions(cat)
        if stack is not None and red is None:
            raise ValueError("catalogue_spectra: a stack needs the redshifts of the catalogue")
        conf = dict(stack or {})
        unknown = set(conf) - {"halfwidth", "line_mhz", "source_weight", "channel_weight"}
        if unknown:
            raise ValueError("catalogue_spectra: unknown stack key(s) %s" % ", ".join(sorted(unknown)))
        tel = self.telescope
        npol, nfreq = int(tel.num_pol_sky), int(tel.nfreq)
        z, sth, phr = skysim._point_arrays(theta, phi, npol)
        ctx = get_context()
        nsrc = z.size
        acc = ctx.zeros((nsrc, npol, nfreq), np.float64)
        dz, ds, dp = (ctx.to_device(z), ctx.to_device(sth), ctx.to_device(phr)) if nsrc else (None, None, None)
        L = int(tel.lmax) + 1
        used = []

        def on_batch(batch, alm):
            used.extend(int(mi) for mi in batch)
            if nsrc and len(batch):
                ctx.alm_at_points(dz, ds, dp, batch, alm, L - 1, nfreq, npol, (npol * L, L, 1, nfreq * npol * L), out=acc,
                                  accumulate=True, max_bytes=int(chunk_gb * (1 << 30)))

        if source == "svd":
            self.generate_modes_batched(chunk_gb=chunk_gb)
            self.alm_svd_batched(chunk_gb=chunk_gb, on_batch=on_batch)
        else:
            if not self.manager.kltransforms[self.klname].inverse:
                raise Exception("Need the inverse to evaluate the KL-filtered sky.")
            self.alm_kl_batched(wiener=wiener, chunk_gb=chunk_gb, on_batch=on_batch)
        parts = parallel.gather_objects((ctx.to_host(acc), used))
        if parallel.rank0():
            spectra = np.zeros((nsrc, npol, nfreq), dtype=np.float64)
            ms_used = []
            for part, ms in parts:                        # in rank order
                spectra += part
                ms_used.extend(ms)
            freq = np.asarray(tel.frequencies, dtype=np.float64)
            os.makedirs(self.output_directory, exist_ok=True)
            with storage.File(fname, "w") as f:
                f.create_dataset("spectra", data=spectra)
                f.create_dataset("theta", data=np.asarray(theta, dtype=np.float64))
                f.create_dataset("phi", data=np.asarray(phi, dtype=np.float64))
                f.create_dataset("freq", data=freq)
                f.create_dataset("ms_used", data=np.asarray(sorted(ms_used), dtype=np.int64))
                if red is not None:
                    line = float(conf.get("line_mhz", skysim.LINE_21CM_MHZ)) / (1.0 + red)
                    st = skysim.stack_spectra(spectra, freq, line, int(conf.get("halfwidth", 2)),
                                              source_weight=conf.get("source_weight"), channel_weight=conf.get("channel_weight"))
                    f.create_dataset("redshift", data=red)
                    f.create_dataset("stack", data=st["stack"])
                    f.create_dataset("hits", data=st["hits"])
                    f.create_dataset("offsets", data=st["offsets"].astype(np.int64))
                    f.create_dataset("stack_weight", data=st["weight"])
                    f.create_dataset("channel", data=st["channel"])
        parallel.barrier()
        return fname

    def _write_map(self, parts, nside, mapname):
        tel = self.telescope
        parts = parallel.gather_objects(parts)
        if parallel.rank0():
            alm = np.zeros((tel.nfreq, tel.num_pol_sky, tel.lmax + 1, tel.lmax + 1), dtype=np.complex128)
            for part in parts:
                for mi, a in part:
                    alm[..., mi] = a
            skymap = healpix.sphtrans_inv_sky(alm, nside)
            with storage.File(self.output_directory + "/" + mapname, "w") as f:
                f.create_dataset("map", data=skymap)
        parallel.barrier()

    def mapmake_svd_batched(self, nside, mapname, chunk_gb=4.0):
        """`mapmake_svd` with its a_lm stage in device batches; returns at once if the map file exists."""
        if os.path.exists(self.output_directory + "/" + mapname):
            return
        self.generate_modes_batched(chunk_gb=chunk_gb)
        self._write_map(self.alm_svd_batched(chunk_gb=chunk_gb), nside, mapname)

    def mapmake_kl_batched(self, nside, mapname, wiener=False, chunk_gb=4.0):
        """`mapmake_kl` with its a_lm stage in device batches: leaves out m = 0 under `no_m_zero`, needs a KL transform
        with `inverse`, returns at once if the map file exists."""
        if os.path.exists(self.output_directory + "/" + mapname):
            return
        if not self.manager.kltransforms[self.klname].inverse:
            raise Exception("Need the inverse to make a meaningful map.")
        self._write_map(self.alm_kl_batched(wiener=wiener, chunk_gb=chunk_gb), nside, mapname)

    # ---- KL m-modes (timestream.py:306-396) ---------------------------------------------------------------
    def set_kltransform(self, klname, threshold=None):
        self.klname = klname
        if threshold is None:
            threshold = self.manager.kltransforms[self.klname].threshold
        self.klthreshold = threshold

    def _klfile(self, mi):
        return self._mdir(mi) + ("/klmode_%s_%f.hdf5" % (self.klname, self.klthreshold))

    def mmode_kl(self, mi):
        with storage.File(self._klfile(mi), "r") as f:
            if f["mmode_kl"].shape[0] == 0:
                return np.zeros((0,), dtype=np.complex128)
            return f["mmode_kl"][:]

    def generate_mmodes_kl(self):
        kl = self.manager.kltransforms[self.klname]
        for mi in parallel.partition(list(range(self.telescope.mmax + 1))):
            if os.path.exists(self._klfile(mi)):
                continue
            klm = kl.project_vector_svd_to_kl(mi, self.mmode_svd(mi), threshold=self.klthreshold)
            with storage.File(self._klfile(mi), "w") as f:
                f.create_dataset("mmode_kl", data=klm)
                f.attrs["m"] = mi
        parallel.barrier()

    def collect_mmodes_kl(self):
        nd = self.beamtransfer.ndofmax

        def evfunc(mi):
            evf = np.zeros(nd, dtype=np.complex128)
            ev = self.mmode_kl(mi)
            if ev.size > 0:
                evf[-ev.size:] = ev
            return evf

        mine = [(mi, evfunc(mi)) for mi in parallel.partition(list(range(self.telescope.mmax + 1)))]
        parts = parallel.gather_objects(mine)
        if parallel.rank0():
            fname = self.output_directory + ("/klmodes_%s_%f.hdf5" % (self.klname, self.klthreshold))
            if os.path.exists(fname):
                return
            arr = np.zeros((self.telescope.mmax + 1, nd), dtype=np.complex128)
            for part in parts:
                for mi, ev in part:
                    arr[mi] = ev
            with storage.File(fname, "w") as f:
                f.create_dataset("evals", data=arr)

    def fake_kl_data(self):
        kl = self.manager.kltransforms[self.klname]
        for mi in parallel.partition(list(range(self.telescope.mmax + 1))):
            evals = kl.evals_m(mi)
            if evals is None:
                klmode = np.array([], dtype=np.complex128)
            else:
                modeamp = ((evals + 1.0) / 2.0) ** 0.5
                klmode = modeamp * (np.array([1.0, 1.0j]) * np.random.standard_normal((modeamp.shape[0], 2))).sum(axis=1)
            with storage.File(self._klfile(mi), "w") as f:
                f.create_dataset("mmode_kl", data=klmode)
                f.attrs["m"] = mi
        parallel.barrier()

    def mapmake_kl(self, nside, mapname, wiener=False):
        mapfile = self.output_directory + "/" + mapname
        if os.path.exists(mapfile):
            return
        kl = self.manager.kltransforms[self.klname]
        if not kl.inverse:
            raise Exception("Need the inverse to make a meaningful map.")

        def make_alm(mi):
            klmode = self.mmode_kl(mi)
            if klmode.size == 0:
                tel = self.telescope
                return np.zeros((tel.nfreq, tel.num_pol_sky, tel.lmax + 1), dtype=np.complex128)
            if wiener:
                evals = kl.evals_m(mi, self.klthreshold)
                if evals is not None:
                    klmode = klmode * (evals / (1.0 + evals))
            isvdmode = kl.project_vector_kl_to_svd(mi, klmode, threshold=self.klthreshold)
            return self.beamtransfer.project_vector_svd_to_sky(mi, isvdmode)

        mlist = list(range(1 if self.no_m_zero else 0, self.telescope.mmax + 1))
        self._alm_to_map(make_alm, nside, mapname, mlist=mlist)

    # ---- power spectrum (timestream.py:463-523) -------------------------------------------------------------------
    @property
    def _psfile(self):
        return self.output_directory + ("/ps_%s.hdf5" % self.psname)

    def set_psestimator(self, psname):
        self.psname = psname

    def _has_inflation(self):
        return any(os.path.exists(self._inflfile(mi)) for mi in range(self.telescope.mmax + 1))

    def flag_noise_bias(self, inflation=None):
        """The noise bias (nbands,) that the flags add to sum_m q_m beyond the `bias` of fisher.hdf5 (DESIGN.md section
        4.16).  The weighted m-mode estimate of flagged data is unbiased, but entry j = (frequency, slot, pair) of the
        m-mode vector carries noise of variance noisepower_j d_{m,j} instead of the nominal noisepower_j
        (`noise_inflation`), diagonal within an m.  With P_m the map the data takes, telescope -> SVD -> KL
        (`project_vectors_telescope_to_svd_device`, which whitens by noisepower^-1/2, then
        `project_vectors_svd_to_kl_device`), E[q_a(P n)] = sum_j noisepower_j d_j q_a(P e_j), so

            delta b_a = sum_m sum_j noisepower_j (d_{m,j} - 1) q_a(P_m e_j).

        The columns P_m e_j are the identity pushed through the two batched projections, in chunks under the estimator's
        `ps_chunk_gb`; their q come from `q_estimator_batch(..., noise=False)`; the weighted sum is taken on the host.
        Entries with d = 1 need no column and an m whose d are all 1 is skipped.  The m are shared over the ranks and the
        result is summed over them.  `inflation`: a function m -> (nfreq, 2, npairs) used in place of the files.

        Only the expectation of the estimate is corrected: the Fisher matrix and the error bars still assume nominal
        noise, and the correlations between different m (which do not enter the expectation of a sum of per-m quadratic
        forms) are ignored.  The band powers become unbiased, not minimum-variance."""
        ps = self.manager.psestimators[self.psname]
        had_bands = ps.clarray is not None
        if not had_bands:
            ps.genbands()
        ctx = get_context()
        kl, bt, tel = ps.kltrans, ps.kltrans.beamtransfer, self.telescope
        nfreq, ntel = int(tel.nfreq), int(bt.ntel)
        npower = bt._noisew() ** -2.0                                             # (nfreq, ntel): noisepower of entry j
        L = int(tel.lmax) + 1
        total = np.zeros(ps.nbands, dtype=np.float64)
        for mi in parallel.partition(_ps_mlist(tel.mmax, self.no_m_zero)):
            d = self.noise_inflation(mi) if inflation is None else inflation(mi)
            wj = (npower * (np.asarray(d, dtype=np.float64).reshape(nfreq, ntel) - 1.0)).ravel()
            cols = np.flatnonzero(wj)
            nd = int(bt.ndof(mi))
            if cols.size == 0 or nd == 0:
                continue
            per_col = 16.0 * (nfreq * ntel + 2 * L * nfreq + 4 * nd) + 8.0 * ps.nbands * (L / 4.0 + 1.0)
            step = int(max(1, min(cols.size, 0.5 * ps.ps_chunk_gb * (1 << 30) // per_col)))
            for c0 in range(0, cols.size, step):
                cc = cols[c0 : c0 + step]
                eye = ctx.zeros((1, nfreq * ntel, len(cc)), np.complex128)
                eye[0, ctx.to_device(cc), ctx.to_device(np.arange(len(cc)))] = 1.0
                svec, off = bt.project_vectors_telescope_to_svd_device([mi], eye.view(1, nfreq, ntel, len(cc)))
                kvec, _ = kl.project_vectors_svd_to_kl_device([mi], svec, off=off[:1])
                del eye, svec
                if kvec.shape[0] == 0:
                    break
                q = ps.q_estimator_batch([mi], [kvec], noise=False)[0]            # (nbands, len(cc))
                total += q[: ps.nbands] @ wj[cc]
        if not had_bands:
            ps.delbands()
        return parallel.allreduce_sum(total)

    def powerspectrum(self):
        """Band powers p = F^-1 (sum_m q_m - bias) of this timestream's KL m-modes, written to `ps_<psname>.hdf5`.

        With `flag_noise_bias_correct` (default False; the key of the same name in a `timestreams:` entry of the
        pipeline file) and inflation files next to the modes, `bias + flag_noise_bias()` is subtracted and the file gets
        `flag_bias` (nbands).  The Fisher matrix and the errors written still assume nominal noise."""
        if os.path.exists(self._psfile):
            return None
        ps = self.manager.psestimators[self.psname]
        ps.genbands()
        mine = parallel.partition(_ps_mlist(self.telescope.mmax, self.no_m_zero))
        qs = ps.q_estimator_batch(mine, [self.mmode_kl(mi) for mi in mine])
        qtotal = parallel.allreduce_sum(np.sum(qs, axis=0) if qs else np.zeros(ps.nbands))
        fisher, bias = ps.fisher_bias()
        flag_bias = None
        if self.flag_noise_bias_correct and self._has_inflation():
            flag_bias = self.flag_noise_bias()
            bias = bias + flag_bias
        powerspectrum = np.dot(np.linalg.inv(fisher), qtotal - bias)
        if parallel.rank0():
            _write_ps(self._psfile, fisher, ps.band_power, powerspectrum, flag_bias=flag_bias)
        ps.delbands()
        parallel.barrier()
        return powerspectrum

    # ---- persistence (timestream.py:525-566) -----------------------------------------------------------------
    def __getstate__(self):
        # The reference pickles its ProductManager along with the object; the manager here owns device buffers, so the
        # pickle carries the directory of the products instead and `load` re-opens them (config.yaml is written there
        # by ProductManager.from_config, manager.py:134-162).
        state = {k: v for k, v in self.__dict__.items() if not k.startswith("_") and k != "manager"}
        state["manager_directory"] = getattr(self.manager, "directory", self.manager)
        return state

    def __setstate__(self, state):
        from . import manager as _manager

        mdir = state.pop("manager_directory", None)
        self.__dict__.update(state)
        self.manager = _manager.ProductManager.from_config(mdir) if isinstance(mdir, str) else mdir

    @property
    def _picklefile(self):
        return self.output_directory + "/timestreamobject.pickle"

    def save(self):
        if parallel.rank0():
            with open(self._picklefile, "wb") as f:
                pickle.dump(self, f)

    @classmethod
    def load(cls, tsdir):
        with open(cls(tsdir, tsdir)._picklefile, "rb") as f:
            return pickle.load(f)


class _StepTimer(object):
    """`with` block whose wall time (device idle at both ends) is added to log[what]; a no-op without a log."""

    def __init__(self, log, what):
        self.log, self.what = log, what

    def __enter__(self):
        if self.log is not None:
            get_context().sync()
            self.t0 = time.perf_counter()

    def __exit__(self, *exc):
        if self.log is not None:
            get_context().sync()
            self.log[self.what] = self.log.get(self.what, 0.0) + time.perf_counter() - self.t0
        return False


# ---- m-modes of flagged timestreams: the host statement -------------------------------------
def mmodes_weighted_host(x, w, mmax, ridge=0.0, inflation=False):
    """Weighted least-squares m-modes in numpy, the oracle of `Context.mmode_transform_weighted`: x (nf, npairs, ntime)
    complex, w >= 0 broadcastable to it from (nf, npairs, ntime), (nf, ntime) or (ntime,).  Per (frequency, pair) the normal
    equations A a = b are built from the explicit Fourier matrix F[t, k] = e^{2 pi i k t / ntime}, k = -mmax .. mmax,
    A = F^H diag(w) F / ntime + ridge mean(w) I, b = F^H (w x) / ntime, and solved with a dense solver (LAPACK's LU: not
    the device's algorithm).  Returns (modes (mmax + 1, nf, 2, npairs) in the layout of the mode files, info (nf, npairs)
    int32: 0 solved, -1 fewer than 2 mmax + 1 samples of weight > 0 with ridge = 0, or none at all — not solved, zeros).

    inflation=True: a third value, float64 (mmax + 1, nf, 2, npairs) in the layout of the modes, the diagonal of the dense
    inverse `np.linalg.inv(A)` at k = +m (slot 0) and k = -m (slot 1): with circular white noise of per-sample variance
    ntime * noisepower on the data, noisepower times it is the noise variance of the mode (exact for ridge = 0, an upper
    bound for ridge > 0).  1.0 at (m = 0, slot 1); exactly 1 / w_0 on a row of constant weight w_0 with ridge = 0 (as the
    device, whose shortcut this restates); 0.0 on rows that are not solved."""
    x = np.asarray(x, dtype=np.complex128)
    if x.ndim != 3:
        raise ValueError("mmodes_weighted_host: x (nf, npairs, ntime) expected")
    nf, npairs, ntime = x.shape
    mmax, ridge = int(mmax), float(ridge)
    N = 2 * mmax + 1
    w = np.asarray(w, dtype=np.float64)
    if w.shape not in ((nf, npairs, ntime), (nf, ntime), (ntime,)):
        raise ValueError("mmodes_weighted_host: weights %s do not fit x %s" % (w.shape, x.shape))
    if w.size and not np.all(np.isfinite(w) & (w >= 0)):
        raise ValueError("mmodes_weighted_host: weights must be finite and not negative")
    if mmax < 0 or ntime < N or not (ridge >= 0.0 and np.isfinite(ridge)):
        raise ValueError("mmodes_weighted_host: %d time samples cannot hold m up to %d, or a bad ridge" % (ntime, mmax))
    w = np.broadcast_to(w[:, None, :] if w.ndim == 2 else w, x.shape)
    k = np.arange(-mmax, mmax + 1)
    F = np.exp(2j * np.pi * ((np.arange(ntime)[:, None] * k[None, :]) % ntime) / ntime)       # (ntime, N)
    modes = np.zeros((mmax + 1, nf, 2, npairs), dtype=np.complex128)
    info = np.zeros((nf, npairs), dtype=np.int32)
    infl = np.zeros((mmax + 1, nf, 2, npairs), dtype=np.float64)
    infl[0, :, 1] = 1.0
    for fi in range(nf):
        for p in range(npairs):
            wr = w[fi, p]
            if np.count_nonzero(wr > 0) < (N if ridge == 0.0 else 1):     # (the ridge is relative to mean(w): 0 of 0)
                info[fi, p] = -1
                continue
            A = (F.conj().T * wr[None, :]) @ F / ntime + ridge * wr.mean() * np.eye(N)
            a = np.linalg.solve(A, F.conj().T @ (wr * x[fi, p]) / ntime)
            modes[:, fi, 0, p] = a[mmax:]
            modes[1:, fi, 1, p] = a[:mmax][::-1].conj()
            if inflation:
                if wr.min() == wr.max():                                  # A = w_0 (1 + ridge) I exactly
                    d = np.full(N, 1.0 / (wr[0] + ridge * wr[0]))
                else:
                    d = np.linalg.inv(A).diagonal().real
                infl[:, fi, 0, p] = d[mmax:]
                infl[1:, fi, 1, p] = d[:mmax][::-1]
    return (modes, info, infl) if inflation else (modes, info)


def toeplitz_inverse_diag_host(col):
    """The diagonal of the inverse of a Hermitian positive-definite Toeplitz matrix as `dm_toeplitz_solve_diag` computes
    it, restated in numpy (not its summation order): the recursion of `toeplitz_levinson_host` for f and beta, then the
    Gohberg-Semencul prefix sum d_i = sum_{j <= i} (|f_j|^2 - |f_{n-j}|^2) / (beta c_0), f_n := 0.  col (n,) or (batch, n).
    Returns (d float64 of col's shape, info int32 per system: 0, the failing step k, or n for c_0 <= 0; d = 0 on failure)."""
    col = np.asarray(col, dtype=np.complex128)
    single = col.ndim == 1
    cols = col[None] if single else col
    batch, n = cols.shape
    ds = np.zeros((batch, n), dtype=np.float64)
    info = np.zeros(batch, dtype=np.int32)
    for s in range(batch):
        c0 = cols[s, 0].real
        if not (c0 > 0 and np.isfinite(c0)):
            info[s] = n
            continue
        r = cols[s] / c0
        r[0] = 1.0
        f = np.zeros(n, dtype=np.complex128)
        f[0] = 1.0
        beta = 1.0
        for k in range(1, n):
            gamma = -np.dot(r[k:0:-1], f[:k]) / beta
            f[: k + 1] = f[: k + 1] + gamma * f[k::-1].conj()
            beta *= 1.0 - abs(gamma) ** 2
            if not (beta > 0 and np.isfinite(beta)):
                info[s] = k
                break
        if info[s]:
            continue
        p = f.real**2 + f.imag**2
        g = p.copy()
        g[1:] -= p[:0:-1]                                        # |f_{n-i}|^2, i = 1 .. n - 1
        ds[s] = np.cumsum(g) / (beta * c0)
    return (ds[0], info[0]) if single else (ds, info)


def toeplitz_levinson_host(col, b):
    """The recursion of `dm_toeplitz_solve` restated in numpy (not its summation order): col (n,) or (batch, n) first
    columns of Hermitian Toeplitz systems, b (n,), (nrhs, n) or (batch, nrhs, n) right-hand sides.  Returns (x of b's
    shape, info int32 per system): 0 solved, k the step at which beta <= 0 or not finite, n for c_0 <= 0; the solutions of a
    failed system are zeros."""
    col = np.asarray(col, dtype=np.complex128)
    b = np.asarray(b, dtype=np.complex128)
    single = col.ndim == 1
    cols = col[None] if single else col
    batch, n = cols.shape
    bs = b.reshape(batch, -1, n)
    xs = np.zeros_like(bs)
    info = np.zeros(batch, dtype=np.int32)
    for s in range(batch):
        c0 = cols[s, 0].real
        if not (c0 > 0 and np.isfinite(c0)):
            info[s] = n
            continue
        r = cols[s] / c0
        r[0] = 1.0
        bp = bs[s] / c0
        f = np.zeros(n, dtype=np.complex128)
        f[0] = 1.0
        x = np.zeros_like(bp)
        x[:, 0] = bp[:, 0]
        beta = 1.0
        for k in range(1, n):
            rev = r[k:0:-1]                                  # r_{k-i}, i = 0 .. k - 1
            gamma = -np.dot(rev, f[:k]) / beta
            f[: k + 1] = f[: k + 1] + gamma * f[k::-1].conj()        # (f_k is 0 before the step)
            beta *= 1.0 - abs(gamma) ** 2
            if not (beta > 0 and np.isfinite(beta)):
                info[s] = k
                x[:] = 0
                break
            coef = (bp[:, k] - x[:, :k] @ rev) / beta
            x[:, : k + 1] += coef[:, None] * f[k::-1].conj()[None, :]   # conj(f_{k-i}), i = 0 .. k
        xs[s] = x
    return xs.reshape(b.shape), (info[0] if single else info)


def m_batches(ms, per_m_bytes, chunk_gb):
    """`ms` cut into runs whose summed `per_m_bytes(mi)` stays within chunk_gb (at least one m per batch)."""
    budget = chunk_gb * (1 << 30)
    out, cur, used = [], [], 0.0
    for mi in ms:
        need = float(per_m_bytes(mi))
        if cur and used + need > budget:
            out.append(cur)
            cur, used = [], 0.0
        cur.append(mi)
        used += need
    if cur:
        out.append(cur)
    return out


def _ps_mlist(mmax, no_m_zero):
    return list(range(1 if no_m_zero else 0, mmax + 1))


def _write_ps(psfile, fisher, band_power, powerspectrum, flag_bias=None):
    cv = np.linalg.inv(fisher)
    err = cv.diagonal() ** 0.5
    with storage.File(psfile, "w") as f:
        f.create_dataset("fisher", data=fisher)
        f.create_dataset("covariance", data=cv)
        f.create_dataset("error", data=err)
        f.create_dataset("correlation", data=cv / np.outer(err, err))
        f.create_dataset("bandpower", data=band_power)
        f.create_dataset("powerspectrum", data=powerspectrum)
        if flag_bias is not None:
            f.create_dataset("flag_bias", data=flag_bias)


def cross_powerspectrum(timestreams, psname, psfile):
    """Cross band powers (nstream, nstream, nbands) of every pair of timestreams (timestream.py:570-642): the pairs
    ti < tj are estimated and mirrored, the diagonal stays zero.  Every pair of an m is a column of one q call."""
    if os.path.exists(psfile):
        return None
    products = timestreams[0].manager
    ps = products.psestimators[psname]
    ps.genbands()
    nstream = len(timestreams)
    pairs = [(ti, tj) for ti in range(nstream) for tj in range(ti + 1, nstream)]
    mine = parallel.partition(_ps_mlist(products.telescope.mmax, timestreams[0].no_m_zero))
    qloc = np.zeros((nstream, nstream, ps.nbands), dtype=np.float64)
    if pairs and mine:
        xs, ys = [], []
        for mi in mine:
            data = [ts.mmode_kl(mi) for ts in timestreams]
            xs.append(np.stack([data[ti] for ti, _ in pairs], axis=1))
            ys.append(np.stack([data[tj] for _, tj in pairs], axis=1))
        for q in ps.q_estimator_batch(mine, xs, ys):   # (nbands, npairs)
            for k, (ti, tj) in enumerate(pairs):
                qloc[ti, tj] += q[:, k]
                qloc[tj, ti] += q[:, k]
    qtotal = parallel.allreduce_sum(qloc)
    fisher, bias = ps.fisher_bias()
    qtotal = (qtotal - bias).reshape(nstream**2, ps.nbands).T
    powerspectrum = np.dot(np.linalg.inv(fisher), qtotal).T.reshape(nstream, nstream, ps.nbands)
    if parallel.rank0():
        _write_ps(psfile, fisher, ps.band_power, powerspectrum)
    ps.delbands()
    parallel.barrier()
    return powerspectrum


def _sky_covariance(m, model, klname):
    """[pol, pol, l, freq, freq] of `model` ("signal" / "foreground"): that of KL transform `klname` of the products
    (the first one by default), or the committed model for the telescope when the products hold no KL transform."""
    from . import skymodel

    if model not in ("signal", "foreground"):
        raise ValueError("skymodels: 'signal' or 'foreground', not %r" % (model,))
    kls = getattr(m, "kltransforms", None) or {}
    if klname is not None and klname not in kls:
        raise ValueError("klname %r is not a KL transform of these products" % (klname,))
    if kls:
        kl = kls[klname] if klname is not None else next(iter(kls.values()))
        return kl.signal() if model == "signal" else kl.foreground()
    tel = m.beamtransfer.telescope
    make = skymodel.im21cm_model if model == "signal" else skymodel.foreground_model
    return make(tel.lmax, tel.frequencies, tel.num_pol_sky)


def _as_sources(sources):
    return (sources,) if isinstance(sources, (str, bytes, dict)) else tuple(sources)


def _sources_alm(sources, tel, freqs, to_host):
    """Sum of the exact a_lm (len(freqs), num_pol_sky, lmax + 1, mmax + 1) of the point-source catalogues `sources`
    (`skysim.source_alm`) at the telescope's frequencies `freqs`; a device tensor with to_host=False.  An unpolarised
    telescope takes I alone, an unpolarised catalogue has zero Q, U, V."""
    from . import skysim

    npol = int(tel.num_pol_sky)
    total = None
    for cat in sources:
        cat = skysim.read_catalogue(cat)
        flux = skysim.source_spectra(cat, np.asarray(tel.frequencies, dtype=np.float64)[list(freqs)])
        if npol == 1:
            flux = flux[:, :1]
        elif flux.shape[1] == 1:
            flux = np.concatenate([flux, np.zeros((flux.shape[0], 3, flux.shape[2]))], axis=1)
        a = skysim.source_alm((cat["theta"], cat["phi"], flux), int(tel.lmax), mmax=int(tel.mmax), to_host=to_host)
        if a.shape[1] != npol:
            a = a[:, :npol] if to_host else a[:, :npol].contiguous()
        total = a if total is None else total + a
    return total


def simulate(m, outdir, maps=(), ndays=None, resolution=0, seed=None, skymodels=(), klname=None, sky_seed=0,
             sky_realisation=0, sources=(), gains=None, weights=None, **kwargs):
    """Simulated timestream of the telescope of ProductManager `m` (timestream.py:645-829).

    maps: list of files holding a dataset `map` [freq, pol, pixel] whose sum is the sky; ndays = 0: no noise;
    resolution = 0: 2 mmax + 1 time samples.  skymodels: any of "signal", "foreground" — a Gaussian realisation
    (`sky_seed`, `sky_realisation`) of that covariance of KL transform `klname` is drawn on the device (`skysim.draw_alm`,
    every rank the rows of its own frequencies) and its a_lm are added to those of the maps.  sources: point-source
    catalogues (dicts or files, `skysim.read_catalogue`) whose exact a_lm (`skysim.source_alm`) are added too.

    gains: per-feed gain errors — a `skysim.GainModel`, a dict of its arguments (the YAML
    `gains:` mapping) or an explicit complex128 array (nf, nfeed, ntime) / (1, nf, nfeed, ntime) over the
    telescope's frequencies (every rank takes the rows of its own).  A model is evaluated for realisation `sky_realisation` (`skysim.gains_host`).  The time stream of the
    sky is multiplied by the stacked baseline gain G (`skysim.baseline_gains_host` on `redundant_pairs()`), all in numpy;
    the noise is transformed by itself and added after: gains multiply the sky part only and the noise level is
    unchanged.  With gains=None nothing of this runs.

    weights: flags — a `skysim.FlagModel`, a dict of its arguments (the YAML `weights:` mapping)
    or a float64 array >= 0 of shape (nfreq, npairs, ntime), (nfreq, ntime) or (ntime,) over the telescope's frequencies.
    Samples of weight 0 are set to exactly 0 after sky, gains and noise, and every frequency file gets the dataset
    `weight` (npairs, ntime), from which `generate_mmodes` / `generate_modes_batched` take the weighted estimate of the
    m-modes.  With weights=None nothing of this runs.  Returns the Timestream."""
    bt = m.beamtransfer
    tel = bt.telescope
    lmax, mmax, nfreq, npol = tel.lmax, tel.mmax, tel.nfreq, tel.num_pol_sky
    if ndays is None:
        ndays = tel.ndays
    ntime = _sim_ntime(tel, resolution)
    nranks = parallel.size() if parallel._dist() else 1
    me = parallel.rank() if parallel._dist() else 0
    local_freq = _sim_freqs(tel, None)
    lfreq = len(local_freq)
    col_vis = np.zeros((tel.npairs, lfreq, ntime), dtype=np.complex128)

    skymodels, sources = _as_models(skymodels), _as_sources(sources)
    if len(maps) > 0 or len(skymodels) > 0 or len(sources) > 0:
        # The reference's two MPI transposes (timestream.py:700-760): every rank transforms the maps of ITS frequencies,
        # the a_lm are regrouped by m, every rank projects ITS m through the beam (all frequencies of an m in one grouped
        # product on the device), and the visibilities come back regrouped by frequency.
        m_of = [parallel.partition_for(list(range(mmax + 1)), r, nranks) for r in range(nranks)]
        f_of = [parallel.partition_for(list(range(nfreq)), r, nranks) for r in range(nranks)]
        skymap = _read_maps(maps, local_freq)
        alm_loc = (healpix.sphtrans_sky(skymap, lmax) if lfreq and len(maps) > 0 else
                   np.zeros((lfreq, npol, lmax + 1, lmax + 1), dtype=np.complex128))   # (lfreq, npol, L, L): [l, m]
        for model in skymodels:
            from . import skysim

            stream = skysim.STREAM_SKY_SIGNAL if model == "signal" else skysim.STREAM_SKY_FOREGROUND
            cv = _sky_covariance(m, model, klname)
            if lfreq:   # straight to a_lm (no map in between), only the m the telescope measures
                alm_loc[..., : mmax + 1] += skysim.draw_alm(cv, 1, sky_seed, stream, sky_realisation, mmax, local_freq)[0]
        if lfreq and len(sources) > 0:
            alm_loc[..., : mmax + 1] += _sources_alm(sources, tel, local_freq, True)
        got = parallel.exchange([np.ascontiguousarray(alm_loc[..., m_of[r]]) for r in range(nranks)])
        my_m = m_of[me]
        alm_m = np.zeros((nfreq, npol, lmax + 1, len(my_m)), dtype=np.complex128)
        for src, part in enumerate(got):
            if len(f_of[src]):
                alm_m[f_of[src]] = part
        vis_m = np.zeros((len(my_m), nfreq, 2, tel.npairs), dtype=np.complex128)
        for k, mi in enumerate(my_m):
            vis_m[k] = bt.project_vector_sky_to_telescope(mi, np.ascontiguousarray(alm_m[..., k])).reshape(nfreq, 2, tel.npairs)
        back = parallel.exchange([np.ascontiguousarray(vis_m[:, f_of[r]]) for r in range(nranks)])
        for src, part in enumerate(back):
            for k, mi in enumerate(m_of[src]):
                vis = part[k]                                  # (lfreq, 2, npairs)
                if mi == 0:
                    col_vis[..., 0] = vis[:, 0].T
                else:
                    col_vis[..., mi] = vis[:, 0].T
                    col_vis[..., -mi] = vis[:, 1].T.conj()   # conjugate only, not (-1)^m (timestream.py:759-761)

    if ndays > 0 and lfreq > 0:
        noise_ps = _noisepower(tel, local_freq, ndays).T[:, :, np.newaxis]
        if seed is not None:
            np.random.seed(seed + parallel.rank())   # ranks must not share a noise realisation
        noise_vis = (np.array([1.0, 1.0j]) * np.random.standard_normal(col_vis.shape + (2,))).sum(axis=-1)
        noise_vis *= (noise_ps / 2.0) ** 0.5
        if seed is not None:
            np.random.seed()
        if gains is None:
            col_vis += noise_vis
    else:
        noise_vis = None

    vis_stream = np.fft.ifft(col_vis, axis=-1) * ntime
    gain_f = None
    if gains is not None:
        from . import skysim

        gains = skysim.as_gains(gains)
        if isinstance(gains, skysim.GainModel):
            gain_f = skysim.gains_host(gains, tel.nfeed, local_freq, ntime, 1, first=int(sky_realisation))[0]
        else:
            if hasattr(gains, "data_ptr"):
                gains = gains.cpu().numpy()
            gain_f = skysim.explicit_gains(gains, 1, nfreq, 0, 1, list(local_freq), tel.nfeed, ntime)[0]
        if lfreq:
            vis_stream = vis_stream * skysim.baseline_gains_host(gain_f, *tel.redundant_pairs()).transpose(1, 0, 2)
        if noise_vis is not None:
            vis_stream = vis_stream + np.fft.ifft(noise_vis, axis=-1) * ntime
    weight_f = None
    if weights is not None:
        from . import skysim

        w = skysim.as_weights(weights, nfreq, tel.npairs, ntime, range(nfreq))
        weight_f = np.broadcast_to(w[local_freq] if w.ndim == 3 else w, (lfreq, tel.npairs, ntime))
        vis_stream = np.where(weight_f.transpose(1, 0, 2) == 0, 0.0, vis_stream)
    tphi = np.linspace(0, 2 * np.pi, ntime, endpoint=False)
    tstream = Timestream(outdir, m)
    for lfi, fi in enumerate(local_freq):
        _write_sim_file(tstream, fi, vis_stream[:, lfi], tphi, gain=None if gain_f is None else gain_f[lfi],
                        weight=None if weight_f is None else weight_f[lfi])
    parallel.barrier()
    tstream.save()
    parallel.barrier()
    return tstream


# ---- ensembles of simulated timestreams on the device -------------------------------------------
# Opt-in log of `simulate_visibilities` / `simulate_ensemble`: a dict set here collects wall seconds per kind of step
# ("sky": map transforms, covariance roots and a_lm draws; "beam": reading and uploading beam blocks; "project"; "noise";
# "synthesis"; "gains": drawing the feed gains and applying them; "download"; "write"), waiting for the device at every
# boundary.  None: no waits added.
sim_log = None


def _sim_freqs(tel, freqs):
    if freqs is None:
        nranks = parallel.size() if parallel._dist() else 1
        me = parallel.rank() if parallel._dist() else 0
        return parallel.partition_for(list(range(tel.nfreq)), me, nranks)
    freqs = [int(f) for f in freqs]
    if sorted(set(freqs)) != freqs or (freqs and not 0 <= freqs[0] <= freqs[-1] < tel.nfreq):
        raise ValueError("freqs must be sorted, distinct frequency indices")
    return freqs


def _sim_ntime(tel, resolution):
    return 2 * tel.mmax + 1 if resolution == 0 else int(np.round(24 * 3600.0 / resolution))


def _as_models(skymodels):
    return (skymodels,) if isinstance(skymodels, str) else tuple(skymodels)


def _read_maps(maps, freqs):
    """Sum of the datasets `map` [freq, pol, pixel] of the files `maps` at the sorted frequencies `freqs`; None when
    either is empty."""
    skymap = None
    for mapfile in maps if len(freqs) else ():
        with storage.File(mapfile, "r") as f:
            part = f["map"][freqs[0] : freqs[-1] + 1][[fi - freqs[0] for fi in freqs]]
        skymap = part if skymap is None else skymap + part
    return skymap


def _noisepower(tel, freqs, ndays):
    """`tel.noisepower` of every unique pair at the frequencies `freqs`: (nf, npairs) float64."""
    npairs = int(tel.npairs)
    return np.asarray(tel.noisepower(np.arange(npairs)[np.newaxis, :], np.array(freqs)[:, np.newaxis], ndays=ndays),
                      dtype=np.float64).reshape(len(freqs), npairs)


def _sim_conf(m, freqs, resolution, ndays, default_ndays=None, **given):
    """The arguments of the device simulators checked once.  `given`: nreal, first, seed, sky_seed, klname, maps,
    skymodels, sources, gains and chunk_gb of the caller, all of them.  Fields: m, bt and tel; freqs, the sorted rows
    (None: this rank's share); ntime; ndays, with `default_ndays` (None: the telescope's) for None; nreal, first, seed,
    sky_seed, klname and chunk_gb; maps, skymodels and sources as tuples, and have_sky; gains after `skysim.as_gains`;
    the class table (class_off, members), nfeed, npairs and nmem; rmax, the realisations of a full group.

    Refused here, before any work: `freqs` that are not sorted indices, ntime < 2 mmax + 1, and explicit gains of another
    shape than the call's.  The names in `skymodels` and `klname` are refused by `_sky_covariance`, which the sky
    preparation (`_sim_sky`) calls first for every model."""
    from . import skysim
    from ._lib import BLOCKVEC_MAX_R

    c = SimpleNamespace(m=m, bt=m.beamtransfer, tel=m.beamtransfer.telescope, **given)
    c.freqs = _sim_freqs(c.tel, freqs)
    c.ntime = _sim_ntime(c.tel, resolution)
    if c.ntime < 2 * int(c.tel.mmax) + 1:
        raise ValueError("%d time samples cannot hold m up to %d" % (c.ntime, int(c.tel.mmax)))
    c.ndays = ndays if ndays is not None else c.tel.ndays if default_ndays is None else default_ndays
    c.nreal, c.first = int(c.nreal), int(c.first)
    c.maps, c.skymodels, c.sources = tuple(c.maps), _as_models(c.skymodels), _as_sources(c.sources)
    c.have_sky = len(c.maps) > 0 or len(c.skymodels) > 0 or len(c.sources) > 0
    c.class_off, c.members = c.tel.redundant_pairs()
    c.nfeed, c.npairs, c.nmem = int(c.tel.nfeed), int(c.tel.npairs), int(c.class_off[-1])
    c.rmax = min(BLOCKVEC_MAX_R, c.nreal)
    c.gains = skysim.as_gains(c.gains)
    if c.gains is not None and not isinstance(c.gains, skysim.GainModel) and len(c.freqs) and c.nreal > 0:
        skysim.check_explicit_gains(c.gains, c.nreal, len(c.freqs), c.nfeed, c.ntime)   # before any work
    return c


def _sim_weights(c, weights, nrow, ntime=None):
    """`weights` of the simulators as a host array broadcastable to (nf, nrow, ntime) over the rows `c.freqs` (ntime=None:
    c.ntime): a FlagModel is evaluated for their global frequency indices, an array has one row per entry."""
    if weights is None:
        return None
    from . import skysim

    return skysim.as_weights(weights, len(c.freqs), nrow, c.ntime if ntime is None else ntime, c.freqs)


def _sim_flagged(weights, f0, f1):
    """The samples of weight 0 of the rows f0:f1 of `weights` (`_sim_weights`) as a device mask, or None."""
    if weights is None:
        return None
    wf = weights[f0:f1] if np.ndim(weights) == 3 else weights
    return get_context().to_device(np.ascontiguousarray(wf == 0))


def _sim_sigma(c, freqs, members=False, ndays=None, ntime=None):
    """The noise level on the host, sigma[f, p] = sqrt(ntime noisepower(p, f, ndays)) (nf, npairs); with `members`
    sigma[f, m] = sqrt(n_c ntime noisepower(c, f, ndays)) (nf, nmem): the plain mean of a complete class then has the
    noise level of the stacked simulators.  ndays, ntime: c's, or those given (`simulate_days`: samples per turn)."""
    ntime = c.ntime if ntime is None else ntime
    noise_ps = _noisepower(c.tel, freqs, c.ndays if ndays is None else ndays)
    if not members:
        return np.sqrt(ntime * noise_ps)
    n = np.diff(c.class_off)
    return np.repeat(np.sqrt(n[np.newaxis, :] * ntime * noise_ps), n, axis=1)


def _sim_sky(c, freqs):
    """Sky preparation for the rows `freqs`: fixed, the a_lm (nf, npol, lmax + 1, mmax + 1) of maps and sources on the
    device (or None); models, (covariance, stream, roots) of every sky model; batches, the m whose beam blocks fit
    `chunk_gb` together.  None without a sky."""
    if not c.have_sky:
        return None
    from . import skysim

    ctx = get_context()
    lmax, mmax = int(c.tel.lmax), int(c.tel.mmax)
    fixed, models = None, []
    with _StepTimer(sim_log, "sky"):
        if len(c.maps) > 0:
            alm = healpix.sphtrans_sky(_read_maps(c.maps, freqs), lmax)            # (nf, npol, L, L): [l, m]
            fixed = ctx.to_device(np.ascontiguousarray(alm[..., : mmax + 1]))
        if len(c.sources) > 0:   # fixed like the maps, and never on the host
            a = _sources_alm(c.sources, c.tel, freqs, False)
            fixed = a if fixed is None else fixed.add_(a)
        for model in c.skymodels:
            stream = skysim.STREAM_SKY_SIGNAL if model == "signal" else skysim.STREAM_SKY_FOREGROUND
            cv = _sky_covariance(c.m, model, c.klname)
            models.append((cv, stream, skysim.covariance_roots(cv)))
    batches = m_batches(list(range(mmax + 1)), lambda mi: 16.0 * len(freqs) * c.bt.ntel * c.bt.nsky, c.chunk_gb)
    return SimpleNamespace(fixed=fixed, models=models, batches=batches)


def _sim_group_sky(c, freqs, sky, r0, out, accumulate):
    """The sky (`_sim_sky` of `freqs`) of the realisations first + r0 .. first + r0 + R - 1 into `out` (R, nf, npairs,
    ntime), adding to it with `accumulate`: the a_lm are drawn, the fixed ones added, projected batch by batch
    (`BeamTransfer.project_vectors_sky_to_telescope_device`) and synthesised (`Context.mmode_synthesis`)."""
    from . import skysim

    ctx, bt, log = get_context(), c.bt, sim_log
    lmax, mmax, npol, nf, R = int(c.tel.lmax), int(c.tel.mmax), int(c.tel.num_pol_sky), len(freqs), int(out.shape[0])
    with _StepTimer(log, "sky"):
        alm = ctx.zeros((R, nf, npol, lmax + 1, mmax + 1), np.complex128) if not sky.models else None
        for cv, stream, roots in sky.models:
            a = skysim.draw_alm(cv, R, c.sky_seed, stream, c.first + r0, mmax, freqs, to_host=False, roots=roots)
            alm = a if alm is None else alm.add_(a)
        if sky.fixed is not None:
            alm.add_(sky.fixed[None])
        alm_m = alm.permute(4, 1, 2, 3, 0).contiguous()                # (m, nf, npol, L, R)
        del alm
    vis = ctx.empty((mmax + 1, nf, bt.ntel, R), np.complex128)
    for batch in sky.batches:
        with _StepTimer(log, "beam"):
            beam = bt._device_beam_blocks_of(batch, freqs)
        with _StepTimer(log, "project"):
            vis[batch[0] : batch[-1] + 1] = bt.project_vectors_sky_to_telescope_device(
                batch, alm_m[batch[0] : batch[-1] + 1], freqs=freqs, products=beam)
        del beam
    del alm_m
    with _StepTimer(log, "synthesis"):
        cols = vis.view(mmax + 1, nf, 2, c.npairs, R)
        for r in range(R):
            ctx.mmode_synthesis(cols[..., r], c.ntime, out=out[r], accumulate=accumulate)


def _sim_gain_chunk(c, freqs, f0, f1, r0, R):
    """The gains (1 or R, f1 - f0, nfeed, ntime) of the rows f0:f1 of `freqs` for realisations first + r0 ..
    first + r0 + R - 1 on the device: the model's (`skysim.gains_device`) or the rows of the explicit array."""
    from . import skysim

    if isinstance(c.gains, skysim.GainModel):
        return skysim.gains_device(c.gains, c.nfeed, freqs[f0:f1], c.ntime, R, c.first + r0)
    g = skysim.explicit_gains(c.gains, c.nreal, len(freqs), r0, R, range(f0, f1), c.nfeed, c.ntime)
    return g.contiguous() if hasattr(g, "data_ptr") else get_context().to_device(np.ascontiguousarray(g))


def _visibility_groups(c, freqs, out=None, gain_sink=None, weights=None, noise=True):
    """The passes of `simulate_visibilities` over the rows `freqs` of the run `c` (`_sim_conf`): yields (r0, device tensor
    (R, nf, npairs, ntime)) for the realisations first + r0 .. first + r0 + R - 1, R <= BLOCKVEC_MAX_R.  With `out`
    (nreal, nf, npairs, ntime) the groups are views of it; without, ONE buffer is used for every group (the caller is
    done with a group when it asks for the next).  noise=False: as with ndays = 0.

    With gains the sky of a group is synthesised into a scratch buffer of the group's size and reaches the result
    through `Context.ts_gain_apply` (adding to the noise when there is any).  The gains g (1 or R, nfc, nfeed, ntime) are
    made for chunks of nfc frequencies at a time (`skysim.gains_device`, which needs three buffers of that size) so that
    they fit in `chunk_gb` together with the scratch buffer — one frequency at the least; `gain_sink(r0, f0, g)` is
    called with every chunk.  `weights`: a host array broadcastable to (nf, npairs, ntime) (`_sim_weights`); the samples
    of weight 0 of every group are set to exactly 0, last of all."""
    from ._lib import BLOCKVEC_MAX_R

    ctx, log, nf = get_context(), sim_log, len(freqs)
    if nf == 0 or c.nreal <= 0:
        return
    if c.gains is not None:
        scratch_bytes = 16.0 * c.rmax * nf * c.npairs * c.ntime
        per_freq = 3 * 16.0 * c.rmax * c.nfeed * c.ntime
        nfc = int(min(nf, max(1, (c.chunk_gb * 2.0**30 - scratch_bytes) // per_freq)))
    flagged = _sim_flagged(weights, 0, nf)
    sigma = ctx.to_device(_sim_sigma(c, freqs)) if noise and c.ndays > 0 else None
    sky = _sim_sky(c, freqs)
    buf = skybuf = None
    for r0 in range(0, c.nreal, BLOCKVEC_MAX_R):
        R = min(BLOCKVEC_MAX_R, c.nreal - r0)
        if out is None and buf is None:
            buf = ctx.empty((c.rmax, nf, c.npairs, c.ntime), np.complex128)
        grp = buf[:R] if out is None else out[r0 : r0 + R]
        if sigma is not None:
            with _StepTimer(log, "noise"):
                ctx.ts_noise(sigma, freqs, c.ntime, R, c.seed, c.first + r0, out=grp)
        elif sky is None:
            grp.zero_()
        if sky is not None and c.gains is None:
            _sim_group_sky(c, freqs, sky, r0, grp, sigma is not None)
        elif sky is not None:
            if skybuf is None:
                skybuf = ctx.empty((c.rmax, nf, c.npairs, c.ntime), np.complex128)
            _sim_group_sky(c, freqs, sky, r0, skybuf[:R], False)
        if c.gains is not None and (sky is not None or gain_sink is not None):
            with _StepTimer(log, "gains"):
                for f0 in range(0, nf, nfc):
                    f1 = min(nf, f0 + nfc)
                    g = _sim_gain_chunk(c, freqs, f0, f1, r0, R)
                    if sky is not None:
                        ctx.ts_gain_apply(g, c.class_off, c.members, skybuf[:R, f0:f1], out=grp[:, f0:f1],
                                          accumulate=sigma is not None)
                    if gain_sink is not None:
                        gain_sink(r0, f0, g)
                    del g
        if flagged is not None:
            grp.masked_fill_(flagged, 0.0)
        yield r0, grp


def _real_dtype(dtype):
    return np.zeros(0, dtype=dtype).real.dtype


def vis_expand_host(sky, class_off, members, g=None, out=None, accumulate=False, dtype=np.complex128):
    """`Context.vis_expand` in numpy, computed in `dtype` (np.clongdouble for the tests): the statement
    V[..., m, t] (+)= g[..., i, t] conj(g[..., j, t]) sky[..., c(m), t] of DESIGN.md section 4.17 for member m = (i, j) of
    class c(m); sky [..., npairs, ntime], g [..., nfeed, ntime] broadcastable against it or None (ones)."""
    class_off = np.asarray(class_off, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    n = np.diff(class_off)
    if class_off[0] != 0 or np.any(n <= 0) or class_off[-1] != members.shape[0]:
        raise ValueError("vis_expand_host: class offsets must start at 0, ascend strictly and end at len(members)")
    cls = np.repeat(np.arange(n.shape[0]), n)
    v = np.asarray(sky).astype(dtype)[..., cls, :]
    if g is not None:
        gl = np.asarray(g).astype(dtype)
        v = gl[..., members[:, 0], :] * gl[..., members[:, 1], :].conj() * v
    if accumulate:
        v = np.asarray(out).astype(dtype) + v
    return v


def vis_stack_host(vis, class_off, members, w=None, g=None, feed_weight=None, dtype=np.complex128):
    """`Context.vis_stack` in numpy, computed in `dtype`: (out, wout) [..., npairs, ntime] of the statement of DESIGN.md
    section 4.17,

        N_c = sum_{m in c} w_m conj(g_i) g_j V_m,  D_c = sum_{m in c} w_m |g_i|^2 |g_j|^2,  out = N / D,  wout = D / n_c

    with w_m = w[..., m, t] feed_weight[i] feed_weight[j] (each factor 1 when not given) and both results 0 where
    D == 0.  The members of a class are added in the table's order."""
    class_off = np.asarray(class_off, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    n = np.diff(class_off)
    if class_off[0] != 0 or np.any(n <= 0) or class_off[-1] != members.shape[0]:
        raise ValueError("vis_stack_host: class offsets must start at 0, ascend strictly and end at len(members)")
    real = _real_dtype(dtype)
    i, j = members[:, 0], members[:, 1]
    num = np.asarray(vis).astype(dtype)
    den = np.ones(num.shape, dtype=real)
    if g is not None:
        gl = np.asarray(g).astype(dtype)
        gi, gj = gl[..., i, :], gl[..., j, :]
        num = gi.conj() * gj * num
        den = den * ((gi.real**2 + gi.imag**2) * (gj.real**2 + gj.imag**2))
    if w is not None:
        wl = np.broadcast_to(np.asarray(w).astype(real), den.shape)
        num, den = wl * num, wl * den
    if feed_weight is not None:
        fw = np.asarray(feed_weight).astype(real)
        fac = (fw[i] * fw[j])[:, None]
        num, den = fac * num, fac * den
    N = np.add.reduceat(num, class_off[:-1], axis=-2)
    D = np.add.reduceat(den, class_off[:-1], axis=-2)
    some = D > 0
    out = np.where(some, N / np.where(some, D, 1), 0).astype(dtype)
    wout = np.where(some, D / n[:, None].astype(real), 0).astype(real)
    return out, wout


def redcal_weights(class_off, members, nfeed, feed_weight=None):
    """(yfac, gfac) float64 (nmem) of the redundant-calibration solver: yfac = fw_i fw_j, 0 for
    an autocorrelation — the member factor of the y step; gfac = yfac, 0 on every member of a class with fewer than two
    members of yfac > 0 — the factor of the gain step and of chi^2.  A function of the table and the feed weights."""
    class_off = np.asarray(class_off, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    n = np.diff(class_off)
    if class_off[0] != 0 or np.any(n <= 0) or class_off[-1] != members.shape[0]:
        raise ValueError("redcal: class offsets must start at 0, ascend strictly and end at len(members)")
    fw = np.ones(nfeed, dtype=np.float64) if feed_weight is None else np.asarray(feed_weight, dtype=np.float64)
    if fw.shape != (nfeed,) or (members.size and members.max() >= nfeed) or np.any(fw < 0):
        raise ValueError("redcal: feed_weight (nfeed) >= 0 and feed indices below nfeed expected")
    i, j = members[:, 0], members[:, 1]
    yfac = np.where(i != j, fw[i] * fw[j], 0.0)
    live = np.add.reduceat((yfac > 0).astype(np.int64), class_off[:-1])
    gfac = np.where(np.repeat(live, n) >= 2, yfac, 0.0)
    return yfac, gfac


def redcal_step_host(vis, class_off, members, g, w=None, feed_weight=None, damping=0.4, dtype=np.complex128):
    """One iteration of `Context.redcal_solve` in numpy, computed in `dtype`: (g_new, y, step) of the statement of
    DESIGN.md section 4.18 from the gains g [..., nfeed, ntime] —

        y_c  = sum_{m in c} omega' conj(g_i) g_j V_m / sum_{m in c} omega' |g_i|^2 |g_j|^2        (0 where the denominator is 0)
        gh_a = [sum_{m=(a,j)} omega V_m g_j conj(y_c) + sum_{m=(i,a)} omega conj(V_m) g_i y_c]
               / [sum_{m=(a,j)} omega |g_j|^2 |y_c|^2 + sum_{m=(i,a)} omega |g_i|^2 |y_c|^2]       (g_a where the denominator is 0)
        g_new = (1 - damping) g + damping gh,   step = max_a |g_new_a - g_a| / |g_a|  [..., ntime]

    with omega' = w yfac and omega = w gfac of `redcal_weights`.  The y line is `vis_stack_host` with those weights."""
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    real = _real_dtype(dtype)
    gl = np.asarray(g).astype(dtype)
    nfeed = gl.shape[-2]
    yfac, gfac = redcal_weights(class_off, members, nfeed, feed_weight)
    n = np.diff(np.asarray(class_off, dtype=np.int64))
    cls = np.repeat(np.arange(n.shape[0]), n)
    wy = yfac[:, None].astype(real) if w is None else np.asarray(w).astype(real) * yfac[:, None].astype(real)
    y, _ = vis_stack_host(vis, class_off, members, w=wy, g=gl, dtype=dtype)
    use = np.nonzero(gfac > 0)[0]
    i, j = members[use, 0], members[use, 1]
    v = np.asarray(vis).astype(dtype)[..., use, :]
    om = np.broadcast_to(gfac[use, None].astype(real), v.shape)
    if w is not None:
        om = om * np.broadcast_to(np.asarray(w).astype(real), np.shape(vis))[..., use, :]
    gb = np.broadcast_to(gl, v.shape[:-2] + gl.shape[-2:])
    gi, gj, yc = gb[..., i, :], gb[..., j, :], y[..., cls[use], :]
    ay2 = yc.real**2 + yc.imag**2
    num = np.zeros((nfeed,) + v.shape[:-2] + v.shape[-1:], dtype=dtype)
    den = np.zeros(num.shape, dtype=real)
    first = lambda x: np.moveaxis(x, -2, 0)
    np.add.at(num, i, first(om * (v * gj * yc.conj())))
    np.add.at(num, j, first(om * (v.conj() * gi * yc)))
    np.add.at(den, i, first(om * ((gj.real**2 + gj.imag**2) * ay2)))
    np.add.at(den, j, first(om * ((gi.real**2 + gi.imag**2) * ay2)))
    num, den = np.moveaxis(num, 0, -2), np.moveaxis(den, 0, -2)
    some = den > 0
    gh = np.where(some, num / np.where(some, den, 1), gb)
    gn = ((1 - real.type(damping)) * gb + real.type(damping) * gh).astype(dtype)
    gn = np.where(some, gn, gb)
    d = np.abs(gn - gb)
    step = np.where(d == 0, 0, d / np.where(d == 0, 1, np.abs(gb))).max(axis=-2)
    return gn, y, step


def redcal_solve_host(vis, class_off, members, w=None, feed_weight=None, g0=None, damping=0.4, tol=1e-10, maxiter=500,
                      dtype=np.complex128, nfeed=None):
    """`Context.redcal_solve` in numpy, computed in `dtype`: (g, y, info) with info = dict(iters, step, chi2), each
    [..., ntime].  A sample freezes after the first iteration whose step is below tol (its y is then computed once more
    from its final g); one that reaches maxiter with step >= tol keeps the y of its last iteration."""
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    real = _real_dtype(dtype)
    vl = np.asarray(vis).astype(dtype)
    if g0 is None:
        nfeed = (int(members.max()) + 1 if members.size else 0) if nfeed is None else nfeed
        if feed_weight is not None:
            nfeed = len(feed_weight)
        g = np.ones(vl.shape[:-2] + (nfeed, vl.shape[-1]), dtype=dtype)
    else:
        g = np.array(np.broadcast_to(np.asarray(g0).astype(dtype), vl.shape[:-2] + np.shape(g0)[-2:]))
    if not (0 < damping <= 1) or not (tol >= 0 and np.isfinite(tol)) or maxiter < 1:
        raise ValueError("redcal_solve_host: damping in (0, 1], tol >= 0 and finite, maxiter >= 1 expected")
    sshape = vl.shape[:-2] + vl.shape[-1:]
    active = np.ones(sshape, dtype=bool)
    iters = np.zeros(sshape, dtype=np.int32)
    step = np.zeros(sshape, dtype=real)
    y = None
    for k in range(1, maxiter + 1):
        gn, yk, st = redcal_step_host(vl, class_off, members, g, w=w, feed_weight=feed_weight, damping=damping, dtype=dtype)
        a = active[..., None, :]
        y = yk if y is None else np.where(a, yk, y)
        g = np.where(a, gn, g)
        step = np.where(active, st, step)
        iters[active] = k
        active = active & ~(st < tol)
        if not active.any():
            break
    done = ~active
    if done.any():
        _, yk, _ = redcal_step_host(vl, class_off, members, g, w=w, feed_weight=feed_weight, damping=damping, dtype=dtype)
        y = np.where(done[..., None, :], yk, y)
    return g, y, dict(iters=iters, step=step, chi2=redcal_chi2_host(vl, class_off, members, g, y, w=w, feed_weight=feed_weight,
                                                                   dtype=dtype))


def redcal_chi2_host(vis, class_off, members, g, y, w=None, feed_weight=None, dtype=np.complex128):
    """chi^2 = sum_m omega_m |V_m - g_i conj(g_j) y_c|^2 [..., ntime] in `dtype`, omega = w gfac of `redcal_weights`."""
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    real = _real_dtype(dtype)
    gl = np.asarray(g).astype(dtype)
    _, gfac = redcal_weights(class_off, members, gl.shape[-2], feed_weight)
    res = np.asarray(vis).astype(dtype) - vis_expand_host(y, class_off, members, g=gl, dtype=dtype)
    om = gfac[:, None].astype(real)
    if w is not None:
        om = om * np.asarray(w).astype(real)
    return (om * (res.real**2 + res.imag**2)).sum(axis=-2)


def redcal_degeneracies(class_off, members, nfeed, feed_weight=None):
    """(D_amp, D_ph): orthonormal bases (nfeed, k) of the gain transformations chi^2 of the redundant calibration cannot
    see: ln |g_a| -> ln |g_a| + eta_a with eta_i + eta_j constant on every class, and
    arg g_a -> arg g_a + psi_a with psi_i - psi_j constant on every class — the null spaces of the integer matrices with one
    row per constrained member (gfac > 0 of `redcal_weights`) beyond the first of its class, e_i + e_j - e_i0 - e_j0 and
    e_i - e_j - e_i0 + e_j0.  The nfeed x nfeed Gram matrices are accumulated from the four non-zeros of each row; kept
    are the eigenvectors of `numpy.linalg.eigh` whose eigenvalue is at most 1e-9 of the largest."""
    class_off = np.asarray(class_off, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    _, gfac = redcal_weights(class_off, members, nfeed, feed_weight)
    n = np.diff(class_off)
    cls = np.repeat(np.arange(n.shape[0]), n)
    use = np.nonzero(gfac > 0)[0]
    head = np.full(n.shape[0], -1, dtype=np.int64)
    head[cls[use][::-1]] = use[::-1]                                        # the first constrained member of every class
    rest = use[use != head[cls[use]]]
    idx = np.concatenate([members[rest], members[head[cls[rest]]]], axis=1)  # (rows, 4): i, j, i0, j0
    bases = []
    for sign in (np.array([1.0, 1.0, -1.0, -1.0]), np.array([1.0, -1.0, -1.0, 1.0])):
        gram = np.zeros((nfeed, nfeed))
        np.add.at(gram, (idx[:, :, None], idx[:, None, :]), np.broadcast_to(np.outer(sign, sign), (idx.shape[0], 4, 4)))
        lam, vec = np.linalg.eigh(gram)
        bases.append(np.ascontiguousarray(vec[:, lam <= 1e-9 * max(lam.max(), 0.0)]) if nfeed else np.zeros((0, 0)))
    return bases[0], bases[1]


def fix_degeneracies(g, y, class_off, members, ref=None, feed_weight=None, bases=None):
    """Take out of the solved gains g [..., nfeed, ntime] what the redundancy cannot determine, per sample: from
    ln(g / ref) the projection of its real part on D_amp and of its imaginary part on D_ph (`redcal_degeneracies`, or
    `bases` = (D_amp, D_ph)) is removed; ref (broadcastable against g) defaults to ones.  y_c [..., npairs, ntime] is
    multiplied by the inverse factor of one weighted member of its class, so that every g_i conj(g_j) y_c is unchanged.
    Returns (g, y) complex128.  The phase part assumes |arg(g / ref)| < pi.  Numpy on the host: not a kernel."""
    class_off = np.asarray(class_off, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    g = np.asarray(g, dtype=np.complex128)
    y = np.asarray(y, dtype=np.complex128)
    nfeed = g.shape[-2]
    d_amp, d_ph = redcal_degeneracies(class_off, members, nfeed, feed_weight) if bases is None else bases
    ratio = g if ref is None else g / np.broadcast_to(np.asarray(ref, dtype=np.complex128), g.shape)
    la, lp = np.log(np.abs(ratio)), np.angle(ratio)
    pa = np.einsum("ab,cb,...ct->...at", d_amp, d_amp, la)
    pp = np.einsum("ab,cb,...ct->...at", d_ph, d_ph, lp)
    h = np.exp(-(pa + 1j * pp))                                             # g_new = h g
    yfac, _ = redcal_weights(class_off, members, nfeed, feed_weight)
    n = np.diff(class_off)
    cls = np.repeat(np.arange(n.shape[0]), n)
    use = np.nonzero(yfac > 0)[0]
    head = np.full(n.shape[0], -1, dtype=np.int64)
    head[cls[use][::-1]] = use[::-1]
    has = head >= 0
    fac = np.ones(y.shape, dtype=np.complex128)
    fac[..., has, :] = h[..., members[head[has], 0], :] * h[..., members[head[has], 1], :].conj()
    return h * g, y / fac


def modelcal_weights(class_off, members, nfeed, feed_weight=None):
    """The member factor fw_i fw_j float64 (nmem) of the sky-model calibration, 0 for an
    autocorrelation: `yfac` of `redcal_weights`.  The "fewer than two members" exclusion does not apply: against a given
    model a class of one member constrains its two feeds."""
    return redcal_weights(class_off, members, nfeed, feed_weight)[0]


def _modelcal_nint(ntime, interval):
    if int(interval) < 1:
        raise ValueError("modelcal: interval must be at least 1")
    return -(-int(ntime) // int(interval))


def _modelcal_sums(vis, model, class_off, members, g, interval, w, feed_weight, dtype):
    """(g, num, den) [..., nfeed, nint] in `dtype`: numerator and denominator of the gain line of section 4.21 at the
    gains g, summed over the incidences of every feed and the samples of every interval."""
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    real = _real_dtype(dtype)
    gl = np.asarray(g).astype(dtype)
    vl = np.asarray(vis).astype(dtype)
    nfeed, ntime = gl.shape[-2], vl.shape[-1]
    if gl.shape[-1] != _modelcal_nint(ntime, interval):
        raise ValueError("modelcal: g has %d intervals, %d samples of interval %d make %d"
                         % (gl.shape[-1], ntime, interval, _modelcal_nint(ntime, interval)))
    fac = modelcal_weights(class_off, members, nfeed, feed_weight)
    n = np.diff(np.asarray(class_off, dtype=np.int64))
    cls = np.repeat(np.arange(n.shape[0]), n)
    use = np.nonzero(fac > 0)[0]
    i, j = members[use, 0], members[use, 1]
    v = vl[..., use, :]
    om = np.broadcast_to(fac[use, None].astype(real), v.shape)
    if w is not None:
        om = om * np.broadcast_to(np.asarray(w).astype(real), vl.shape)[..., use, :]
    gb = np.broadcast_to(gl, v.shape[:-2] + gl.shape[-2:])
    gs = gb[..., np.arange(ntime) // int(interval)]                         # every sample takes its interval's gain
    ml = np.asarray(model).astype(dtype)
    mc = np.broadcast_to(ml, v.shape[:-2] + ml.shape[-2:])[..., cls[use], :]
    gi, gj = gs[..., i, :], gs[..., j, :]
    am2 = mc.real**2 + mc.imag**2
    num = np.zeros((nfeed,) + gb.shape[:-2] + gb.shape[-1:], dtype=dtype)
    den = np.zeros(num.shape, dtype=real)
    starts = np.arange(0, ntime, int(interval))
    if ntime and use.size:                                                  # the samples of an interval first, then the feeds
        first = lambda x: np.moveaxis(np.add.reduceat(x, starts, axis=-1), -2, 0)
        np.add.at(num, i, first(om * (v * gj * mc.conj())))
        np.add.at(num, j, first(om * (v.conj() * gi * mc)))
        np.add.at(den, i, first(om * ((gj.real**2 + gj.imag**2) * am2)))
        np.add.at(den, j, first(om * ((gi.real**2 + gi.imag**2) * am2)))
    return gb, np.moveaxis(num, 0, -2), np.moveaxis(den, 0, -2)


def modelcal_step_host(vis, model, class_off, members, g, interval, w=None, feed_weight=None, damping=0.5,
                       dtype=np.complex128):
    """One iteration of `Context.modelcal_solve` in numpy, computed in `dtype`: (g_new, step, den) of the statement of
    DESIGN.md section 4.21 from the gains g [..., nfeed, nint] —

        gh_a = [sum_t sum_{m=(a,j)} omega V_m g_j conj(M_c) + sum_t sum_{m=(i,a)} omega conj(V_m) g_i M_c]
               / [sum_t sum_{m=(a,j)} omega |g_j|^2 |M_c|^2 + sum_t sum_{m=(i,a)} omega |g_i|^2 |M_c|^2]   (g_a where it is 0)
        g_new = (1 - damping) g + damping gh,   step = max_a |g_new_a - g_a| / |g_a|  [..., nint]

    with omega = w `modelcal_weights`, t over the samples q L <= t < min((q + 1) L, ntime) of interval q, vis [..., nmem,
    ntime] and the stacked model [..., npairs, ntime] broadcastable against it.  den [..., nfeed, nint] is the denominator
    at g: `gweight` of the solver when g is its result."""
    real = _real_dtype(dtype)
    gb, num, den = _modelcal_sums(vis, model, class_off, members, g, interval, w, feed_weight, dtype)
    some = den > 0
    gh = np.where(some, num / np.where(some, den, 1), gb)
    gn = ((1 - real.type(damping)) * gb + real.type(damping) * gh).astype(dtype)
    gn = np.where(some, gn, gb)
    d = np.abs(gn - gb)
    step = np.where(d == 0, 0, d / np.where(d == 0, 1, np.abs(gb)))
    step = step.max(axis=-2) if step.shape[-2] else np.zeros(step.shape[:-2] + step.shape[-1:], dtype=real)
    return gn, step, den


def modelcal_chi2_host(vis, model, class_off, members, g, interval, w=None, feed_weight=None, dtype=np.complex128):
    """chi^2 = sum_{t in q} sum_m omega_m |V_m - g_i conj(g_j) M_c|^2 [..., nint] in `dtype`, omega = w
    `modelcal_weights`, g [..., nfeed, nint]."""
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    real = _real_dtype(dtype)
    gl = np.asarray(g).astype(dtype)
    vl = np.asarray(vis).astype(dtype)
    ntime = vl.shape[-1]
    fac = modelcal_weights(class_off, members, gl.shape[-2], feed_weight)
    gs = gl[..., np.arange(ntime) // int(interval)]
    res = vl - vis_expand_host(model, class_off, members, g=gs, dtype=dtype)
    om = fac[:, None].astype(real)
    if w is not None:
        om = om * np.asarray(w).astype(real)
    per = (om * (res.real**2 + res.imag**2)).sum(axis=-2)
    return np.add.reduceat(per, np.arange(0, ntime, int(interval)), axis=-1) if ntime else per


def modelcal_solve_host(vis, model, class_off, members, interval, w=None, feed_weight=None, g0=None, active=None,
                        damping=0.5, tol=1e-10, maxiter=500, dtype=np.complex128, nfeed=None):
    """`Context.modelcal_solve` in numpy, computed in `dtype`: (g, info) with g [..., nfeed, nint] and info =
    dict(iters, step, chi2 [..., nint], gweight [..., nfeed, nint]).  An interval freezes after the first iteration whose
    step is below tol; one that reaches maxiter with step >= tol reports iters = maxiter.  active [nf, nint] (or
    broadcastable against [..., nint]): an interval whose entry is 0 keeps g0 and reports 0 throughout."""
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    real = _real_dtype(dtype)
    vl = np.asarray(vis).astype(dtype)
    nint = _modelcal_nint(vl.shape[-1], interval)
    if g0 is None:
        nfeed = (int(members.max()) + 1 if members.size else 0) if nfeed is None else nfeed
        if feed_weight is not None:
            nfeed = len(feed_weight)
        g = np.ones(vl.shape[:-2] + (nfeed, nint), dtype=dtype)
    else:
        g = np.array(np.broadcast_to(np.asarray(g0).astype(dtype), vl.shape[:-2] + np.shape(g0)[-2:]))
    if not (0 < damping <= 1) or not (tol >= 0 and np.isfinite(tol)) or maxiter < 1:
        raise ValueError("modelcal_solve_host: damping in (0, 1], tol >= 0 and finite, maxiter >= 1 expected")
    sshape = vl.shape[:-2] + (nint,)
    asked = np.ones(sshape, dtype=bool) if active is None else np.array(np.broadcast_to(np.asarray(active) != 0, sshape))
    live = asked.copy()
    iters = np.zeros(sshape, dtype=np.int32)
    step = np.zeros(sshape, dtype=real)
    for k in range(1, maxiter + 1):
        if not live.any():
            break
        gn, st, _ = modelcal_step_host(vl, model, class_off, members, g, interval, w=w, feed_weight=feed_weight,
                                       damping=damping, dtype=dtype)
        g = np.where(live[..., None, :], gn, g)
        step = np.where(live, st, step)
        iters[live] = k
        live = live & ~(st < tol)
    _, _, den = _modelcal_sums(vl, model, class_off, members, g, interval, w, feed_weight, dtype)
    chi2 = modelcal_chi2_host(vl, model, class_off, members, g, interval, w=w, feed_weight=feed_weight, dtype=dtype)
    return g, dict(iters=iters, step=step, chi2=np.where(asked, chi2, 0), gweight=np.where(asked[..., None, :], den, 0))


def modelcal_components(class_off, members, nfeed, model_power, feed_weight=None, edge_floor=1e-6):
    """Labels (nfeed) int64 of the connected components of the feed graph a model connects: the
    edges are the members of `modelcal_weights` > 0 whose class has model_power[c] = sum_t |M_c|^2 of the interval of at
    least edge_floor times the largest class (and above 0).  A fixed model leaves one free phase per component: an
    unpolarised source on a polarised array has no XY model, so the X and the Y feeds are two components.  The labels
    count the components from 0 in the order of their first feed; a feed no edge reaches is a component of its own."""
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    power = np.asarray(model_power, dtype=np.float64)
    n = np.diff(np.asarray(class_off, dtype=np.int64))
    if power.shape != n.shape:
        raise ValueError("modelcal_components: model_power (npairs,) expected")
    fac = modelcal_weights(class_off, members, nfeed, feed_weight)
    top = power.max() if power.size else 0.0
    keep = np.repeat((power >= edge_floor * top) & (power > 0), n) & (fac > 0)
    root = np.arange(nfeed)

    def find(a):
        while root[a] != a:
            root[a] = root[root[a]]
            a = root[a]
        return a

    for i, j in members[keep]:
        ri, rj = find(i), find(j)
        if ri != rj:
            root[max(ri, rj)] = min(ri, rj)
    heads = np.array([find(a) for a in range(nfeed)], dtype=np.int64)
    return np.unique(heads, return_inverse=True)[1].astype(np.int64).reshape(nfeed)


def modelcal_fix_phase(g, components, ref=None, feed_weight=None):
    """Remove the only freedom a fixed model leaves in the gains g [..., nfeed, nint]: per interval and component
    (`modelcal_components`: labels (nfeed,), or an array broadcastable against g when they differ between intervals) g is
    rotated so that sum_a fw_a g_a conj(ref_a) over the component is real and positive; ref (broadcastable against g)
    defaults to ones.  A component whose sum is 0 is left alone.  Every g_i conj(g_j) inside a component is unchanged.
    Returns complex128.  Numpy on the host: not a kernel."""
    g = np.asarray(g, dtype=np.complex128)
    nfeed = g.shape[-2]
    comp = np.asarray(components, dtype=np.int64)
    comp = np.broadcast_to(comp[:, None] if comp.ndim == 1 else comp, g.shape)
    fw = np.ones(nfeed) if feed_weight is None else np.asarray(feed_weight, dtype=np.float64)
    r = np.ones(g.shape, dtype=np.complex128) if ref is None else np.broadcast_to(np.asarray(ref, dtype=np.complex128), g.shape)
    prod = fw[:, None] * g * r.conj()
    out = g.copy()
    for label in np.unique(comp):
        mask = comp == label
        s = np.where(mask, prod, 0).sum(axis=-2, keepdims=True)
        mag = np.abs(s)
        rot = np.where(mag > 0, s.conj() / np.where(mag > 0, mag, 1), 1.0)
        out = np.where(mask, g * rot, out)
    return out


def modelcal_spread(g, valid, interval, ntime):
    """Interval gains g (nfeed, nint) spread over their samples: (gains (nfeed, ntime) complex128, found).  Sample t takes
    the gain of interval t // interval; an interval that is not `valid` (nint) takes the gain of the nearest valid one, the
    earlier on a tie.  Where no interval is valid the gains are all ones and `found` is False."""
    g = np.asarray(g, dtype=np.complex128)
    valid = np.asarray(valid, dtype=bool)
    nint = _modelcal_nint(ntime, interval)
    if g.ndim != 2 or g.shape[1] != nint or valid.shape != (nint,):
        raise ValueError("modelcal_spread: g (nfeed, nint) and valid (nint) expected, nint = %d" % nint)
    good = np.nonzero(valid)[0]
    if good.size == 0:
        return np.ones((g.shape[0], int(ntime)), dtype=np.complex128), False
    src = good[np.abs(np.arange(nint)[:, None] - good[None, :]).argmin(axis=1)]   # argmin: the first, so the earlier
    return np.ascontiguousarray(g[:, src[np.arange(int(ntime)) // int(interval)]]), True


def _unstacked_chunks(c, freqs, out=None, want_gains=False, weights=None, noise=True):
    """The passes of the unstacked simulators over the rows `freqs` of the run `c` (`_sim_conf`):
    yields (r0, f0, device tensor (R, nfc, nmem, ntime), g) for realisations first + r0 .. first + r0 + R - 1
    (R <= BLOCKVEC_MAX_R) and the frequencies freqs[f0 : f0 + nfc]; g is the gain chunk (1 or R, nfc, nfeed, ntime) when
    `want_gains`, else None.  With `out` (nreal, nf, nmem, ntime) the chunks are views of it; without, ONE buffer serves
    every chunk.  noise=False: as with ndays = 0.

    Per chunk of frequencies the stacked sky of a group is made as in `_visibility_groups` (`_sim_sky`,
    `_sim_group_sky`: no noise, gains or flags on it), the noise is drawn at the per-member level (`Context.ts_noise` with
    npairs := nmem, sigma of `_sim_sigma`) and the sky is spread over the members with the gains on it
    (`Context.vis_expand`, adding to the noise).  nfc is chosen so that the unstacked chunk, the stacked sky and the
    three gain buffers of `skysim.gains_device` fit in `chunk_gb`, one frequency at the least.  Every draw is counter
    based, so the chunking changes which calls make a row, not its distribution or, for the noise, its bits."""
    from ._lib import BLOCKVEC_MAX_R

    ctx, log, nf = get_context(), sim_log, len(freqs)
    if nf == 0 or c.nreal <= 0:
        return
    per_freq = 16.0 * c.rmax * c.ntime * (c.nmem + c.npairs + (3 * c.nfeed if c.gains is not None else 0))
    nfc = int(min(nf, max(1, c.chunk_gb * 2.0**30 // per_freq)))
    buf = None
    for f0 in range(0, nf, nfc):
        f1 = min(nf, f0 + nfc)
        fs = freqs[f0:f1]
        sigma = ctx.to_device(_sim_sigma(c, fs, members=True)) if noise and c.ndays > 0 else None
        flagged = _sim_flagged(weights, f0, f1)
        sky = _sim_sky(c, fs)
        skybuf = None
        for r0 in range(0, c.nreal, BLOCKVEC_MAX_R):
            R = min(BLOCKVEC_MAX_R, c.nreal - r0)
            if sky is not None:
                if skybuf is None:
                    skybuf = ctx.empty((c.rmax, f1 - f0, c.npairs, c.ntime), np.complex128)
                _sim_group_sky(c, fs, sky, r0, skybuf[:R], False)
            if out is None and buf is None:
                buf = ctx.empty((c.rmax, nfc, c.nmem, c.ntime), np.complex128)
            grp = buf[:R, : f1 - f0] if out is None else out[r0 : r0 + R, f0:f1]
            if sigma is not None:
                with _StepTimer(log, "noise"):
                    if grp.is_contiguous():
                        ctx.ts_noise(sigma, fs, c.ntime, R, c.seed, c.first + r0, out=grp)
                    else:   # a frequency slice of the result: ts_noise writes contiguous arrays
                        grp.copy_(ctx.ts_noise(sigma, fs, c.ntime, R, c.seed, c.first + r0))
            g = None
            if c.gains is not None and (sky is not None or want_gains):
                with _StepTimer(log, "gains"):
                    g = _sim_gain_chunk(c, freqs, f0, f1, r0, R)
            with _StepTimer(log, "expand"):
                if sky is not None:
                    ctx.vis_expand(skybuf[:R], c.class_off, c.members, g=g, out=grp, accumulate=sigma is not None)
                elif sigma is None:
                    grp.zero_()
            if flagged is not None:
                grp.masked_fill_(flagged, 0.0)
            yield r0, f0, grp, (g if want_gains else None)
            del g


def _write_sim_file(tstream, fi, data, tphi, gain=None, weight=None, table=None, extra=None):
    """One per-frequency file with the datasets and attributes of `simulate_ensemble`; `table` (class_off, members) marks
    it unstacked (attribute `unstacked`, datasets `members` and `class_off`); `extra`: further datasets by name."""
    tel, bt = tstream.telescope, tstream.beamtransfer
    os.makedirs(tstream._fdir(fi), exist_ok=True)
    with storage.File(tstream._ffile(fi), "w") as f:
        f.create_dataset("timestream", data=np.ascontiguousarray(data))
        f.create_dataset("phi", data=tphi)
        if gain is not None:
            f.create_dataset("gain", data=np.ascontiguousarray(gain))
        if weight is not None:
            f.create_dataset("weight", data=np.ascontiguousarray(weight))
        for name, value in (extra or {}).items():
            f.create_dataset(name, data=np.ascontiguousarray(value))
        if table is not None:
            f.create_dataset("class_off", data=np.asarray(table[0]))
            f.create_dataset("members", data=np.asarray(table[1]))
            f.attrs["unstacked"] = 1
        f.create_dataset("feedmap", data=np.asarray(tel.feedmap))
        f.create_dataset("feedconj", data=np.asarray(tel.feedconj))
        f.create_dataset("feedmask", data=np.asarray(tel.feedmask))
        f.create_dataset("uniquepairs", data=np.asarray(tel.uniquepairs))
        f.create_dataset("baselines", data=np.asarray(tel.baselines))
        f.attrs["beamtransfer_path"] = os.path.abspath(bt.directory)
        f.attrs["ntime"] = int(data.shape[-1])


def _conf_filled(given, defaults, complaint, show=sorted):
    """`defaults` with the entries of the dict `given` (or None) over them; a key that `defaults` lacks raises ValueError:
    `complaint` % (the unknown keys, the known ones), each through `show`."""
    given = dict(given or {})
    unknown = sorted(set(given) - set(defaults))
    if unknown:
        raise ValueError(complaint % (show(unknown), show(sorted(defaults))))
    return dict(defaults, **given)


def _host_c128(x, shape, what, names):
    """The tensor or array `x` as a complex128 host array of `shape` (its axes are `names`), else ValueError."""
    arr = np.asarray(x.cpu().numpy() if hasattr(x, "data_ptr") else x, dtype=np.complex128)
    if arr.shape != tuple(shape):
        raise ValueError("%s %s is not (%s) = (%s)" % (what, arr.shape, names, ", ".join("%d" % v for v in shape)))
    return arr


def _dir_phi(tstream, ntime=None):
    """The sample positions of a Timestream directory: the dataset `phi` of its first file, or the uniform grid of
    `ntime` samples (None: the file's attribute `ntime`)."""
    with storage.File(tstream._ffile(0), "r") as f:
        if "phi" in f:
            return np.asarray(f["phi"][:])
        return np.linspace(0, 2 * np.pi, int(f.attrs["ntime"]) if ntime is None else ntime, endpoint=False)


def _freq_chunks(freqs, chunk_gb, per_f):
    """`freqs` in runs that fit `chunk_gb` at `per_f` bytes a frequency, one frequency at the least."""
    step = max(1, int(chunk_gb * 2.0**30 // max(per_f, 1.0)))
    return [freqs[c0 : c0 + step] for c0 in range(0, len(freqs), step)]


def _save_all(tss):
    """How every driver ends: once all ranks have written their files, rank 0 saves the Timestream objects."""
    parallel.barrier()
    if parallel.rank0():
        for ts in tss:
            os.makedirs(ts.directory, exist_ok=True)
            ts.save()
    parallel.barrier()


# ---- the I/O stages of the routes that take a Timestream directory through one device kernel:
# ---- sidereal_stack, rfi_flag, delay_filter, ringmap, formed_beam and delay_spectrum ----------------------------------
def _route_open(who, m, indir, stacked_only=True, rows=True):
    """The source of a route: (the Timestream of `indir`, nrow, nt), the shape of the `timestream` of its file 0.  With
    `stacked_only` an unstacked directory is refused, with `rows` a row count other than the telescope's baselines."""
    src = Timestream(indir, m)
    if stacked_only:
        src._refuse_unstacked()
    with storage.File(src._ffile(0), "r") as f:
        nrow, nt = (int(v) for v in f["timestream"].shape)
    npairs = int(m.beamtransfer.telescope.npairs)
    if rows and nrow != npairs:
        raise ValueError("%s: %s holds %d rows, the telescope has %d baselines" % (who, src.directory, nrow, npairs))
    return src, nrow, nt


def _route_read(who, src, fs, nrow, nt, whole=False):
    """The frequencies `fs` of `src` as one chunk, every file opened once: `x`, per file the `timestream` (nrow, nt) as
    complex128, and `w`, per file the float64 `weight` — ones for a file without one, and None in place of the list when
    no file of the chunk has one.  With `whole` also `files`, per file (every dataset, the attributes), for
    `_route_rewrite`.  A file of another shape raises the ValueError that names it."""
    x, w, files = [], [], []
    for fi in fs:
        with storage.File(src._ffile(fi), "r") as f:
            data = {k: np.asarray(f[k][:]) for k in (f.keys() if whole else ("timestream", "weight")) if k in f}
            files.append((data, dict(f.attrs) if whole else None))
        if data["timestream"].shape != (nrow, nt):
            raise ValueError("%s: %s holds %s, not (%d, %d)" % (who, src._ffile(fi), data["timestream"].shape, nrow, nt))
        x.append(np.asarray(data["timestream"], dtype=np.complex128))
        w.append(np.asarray(data["weight"], dtype=np.float64) if "weight" in data else None)
    if all(v is None for v in w):
        w = None
    else:
        ones = np.ones((nrow, nt), dtype=np.float64)
        w = [ones if v is None else v for v in w]
    return SimpleNamespace(fs=list(fs), x=x, w=w, files=files if whole else None)


def _route_upload(ctx, chunk, r0=None, r1=None):
    """(x_d, w_d) of a chunk on the device, (len(fs), rows, nt) complex128 and float64 or None: all rows, or r0:r1."""
    x_d = ctx.to_device(np.stack([a[r0:r1] for a in chunk.x]))
    return x_d, None if chunk.w is None else ctx.to_device(np.stack([a[r0:r1] for a in chunk.w]))


def _row_chunks(who, nrow, chunk_gb, bytes_per_row):
    """The rows 0 .. nrow as ranges (r0, r1) that fit `chunk_gb` at `bytes_per_row` over all frequencies."""
    rows_per = int(chunk_gb * 2.0**30 // bytes_per_row)
    if rows_per < 1:
        raise ValueError("%s: one row over all frequencies needs chunk_gb >= %.4g (given: %g)"
                         % (who, bytes_per_row / 2.0**30 * 1.001, chunk_gb))
    return [(r0, min(nrow, r0 + rows_per)) for r0 in range(0, nrow, rows_per)]


def _write_hdf5(path, datasets, attrs):
    """One file from a dict of arrays (written contiguous) and a dict of attributes: a root file, or one of the two
    below."""
    with storage.File(path, "w") as f:
        for name, value in datasets.items():
            f.create_dataset(name, data=np.ascontiguousarray(value))
        for name, value in attrs.items():
            f.attrs[name] = value


def _product_file(src, fi, prefix, name):
    return os.path.join(src._fdir(fi), "%s_%s.hdf5" % (prefix, name))


def _route_write_products(src, fs, prefix, name, data):
    """`<prefix>_<name>.hdf5` beside the timestream file of every frequency of `fs`: entry k of every array of `data`
    (their first axis is the chunk), and the attribute `frequency`."""
    for k, fi in enumerate(fs):
        os.makedirs(src._fdir(fi), exist_ok=True)
        _write_hdf5(_product_file(src, fi, prefix, name), {key: value[k] for key, value in data.items()},
                    dict(frequency=float(src.telescope.frequencies[fi])))


def _route_rewrite(dst, chunk, updates):
    """The files of a chunk read `whole`, written to `dst` with entry k of every array of `updates` over the datasets of
    file k; every other dataset and all attributes are kept.  The weight a file arrived with is kept as `weight_input`,
    unless it holds one already: a second pass keeps the first input."""
    for k, (fi, (data, attrs)) in enumerate(zip(chunk.fs, chunk.files)):
        if "weight" in data and "weight_input" not in data:
            data["weight_input"] = data["weight"]
        data.update({name: value[k] for name, value in updates.items()})
        os.makedirs(dst._fdir(fi), exist_ok=True)
        _write_hdf5(dst._ffile(fi), data, attrs)


def _sim_filled(c, unstacked, weights=None, noise=True):
    """The tensor (nreal, nf, npairs or nmem, ntime) of the run `c`, filled by the generator of its layout; `weights` as
    given to the simulators."""
    nrow = c.nmem if unstacked else c.npairs
    weights = _sim_weights(c, weights, nrow)
    out = get_context().empty((max(c.nreal, 0), len(c.freqs), nrow, c.ntime), np.complex128)
    for _ in (_unstacked_chunks if unstacked else _visibility_groups)(c, c.freqs, out=out, weights=weights, noise=noise):
        pass
    return out


def _sim_written(c, dirs, weights, unstacked):
    """The realisations of the run `c` written to the Timestream directories `dirs` as they come off the device, one
    device-to-host copy per group of realisations (and, unstacked, per chunk of frequencies); returns the Timestreams."""
    ctx, freqs = get_context(), c.freqs
    nrow, table = (c.nmem, (c.class_off, c.members)) if unstacked else (c.npairs, None)
    weights = _sim_weights(c, weights, nrow)
    weight_f = None if weights is None else np.broadcast_to(weights, (len(freqs), nrow, c.ntime))
    tphi = np.linspace(0, 2 * np.pi, c.ntime, endpoint=False)
    tss = [Timestream(d, c.m) for d in dirs]

    def write(r0, f0, host, gh):   # host (R, nfc, nrow, ntime) from row f0 on, gh (1 or R, nfc, nfeed, ntime) or None
        with _StepTimer(sim_log, "write"):
            for r in range(host.shape[0]):
                for k in range(host.shape[1]):
                    _write_sim_file(tss[r0 + r], freqs[f0 + k], host[r, k], tphi,
                                    gain=None if gh is None else gh[r if gh.shape[0] > 1 else 0, k],
                                    weight=None if weight_f is None else weight_f[f0 + k], table=table)

    if unstacked:
        for r0, f0, grp, g in _unstacked_chunks(c, freqs, want_gains=c.gains is not None, weights=weights):
            with _StepTimer(sim_log, "download"):
                host = ctx.to_host(grp)
                gh = None if g is None else ctx.to_host(g)
            write(r0, f0, host, gh)
    else:
        chunks = []   # the gain chunks of a group in the order of their frequencies, on the host
        sink = None if c.gains is None else lambda r0, f0, g: chunks.append(ctx.to_host(g))
        for r0, grp in _visibility_groups(c, freqs, gain_sink=sink, weights=weights):
            with _StepTimer(sim_log, "download"):
                host = ctx.to_host(grp)
            write(r0, 0, host, np.concatenate(chunks, axis=1) if chunks else None)
            chunks.clear()
    _save_all(tss)
    return tss


def simulate_visibilities(m, nreal, maps=(), ndays=None, resolution=0, seed=0, skymodels=(), klname=None, sky_seed=0,
                          first=0, freqs=None, chunk_gb=4.0, sources=(), gains=None, weights=None, unstacked=False):
    """`nreal` simulated timestreams of the telescope of ProductManager `m` as ONE device tensor
    (nreal, len(freqs), npairs, ntime): what `simulate` writes per frequency, for many statistically independent data
    sets, without leaving the device between the draws and the result.

    Realisation first + i uses `sky_realisation = first + i` of every model of `skymodels` ("signal", "foreground": the
    a_lm of `skysim.draw_alm` with `sky_seed`) and noise realisation first + i of `seed`; `maps` and `sources`
    (point-source catalogues, `skysim.source_alm`) are fixed skies shared by all.  `freqs` (sorted; default: this rank's share of the frequencies) are the rows computed: every draw is
    counter based, so a rank draws, projects and synthesises its own frequencies and the union of the ranks' results is
    the single-process result — there are no collectives.

    Realisations go in groups of up to 8: per group the beam blocks of every m are read once (from the resident
    products or the files, batches of at most `chunk_gb`) and applied to the a_lm of the whole group in one launch per
    batch (`BeamTransfer.project_vectors_sky_to_telescope_device`); the noise is drawn into the result
    (`Context.ts_noise`) and the m -> time transform adds to it (`Context.mmode_synthesis`).

    Noise: `simulate` adds complex noise of variance `noisepower` to each of the ntime Fourier bins before
    ifft * ntime; in the time domain that is white noise of variance ntime * noisepower, exactly, and that is what is
    drawn here, sigma[f, p] = sqrt(ntime * noisepower(p, f, ndays)).  It is the same DISTRIBUTION as `simulate`'s, not
    the same numbers.  ndays = 0: no noise.

    gains: per-feed gain errors — a `skysim.GainModel` (or the dict of its arguments), whose
    realisation first + i belongs to data set i, or an explicit complex128 array / device tensor (len(freqs), nfeed,
    ntime) for all or (nreal, len(freqs), nfeed, ntime).  Per-feed gains break the redundancy of a stacked baseline: the
    sky part of unique pair c is multiplied by G_c = mean over the feed pairs (i, j) of the class of g_i conj(g_j)
    (`Context.ts_gain_apply`).  The gains multiply the sky part only: receiver noise is added after them and its level
    is unchanged.  They are counter based like the rest, so a frequency subset or a realisation range reproduces the rows
    of the full call.  gains=None: none of this runs and the result is what it was.

    weights: flags — a `skysim.FlagModel` (or the dict of its arguments) or a float64 array >= 0
    of shape (len(freqs), npairs, ntime), (len(freqs), ntime) or (ntime,), the same for every realisation: samples of
    weight 0 are set to exactly 0 after sky, gains and noise.  weights=None: none of this runs.

    unstacked=True: one row per feed pair instead of one per unique baseline, in the order of
    `members` of `TransitTelescope.redundant_pairs` — the result is (nreal, len(freqs), nmem, ntime) with
    V_m = g_i conj(g_j) V_c^sky + n_m: the stacked sky spread over the members with the gains of `gains` on it
    (`Context.vis_expand`), on noise of variance n_c ntime noisepower, so that the plain mean of a complete class has the
    noise of the stacked result.  `weights` then has nmem rows.  The work goes in chunks of frequencies that fit in
    `chunk_gb`.  unstacked=False: none of this runs."""
    c = _sim_conf(m, freqs, resolution, ndays, nreal=nreal, first=first, seed=seed, sky_seed=sky_seed, klname=klname, maps=maps,
                  skymodels=skymodels, sources=sources, gains=gains, chunk_gb=chunk_gb)
    return _sim_filled(c, unstacked, weights)


def simulate_ensemble(m, outdir, nreal, maps=(), ndays=None, resolution=0, seed=0, skymodels=(), klname=None,
                      sky_seed=0, first=0, freqs=None, chunk_gb=4.0, sources=(), gains=None, weights=None, unstacked=False):
    """`simulate_visibilities` written out: realisation first + i as the Timestream directory
    `outdir/real_%04d` % (first + i), each with the per-frequency files, datasets and attributes of `simulate` and the
    saved object.  Every rank writes its own frequencies (one device-to-host copy per group of up to 8 realisations),
    rank 0 saves the objects.  Returns the list of `Timestream`.  With `gains` (see `simulate_visibilities`: they multiply
    the sky part only, the noise is added after at its usual level) every per-frequency file also holds the dataset
    `gain` (nfeed, ntime), the feed gains that were applied to that realisation and frequency.  With `weights` (see
    `simulate_visibilities`) every per-frequency file holds the dataset `weight` (npairs, ntime) and exact zeros where it
    is 0; `generate_modes_batched` then estimates the m-modes from the samples that are there.

    End to end (does the estimator recover the injected spectrum through the real chain?):

        tss = timestream.simulate_ensemble(pm, "ens", 64, skymodels=("signal",), ndays=733)
        for ts in tss:
            ts.generate_modes_batched(klnames=["kl"])
            ts.set_kltransform("kl")
            ts.set_psestimator("ps")
            p = ts.powerspectrum()      # mean over the ensemble -> the injected band powers, scatter -> Fisher errors

    unstacked=True (see `simulate_visibilities`): every per-frequency file holds `timestream`
    (nmem, ntime), one row per feed pair, the attribute `unstacked` = 1 and the class table as the datasets `members` and
    `class_off`, `weight` (nmem, ntime) when weights were given, and everything else as above (`gain` included: what
    `stack_baselines(calibrate="file")` undoes).  Such a directory goes through `stack_baselines` before the m-modes.
    """
    c = _sim_conf(m, freqs, resolution, ndays, nreal=nreal, first=first, seed=seed, sky_seed=sky_seed, klname=klname, maps=maps,
                  skymodels=skymodels, sources=sources, gains=gains, chunk_gb=chunk_gb)
    dirs = [os.path.join(outdir, "real_%04d" % (c.first + i)) for i in range(max(c.nreal, 0))]
    return _sim_written(c, dirs, weights, unstacked)


def simulate_unstacked(m, outdir, maps=(), ndays=None, resolution=0, seed=None, skymodels=(), klname=None, sky_seed=0,
                       sky_realisation=0, sources=(), gains=None, weights=None, chunk_gb=4.0):
    """One unstacked Timestream directory `outdir` with the arguments of `simulate`: realisation `sky_realisation` of
    `simulate_ensemble(unstacked=True)`, written straight into `outdir` (what a `simulate:` block with
    `unstacked: true` of the pipeline runs; seed=None is seed 0, the draws being counter based).  Returns the
    Timestream."""
    c = _sim_conf(m, None, resolution, ndays, nreal=1, first=sky_realisation, seed=0 if seed is None else seed,
                  sky_seed=sky_seed, klname=klname, maps=maps, skymodels=skymodels, sources=sources, gains=gains,
                  chunk_gb=chunk_gb)
    return _sim_written(c, [outdir], weights, True)[0]


REDCAL_DEFAULTS = dict(damping=0.4, tol=1e-10, maxiter=500, reference=None)


MODELCAL_DEFAULTS = dict(model=None, interval=16, damping=0.5, tol=1e-10, maxiter=500, edge_floor=1e-6, min_model=0.0)


def _modelcal_conf(modelcal, m, nfreq, npairs, ntime, tphi):
    """The checked dict `modelcal` of `stack_baselines` as a namespace: solver (the solver's keywords), edge_floor,
    min_model, model (fi -> (npairs, ntime) complex128) and nint, the solution intervals of a frequency."""
    conf = _conf_filled(modelcal, MODELCAL_DEFAULTS, "modelcal holds %s, not in %s")
    model = conf.pop("model")
    if model is None:
        raise ValueError("modelcal needs `model`: a stacked Timestream directory or an array (nfreq, npairs, ntime)")
    edge_floor, min_model = float(conf.pop("edge_floor")), float(conf.pop("min_model"))
    if not (0 <= edge_floor <= 1 and 0 <= min_model <= 1):
        raise ValueError("modelcal edge_floor and min_model lie in [0, 1]")
    solver = dict(interval=int(conf["interval"]), damping=float(conf["damping"]), tol=float(conf["tol"]),
                  maxiter=int(conf["maxiter"]))
    if solver["interval"] < 1:
        raise ValueError("modelcal interval must be at least 1")
    if isinstance(model, (str, os.PathLike)):
        mts = Timestream(os.fspath(model), m)
        if not os.path.exists(mts._ffile(0)):
            raise ValueError("modelcal model: %s holds no timestream" % mts.directory)
        if mts.is_unstacked():
            raise ValueError("modelcal model: %s holds unstacked visibilities, the stacked model is expected" % mts.directory)
        mphi = _dir_phi(mts)
        if mphi.shape != tphi.shape or not np.array_equal(mphi, tphi):
            raise ValueError("modelcal model: %s is sampled at other positions `phi` than the data" % mts.directory)

        def model_f(fi):
            v = np.asarray(mts.timestream_f(fi), dtype=np.complex128)
            if v.shape != (npairs, ntime):
                raise ValueError("modelcal model: %s is %s, not (npairs, ntime) = (%d, %d)" % (mts._ffile(fi), v.shape, npairs, ntime))
            return v
    else:
        arr = _host_c128(model, (nfreq, npairs, ntime), "modelcal model", "nfreq, npairs, ntime")
        model_f = lambda fi: arr[fi]
    return SimpleNamespace(solver=solver, edge_floor=edge_floor, min_model=min_model, model=model_f,
                           nint=_modelcal_nint(ntime, solver["interval"]))


def _modelcal_chunk(ctx, vis_d, w_d, model, class_off, members, nfeed, fw, solver, edge_floor, min_model):
    """The sky-model solve of one chunk of frequencies: vis_d (1, nfc, nmem, ntime) and w_d on
    the device, model (nfc, npairs, ntime) on the host.  Per frequency and interval the classes under edge_floor of the
    largest are zeroed in the copy of the model that goes to the device, the intervals under min_model of the strongest
    are not solved, the free phase of every connected component is fixed against ones and the interval gains are spread
    over their samples.  Returns (gains (nfc, nfeed, ntime), gq (nfc, nfeed, nint), iters (nfc, nint), valid (nfc, nint),
    frequencies without any valid interval)."""
    nfc, npairs, ntime = model.shape
    L = solver["interval"]
    starts = np.arange(0, ntime, L)
    tq = np.arange(ntime) // L
    power = np.add.reduceat(model.real**2 + model.imag**2, starts, axis=-1)             # (nfc, npairs, nint)
    top = power.max(axis=1, keepdims=True) if npairs else np.zeros((nfc, 1, starts.shape[0]))
    keep = (power >= edge_floor * top) & (power > 0)
    model = np.where(keep[..., tq], model, 0.0)
    total = np.where(keep, power, 0.0).sum(axis=1)                                      # (nfc, nint)
    active = total >= min_model * total.max(axis=1, keepdims=True)          # min_model = 0 solves all
    g_d, info = ctx.modelcal_solve(vis_d, ctx.to_device(model[None]), class_off, members, L, w=w_d,
                                   feed_weight=np.ones(nfeed) if fw is None else fw,
                                   active=ctx.to_device(active.astype(np.int32)), damping=solver["damping"],
                                   tol=solver["tol"], maxiter=solver["maxiter"])
    gq, its = ctx.to_host(g_d)[0], ctx.to_host(info["iters"])[0]
    live = np.ones(nfeed, dtype=bool) if fw is None else fw > 0
    valid = active & (ctx.to_host(info["step"])[0] < solver["tol"]) & np.all(ctx.to_host(info["gweight"])[0][:, live] > 0, axis=1)
    gains = np.empty((nfc, nfeed, ntime), dtype=np.complex128)
    fixed = np.empty_like(gq)
    seen, blind = {}, 0
    for k in range(nfc):
        comp = np.empty((nfeed, starts.shape[0]), dtype=np.int64)
        for q in range(starts.shape[0]):                                               # few distinct patterns: solved once each
            key = keep[k, :, q].tobytes()
            if key not in seen:
                seen[key] = modelcal_components(class_off, members, nfeed, keep[k, :, q].astype(np.float64), feed_weight=fw,
                                                edge_floor=0.5)
            comp[:, q] = seen[key]
        fixed[k] = modelcal_fix_phase(gq[k], comp, feed_weight=fw)
        gains[k], found = modelcal_spread(fixed[k], valid[k], L, ntime)
        blind += 0 if found else 1
    return gains, fixed, its, valid, blind


def _stack_gains_arg(calibrate, shape):
    """`calibrate` of `stack_baselines` checked: None, "file", "redundant", "model" or a host array of `shape`."""
    if isinstance(calibrate, str):
        if calibrate not in ("file", "none", "redundant", "model"):
            raise ValueError('calibrate is None, "none", "file", "redundant" or an array (nfreq, nfeed, ntime)')
        return None if calibrate == "none" else calibrate
    return None if calibrate is None else _host_c128(calibrate, shape, "calibrate", "nfreq, nfeed, ntime")


def _redcal_conf(redcal, shape):
    """The checked dict `redcal` of `stack_baselines`: (solver keywords, reference — None, "file", "model" or a host
    array of `shape`)."""
    conf = _conf_filled(redcal, REDCAL_DEFAULTS, "redcal holds %s, not in %s")
    reference = conf.pop("reference")
    solver = dict(damping=float(conf["damping"]), tol=float(conf["tol"]), maxiter=int(conf["maxiter"]))
    if isinstance(reference, str):
        if reference not in ("file", "none", "model"):
            raise ValueError('redcal reference is None, "file" or an array (nfreq, nfeed, ntime)')
        reference = None if reference == "none" else reference
    elif reference is not None:
        reference = _host_c128(reference, shape, "redcal reference", "nfreq, nfeed, ntime")
    return solver, reference


def _feed_weights(feed_weight, dead_feeds, nfeed):
    """feed_weight (nfeed) with the `dead_feeds` at 0, or None when neither is given."""
    if feed_weight is None and len(dead_feeds) == 0:
        return None
    fw = np.ones(nfeed, dtype=np.float64) if feed_weight is None else np.array(feed_weight, dtype=np.float64)
    if fw.shape != (nfeed,) or not np.all(np.isfinite(fw) & (fw >= 0)):
        raise ValueError("feed_weight must be (nfeed,) = (%d,), finite and not negative" % nfeed)
    for a in dead_feeds:
        if not 0 <= int(a) < nfeed:
            raise ValueError("dead feed %d of %d" % (int(a), nfeed))
        fw[int(a)] = 0.0
    return fw


def _stack_conf(m, src, calibrate, feed_weight, dead_feeds, redcal, rfi, modelcal, rfi_freq=None, rfi_dilate=None):
    """The arguments of `stack_baselines` checked once and its modes resolved.  Fields: the class table (class_off,
    members) and nmem, npairs, nfeed, nfreq, ntime; phi, the sample positions of `src`; rfi, the flagger's parameters or
    None; flagging, the steps of `_rfi_route`; redundant, by_model, ref_model: which solvers run and what the model's gains are for; redcal, the redundant
    solver's keywords; bases, its degeneracies; modelcal, the namespace of `_modelcal_conf`, or None; calibrated: the
    stack takes gains; file_gain: the files' `gain` is read, and under which name its absence is refused; given_gain: an
    array (nfreq, nfeed, ntime) handed over — both are the reference on the redundant route and the stack's gains
    otherwise; fw, the feed weights or None; weighted: the chunks carry per-sample weights."""
    c = SimpleNamespace(rfi=None if rfi is None else rfi_params(rfi))
    c.flagging = _rfi_route(rfi, rfi_freq, rfi_dilate)
    tel = m.beamtransfer.telescope
    if not src.is_unstacked():
        raise ValueError("%s does not hold unstacked visibilities" % src.directory)
    c.class_off, c.members = tel.redundant_pairs()
    c.nmem, c.npairs, c.nfeed, c.nfreq, c.ntime = int(c.class_off[-1]), int(tel.npairs), int(tel.nfeed), int(tel.nfreq), src.ntime
    with storage.File(src._ffile(0), "r") as f:
        if not (np.array_equal(f["class_off"][:], c.class_off) and np.array_equal(f["members"][:], c.members)):
            raise ValueError("%s was written for another class table than this telescope's" % src.directory)
    shape = (c.nfreq, c.nfeed, c.ntime)
    calibrate = _stack_gains_arg(calibrate, shape)
    c.calibrated = calibrate is not None
    c.redundant, c.by_model = (isinstance(calibrate, str) and calibrate == mode for mode in ("redundant", "model"))
    if redcal is not None and not c.redundant:
        raise ValueError('redcal belongs to calibrate="redundant"')
    c.redcal, reference = _redcal_conf(redcal, shape) if c.redundant else (None, calibrate)
    c.ref_model = c.redundant and isinstance(reference, str) and reference == "model"
    c.file_gain = None
    if isinstance(reference, str) and reference == "file":
        c.file_gain = 'redcal reference "file"' if c.redundant else 'calibrate="file"'
    c.given_gain = None if reference is None or isinstance(reference, str) else reference
    if modelcal is not None and not (c.by_model or c.ref_model):
        raise ValueError('modelcal belongs to calibrate="model" or to the redcal reference "model"')
    c.phi = _dir_phi(src, c.ntime)   # a day keeps its own sample positions (section 4.19)
    c.modelcal = _modelcal_conf(modelcal, m, c.nfreq, c.npairs, c.ntime, c.phi) if c.by_model or c.ref_model else None
    c.fw = _feed_weights(feed_weight, dead_feeds, c.nfeed)
    c.bases = redcal_degeneracies(c.class_off, c.members, c.nfeed, c.fw) if c.redundant else None
    with storage.File(src._ffile(0), "r") as f:
        c.weighted = "weight" in f or c.flagging.any
    return c


def _stack_per_f(c):
    """Bytes one frequency of a chunk of `stack_baselines` takes, on the host and on the device."""
    per_f = c.ntime * (16.0 * c.nmem + (8.0 * c.nmem if c.weighted else 0.0) + (16.0 * c.nfeed if c.calibrated else 0.0)
                       + 24.0 * c.npairs)
    if c.flagging.freq is not None or c.flagging.dilate is not None:   # the weights between the steps
        per_f += c.ntime * 16.0 * c.nmem
    if c.redundant:   # g, the second gain buffer and y of the solver, its three per-sample outputs and its state words
        per_f += c.ntime * (32.0 * c.nfeed + 16.0 * c.npairs + 20.0 + 24.0)
    if c.modelcal is not None:   # the model and its device copy, the solver's three gain buffers and gweight, its words
        per_f += (c.ntime * 32.0 * c.npairs + c.modelcal.nint * (56.0 * c.nfeed + 64.0)
                  + (0.0 if c.by_model else 16.0 * c.nfeed * c.ntime))
    return per_f


def _stack_read(src, fs, c):
    """The frequencies `fs` of the unstacked directory `src` as one chunk of per-frequency lists: vis (nmem, ntime); w of
    that shape, ones where a file has none, or None when the run is not weighted; g (nfeed, ntime), the gains of the
    files or of the array handed over, or None; vis_d and w_d, the device copies (1, nfc, nmem, ntime) that
    `_stack_on_device` makes."""
    vis, w, g = [], [], []
    for fi in fs:
        with storage.File(src._ffile(fi), "r") as f:
            vis.append(np.asarray(f["timestream"][:], dtype=np.complex128))
            if c.weighted:
                w.append(np.asarray(f["weight"][:], dtype=np.float64) if "weight" in f
                         else np.ones((c.nmem, c.ntime), dtype=np.float64))
            if c.file_gain is not None:
                if "gain" not in f:
                    raise ValueError("%s: %s holds no dataset `gain`" % (c.file_gain, src._ffile(fi)))
                g.append(np.asarray(f["gain"][:], dtype=np.complex128))
    if c.given_gain is not None:
        g = [c.given_gain[fi] for fi in fs]
    return SimpleNamespace(fs=fs, vis=vis, w=w if c.weighted else None, g=g or None, vis_d=None, w_d=None)


def _stack_on_device(ctx, chunk):
    """(vis_d, w_d) of a chunk: uploaded once, by the first stage that needs them (after the flagging)."""
    if chunk.vis_d is None:
        chunk.vis_d = ctx.to_device(np.stack(chunk.vis)[None])
        chunk.w_d = None if chunk.w is None else ctx.to_device(np.stack(chunk.w)[None])
    return chunk.vis_d, chunk.w_d


def _stack_flag(ctx, chunk, route):
    """The RFI steps over a chunk (DESIGN.md sections 4.20 and 4.22): its weights with the flagged samples at 0, on the
    host."""
    x_d = ctx.to_device(np.stack(chunk.vis))
    return list(ctx.to_host(_rfi_steps(ctx, x_d, ctx.to_device(np.stack(chunk.w)), route)[0]))


def _stack_model_solve(ctx, chunk, c):
    """The sky-model solve of a chunk: (spread gains (nfc, nfeed, ntime), the datasets it adds to every frequency's file,
    invalid intervals, frequencies without a valid one)."""
    mc = c.modelcal
    vis_d, w_d = _stack_on_device(ctx, chunk)
    mg, mq, mits, mvalid, blind = _modelcal_chunk(ctx, vis_d, w_d, np.stack([mc.model(fi) for fi in chunk.fs]), c.class_off,
                                                  c.members, c.nfeed, c.fw, mc.solver, mc.edge_floor, mc.min_model)
    datasets = [dict(gain_solution=mg[k], modelcal_gain=mq[k], modelcal_iters=mits[k], modelcal_valid=mvalid[k].astype(np.int32))
                for k in range(len(chunk.fs))]
    return mg, datasets, int((~mvalid).sum()), blind


def _stack_redundant_solve(ctx, chunk, c, ref):
    """The redundant solve of a chunk with its degeneracies fixed against `ref` (nfc, nfeed, ntime), an array or a list
    over the frequencies, or against ones (None): (gains (nfc, nfeed, ntime), the datasets it adds to every frequency's
    file, failed (nfc, ntime): the samples that did not converge)."""
    vis_d, w_d = _stack_on_device(ctx, chunk)
    gs, ys, info = ctx.redcal_solve(vis_d, c.class_off, c.members, w=w_d, feed_weight=np.ones(c.nfeed) if c.fw is None else c.fw,
                                    **c.redcal)
    gfix, _ = fix_degeneracies(ctx.to_host(gs)[0], ctx.to_host(ys)[0], c.class_off, c.members,
                               ref=None if ref is None else np.asarray(ref), feed_weight=c.fw, bases=c.bases)
    its, failed = ctx.to_host(info["iters"])[0], ~(ctx.to_host(info["step"])[0] < c.redcal["tol"])
    return gfix, [dict(gain_solution=gfix[k], redcal_iters=its[k]) for k in range(len(chunk.fs))], failed


def _stack_sum(ctx, chunk, c, g, log):
    """`Context.vis_stack` of a chunk with the gains g (nfc, nfeed, ntime), an array or a list over the frequencies, or
    None: (stacked (nfc, npairs, ntime), weight of that shape: the share of every class that is there, 0 where the kernel
    formed no sample)."""
    with _StepTimer(log, "stack"):
        vis_d, w_d = _stack_on_device(ctx, chunk)
        g_d = None if g is None else ctx.to_device(np.asarray(g)[None])
        out, wout = ctx.vis_stack(vis_d, c.class_off, c.members, w=w_d, g=g_d, feed_weight=c.fw)
        out, wout = ctx.to_host(out)[0], ctx.to_host(wout)[0]
    nmem_c = np.diff(c.class_off)[:, None].astype(np.float64)
    mfac = None if c.fw is None else (c.fw[c.members[:, 0]] * c.fw[c.members[:, 1]])[:, None]
    share = np.ones((c.npairs, 1)) if mfac is None else np.add.reduceat(mfac, c.class_off[:-1], axis=0) / nmem_c
    wts = np.empty(wout.shape, dtype=np.float64)
    for k in range(len(chunk.fs)):
        if c.weighted:
            fac = chunk.w[k] if mfac is None else chunk.w[k] * mfac
            share_k = np.add.reduceat(fac, c.class_off[:-1], axis=0) / nmem_c
        else:
            share_k = np.broadcast_to(share, (c.npairs, c.ntime))
        wts[k] = np.where(wout[k] == 0, 0.0, share_k)
    return out, wts


def _stack_write(dst, freqs, records, phi, log):
    """The stacked files of this rank's frequencies from their records (timestream, weight, datasets)."""
    # every rank writes `weight` or none does: the m-mode routes choose their path by the file of frequency 0
    mine = any(np.any(rec["weight"] != 1.0) for rec in records.values())
    nranks = parallel.size() if parallel._dist() else 1
    write_w = any(parallel.exchange([mine] * nranks))
    with _StepTimer(log, "write"):
        for fi in freqs:
            rec = records[fi]
            _write_sim_file(dst, fi, rec["timestream"], phi, weight=rec["weight"] if write_w else None,
                            extra=rec["datasets"] or None)


def _stack_report(c, nfreq, lost, minvalid, mblind, log):
    """The warnings and the counters of `sim_log` for what the solvers of `stack_baselines` left undone."""
    if c.redundant and lost:
        logging.getLogger(__name__).warning("stack_baselines: the redundant calibration of %d of %d samples did not converge "
                                            "in %d iterations; they are written with weight 0", lost, nfreq * c.ntime,
                                            c.redcal["maxiter"])
        if log is not None:
            log["redcal_not_converged"] = log.get("redcal_not_converged", 0) + lost
    if c.modelcal is not None and minvalid:
        logging.getLogger(__name__).warning("stack_baselines: %d of %d solution intervals of the sky-model calibration are not "
                                            "valid (not solved, not converged in %d iterations or with an unconstrained "
                                            "gain) and take the gains of the nearest valid interval; %d frequencies have "
                                            "none and are stacked with gains of one", minvalid, nfreq * c.modelcal.nint,
                                            c.modelcal.solver["maxiter"], mblind)
        if log is not None:
            log["modelcal_invalid"] = log.get("modelcal_invalid", 0) + minvalid


def stack_baselines(m, indir, outdir, calibrate=None, feed_weight=None, dead_feeds=(), chunk_gb=4.0, redcal=None, rfi=None,
                    modelcal=None, rfi_freq=None, rfi_dilate=None, delay=None):
    """Stack the unstacked Timestream directory `indir` (`simulate_ensemble(unstacked=True)`, or a correlator's per-pair
    data in that layout) into the unique baselines of the telescope of ProductManager `m` and write them to `outdir` in
    the layout of `simulate_ensemble`; returns the `Timestream` of `outdir`.

    Per frequency the rows (nmem, ntime) go through `Context.vis_stack` with the file's `weight` (when it has one) as the
    per-sample weights.  calibrate: None (or "none"), "file" — the dataset `gain` (nfeed, ntime) of every file — an
    explicit complex128 array / tensor (nfreq, nfeed, ntime) of calibration gains, or "redundant": the gains are solved
    from the redundancy of the data itself (`Context.redcal_solve`) per chunk of frequencies,
    their degeneracies are fixed (`fix_degeneracies`) against the `reference` of the dict `redcal` — None: ones, "file":
    the dataset `gain`, or an array (nfreq, nfeed, ntime) — and the stack runs with them; `redcal` also holds the
    solver's `damping`, `tol` and `maxiter` (REDCAL_DEFAULTS).  A sample whose solve did not converge gets weight 0 and is
    counted (a warning of the module's logger, and `redcal_not_converged` of `sim_log`); the stacked files then also hold
    `gain_solution` (nfeed, ntime) and `redcal_iters` (ntime).  feed_weight (nfeed) >= 0 weights
    every pair by the product of its two feeds' entries; dead_feeds lists feeds of weight 0.  Ranks take their own
    frequencies, in chunks that fit in `chunk_gb`.

    calibrate="model" solves the gains against a trusted sky model (`Context.modelcal_solve`),
    constant over solution intervals.  The dict `modelcal` (MODELCAL_DEFAULTS; an unknown key raises ValueError) holds
    `model` — a stacked Timestream directory on the same sample positions `phi` (another `phi` raises ValueError), or an
    array / tensor (nfreq, npairs, ntime) — `interval`, the solver's `damping`, `tol` and `maxiter`, `edge_floor` (a class
    whose sum_t |M_c|^2 over an interval is under this share of the interval's largest class has its model zeroed, so that
    weakly coupled components of the feed graph decouple exactly) and `min_model` (an interval whose model power is under
    this share of the frequency's strongest interval is not solved; 0 solves all).  The free phase of every connected
    component is fixed against ones (`modelcal_fix_phase`).  An interval is valid when it was solved, converged and every
    feed of weight > 0 has gweight > 0; an invalid one takes the gains of the nearest valid one (`modelcal_spread`) and is
    counted (a warning of the module's logger, and `modelcal_invalid` of `sim_log`).  The stack runs with the spread
    gains; the files also hold `gain_solution` (nfeed, ntime), `modelcal_gain` (nfeed, nint), `modelcal_iters` (nint) and
    `modelcal_valid` (nint).  With calibrate="redundant" and `reference: "model"` in `redcal`, the redundant solve runs
    per sample as described above and the spread model gains are the reference of `fix_degeneracies`: the model supplies
    only the degenerate part.

    The stacked files hold `weight` (npairs, ntime) = sum_{m in c} w_m fw_i fw_j / n_c, the share of the class that is
    there — for flags and dead feeds (n_c - k) / n_c exactly, the inverse noise variance relative to nominal of section
    4.16 — only if some weight of some frequency is not exactly 1.0: complete, unflagged data goes on through the plain
    m-mode path, calibrated or not, flagged or thinned data through the weighted one (a class that lost all its members
    has weight 0 throughout and comes out of `generate_modes_batched` with info = -1).  The amplitudes of the calibration
    gains are left out of the file's weight (`Context.vis_stack` keeps them in its own: mean |g_i|^2 |g_j|^2, which moves
    the noise of a calibrated stack by the few per cent the amplitudes are off one); a sample the kernel could not form
    (every gain product of its class zero) gets weight 0.

    rfi: a dict of the parameters of `Context.rfi_flag` (an unknown key raises ValueError).  The feed-pair data of every
    frequency is then flagged on the device before anything is solved or summed, and the flags
    go on as weights 0 of the members, as the file's own flags do.  rfi_freq: a dict of the same keys for the pass along
    frequency (`Context.rfi_flag_freq`), run on the weights of the time pass; rfi_dilate: a dict of `rfi_dilate_params`,
    the dilation of the flags along time, then along frequency.  A step along frequency needs
    every frequency on one device: the one chunk is then all frequencies, and a `chunk_gb` that does not hold them, or
    more than one rank, raises ValueError.  delay: a dict of `delay_params`: `delay_filter` then runs in place on the
    stacked output, with this call's `chunk_gb`."""
    delay = None if delay is None else delay_params(delay)
    if delay is not None:
        _delay_one_rank("stack_baselines")
    src = Timestream(indir, m)
    c = _stack_conf(m, src, calibrate, feed_weight, dead_feeds, redcal, rfi, modelcal, rfi_freq, rfi_dilate)
    freqs = _sim_freqs(m.beamtransfer.telescope, None)
    chunks = _rfi_chunks("stack_baselines", freqs, chunk_gb, _stack_per_f(c), c.flagging)
    ctx = get_context()
    log = sim_log
    records, lost, minvalid, mblind = {}, 0, 0, 0
    for fs in chunks:
        with _StepTimer(log, "read"):
            chunk = _stack_read(src, fs, c)
        if c.flagging.any:
            with _StepTimer(log, "rfi"):
                chunk.w = _stack_flag(ctx, chunk, c.flagging)
        g, datasets, failed = chunk.g, [{} for _ in fs], None
        if c.modelcal is not None:
            with _StepTimer(log, "modelcal"):
                mg, datasets, bad, blind = _stack_model_solve(ctx, chunk, c)
            minvalid, mblind = minvalid + bad, mblind + blind
            g = mg if c.by_model else g
        if c.redundant:
            with _StepTimer(log, "redcal"):
                g, solved, failed = _stack_redundant_solve(ctx, chunk, c, mg if c.ref_model else g)
            datasets = [dict(r, **{name: v for name, v in d.items() if name not in r}) for r, d in zip(solved, datasets)]
            lost += int(failed.sum())
        out, wts = _stack_sum(ctx, chunk, c, g, log)
        for k, fi in enumerate(fs):
            weight = wts[k] if failed is None else np.where(failed[k][None, :], 0.0, wts[k])
            records[fi] = dict(timestream=out[k], weight=weight, datasets=datasets[k])
    dst = Timestream(outdir, m)
    _stack_write(dst, freqs, records, c.phi, log)
    _stack_report(c, len(freqs), lost, minvalid, mblind, log)
    _save_all([dst])
    if delay is not None:
        delay_filter(m, outdir, None, chunk_gb=chunk_gb, **delay)
    return dst


# ---- sidereal stacking -------------------------------------------------------------------

SIDEREAL_SNAP = 1e-9          # positions are known to this fraction of a sample (what `sidereal_stack` asks of `phi`)
T_SIDEREAL_DAY = 86164.0905   # seconds


def _ld_pi():
    return np.longdouble("3.14159265358979323846264338327950288")


def _sidereal_stretch(step):
    """s = max(1, (2 pi / ntime) / dphi): the kernel is stretched to the coarser of the two spacings; a ratio within
    SIDEREAL_SNAP of 1 is 1."""
    one = np.longdouble(1)
    return one if (step <= one or abs(step - one) <= SIDEREAL_SNAP) else step


def _ld_sinc(t):
    """sin(pi t) / (pi t) in long double, sin taken of t - round(t) so that the zeros are exact."""
    t = np.asarray(t, dtype=np.longdouble)
    r = np.round(t)
    sn = np.sin(_ld_pi() * (t - r))
    sn = np.where(np.mod(np.abs(r), 2) == 1, -sn, sn)
    safe = np.where(t == 0, np.longdouble(1), t)
    return np.where(t == 0, np.longdouble(1), sn / (_ld_pi() * safe))


def _dot2(c, x):
    """sum_t c[..., t] x[..., t] over the last axis as if in twice the working precision (the error-free products and
    sums of Ogita, Rump and Oishi's Dot2, products split after Veltkamp), in tap order: the tap sum of
    dm_sidereal_regrid, which needs |xh|^2 to a few ulps even where the taps cancel.  c real, x real or complex."""
    if np.iscomplexobj(x):
        return _dot2(c, x.real) + 1j * _dot2(c, x.imag)
    real = np.result_type(c, x).type
    factor = real(2.0 ** ((np.finfo(real).nmant + 2) // 2) + 1.0)
    shape = np.broadcast_shapes(c.shape, x.shape)[:-1]
    s, e = np.zeros(shape, dtype=real), np.zeros(shape, dtype=real)
    for t in range(c.shape[-1]):
        a, b = c[..., t], x[..., t]
        p = a * b
        ca, cb = factor * a, factor * b
        ah, bh = ca - (ca - a), cb - (cb - b)
        al, bl = a - ah, b - bh
        pe = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        tt = s + p
        z = tt - s
        e = e + (((s - (tt - z)) + (p - z)) + pe)
        s = tt
    return s + e


def sidereal_taps_host(nt_in, ntime, a, phi0, dphi):
    """The tap geometry of one day (dm_sidereal_table.h restates it in C++), in long double: a
    list over the grid samples k of (first, c) — c_j of the input samples j = first, first + 1, ..., with exact zeros
    trimmed from both ends (a zero inside is not a tap); j may lie outside [0, nt_in)."""
    ld = np.longdouble
    twopi = 2 * _ld_pi()
    nt_in, ntime, a = int(nt_in), int(ntime), int(a)
    dp = ld(float(dphi))
    if not (1 <= a <= 8):
        raise ValueError("a outside 1..8")
    if not (np.isfinite(float(phi0)) and np.isfinite(float(dphi)) and dp > 0):
        raise ValueError("phi0 or dphi not finite, or dphi <= 0")
    if ntime < 1 or nt_in < 0 or not (max(nt_in - 1, 0) * dp < twopi):
        raise ValueError("ntime < 1, or the day is not less than one turn")
    P, step = twopi / dp, (twopi / ntime) / dp
    s = _sidereal_stretch(step)
    p0 = np.fmod(ld(float(phi0)), twopi)
    if p0 < 0:
        p0 += twopi
    taps = []
    for k in range(ntime):
        u = (twopi * k / ntime - p0) / dp
        if u < 0:
            u += P
        r = np.round(u)
        if abs(u - r) <= SIDEREAL_SNAP:
            u = ld(0) if r >= P - SIDEREAL_SNAP else r
        jlo, jhi = int(np.ceil(u - a * s)), int(np.floor(u + a * s))
        j = np.arange(jlo, jhi + 1)
        t = (u - j.astype(ld)) / s
        c = np.where(np.abs(t) < a, _ld_sinc(t) * _ld_sinc(t / a), ld(0))
        nz = np.nonzero(c)[0]
        if nz.size:
            taps.append((jlo + int(nz[0]), c[nz[0] : nz[-1] + 1]))
        else:
            taps.append((jlo, np.zeros(0, dtype=ld)))
    return taps


def sidereal_regrid_host(x, w, phi0, dphi, ntime, a=3, min_share=1.0, dtype=np.complex128, details=False):
    """One day resampled onto the sidereal grid, the numpy statement of `Context.sidereal_regrid` (DESIGN.md section
    4.19): x (..., nt_in) sampled at phi0 + j dphi, w of the same shape or None (ones).  Returns (xh, W), both
    (..., ntime): the regridded value and its weight, 0 where the sample is not valid.  The geometry is made in long
    double and rounded to double, as the device's table is: the rounded c_j ARE the coefficients of the method, for
    every `dtype`.  The sums run in `dtype`, which may be np.clongdouble; the tap sum of x is compensated (`_dot2`).  details=True also returns a dict with `bound` = sum_j |c_j / S| |x_j| over the unflagged taps
    and `ntaps` (ntime), the taps of every grid sample."""
    if not (0.0 < float(min_share) <= 1.0):
        raise ValueError("min_share outside (0, 1]")
    real = _real_dtype(dtype).type
    x = np.asarray(x, dtype=dtype)
    nt_in = x.shape[-1]
    ok = np.ones(x.shape, dtype=bool) if w is None else np.asarray(w) > 0
    wi = np.ones(x.shape, dtype=real) if w is None else np.where(ok, 1 / np.where(ok, np.asarray(w, dtype=real), 1), 0)
    xz = np.where(ok, x, 0)
    taps = sidereal_taps_host(nt_in, ntime, a, phi0, dphi)
    shape = x.shape[:-1] + (int(ntime),)
    xh, W, bound = np.zeros(shape, dtype=dtype), np.zeros(shape, dtype=real), np.zeros(shape, dtype=real)
    for k, (first, cl) in enumerate(taps):
        c = cl.astype(np.float64).astype(real)
        A_all, S_all, nt = real(np.float64(np.abs(cl).sum())), real(np.float64(cl.sum())), int(np.count_nonzero(cl))
        j = first + np.arange(c.shape[0])
        inside = (j >= 0) & (j < nt_in) & (c != 0)
        ji, ci = j[inside], c[inside]
        if ji.size == 0:
            continue
        here = ok[..., ji]
        cm = np.where(here, ci, 0)
        A, S, nu = np.abs(cm).sum(axis=-1), cm.sum(axis=-1), here.sum(axis=-1)
        share = (nu == nt) | ((min_share < 1.0) & (A >= real(min_share) * A_all))
        valid = (nu > 0) & share & (S >= S_all / 2) & (S > 0)
        Ss = np.where(valid, S, 1)
        sx = _dot2(cm, xz[..., ji]) / Ss
        sv = (cm * cm * wi[..., ji]).sum(axis=-1)
        xh[..., k] = np.where(valid, sx, 0)
        Wk = Ss * Ss / np.where(valid, sv, 1)
        if w is not None:   # one tap: S^2 / (c^2 / w) is w itself, bit for bit
            Wk = np.where(nu == 1, np.where(here, np.where(here, np.asarray(w, dtype=real)[..., ji], 0), 0).sum(axis=-1), Wk)
        W[..., k] = np.where(valid, Wk, 0)
        bound[..., k] = np.where(valid, (np.abs(cm) * np.abs(xz[..., ji])).sum(axis=-1) / Ss, 0)
    if details:
        return xh, W, dict(bound=bound, ntaps=np.array([int(np.count_nonzero(c)) for _, c in taps]))
    return xh, W


def _day_phi(tstream):
    """(phi0, dphi, nt_in) of a day directory from the dataset `phi` of its first file: uniformly spaced after unwrapping,
    to SIDEREAL_SNAP of dphi."""
    with storage.File(tstream._ffile(0), "r") as f:
        phi = np.asarray(f["phi"][:], dtype=np.float64)
    if phi.ndim != 1 or phi.shape[0] < 2:
        raise ValueError("%s: the dataset phi needs two samples at the least" % tstream.directory)
    ph = np.unwrap(phi)
    n = ph.shape[0]
    dphi = (ph[-1] - ph[0]) / (n - 1)
    if not (np.all(np.isfinite(ph)) and dphi > 0
            and np.max(np.abs(ph - (ph[0] + dphi * np.arange(n)))) <= SIDEREAL_SNAP * dphi):
        raise ValueError("%s: phi is not uniformly spaced (to %g of its step)" % (tstream.directory, SIDEREAL_SNAP))
    return float(phi[0]), float(dphi), n


def sidereal_stack(m, daydirs, outdir, ntime=None, a=3, min_share=1.0, chunk_gb=4.0, rfi=None, rfi_freq=None,
                   rfi_dilate=None, delay=None):
    """Regrid the days `daydirs` onto the sidereal grid and average them with their weights.
    Every entry is a Timestream directory, stacked or unstacked, all of one row layout (and one class table): a stretch
    of samples at the positions of its dataset `phi` (uniformly spaced after unwrapping, else ValueError), with `weight`
    where present.  Ranks take their own frequencies in chunks that fit `chunk_gb`; within a chunk the days go through
    `Context.sidereal_regrid` one after the other into one accumulator.  `outdir` gets the layout of the simulators:
    `timestream` the weighted mean (0 where no day reached the sample), `weight` = wsum / len(daydirs) (always written:
    the data goes on through the weighted m-mode route, where its scale cancels; it is the diagonal only — neighbouring
    samples share taps and are correlated), `day_hits` int32, `day_variance` — the day-to-day scatter
    (sq - |sum|^2 / wsum) / (hits - 1), an estimate of the variance of one nominal input sample, 0 where hits < 2 —
    when there is more than one day, and the attribute `ndays`.  ntime=None: `_sim_ntime(tel, 0)`.  rfi: a dict of the parameters of
    `Context.rfi_flag` (an empty one: the defaults; an unknown key raises ValueError): every day is then flagged on the
    device between the read and the regridding, its weights are the day's own with the flagged
    samples at 0, and nothing is written for the days.  rfi_freq: a dict of the same keys for the pass along frequency
    (`Context.rfi_flag_freq`), which runs on the weights of the time pass; rfi_dilate: a dict of `rfi_dilate_params`, the
    dilation of the flags along time, then along frequency.  A step along frequency needs every
    frequency of a day on one device: the one chunk is then all frequencies, and a `chunk_gb` that does not hold them, or
    more than one rank, raises ValueError.  delay: a dict of `delay_params`: `delay_filter` then runs in place on the
    combined days (stacked days only), with this call's `chunk_gb`.  Returns the Timestream of
    `outdir`."""
    delay = None if delay is None else delay_params(delay)
    if delay is not None:
        _delay_one_rank("sidereal_stack")
    route = _rfi_route(rfi, rfi_freq, rfi_dilate)
    tel = m.beamtransfer.telescope
    daydirs = list(daydirs)
    if not daydirs:
        raise ValueError("sidereal_stack: no days")
    ntime = _sim_ntime(tel, 0) if ntime is None else int(ntime)
    opened = [_route_open("sidereal_stack", m, d, stacked_only=False, rows=False) for d in daydirs]
    days, nrow = [o[0] for o in opened], opened[0][1]
    geo = [_day_phi(d) for d in days]
    unst = [d.is_unstacked() for d in days]
    if any(u != unst[0] for u in unst):
        raise ValueError("sidereal_stack: stacked and unstacked days cannot be mixed")
    if delay is not None and unst[0]:
        raise ValueError("sidereal_stack: delay needs stacked days: stack them first with timestream.stack_baselines")
    table = None
    if unst[0]:
        for d in days:
            with storage.File(d._ffile(0), "r") as f:
                t = (np.asarray(f["class_off"][:]), np.asarray(f["members"][:]))
            if table is None:
                table = t
            elif not (np.array_equal(t[0], table[0]) and np.array_equal(t[1], table[1])):
                raise ValueError("sidereal_stack: %s was written for another class table" % d.directory)
    freqs = _sim_freqs(tel, None)
    nt_max = max(g[2] for g in geo)
    extra_steps = route.freq is not None or route.dilate is not None
    per_f = nrow * ((48.0 if extra_steps else 24.0 if rfi is None else 32.0) * nt_max + 36.0 * ntime + 16.0 * ntime)
    log = sim_log
    dst = Timestream(outdir, m)
    tphi = np.linspace(0, 2 * np.pi, ntime, endpoint=False)
    nd = len(days)
    chunks = _rfi_chunks("sidereal_stack", freqs, chunk_gb, per_f, route)
    ctx = get_context()
    torch = ctx.torch
    for fs in chunks:
        acc = None
        for d, (phi0, dphi, nt_in) in zip(days, geo):
            with _StepTimer(log, "read"):
                chunk = _route_read("sidereal_stack", d, fs, nrow, nt_in)
            with _StepTimer(log, "regrid"):
                x_d, w_d = _route_upload(ctx, chunk)
                if route.any:
                    w_d = _rfi_steps(ctx, x_d, w_d, route)[0]
                acc = ctx.sidereal_regrid(x_d, phi0, dphi, ntime, w=w_d, a=a, min_share=min_share, acc=acc)
                del x_d, w_d
        with _StepTimer(log, "finish"):
            s_, ws_, sq_, h_ = acc
            some = ws_ > 0
            wsafe = torch.where(some, ws_, torch.ones_like(ws_))
            mean = torch.where(some, s_ / wsafe, torch.zeros_like(s_))
            var = None
            if nd > 1:
                two = h_ >= 2
                v = (sq_ - (s_.real**2 + s_.imag**2) / wsafe) / torch.where(two, h_ - 1, torch.ones_like(h_)).to(torch.float64)
                var = ctx.to_host(torch.where(two & some, v, torch.zeros_like(v)))
            mean_h, w_h, hits_h = ctx.to_host(mean), ctx.to_host(ws_ / float(nd)), ctx.to_host(h_)
            del acc, s_, ws_, sq_, h_, mean
        with _StepTimer(log, "write"):
            for k, fi in enumerate(fs):
                extra = dict(day_hits=hits_h[k].astype(np.int32))
                if var is not None:
                    extra["day_variance"] = var[k]
                _write_sim_file(dst, fi, mean_h[k], tphi, weight=w_h[k], table=table, extra=extra)
                with storage.File(dst._ffile(fi), "a") as f:
                    f.attrs["ndays"] = nd
    _save_all([dst])
    if delay is not None:
        delay_filter(m, outdir, None, chunk_gb=chunk_gb, **delay)
    return dst


def _day_weights(weights, d):
    """The `weights` of `simulate_days` for day d: the d-th of a list, and a FlagModel (or its dict) with seed + d."""
    from . import skysim

    wd = weights[d] if isinstance(weights, (list, tuple)) else weights
    if isinstance(wd, dict):
        wd = skysim.FlagModel.from_config(wd)
    if isinstance(wd, skysim.FlagModel):
        wd = skysim.FlagModel(wd.fraction, wd.burst, wd.windows, wd.seed + d)
    return wd


def simulate_days(m, outdirs, starts, nsamples, cadence, maps=(), ndays=None, resolution=0, seed=0, skymodels=(),
                  klname=None, sky_seed=0, first=0, freqs=None, chunk_gb=4.0, sources=(), gains=None, weights=None,
                  unstacked=False, rfi=None):
    """The days that `sidereal_stack` consumes: day d is written to `outdirs[d]` as `nsamples`
    (one number, or one per day) samples at phi_j = starts[d] + j dphi, dphi = 2 pi cadence / T_SIDEREAL_DAY (cadence in
    seconds), in the layout of the simulators with `phi` set to the day's own positions (taken modulo 2 pi).  The
    remaining arguments are those of `simulate_visibilities`.

    The noise-free sky of the device route on the sidereal grid (realisation `first`, ndays = 0) is band-limited, so its
    value at every phi_j is exact: one FFT over the grid and one matrix product against e^{i m phi_j}, both in torch on
    the device.  Unless ndays = 0, day d gets one day's receiver noise, realisation d of `seed`
    (`Context.ts_noise`): sigma = sqrt((2 pi / dphi) noisepower(ndays=1)), the level of `simulate_visibilities` for a grid
    of 2 pi / dphi samples per turn (times n_c per feed pair when unstacked).  weights: as for `simulate_visibilities`
    with nsamples for ntime — one for all days, a list of one per day, or a FlagModel (or its dict), which day d
    evaluates with seed + d; flagged samples are written as exact zeros with `weight` 0.  rfi: a `skysim.RFIModel` (or
    its dict), which day d evaluates with seed + d: its bursts, in units of the row's one-day noise sigma, are added to
    the day and are NOT flagged.  Returns the list of Timestream."""
    from . import skysim

    ctx = get_context()
    torch = ctx.torch
    c = _sim_conf(m, freqs, resolution, ndays, default_ndays=1, nreal=1, first=first, seed=seed, sky_seed=sky_seed,
                  klname=klname, maps=maps, skymodels=skymodels, sources=sources, gains=gains, chunk_gb=chunk_gb)
    freqs, ntime, ndays = c.freqs, c.ntime, c.ndays
    outdirs = list(outdirs)
    nd = len(outdirs)
    starts = [float(v) for v in starts]
    nsamples = [int(nsamples)] * nd if np.ndim(nsamples) == 0 else [int(v) for v in nsamples]
    if len(starts) != nd or len(nsamples) != nd:
        raise ValueError("simulate_days: one start and one sample count per day expected")
    dphi = 2.0 * np.pi * float(cadence) / T_SIDEREAL_DAY
    if not (dphi > 0 and all(n >= 2 and (n - 1) * dphi < 2 * np.pi for n in nsamples)):
        raise ValueError("simulate_days: a day holds two samples at the least and covers less than one turn")
    nrow, table = (c.nmem, (c.class_off, c.members)) if unstacked else (c.npairs, None)
    grid = _sim_filled(c, unstacked, noise=False)
    tss = [Timestream(d, m) for d in outdirs]
    if len(freqs):
        modes = torch.fft.fft(grid[0], dim=-1) / ntime                                  # (nf, nrow, ntime)
        mm = torch.from_numpy(np.fft.fftfreq(ntime, 1.0 / ntime)).to(grid.device)
        if ntime % 2 == 0:   # the Nyquist mode has no sign: drop it (it is empty for a band-limited sky)
            modes[..., ntime // 2] = 0
        del grid
        if isinstance(rfi, dict):
            rfi = skysim.RFIModel.from_config(rfi)
        if ndays > 0 or rfi is not None:
            sigma = ctx.to_device(_sim_sigma(c, freqs, members=unstacked, ndays=1, ntime=2.0 * np.pi / dphi))
        for d in range(nd):
            n = nsamples[d]
            phi = starts[d] + dphi * np.arange(n)
            E = torch.exp(1j * mm[:, None] * torch.from_numpy(phi).to(mm.device)[None, :])   # (ntime, n)
            day = torch.matmul(modes, E).contiguous()                                       # (nf, nrow, n)
            if ndays > 0:
                day.add_(ctx.ts_noise(sigma, freqs, n, 1, seed, d)[0])
            if rfi is not None:
                rd = skysim.RFIModel(rfi.fraction, rfi.burst, rfi.amplitude, rfi.seed + d)
                day.add_(ctx.to_device(rd.bursts(n, freqs, nrow)) * sigma[:, :, None])
            wh = _sim_weights(c, _day_weights(weights, d), nrow, n)
            if wh is not None:
                wh = np.broadcast_to(wh, (len(freqs), nrow, n))
                day.masked_fill_(ctx.to_device(np.ascontiguousarray(wh == 0)), 0.0)
            host = ctx.to_host(day)
            del day, E
            for k, fi in enumerate(freqs):
                _write_sim_file(tss[d], fi, host[k], np.mod(phi, 2 * np.pi), weight=None if wh is None else wh[k], table=table)
    _save_all(tss)
    return tss


# ---- RFI flagging along time ---------------------------------------------------------------
RFI_DEFAULTS = dict(segment=1024, kernel_sigma=2.5, windows=(1, 2, 4, 8, 16), chi1=6.0, rho=1.5, niter=3, base=2.0,
                    min_good=16, row_share=1.0)
RFI_MAX_H, RFI_MAX_WINDOW, RFI_MAX_ITER = 32, 64, 8
RFI_SQRT_LN2 = 0.83255461115769775635   # sigma = median / sqrt(ln 2) for a Rayleigh amplitude


def rfi_params(params=None):
    """The parameters of the RFI flagger with their defaults filled in; an unknown key raises ValueError."""
    out = _conf_filled(params, RFI_DEFAULTS, "rfi: unknown key(s) %s (known: %s)", show=", ".join)
    out["windows"] = tuple(int(v) for v in out["windows"])
    return out


def rfi_tables_host(kernel_sigma=2.5, windows=(1, 2, 4, 8, 16), chi1=6.0, rho=1.5, niter=3, base=2.0):
    """The two tables of the RFI flagger (dm_rfi_table.h), made in long double and rounded to double once: g (H + 1,), the
    background kernel exp(-d^2 / (2 kernel_sigma^2)), and t (niter, len(windows)), the thresholds
    alpha + chi1 rho^(-log2 M) base^(niter - 1 - it) beta in units of the median amplitude.  Refuses what dm_rfi_flag
    refuses about these parameters."""
    L = np.longdouble
    windows = [int(v) for v in windows]
    if not (np.isfinite(kernel_sigma) and kernel_sigma > 0):
        raise ValueError("rfi: kernel_sigma not finite or <= 0")
    H = int(np.ceil(L(3) * L(kernel_sigma)))
    if H > RFI_MAX_H:
        raise ValueError("rfi: H = ceil(3 kernel_sigma) > %d" % RFI_MAX_H)
    if not (1 <= len(windows) <= 7) or any(M < 1 or M > RFI_MAX_WINDOW or M & (M - 1) for M in windows) or \
            any(b <= a for a, b in zip(windows, windows[1:])):
        raise ValueError("rfi: windows are not ascending powers of two <= %d" % RFI_MAX_WINDOW)
    if not (np.isfinite(chi1) and chi1 > 0 and np.isfinite(rho) and rho >= 1 and np.isfinite(base) and base >= 1):
        raise ValueError("rfi: chi1 <= 0, rho < 1 or base < 1, or one of them not finite")
    if not (1 <= int(niter) <= RFI_MAX_ITER):
        raise ValueError("rfi: niter outside 1..%d" % RFI_MAX_ITER)
    pi, ln2 = L("3.14159265358979323846264338327950288"), L("0.693147180559945309417232121458176568")
    alpha, beta = np.sqrt(pi / (L(4) * ln2)), np.sqrt((L(1) - pi / L(4)) / ln2)
    d = np.arange(H + 1).astype(L)
    g = np.exp(-(d * d) / (L(2) * L(kernel_sigma) * L(kernel_sigma))).astype(np.float64)
    t = np.zeros((int(niter), len(windows)), dtype=np.float64)
    for it in range(int(niter)):
        for i, M in enumerate(windows):
            chi = L(chi1) * np.power(L(rho), -L(M.bit_length() - 1))
            t[it, i] = np.float64(alpha + chi * np.power(L(base), L(int(niter) - 1 - it)) * beta)
    return g, t


def rfi_segments(nt, segment):
    """The balanced segments of a series of nt samples: [(j0, j1)], nseg = ceil(nt / segment)."""
    nseg = -(-int(nt) // int(segment))
    return [((s * nt) // nseg, ((s + 1) * nt) // nseg) for s in range(nseg)]


def rfi_flag_host(x, w=None, segment=1024, kernel_sigma=2.5, windows=(1, 2, 4, 8, 16), chi1=6.0, rho=1.5, niter=3, base=2.0,
                  min_good=16, row_share=1.0, dtype=np.float64, details=False):
    """The numpy statement of `Context.rfi_flag`: x (nf, nrow, nt) complex, w of that shape or
    None.  Returns (w_out, noise, nflag, occupancy) as the device does.  The tables are those of `rfi_tables_host` for
    every `dtype`; the sums, the amplitudes and the comparisons run in `dtype`, np.float64 or np.longdouble.
    details=True also returns a dict per segment, each (nf, nrow, nseg): `eps` = (2H + 17) 2^-53 max_j (sum g |x| /
    sum g + |x_j|), the error a double evaluation of an amplitude can have; `margin`, the smallest
    |S - c m t| - c eps (1 + t) over every window decision of every pass (inf where none was made); and `decided` =
    margin > 0: no rounding of that size can change a flag of the segment.  `row_flags` (nf, nrow, nt) are the flags
    before the occupancy step."""
    real = np.dtype(dtype).type
    cdt = np.clongdouble if real is np.longdouble else np.complex128
    x = np.asarray(x)
    if x.ndim != 3:
        raise ValueError("rfi_flag_host: x (nf, nrow, nt) expected")
    segment, niter, min_good = int(segment), int(niter), int(min_good)
    if segment < 1 or min_good < 1 or not (0.0 < float(row_share) <= 1.0):
        raise ValueError("rfi: segment < 1, min_good < 1 or row_share outside (0, 1]")
    windows = [int(v) for v in windows]
    g64, t64 = rfi_tables_host(kernel_sigma, windows, chi1, rho, niter, base)
    g, tt = g64.astype(real), t64.astype(real)
    H = g.shape[0] - 1
    nf, nrow, nt = x.shape
    inflag = np.zeros(x.shape, dtype=bool) if w is None else ~(np.asarray(w) > 0)
    xz = np.where(inflag, 0, x).astype(cdt)
    segs = rfi_segments(nt, segment) if nt else []
    nseg = len(segs)
    flags = np.zeros(x.shape, dtype=bool)
    noise = np.zeros((nf, nrow, nseg), dtype=real)
    eps_o = np.zeros((nf, nrow, nseg), dtype=np.float64)
    margin_o = np.full((nf, nrow, nseg), np.inf, dtype=np.float64)
    for s, (j0, j1) in enumerate(segs):
        n = j1 - j0
        X = xz[..., j0:j1].reshape(nf * nrow, n)
        I = inflag[..., j0:j1].reshape(nf * nrow, n)
        R = X.shape[0]
        B = I.copy()
        active, allflag = np.ones(R, dtype=bool), np.zeros(R, dtype=bool)
        med = np.zeros(R, dtype=real)
        eps = np.zeros(R, dtype=np.float64)
        margin = np.full(R, np.inf, dtype=np.float64)
        absX = np.abs(X).astype(np.float64)
        for it in range(niter):
            cnt = (~B).sum(axis=1)
            dead = active & (cnt < min_good)
            allflag |= dead
            active &= ~dead
            if not active.any():
                break
            sx, sg, sa = np.zeros((R, n), dtype=cdt), np.zeros((R, n), dtype=real), np.zeros((R, n), dtype=np.float64)
            used = np.zeros((R, n), dtype=np.int64)
            for d in range(-H, H + 1):
                lo, hi = max(0, -d), min(n, n - d)   # j in [lo, hi): k = j + d inside the segment
                if hi <= lo:
                    continue
                ok = ~B[:, lo + d : hi + d]
                gd = g[abs(d)]
                sx[:, lo:hi] += np.where(ok, gd * X[:, lo + d : hi + d], 0)
                sg[:, lo:hi] += np.where(ok, gd, 0)
                sa[:, lo:hi] += np.where(ok, np.float64(gd) * absX[:, lo + d : hi + d], 0)
                used[:, lo:hi] += ok
            unj = ~I & (used == 0)
            sgs = np.where(used > 0, sg, 1)
            r = X - sx / sgs
            a = np.where(I | unj, 0, np.sqrt(r.real * r.real + r.imag * r.imag)).astype(real)
            e_it = np.where(I | unj, 0, sa / sgs.astype(np.float64) + absX).max(axis=1) * (2 * H + 17) * 2.0**-53
            eps = np.where(active, np.maximum(eps, e_it), eps)
            srt = np.sort(np.where(B, np.inf, a), axis=1)
            m_it = srt[np.arange(R), np.maximum(cnt - 1, 0) // 2]
            med = np.where(active, m_it, med)
            D = I | unj
            for i, M in enumerate(windows):
                if M > n:
                    break
                nst = n - M + 1
                notD = ~D
                c = np.zeros((R, nst), dtype=np.int64)
                S = np.zeros((R, nst), dtype=real)
                for k in range(M):
                    c += notD[:, k : k + nst]
                    S = S + np.where(notD[:, k : k + nst], a[:, k : k + nst], 0)
                thr = m_it * tt[it, i]
                lim = c.astype(real) * thr[:, None]
                hit = (c >= 1) & (S > lim)
                mg = np.where(c >= 1, np.abs(S - lim).astype(np.float64) - c * e_it[:, None] * (1.0 + t64[it, i]), np.inf)
                margin = np.where(active, np.minimum(margin, mg.min(axis=1)), margin)
                newD = D.copy()
                for k in range(M):
                    newD[:, k : k + nst] |= hit
                D = newD
            B = np.where(active[:, None], D, B)
        fl = B | allflag[:, None]
        flags[..., j0:j1] = fl.reshape(nf, nrow, n)
        noise[..., s] = np.where(allflag, 0, med / real(RFI_SQRT_LN2)).reshape(nf, nrow)
        eps_o[..., s] = eps.reshape(nf, nrow)
        margin_o[..., s] = margin.reshape(nf, nrow)
    new = flags & ~inflag
    nflag = new.sum(axis=2).astype(np.int32)
    occupancy = new.sum(axis=1).astype(np.int32)
    n_in = (~inflag).sum(axis=1)
    col = (n_in > 0) & (occupancy.astype(np.float64) > np.float64(row_share) * n_in.astype(np.float64))
    final = flags | col[:, None, :]
    wv = np.ones(x.shape, dtype=np.float64) if w is None else np.asarray(w, dtype=np.float64)
    w_out = np.where(final, 0.0, wv)
    if details:
        return w_out, noise, nflag, occupancy, dict(eps=eps_o, margin=margin_o, decided=margin_o > 0, row_flags=flags)
    return w_out, noise, nflag, occupancy


# ---- RFI flagging along frequency and the dilation of flags -------------------------------
RFI_DILATE_DEFAULTS = dict(time=0.0, freq=0.0, new_only=True)
RFI_DILATE_ONE = 65536   # shares of flagged samples are compared in units of 1 / 65536


def rfi_flag_freq_host(x, w=None, dtype=np.float64, details=False, **params):
    """The numpy statement of `Context.rfi_flag_freq`: `rfi_flag_host` on the data transposed
    to (nt, nrow, nf), and its answer transposed back: (w_out (nf, nrow, nt), noise (nseg, nrow, nt), nflag (nrow, nt),
    occupancy (nf, nt)), and with details=True the dict of `rfi_flag_host` with eps, margin and decided
    (nseg, nrow, nt) and row_flags (nf, nrow, nt)."""
    x = np.asarray(x)
    if x.ndim != 3:
        raise ValueError("rfi_flag_freq_host: x (nf, nrow, nt) expected")
    back = lambda a: np.ascontiguousarray(np.transpose(a))   # reverses the axes
    out = rfi_flag_host(back(x), None if w is None else back(np.asarray(w)), dtype=dtype, details=details, **params)
    res = tuple(back(a) for a in out[:4])
    return res + ({k: back(v) for k, v in out[4].items()},) if details else res


def rfi_dilate_kappa(eta):
    """kappa = rint((1 - eta) 65536), the share of flagged samples a window needs, in units of 1 / 65536; ValueError for
    an eta that is not finite, outside [0, 1) or so close to 1 that kappa < 1."""
    eta = float(eta)
    if not (np.isfinite(eta) and 0.0 <= eta < 1.0):
        raise ValueError("rfi_dilate: eta not finite or outside [0, 1)")
    kappa = int(np.rint((1.0 - eta) * float(RFI_DILATE_ONE)))
    if kappa < 1:
        raise ValueError("rfi_dilate: kappa = rint((1 - eta) 65536) < 1")
    return kappa


def rfi_dilate_host(w, eta, axis="time", ref=None):
    """The numpy statement of `Context.rfi_dilate`, in the two-scan form: w (nf, nrow, nt); on
    every series along `axis` ("time" or "freq") F = the samples where `w > 0` is false, I = those where `ref > 0` is
    false (none without ref), psi = 0 on I, 65536 - kappa on F \\ I and -kappa elsewhere, P its prefix sums from P_0 = 0;
    sample j outside I is flagged iff max_{b > j} P_b >= min_{a <= j} P_a.  Returns (w_out, nadded): w where kept and 0
    where newly flagged; the new flags of every series, int32, (nf, nrow) along time and (nrow, nt) along frequency."""
    if axis not in ("time", "freq"):
        raise ValueError('rfi_dilate: axis is "time" or "freq"')
    kappa = rfi_dilate_kappa(eta)
    w = np.asarray(w, dtype=np.float64)
    if w.ndim != 3 or (ref is not None and np.shape(ref) != w.shape):
        raise ValueError("rfi_dilate_host: w (nf, nrow, nt) and ref of that shape or None expected")
    ax = 2 if axis == "time" else 0
    F = np.moveaxis(~(w > 0), ax, -1)
    I = np.zeros(F.shape, dtype=bool) if ref is None else np.moveaxis(~(np.asarray(ref) > 0), ax, -1)
    psi = np.where(I, 0, np.where(F, RFI_DILATE_ONE - kappa, -kappa)).astype(np.int64)
    P = np.concatenate([np.zeros(psi.shape[:-1] + (1,), dtype=np.int64), np.cumsum(psi, axis=-1)], axis=-1)
    lo = np.minimum.accumulate(P[..., :-1], axis=-1)                           # min_{a <= j} P_a
    hi = np.maximum.accumulate(P[..., :0:-1], axis=-1)[..., ::-1]              # max_{b > j} P_b
    new = ~I & ~F & (hi >= lo)
    nadded = new.sum(axis=-1).astype(np.int32)
    new = np.moveaxis(new, -1, ax)
    return np.where(new, 0.0, w), nadded


def rfi_dilate_params(d=None):
    """The dilation of a route with its defaults filled in: `time` and `freq`, the eta of `Context.rfi_dilate` along each
    axis (0: off), and `new_only` (True: the flags the data arrived with are the missing set, so that a daytime cut is
    not grown by eta / (1 - eta) of its length; False: they dilate too).  An unknown key raises ValueError, and so does
    an eta `rfi_dilate_kappa` refuses."""
    out = _conf_filled(d, RFI_DILATE_DEFAULTS, "rfi_dilate: unknown key(s) %s (known: %s)", show=", ".join)
    out["time"], out["freq"], out["new_only"] = float(out["time"]), float(out["freq"]), bool(out["new_only"])
    rfi_dilate_kappa(out["time"])
    rfi_dilate_kappa(out["freq"])
    return out


def _rfi_route(rfi, rfi_freq, rfi_dilate):
    """What a route was asked to flag: the parameters of the time pass and of the frequency pass (None: not run), the
    dilation (None: neither axis), and whether a step needs every frequency on one device at once."""
    r = SimpleNamespace(time=None if rfi is None else rfi_params(rfi), freq=None if rfi_freq is None else rfi_params(rfi_freq),
                        dilate=None if rfi_dilate is None else rfi_dilate_params(rfi_dilate))
    if r.dilate is not None and not (r.dilate["time"] > 0 or r.dilate["freq"] > 0):
        r.dilate = None
    r.any = r.time is not None or r.freq is not None or r.dilate is not None
    r.all_freqs = r.freq is not None or (r.dilate is not None and r.dilate["freq"] > 0)
    return r


def _rfi_chunks(who, freqs, chunk_gb, per_f, route):
    """`_freq_chunks`, unless a step of `route` runs along frequency: the one chunk is then all frequencies, and a
    `chunk_gb` it does not fit or more than one rank is a ValueError (ranks own frequencies, files are read whole)."""
    if not route.all_freqs:
        return _freq_chunks(freqs, chunk_gb, per_f)
    if parallel.size() > 1:
        raise ValueError("%s: flagging or dilation along frequency needs every frequency on one device, and this run has "
                         "%d ranks that own frequencies; run it on one rank" % (who, parallel.size()))
    need = per_f * len(freqs) / 2.0**30
    if need > chunk_gb:
        raise ValueError("%s: flagging or dilation along frequency needs every frequency on one device: chunk_gb >= %.4g "
                         "(given: %g)" % (who, need * 1.001, chunk_gb))
    return [freqs] if freqs else []


def _rfi_steps(ctx, x_d, w_d, route):
    """The steps of `route` on one chunk on the device, in their order: the time pass, the frequency pass on its
    weights, dilation along time, dilation along frequency.  Returns (w_d, the outputs of the time pass or None,
    the new flags of the frequency pass (nf, nrow) int32 or None, those added by dilation or None)."""
    torch = ctx.torch

    def fresh(before, after):
        new = (after == 0) if before is None else (after == 0) & (before > 0)
        return new.sum(dim=2).to(torch.int32)

    ref, tout, nfreq, ndil = w_d, None, None, None
    if route.time is not None:
        tout = ctx.rfi_flag(x_d, w=w_d, **route.time)
        w_d = tout[0]
    if route.freq is not None:
        w1 = ctx.rfi_flag_freq(x_d, w=w_d, **route.freq)[0]
        nfreq, w_d = fresh(w_d, w1), w1
    if route.dilate is not None:
        w0 = w_d
        if w_d is None:
            w_d = torch.ones(tuple(x_d.shape), dtype=torch.float64, device=x_d.device)
        for axis in ("time", "freq"):
            if route.dilate[axis] > 0:
                w_d = ctx.rfi_dilate(w_d, route.dilate[axis], axis=axis, ref=ref if route.dilate["new_only"] else None)[0]
        ndil = fresh(w0, w_d)
    return w_d, tout, nfreq, ndil


def rfi_flag(m, indir, outdir=None, chunk_gb=4.0, freq=None, dilate=None, **params):
    """Flag the interference in the Timestream directory `indir`, stacked or unstacked, along time on the device
    (`Context.rfi_flag`) and write the result to `outdir` (None: in place).  `params` are the
    parameters of `Context.rfi_flag` (an unknown key raises ValueError).  Every file keeps all its datasets and
    attributes; `weight` becomes the file's weight (ones where it had none) with the flagged samples at 0, the input
    weight is kept as `weight_input` when one was present, and `rfi_noise` (nrow, nseg), `rfi_nflag` (nrow,) and
    `rfi_occupancy` (ntime,) are the flagger's other outputs.  Ranks take their own frequencies in chunks that fit
    `chunk_gb`.  Returns the Timestream of the output.

    freq: a dict of the parameters of `Context.rfi_flag_freq` (the keys of `params`): the frequency pass then runs on the
    weights of the time pass.  dilate: a dict of `rfi_dilate_params` — the flags are then dilated along time, then along
    frequency.  Each file then also holds `rfi_freq_nflag` (nrow,) int32, the new flags of the
    frequency pass in that file, and `rfi_dilate_nflag` (nrow,), those added by dilation, for the steps that ran.  A step
    along frequency needs every frequency on one device: the one chunk is then all frequencies, and a `chunk_gb` that
    does not hold them, or more than one rank, raises ValueError."""
    p = rfi_params(params)
    route = _rfi_route(p, freq, dilate)
    tel = m.beamtransfer.telescope
    src, nrow, nt = _route_open("rfi_flag", m, indir, stacked_only=False, rows=False)
    inplace = outdir is None or os.path.abspath(outdir) == os.path.abspath(src.directory)
    dst = src if inplace else Timestream(outdir, m)
    freqs = _sim_freqs(tel, None)
    log = sim_log
    extra_steps = route.freq is not None or route.dilate is not None
    chunks = _rfi_chunks("rfi_flag", freqs, chunk_gb, nrow * nt * (48.0 if extra_steps else 32.0), route)
    ctx = get_context()
    for fs in chunks:
        with _StepTimer(log, "read"):
            chunk = _route_read("rfi_flag", src, fs, nrow, nt, whole=True)
        with _StepTimer(log, "rfi"):
            x_d, w_d = _route_upload(ctx, chunk)
            w_last, tout, nfreq, ndil = _rfi_steps(ctx, x_d, w_d, route)
            names = ("weight", "rfi_noise", "rfi_nflag", "rfi_occupancy", "rfi_freq_nflag", "rfi_dilate_nflag")
            new = {name: ctx.to_host(t) for name, t in zip(names, (w_last,) + tuple(tout[1:]) + (nfreq, ndil)) if t is not None}
            del x_d, w_d, w_last, tout, nfreq, ndil
        with _StepTimer(log, "write"):
            _route_rewrite(dst, chunk, new)
    _save_all([] if inplace else [dst])
    return dst


# ---- the delay fit along frequency -------------------------------------------------------

DELAY_MODES = ("model", "filter", "inpaint")
DELAY_C = 299.792458   # metres per microsecond
DELAY_DEFAULTS = dict(mode="inpaint", ridge=0.0, min_valid=None, horizon=1.0, buffer=2.0, nclass=8, eigencut=1e-10)


def _delay_limits():
    """(the most frequencies, the largest rank) `Context.delay_fit` takes: host-only queries of the library."""
    from . import _lib

    lib = _lib.load()
    return int(lib.dm_delay_max_nf()), int(lib.dm_delay_max_rank())


def _delay_cholesky_host(G):
    """Row by row (Cholesky-Banachiewicz) in the dtype of G: (L, info) with info = 0, or j + 1 for the first column j
    whose pivot is not finite or not > 0 (L is then filled up to that column only)."""
    r = G.shape[0]
    L = np.zeros_like(G)
    for j in range(r):
        d = G[j, j] - np.dot(L[j, :j], L[j, :j])
        if not (d > 0 and np.isfinite(d)):
            return L, j + 1
        L[j, j] = np.sqrt(d)
        if j + 1 < r:
            L[j + 1 :, j] = (G[j + 1 :, j] - L[j + 1 :, :j] @ L[j, :j]) / L[j, j]
    return L, 0


def _delay_lower_solve_host(L, B, transpose=False):
    """L Y = B (or L^T Y = B) by substitution in the dtype of L; B (r, n)."""
    r = L.shape[0]
    Y = np.array(B, dtype=np.result_type(L.dtype, B.dtype), copy=True)
    order = range(r - 1, -1, -1) if transpose else range(r)
    for j in order:
        Y[j] = Y[j] / L[j, j]
        if transpose:
            Y[:j] -= np.outer(L[j, :j], Y[j])
        else:
            Y[j + 1 :] -= np.outer(L[j + 1 :, j], Y[j])
    return Y


def delay_fit_host(x, w, basis, basis_of, mode="inpaint", ridge=0.0, min_valid=None, dtype=np.float64, details=False):
    """The numpy statement of `Context.delay_fit`: x (nf, nrow, nt) complex, w of that shape or
    None, basis a sequence of real matrices A_k (nf, r_k), basis_of (nrow,) ints.  Per (row, t): kept iff w > 0, omega =
    w on kept samples and 0 elsewhere, x under a flag is selected out; nvalid < min_valid (None or <= 0: the rank) or
    nvalid = 0 gives info = -1; G = A^T diag(omega) A + ridge mean(omega) I; a Cholesky pivot that is not finite or not
    > 0 at column j gives info = j + 1; c = G^-1 A^T diag(omega) x, model = A c, v_f = a_f^T G^-1 a_f; a basis_of entry
    outside the table gives info = -2.  dtype float64 solves with LAPACK (`numpy.linalg.solve`), longdouble with the
    factor in long double.  Returns (x_out, w_out, info) as the modes of the device define them, x_out complex of twice
    `dtype`'s width; with details=True also a dict with model (nf, nrow, nt), c (nrow, nt, rmax), v (nf, nrow, nt), kappa
    (nrow, nt) — kappa_2(G) — kept (nf, nrow, nt), and anorm (nf, nrow), |a_f|_2 of the row's basis."""
    if mode not in DELAY_MODES:
        raise ValueError('delay_fit: mode is "model", "filter" or "inpaint"')
    real = np.dtype(dtype).type
    if real not in (np.float64, np.longdouble):
        raise ValueError("delay_fit_host: dtype is float64 or longdouble")
    ctype = np.complex128 if real is np.float64 else np.clongdouble
    if not (np.isfinite(ridge) and ridge >= 0):
        raise ValueError("delay_fit: ridge not finite or negative")
    x = np.asarray(x)
    if x.ndim != 3 or (w is not None and np.shape(w) != x.shape):
        raise ValueError("delay_fit_host: x (nf, nrow, nt) and w of that shape or None expected")
    nf, nrow, nt = x.shape
    bases = [np.asarray(a, dtype=np.float64) for a in basis]
    if any(a.ndim != 2 or a.shape[0] != nf or not 1 <= a.shape[1] <= nf for a in bases):
        raise ValueError("delay_fit_host: basis must be a sequence of real matrices (nf, r_k), 1 <= r_k <= nf")
    rmax = max([a.shape[1] for a in bases] + [1])
    wv = np.ones(x.shape) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        kept = wv > 0
    om = np.where(kept, wv, 0.0)
    xk = np.where(kept, x, 0.0).astype(ctype)
    x_out = np.zeros(x.shape, dtype=ctype) if mode == "model" else xk.copy()
    w_out = om.astype(real)
    info = np.zeros((nrow, nt), dtype=np.int32)
    model = np.zeros(x.shape, dtype=ctype)
    cs = np.zeros((nrow, nt, rmax), dtype=ctype)
    v = np.zeros(x.shape, dtype=real)
    kappa = np.zeros((nrow, nt))
    anorm = np.zeros((nf, nrow))
    for row in range(nrow):
        k = int(basis_of[row])
        if not 0 <= k < len(bases):
            info[row] = -2
            continue
        A = bases[k].astype(real)
        r = A.shape[1]
        anorm[:, row] = np.sqrt((bases[k] ** 2).sum(axis=1))
        need = r if min_valid is None or int(min_valid) <= 0 else int(min_valid)
        for t in range(nt):
            o = om[:, row, t].astype(real)
            nvalid = int(kept[:, row, t].sum())
            if nvalid < need or nvalid == 0:
                info[row, t] = -1
                continue
            G = (A * o[:, None]).T @ A + real(ridge) * (o.sum() / real(nf)) * np.eye(r, dtype=real)
            L, bad = _delay_cholesky_host(G)
            if bad:
                info[row, t] = bad
                continue
            rhs = A.T @ (o * xk[:, row, t])
            if real is np.float64:
                sol = np.linalg.solve(G, np.concatenate([rhs[:, None], A.T.astype(ctype)], axis=1))
                c, Z = sol[:, 0], sol[:, 1:].real
                vf = np.einsum("fr,rf->f", A, Z)
            else:
                c = _delay_lower_solve_host(L, _delay_lower_solve_host(L, rhs[:, None]), transpose=True)[:, 0]
                Y = _delay_lower_solve_host(L, A.T)
                vf = (Y * Y).sum(axis=0)
            mod = A @ c
            model[:, row, t], cs[row, t, :r], v[:, row, t] = mod, c, vf
            kappa[row, t] = np.linalg.cond(G.astype(np.float64))
            kp = kept[:, row, t]
            if mode == "model":
                x_out[:, row, t] = mod
            elif mode == "filter":
                x_out[kp, row, t] = xk[kp, row, t] - mod[kp]
            else:
                x_out[~kp, row, t] = mod[~kp]
                with np.errstate(divide="ignore", invalid="ignore"):
                    fill = np.where((vf > 0) & np.isfinite(vf), 1 / vf, 0)
                w_out[~kp, row, t] = fill[~kp]
    if details:
        return x_out, w_out, info, dict(model=model, c=cs, v=v, kappa=kappa, kept=kept, anorm=anorm)
    return x_out, w_out, info


def delay_basis(freqs_mhz, tau_us, eigencut=1e-10):
    """The band-limited basis of the delays |tau| <= tau_us on the frequency grid freqs_mhz (any grid, gaps included):
    the eigenvectors of S_ij = sinc(2 tau (nu_i - nu_j)) (numpy's normalised sinc: the covariance of a flat delay
    spectrum over the band) with eigenvalue >= eigencut lambda_max, in descending order.  Returns (A (nf, r), the r
    eigenvalues).  A rank above `dm_delay_max_rank()` raises ValueError."""
    nu = np.asarray(freqs_mhz, dtype=np.float64).reshape(-1)
    tau = float(tau_us)
    if nu.size < 1 or not (np.isfinite(tau) and tau >= 0) or not (0 < eigencut < 1):
        raise ValueError("delay_basis: at least one frequency, a finite tau >= 0 and 0 < eigencut < 1 expected")
    S = np.sinc(2.0 * tau * (nu[:, None] - nu[None, :]))
    lam, vec = np.linalg.eigh(S)
    lam, vec = lam[::-1], vec[:, ::-1]
    r = int((lam >= eigencut * lam[0]).sum())
    rmax = _delay_limits()[1]
    if r > rmax:
        raise ValueError("delay_basis: rank %d > %d: the bandwidth x delay product 2 B tau = %.4g (B = %.6g MHz, tau = %.6g us) "
                         "is too large; lower the horizon or buffer, raise eigencut or fit fewer frequencies"
                         % (r, rmax, 2.0 * (nu.max() - nu.min()) * tau, nu.max() - nu.min(), tau))
    return np.ascontiguousarray(vec[:, :r]), lam[:r].copy()


def delay_class_ceilings(tau, nclass=8):
    """At most nclass ceilings equally spaced over [min tau, max tau] (the last one max tau itself) and, per row, the
    index of the smallest ceiling >= its tau among those in use: (ceilings in use, ascending; basis_of int32)."""
    tau = np.asarray(tau, dtype=np.float64).reshape(-1)
    nclass = int(nclass)
    if nclass < 1 or tau.size < 1 or not np.all(np.isfinite(tau)):
        raise ValueError("delay_classes: nclass >= 1 and finite tau expected")
    lo, hi = float(tau.min()), float(tau.max())
    ceil = np.array([lo + (hi - lo) * (k + 1) / nclass for k in range(nclass)])
    ceil[-1] = hi
    ceil = np.maximum.accumulate(ceil)
    which = np.array([int(np.nonzero(ceil >= t)[0][0]) for t in tau])
    used = np.unique(which)
    return ceil[used], np.searchsorted(used, which).astype(np.int32)


def delay_classes(tel, horizon=1.0, buffer=2.0, nclass=8, eigencut=1e-10):
    """The delay classes of the stacked rows of telescope `tel`: tau_row = horizon |b_row| / c + buffer / (nf dnu) in
    microseconds (c = 299.792458 m / us; the buffer in delay-resolution elements of the band), binned by
    `delay_class_ceilings`, one `delay_basis` per ceiling in use.  Returns (table, ranks, basis_of, tau): the packed
    table of `Context.delay_fit` (float64, basis k as (r_k, nf) row-major behind the bases before it), ranks int32,
    basis_of (nrow,) int32 and the tau of every row."""
    nu = np.asarray(tel.frequencies, dtype=np.float64)
    nf = nu.size
    if nf < 2:
        raise ValueError("delay_classes: at least two frequencies expected")
    if not (np.isfinite(horizon) and horizon >= 0 and np.isfinite(buffer) and buffer >= 0):
        raise ValueError("delay_classes: horizon and buffer must be finite and >= 0")
    dnu = float(np.median(np.abs(np.diff(nu))))
    blen = np.sqrt((np.asarray(tel.baselines, dtype=np.float64) ** 2).sum(axis=1))
    tau = float(horizon) * blen / DELAY_C + float(buffer) / (nf * dnu)
    ceil, basis_of = delay_class_ceilings(tau, nclass)
    bases = [delay_basis(nu, t, eigencut)[0] for t in ceil]
    table = np.concatenate([a.T.reshape(-1) for a in bases])
    return table, np.array([a.shape[1] for a in bases], dtype=np.int32), basis_of, tau


def delay_params(d=None):
    """The `delay` dict of a route with its defaults filled in: `mode`, `ridge` and `min_valid` of `Context.delay_fit`,
    `horizon`, `buffer`, `nclass` and `eigencut` of `delay_classes`.  An unknown key raises ValueError, and so does a
    value the steps refuse."""
    out = _conf_filled(d, DELAY_DEFAULTS, "delay: unknown key(s) %s (known: %s)", show=", ".join)
    if out["mode"] not in DELAY_MODES:
        raise ValueError('delay: mode is "model", "filter" or "inpaint"')
    out["ridge"], out["horizon"], out["buffer"] = float(out["ridge"]), float(out["horizon"]), float(out["buffer"])
    out["eigencut"], out["nclass"] = float(out["eigencut"]), int(out["nclass"])
    out["min_valid"] = None if out["min_valid"] is None else int(out["min_valid"])
    if not (np.isfinite(out["ridge"]) and out["ridge"] >= 0):
        raise ValueError("delay: ridge not finite or negative")
    if not (np.isfinite(out["horizon"]) and out["horizon"] >= 0 and np.isfinite(out["buffer"]) and out["buffer"] >= 0):
        raise ValueError("delay: horizon and buffer must be finite and >= 0")
    if out["nclass"] < 1 or not 0 < out["eigencut"] < 1:
        raise ValueError("delay: nclass >= 1 and 0 < eigencut < 1 expected")
    return out


def _delay_one_rank(who):
    if parallel.size() > 1:
        raise ValueError("%s: the fit along frequency needs every frequency on one device, and this run has "
                         "%d ranks that own frequencies; run it on one rank" % (who, parallel.size()))


def delay_filter(m, indir, outdir=None, mode="inpaint", chunk_gb=4.0, ridge=0.0, min_valid=None, **classes):
    """The delay fit along frequency on the stacked Timestream directory `indir` (`Context.delay_fit`, DESIGN.md section
    4.23), written to `outdir` (None: in place): every row is fitted with the band-limited basis of its delay class
    (`delay_classes` with the keywords `classes`), and by `mode` the flagged samples are filled from the fit
    ("inpaint"), the fit is subtracted ("filter") or the fit replaces the data ("model").  Every file keeps its datasets
    and attributes; `timestream` and `weight` are replaced (ones where the file had no weight), the first input weight
    is kept as `weight_input`, and `delay_filled` (nrow,) int32 counts the samples of the file that were filled.
    `delay_fit.hdf5` at the root of the output holds `info` (nrow, ntime) int32, `basis_of`, `tau`, `rank` and the
    parameters as attributes.  The fit needs every frequency of a row at once, so the device takes chunks of rows over
    all frequency files that fit `chunk_gb`; more than one rank raises ValueError, and so does an unstacked directory.
    `chunk_gb` bounds the device only: the host holds every dataset of every frequency file and the two outputs at
    once, a little over twice the directory.  Returns the Timestream of the output."""
    p = delay_params(dict(classes, mode=mode, ridge=ridge, min_valid=min_valid))
    _delay_one_rank("delay_filter")
    tel = m.beamtransfer.telescope
    src, nrow, nt = _route_open("delay_filter", m, indir)
    inplace = outdir is None or os.path.abspath(outdir) == os.path.abspath(src.directory)
    dst = src if inplace else Timestream(outdir, m)
    nf = int(tel.nfreq)
    table, ranks, basis_of, tau = delay_classes(tel, horizon=p["horizon"], buffer=p["buffer"], nclass=p["nclass"],
                                                eigencut=p["eigencut"])
    log = sim_log
    with _StepTimer(log, "read"):
        chunk = _route_read("delay_filter", src, range(nf), nrow, nt, whole=True)
    ranges = _row_chunks("delay_filter", nrow, chunk_gb, 48.0 * nf * nt)
    ctx = get_context()
    torch = ctx.torch
    x_out = np.empty((nf, nrow, nt), dtype=np.complex128)
    w_out = np.empty((nf, nrow, nt), dtype=np.float64)
    info = np.empty((nrow, nt), dtype=np.int32)
    filled = np.zeros((nf, nrow), dtype=np.int32)
    with _StepTimer(log, "delay"):
        table_d = ctx.to_device(table)
        for r0, r1 in ranges:
            x_d, w_d = _route_upload(ctx, chunk, r0, r1)
            of_d = ctx.to_device(np.ascontiguousarray(basis_of[r0:r1]))
            xo, wo, io = ctx.delay_fit(x_d, w=w_d, basis=(table_d, ranks), basis_of=of_d, mode=p["mode"], ridge=p["ridge"],
                                       min_valid=p["min_valid"])
            if p["mode"] == "inpaint" and w_d is not None:
                filled[:, r0:r1] = ctx.to_host((~(w_d > 0) & (io == 0)[None]).sum(dim=2).to(torch.int32))
            x_out[:, r0:r1], w_out[:, r0:r1], info[r0:r1] = ctx.to_host(xo), ctx.to_host(wo), ctx.to_host(io)
            del x_d, w_d, of_d, xo, wo, io
    with _StepTimer(log, "write"):
        _route_rewrite(dst, chunk, dict(timestream=x_out, weight=w_out, delay_filled=filled))
        os.makedirs(dst.directory, exist_ok=True)
        _write_hdf5(os.path.join(dst.directory, "delay_fit.hdf5"), dict(info=info, basis_of=basis_of, tau=tau, rank=ranks),
                    {name: -1 if value is None else value for name, value in p.items()})
    unsolved = int((info != 0).sum())
    if unsolved:
        logging.getLogger(__name__).warning("delay_filter: %d of %d series were not solved (info in delay_fit.hdf5)", unsolved, info.size)
    _save_all([] if inplace else [dst])
    return dst


# ---- ring maps: the north-south beamformer of stacked visibilities -----------------------

RINGMAP_WEIGHTINGS = ("natural", "uniform")
RINGMAP_WINDOWS = (None, "hann", "blackman")


def ringmap_groups(tel, ew=None, intracyl=True):
    """The groups of a ring map of telescope `tel` (any TransitTelescope): a group is the set of unique baselines with
    the same (beam class of feed i, beam class of feed j, rounded east-west separation u).  Returns a dict: `group_off`
    (ngroup + 1) int32, `members` int32 (rows of the stacked data) and `v` (their signed north-south separation in m,
    north positive), and per group `u` (m) and `pol` (ngroup, 2), the class pair.  Groups are ordered by (class pair, u),
    the members of a group by v, then index.  `ew` picks east-west separations (in m, compared as the baselines are:
    rounded to the telescope's tolerance); intracyl=False drops u = 0."""
    pairs = np.asarray(tel.uniquepairs).reshape(-1, 2)
    cls = np.asarray(tel.beamclass)
    bl = np.asarray(tel.baselines, dtype=np.float64).reshape(-1, 2)
    tol = int(getattr(tel, "_bl_tol", 6))
    u = np.around(bl[:, 0], tol) + 0.0   # -0 -> 0
    keep = np.ones(u.shape[0], dtype=bool)
    if ew is not None:
        want = np.around(np.atleast_1d(np.asarray(ew, dtype=np.float64)), tol)
        if want.ndim != 1:
            raise ValueError("ringmap_groups: ew must be a list of east-west separations")
        keep &= np.isin(u, want)
    if not intracyl:
        keep &= u != 0
    idx = np.nonzero(keep)[0]
    ci, cj = cls[pairs[idx, 0]], cls[pairs[idx, 1]]
    order = np.lexsort((idx, bl[idx, 1], u[idx], cj, ci))   # last key first: (ci, cj, u, v, index)
    idx, ci, cj = idx[order], ci[order], cj[order]
    ug = u[idx]
    new = np.ones(idx.shape[0], dtype=bool)
    new[1:] = (ci[1:] != ci[:-1]) | (cj[1:] != cj[:-1]) | (ug[1:] != ug[:-1])
    first = np.nonzero(new)[0]
    return dict(group_off=np.concatenate([first, [idx.shape[0]]]).astype(np.int32), members=idx.astype(np.int32),
                v=np.ascontiguousarray(bl[idx, 1]), u=np.ascontiguousarray(ug[first]),
                pol=np.stack([ci[first], cj[first]], axis=1).astype(np.int32).reshape(-1, 2))


def ringmap_taper(tel, groups, weighting="natural", window=None):
    """The taper T_b of every member of `groups` (`ringmap_groups`): the redundancy of the baseline ("natural") or 1
    ("uniform"), times the window "hann" or "blackman" evaluated at v / v_edge; v_edge is the largest |v| plus the
    smallest nonzero |v| of the table, so that no baseline gets weight 0."""
    if weighting not in RINGMAP_WEIGHTINGS:
        raise ValueError('ringmap_taper: weighting is "natural" or "uniform"')
    if window not in RINGMAP_WINDOWS:
        raise ValueError('ringmap_taper: window is None, "hann" or "blackman"')
    members, v = np.asarray(groups["members"]), np.asarray(groups["v"], dtype=np.float64)
    t = np.asarray(tel.redundancy, dtype=np.float64)[members] if weighting == "natural" else np.ones(members.shape[0])
    if window is not None and v.size:
        av = np.abs(v)
        edge = av.max() + (av[av > 0].min() if np.any(av > 0) else 0.0)
        x = v / edge if edge > 0 else np.zeros_like(v)
        if window == "hann":
            t = t * (0.5 + 0.5 * np.cos(np.pi * x))
        else:
            t = t * (0.42 + 0.5 * np.cos(np.pi * x) + 0.08 * np.cos(2 * np.pi * x))
    return np.ascontiguousarray(t, dtype=np.float64)


def ringmap_sinza(tel, groups, nel=None):
    """`nel` points uniform on [-1, 1], the sin(zenith angle) grid of a ring map (north positive).  The default is the
    smallest odd count (3 at the least) with two points per period of the finest fringe, that of the largest |v| of
    `groups` at the highest frequency: a step of at most 1 / (2 |v| nu / c)."""
    if nel is None:
        v = np.asarray(groups["v"], dtype=np.float64)
        turns = float(np.abs(v).max() / np.min(tel.wavelengths)) if v.size else 0.0   # the fringe rate over s, periods per unit
        nel = max(3, int(np.ceil(4.0 * turns)) + 1)
        nel += 1 - nel % 2
    nel = int(nel)
    if nel < 1:
        raise ValueError("ringmap_sinza: nel < 1")
    return np.linspace(-1.0, 1.0, nel) if nel > 1 else np.zeros(1)


def ringmap_host(vis, w, group_off, members, v, scale, sinza, taper=None, parts=1, dtype=np.float64):
    """The numpy statement of `Context.ringmap` in `dtype`, np.float64 or np.longdouble: for
    frequency f, group g, elevation e and sample t
        x_b(t) = T_b w_b(t) where w_b(t) > 0 and 0 elsewhere,   D = sum_b x_b,   D2 = sum_b T_b x_b,
        tau = (scale_f v_b) s_e,   phi = tau - rint(tau),   map[0] = sum_b x_b Re(V_b exp(-2 pi i phi)) / D,
        map[1] the imaginary part (parts = 2); 0 where D = 0,
    with cos and sin of pi (2 phi) taken of the fraction of a turn, never of the large argument.  vis (nf, nrow, nt)
    complex, w of that shape or None (ones), taper per member or None (ones).  Samples that are not kept enter no
    arithmetic.  Returns (map (nf, ngroup, parts, nel, nt), D, D2 (nf, ngroup, nt))."""
    if dtype not in (np.float64, np.longdouble):
        raise ValueError("ringmap_host: dtype is np.float64 or np.longdouble")
    if parts not in (1, 2):
        raise ValueError("ringmap_host: parts is 1 or 2")
    vis = np.asarray(vis)
    if vis.ndim != 3 or not np.iscomplexobj(vis):
        raise ValueError("ringmap_host: complex vis (nf, nrow, nt) expected")
    nf, nrow, nt = vis.shape
    if w is not None and np.shape(w) != vis.shape:
        raise ValueError("ringmap_host: w must have the shape of vis")
    off, mem = np.asarray(group_off, dtype=np.int64), np.asarray(members, dtype=np.int64)
    if off.ndim != 1 or off.size < 1 or mem.ndim != 1 or off[0] != 0 or np.any(np.diff(off) < 0) or mem.size != off[-1]:
        raise ValueError("ringmap_host: group_off (ngroup + 1), from 0 and not decreasing, and members (group_off[-1]) expected")
    if mem.size and (mem.min() < 0 or mem.max() >= nrow):
        raise ValueError("ringmap_host: a member is no row of vis")
    v, scale, sinza = (np.asarray(a, dtype=np.float64) for a in (v, scale, sinza))
    if v.shape != mem.shape or scale.shape != (nf,) or sinza.ndim != 1:
        raise ValueError("ringmap_host: v per member, scale (nf,) and sinza (nel,) expected")
    if taper is not None and np.shape(taper) != mem.shape:
        raise ValueError("ringmap_host: taper must hold one value per member")
    T = np.ones(mem.size, dtype=dtype) if taper is None else np.asarray(taper, dtype=np.float64).astype(dtype)
    ngroup, nel = off.size - 1, sinza.size
    pi = _ld_pi() if dtype is np.longdouble else np.pi
    out = np.zeros((nf, ngroup, parts, nel, nt), dtype=dtype)
    D, D2 = np.zeros((nf, ngroup, nt), dtype=dtype), np.zeros((nf, ngroup, nt), dtype=dtype)
    for f in range(nf):
        for g in range(ngroup):
            sl = slice(off[g], off[g + 1])
            rows = mem[sl]
            if rows.size == 0:
                continue
            kept = np.ones((rows.size, nt), dtype=bool) if w is None else np.asarray(w[f, rows]) > 0
            wg = np.ones((rows.size, nt), dtype=dtype) if w is None else np.where(kept, np.asarray(w[f, rows]), 0.0).astype(dtype)
            x = np.where(kept, T[sl, None] * wg, 0)
            xr = np.where(kept, x * np.where(kept, vis[f, rows].real, 0).astype(dtype), 0)
            xi = np.where(kept, x * np.where(kept, vis[f, rows].imag, 0).astype(dtype), 0)
            tau = (scale[f].astype(dtype) * v[sl].astype(dtype))[:, None] * sinza.astype(dtype)[None, :]   # (nb, nel)
            ph = pi * (2 * (tau - np.rint(tau)))   # sincospi of twice the exact fraction of a turn
            c, s = np.cos(ph), np.sin(ph)
            d = x.sum(axis=0) if dtype is np.longdouble else np.add.accumulate(x, axis=0)[-1]
            d2 = (T[sl, None] * x).sum(axis=0) if dtype is np.longdouble else np.add.accumulate(T[sl, None] * x, axis=0)[-1]
            ok = d != 0
            dd = np.where(ok, d, 1)
            out[f, g, 0] = np.where(ok, (c.T @ xr + s.T @ xi) / dd, 0)
            if parts == 2:
                out[f, g, 1] = np.where(ok, (c.T @ xi - s.T @ xr) / dd, 0)
            D[f, g], D2[f, g] = np.where(ok, d, 0), np.where(ok, d2, 0)
    return out, D, D2


RINGMAP_DEFAULTS = dict(name="ringmap", nel=None, weighting="natural", window=None, ew=None, intracyl=True, parts=1,
                        collapse_ew=False)


def ringmap_params(d=None):
    """One entry of the pipeline's `ringmaps` list with its defaults filled in; an unknown key raises ValueError."""
    out = _conf_filled(d, RINGMAP_DEFAULTS, "ringmaps: unknown key(s) %s (known: %s)", show=", ".join)
    if out["weighting"] not in RINGMAP_WEIGHTINGS or out["window"] not in RINGMAP_WINDOWS or out["parts"] not in (1, 2):
        raise ValueError('ringmaps: weighting is "natural" or "uniform", window None, "hann" or "blackman", parts 1 or 2')
    return out


def ringmap(m, indir, name="ringmap", nel=None, sinza=None, weighting="natural", window=None, ew=None, intracyl=True,
            parts=1, collapse_ew=False, chunk_gb=4.0):
    """Ring maps of the stacked Timestream directory `indir` (`Context.ringmap`): the
    visibilities of every sample beamformed north-south onto the grid `sinza` (None: `ringmap_sinza` with `nel`), one
    map per frequency and group of `ringmap_groups(tel, ew, intracyl)`, tapered by `ringmap_taper(weighting, window)`.
    It needs no products beyond the telescope; the dataset `weight` of a file is honoured sample by sample.  Ranks take
    their own frequencies in chunks that fit `chunk_gb`; each frequency gets `ringmap_<name>.hdf5` beside its
    timestream file, holding `map` (ngroup, parts, nel, ntime), `norm` and `norm2` (ngroup, ntime), and with
    collapse_ew `map_sum` (npol, parts, nel, ntime): the groups of one class pair combined as sum_g D_g map_g / sum_g D_g
    (0 where that sum is 0) and `norm_sum`.  Rank 0 writes `ringmap_<name>.hdf5` at the root: `sinza`, `phi`,
    `group_off`, `members`, `v`, `u`, `pol`, `taper`, with collapse_ew `pol_sum` and `group_pol` (the row of `map_sum`
    every group goes to), and the parameters as attributes.  The written bits do not depend on `chunk_gb`.  An unstacked
    directory raises ValueError.  Returns the path of the root file."""
    ringmap_params(dict(weighting=weighting, window=window, parts=parts))
    tel = m.beamtransfer.telescope
    src, nrow, nt = _route_open("ringmap", m, indir)
    groups = ringmap_groups(tel, ew=ew, intracyl=intracyl)
    ngroup = groups["group_off"].shape[0] - 1
    if ngroup == 0:
        raise ValueError("ringmap: no baseline is selected (ew = %s, intracyl = %s)" % (ew, intracyl))
    taper = ringmap_taper(tel, groups, weighting=weighting, window=window)
    sinza = ringmap_sinza(tel, groups, nel) if sinza is None else np.ascontiguousarray(sinza, dtype=np.float64)
    if sinza.ndim != 1 or sinza.size < 1 or (nel is not None and int(nel) != sinza.size) or not np.all(np.abs(sinza) <= 1):
        raise ValueError("ringmap: sinza must be a list of values in [-1, 1]%s" % ("" if nel is None else " of nel entries"))
    nel = int(sinza.size)
    scale = np.ascontiguousarray(1.0 / np.asarray(tel.wavelengths, dtype=np.float64))
    freqs = _sim_freqs(tel, None)
    upol, group_pol = np.unique(groups["pol"], axis=0, return_inverse=True)
    group_pol = np.asarray(group_pol).reshape(-1)
    per_f = 24.0 * nrow * nt + 8.0 * ngroup * nt * (parts * nel + 2) + (16.0 * len(upol) * nt * parts * nel if collapse_ew else 0.0)
    log = sim_log
    ctx = get_context()
    torch = ctx.torch
    tabs = {k: ctx.to_device(a) for k, a in (("v", groups["v"]), ("taper", taper), ("sinza", sinza))}
    for fs in _freq_chunks(freqs, chunk_gb, per_f):
        with _StepTimer(log, "read"):
            chunk = _route_read("ringmap", src, fs, nrow, nt)
        with _StepTimer(log, "ringmap"):
            x_d, w_d = _route_upload(ctx, chunk)
            mp, nm, nm2 = ctx.ringmap(x_d, groups["group_off"], groups["members"], tabs["v"], ctx.to_device(scale[fs]),
                                      tabs["sinza"], w=w_d, taper=tabs["taper"], parts=parts)
            data = dict(map=ctx.to_host(mp), norm=ctx.to_host(nm), norm2=ctx.to_host(nm2))
            if collapse_ew:
                msum = torch.zeros((len(fs), len(upol), parts, nel, nt), dtype=torch.float64, device=mp.device)
                dsum = torch.zeros((len(fs), len(upol), nt), dtype=torch.float64, device=mp.device)
                for g in range(ngroup):   # in group order: the bits of a sum do not depend on the chunk
                    msum[:, group_pol[g]] += nm[:, g, None, None, :] * mp[:, g]
                    dsum[:, group_pol[g]] += nm[:, g]
                ok = dsum != 0
                msum = torch.where(ok[:, :, None, None, :], msum / torch.where(ok, dsum, torch.ones_like(dsum))[:, :, None, None, :],
                                   torch.zeros_like(msum))
                data.update(map_sum=ctx.to_host(msum), norm_sum=ctx.to_host(dsum))
                del msum, dsum
            del x_d, w_d, mp, nm, nm2
        with _StepTimer(log, "write"):
            _route_write_products(src, fs, "ringmap", name, data)
    root = os.path.join(src.directory, "ringmap_%s.hdf5" % name)
    if parallel.rank0():
        tables = dict({key: groups[key] for key in ("group_off", "members", "v", "u", "pol")}, sinza=sinza, phi=_dir_phi(src, nt),
                      taper=taper)
        if collapse_ew:
            tables.update(pol_sum=upol.astype(np.int32), group_pol=group_pol.astype(np.int32))
        if ew is not None:
            tables["ew"] = np.atleast_1d(np.asarray(ew, dtype=np.float64))
        _write_hdf5(root, tables, dict(nel=nel, weighting=weighting, window=window or "none", intracyl=int(bool(intracyl)),
                                       parts=int(parts), collapse_ew=int(bool(collapse_ew)), ntime=nt))
    parallel.barrier()
    return root


# ---- formed beams: tracking beams on catalogue positions from stacked visibilities --------

def formedbeam_groups(tel, ew=None, intracyl=True):
    """The groups of a formed beam of telescope `tel`: a group is a beam-class pair, the groups of `ringmap_groups` (same
    selection `ew`, `intracyl`) merged over u.  Returns a dict: `group_off` (ngroup + 1) int32, `members` int32 (rows of
    the stacked data), `u` and `v` per member (m, east and north positive, both rounded to the telescope's tolerance, so
    that baselines the telescope holds equal share their phase), `pol` (ngroup, 2), and the distinct values `uvals`,
    `vvals` (ascending) with `iu`, `iv` int32 per member: uvals[iu] == u and vvals[iv] == v exactly.  Groups are ordered
    by class pair, the members of a group by (v, u, index): runs of equal v are neighbours."""
    rg = ringmap_groups(tel, ew=ew, intracyl=intracyl)
    rows = np.asarray(rg["members"], dtype=np.int64)
    cls = np.asarray(tel.beamclass)
    pairs = np.asarray(tel.uniquepairs).reshape(-1, 2)
    bl = np.asarray(tel.baselines, dtype=np.float64).reshape(-1, 2)
    tol = int(getattr(tel, "_bl_tol", 6))
    u, v = np.around(bl[rows, 0], tol) + 0.0, np.around(bl[rows, 1], tol) + 0.0
    ci, cj = cls[pairs[rows, 0]], cls[pairs[rows, 1]]
    order = np.lexsort((rows, u, v, cj, ci))
    rows, u, v, ci, cj = rows[order], u[order], v[order], ci[order], cj[order]
    new = np.ones(rows.shape[0], dtype=bool)
    new[1:] = (ci[1:] != ci[:-1]) | (cj[1:] != cj[:-1])
    first = np.nonzero(new)[0]
    uvals, iu = np.unique(u, return_inverse=True)
    vvals, iv = np.unique(v, return_inverse=True)
    return dict(group_off=np.concatenate([first, [rows.shape[0]]]).astype(np.int32), members=rows.astype(np.int32),
                u=np.ascontiguousarray(u), v=np.ascontiguousarray(v),
                pol=np.stack([ci[first], cj[first]], axis=1).astype(np.int32).reshape(-1, 2),
                uvals=np.ascontiguousarray(uvals, dtype=np.float64), vvals=np.ascontiguousarray(vvals, dtype=np.float64),
                iu=np.asarray(iu).reshape(-1).astype(np.int32), iv=np.asarray(iv).reshape(-1).astype(np.int32))


def formedbeam_tables(theta_zenith, theta):
    """The per-source constants of the formed beam for sources at polar angle `theta` under a zenith at `theta_zenith`,
    computed in long double and rounded to float64: `sinth` = sin(theta), `yc0` = sin(theta_z) cos(theta), `yc1` =
    cos(theta_z) sin(theta) (y = yc0 - yc1 cos(D)), `zc0` = cos(theta_z) cos(theta), `zc1` = sin(theta_z) sin(theta)
    (z = zc0 + zc1 cos(D))."""
    ld = np.longdouble
    tz, th = ld(theta_zenith), np.asarray(theta, dtype=np.float64).reshape(-1).astype(ld)
    f64 = lambda a: np.ascontiguousarray(np.asarray(a, dtype=ld).astype(np.float64))
    return dict(sinth=f64(np.sin(th)), yc0=f64(np.sin(tz) * np.cos(th)), yc1=f64(np.cos(tz) * np.sin(th)),
                zc0=f64(np.cos(tz) * np.cos(th)), zc1=f64(np.sin(tz) * np.sin(th)))


def formedbeam_z(tabs, turn, k, ntime):
    """z = zc0 + zc1 cos(2 pi (turn - k / ntime)) of every source at its sample k, in long double from the tables."""
    ld = np.longdouble
    d = np.asarray(turn, dtype=np.float64).astype(ld) - np.asarray(k).astype(ld) / ld(ntime)
    d = d - np.rint(d)
    return tabs["zc0"].astype(ld) + tabs["zc1"].astype(ld) * np.cos(2 * _ld_pi() * d)


def formedbeam_windows(tel, theta, phi, ntime, ha_max, zmin=0.05, scale_dec=True):
    """The windows of the sources at (theta, phi) in data of `ntime` uniform samples (the zenith is at phi_k = 2 pi k /
    ntime at sample k): a dict with `turn` (phi as a fraction of a turn in [0, 1), float64), `k0` = rint(turn ntime) mod
    ntime and `half` = H, int32; source s takes the samples k0 - H .. k0 + H (mod ntime).  H = floor(ha / (2 pi / ntime))
    with ha = ha_max, or with scale_dec ha_max / sin(theta) capped at a quarter turn (the same arc on the sky at every
    declination); 2 H + 1 <= ntime; H is then lowered until z >= zmin at both ends of the window, to -1 (the source is
    dropped) where even the transit sample is below zmin.  Computed in long double from the float64 tables."""
    ld = np.longdouble
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    phi = np.asarray(phi, dtype=np.float64).reshape(-1)
    ntime = int(ntime)
    if theta.shape != phi.shape or ntime < 1 or not ha_max >= 0:
        raise ValueError("formedbeam_windows: theta and phi of one length, ntime >= 1 and ha_max >= 0 expected")
    two_pi = 2 * _ld_pi()
    t = phi.astype(ld) / two_pi
    turn = np.asarray(t - np.floor(t), dtype=ld).astype(np.float64)
    turn = np.where(turn >= 1.0, 0.0, turn)
    k0 = np.rint(turn.astype(ld) * ntime).astype(np.int64) % ntime
    steps = np.full(theta.shape, ld(ha_max) / (two_pi / ntime), dtype=ld)
    cap = (ntime - 1) // 2
    if scale_dec:
        sth = np.abs(np.sin(theta.astype(ld)))
        steps = np.where(sth * ntime > steps, steps / np.where(sth > 0, sth, 1), ntime)
        cap = min(cap, ntime // 4)
    half = np.minimum(np.floor(np.minimum(steps, ntime)).astype(np.int64), cap)
    tabs = formedbeam_tables(tel.zenith[0], theta)
    while True:
        live = half >= 0
        hh = np.where(live, half, 0)
        low = live & ((formedbeam_z(tabs, turn, k0 - hh, ntime) < zmin) | (formedbeam_z(tabs, turn, k0 + hh, ntime) < zmin))
        if not low.any():
            break
        half = np.where(low, half - 1, half)
    return dict(turn=np.ascontiguousarray(turn), k0=k0.astype(np.int32), half=half.astype(np.int32))


def formedbeam_env(wavelengths, envelope_fwhm):
    """env_f = 4 ln 2 / (envelope_fwhm lambda_f)^2, the exponent of the east-west envelope exp(-env x^2) whose full width
    at half maximum in the direction cosine x is envelope_fwhm per metre of wavelength; None: zeros (no envelope)."""
    lam = np.asarray(wavelengths, dtype=np.float64).reshape(-1)
    if envelope_fwhm is None:
        return np.zeros(lam.shape)
    if not envelope_fwhm > 0:
        raise ValueError("formedbeam: envelope_fwhm is None or > 0")
    return 4.0 * np.log(2.0) / (float(envelope_fwhm) * lam) ** 2


def formed_beam_host(vis, w, group_off, members, u, v, scale, env, k0, half, turn, sinth, yc0, yc1, taper=None, parts=1,
                     dtype=np.float64):
    """The numpy statement of `Context.formed_beam` in `dtype`, np.float64 or np.longdouble: for
    frequency f, group p and source s, over the samples k = k0_s + j (mod nt), j = -H_s .. H_s, and the members b
        D = turn_s - k / nt reduced to [-1/2, 1/2],   x = sinth_s sin(2 pi D),   y = yc0_s - yc1_s cos(2 pi D),
        A = exp(-env_f x^2),   x_b(k) = T_b w_b(k) where w_b(k) > 0 and 0 elsewhere,
        tau = (scale_f u_b) x + (scale_f v_b) y, each product reduced by rint,
        num = sum A x_b Re(V_b(k) exp(-2 pi i tau)),   D = sum A x_b,   D2 = sum A^2 x_b,   beam = num / D
    and the imaginary part in plane 1 with parts = 2; beam, D and D2 are 0 where D = 0 and for H_s = -1.  cos and sin are
    taken of pi times twice a fraction of a turn, never of a large argument.  Samples that are not kept enter no
    arithmetic.  vis (nf, nrow, nt) complex, w of that shape or None (ones), u, v and taper (None: ones) per member.
    Returns (beam (nf, ngroup, parts, nsrc), D, D2 (nf, ngroup, nsrc))."""
    if dtype not in (np.float64, np.longdouble):
        raise ValueError("formed_beam_host: dtype is np.float64 or np.longdouble")
    if parts not in (1, 2):
        raise ValueError("formed_beam_host: parts is 1 or 2")
    vis = np.asarray(vis)
    if vis.ndim != 3 or not np.iscomplexobj(vis):
        raise ValueError("formed_beam_host: complex vis (nf, nrow, nt) expected")
    nf, nrow, nt = vis.shape
    if w is not None and np.shape(w) != vis.shape:
        raise ValueError("formed_beam_host: w must have the shape of vis")
    off, mem = np.asarray(group_off, dtype=np.int64), np.asarray(members, dtype=np.int64)
    if off.ndim != 1 or off.size < 1 or mem.ndim != 1 or off[0] != 0 or np.any(np.diff(off) < 0) or mem.size != off[-1]:
        raise ValueError("formed_beam_host: group_off (ngroup + 1), from 0 and not decreasing, and members (group_off[-1]) expected")
    if mem.size and (mem.min() < 0 or mem.max() >= nrow):
        raise ValueError("formed_beam_host: a member is no row of vis")
    u, v, scale, env = (np.asarray(a, dtype=np.float64) for a in (u, v, scale, env))
    if u.shape != mem.shape or v.shape != mem.shape or scale.shape != (nf,) or env.shape != (nf,):
        raise ValueError("formed_beam_host: u and v per member, scale and env (nf,) expected")
    if not np.all(np.isfinite(env) & (env >= 0)):
        raise ValueError("formed_beam_host: env holds finite values >= 0")
    if taper is not None and np.shape(taper) != mem.shape:
        raise ValueError("formed_beam_host: taper must hold one value per member")
    k0, half = np.asarray(k0, dtype=np.int64), np.asarray(half, dtype=np.int64)
    turn, sinth, yc0, yc1 = (np.asarray(a, dtype=np.float64) for a in (turn, sinth, yc0, yc1))
    nsrc = k0.size
    if k0.ndim != 1 or any(a.shape != (nsrc,) for a in (half, turn, sinth, yc0, yc1)):
        raise ValueError("formed_beam_host: k0, half, turn, sinth, yc0 and yc1 (nsrc,) expected")
    if nsrc and (k0.min() < 0 or k0.max() >= max(nt, 1) or half.min() < -1 or 2 * half.max() + 1 > nt):
        raise ValueError("formed_beam_host: k0 in [0, nt), half >= -1 and 2 half + 1 <= nt expected")
    T = np.ones(mem.size, dtype=dtype) if taper is None else np.asarray(taper, dtype=np.float64).astype(dtype)
    ngroup = off.size - 1
    pi = _ld_pi() if dtype is np.longdouble else np.pi
    beam = np.zeros((nf, ngroup, parts, nsrc), dtype=dtype)
    D, D2 = np.zeros((nf, ngroup, nsrc), dtype=dtype), np.zeros((nf, ngroup, nsrc), dtype=dtype)
    for s in range(nsrc):
        if half[s] < 0:
            continue
        ks = (k0[s] + np.arange(-half[s], half[s] + 1)) % nt
        d = turn[s].astype(dtype) - ks.astype(dtype) / dtype(nt)
        d = d - np.rint(d)
        x = sinth[s].astype(dtype) * np.sin(pi * (2 * d))
        y = yc0[s].astype(dtype) - yc1[s].astype(dtype) * np.cos(pi * (2 * d))
        for f in range(nf):
            A = np.exp(-(env[f].astype(dtype) * (x * x))) if env[f] != 0 else np.ones(ks.size, dtype=dtype)
            for p in range(ngroup):
                sl = slice(off[p], off[p + 1])
                rows = mem[sl]
                if rows.size == 0:
                    continue
                kept = np.ones((rows.size, ks.size), dtype=bool) if w is None else np.asarray(w[f][np.ix_(rows, ks)]) > 0
                wg = np.ones(kept.shape, dtype=dtype) if w is None else np.where(kept, w[f][np.ix_(rows, ks)], 0.0).astype(dtype)
                xb = np.where(kept, T[sl, None] * wg, 0)
                V = np.where(kept, vis[f][np.ix_(rows, ks)], 0)
                xr, xi = xb * V.real.astype(dtype), xb * V.imag.astype(dtype)
                tu = (scale[f].astype(dtype) * u[sl].astype(dtype))[:, None] * x[None, :]
                tv = (scale[f].astype(dtype) * v[sl].astype(dtype))[:, None] * y[None, :]
                ph = pi * (2 * ((tu - np.rint(tu)) + (tv - np.rint(tv))))
                c, sn = np.cos(ph), np.sin(ph)
                d1 = (A[None, :] * xb).sum()
                if d1 == 0:
                    continue
                beam[f, p, 0, s] = (A[None, :] * (xr * c + xi * sn)).sum() / d1
                if parts == 2:
                    beam[f, p, 1, s] = (A[None, :] * (xi * c - xr * sn)).sum() / d1
                D[f, p, s], D2[f, p, s] = d1, ((A * A)[None, :] * xb).sum()
    return beam, D, D2


FORMEDBEAM_DEFAULTS = dict(name="formedbeam", catalogue=None, ha_max=0.05, envelope_fwhm=None, weighting="natural", window=None,
                           ew=None, intracyl=True, parts=1, stack=None)
FORMEDBEAM_STACK_KEYS = ("halfwidth", "line_mhz", "source_weight", "channel_weight")


def formedbeam_params(d=None):
    """One entry of the pipeline's `formedbeams` list with its defaults filled in; an unknown key raises ValueError."""
    out = _conf_filled(d, FORMEDBEAM_DEFAULTS, "formedbeams: unknown key(s) %s (known: %s)", show=", ".join)
    if out["weighting"] not in RINGMAP_WEIGHTINGS or out["window"] not in RINGMAP_WINDOWS or out["parts"] not in (1, 2):
        raise ValueError('formedbeams: weighting is "natural" or "uniform", window None, "hann" or "blackman", parts 1 or 2')
    if out["stack"] is not None:
        _conf_filled(out["stack"], dict.fromkeys(FORMEDBEAM_STACK_KEYS), "formedbeams: unknown stack key(s) %s (known: %s)",
                     show=", ".join)
    if not (out["ha_max"] >= 0) or (out["envelope_fwhm"] is not None and not out["envelope_fwhm"] > 0):
        raise ValueError("formedbeams: ha_max >= 0 and envelope_fwhm None or > 0 expected")
    return out


def formed_beam(m, indir, cat, name="formedbeam", ha_max=0.05, envelope_fwhm=None, weighting="natural", window=None, ew=None,
                intracyl=True, parts=1, stack=None, zmin=0.05, scale_dec=True, chunk_gb=4.0):
    """Formed beams of the stacked Timestream directory `indir` on the positions of the catalogue `cat`
    (`skysim.read_positions`: arrays, a dict or a file): every baseline is fringestopped at the object's position while
    it drifts through the primary beam and the weighted sum over the baselines of a class pair (`formedbeam_groups(tel,
    ew, intracyl)`, tapered by `ringmap_taper(weighting, window)`) and over the samples of the transit
    (`formedbeam_windows(ha_max, zmin, scale_dec)`; ha_max in radians of hour angle at the equator) gives one spectrum per
    object (`Context.formed_beam`).  `envelope_fwhm` (direction cosine per metre of wavelength)
    weights the samples by a Gaussian east-west envelope; None: none.  It needs no products beyond the telescope; the
    dataset `weight` of a file is honoured sample by sample.  Ranks take their own frequencies in chunks that fit
    `chunk_gb`; each frequency gets `formedbeam_<name>.hdf5` beside its timestream file, holding `beam` (ngroup, parts,
    nsrc), `norm` and `norm2` (ngroup, nsrc).  After the barrier rank 0 writes `formedbeam_<name>.hdf5` at the root:
    `beam` (nsrc, ngroup, nfreq) (plane 0; `beam_imag` with parts = 2), `norm`, `norm2` of that shape, `theta`, `phi`,
    `freq` (MHz), `k0`, `half`, `pol`, the parameters as attributes, and — when the catalogue has `redshift` or `stack` (a
    dict: `halfwidth` (2), `line_mhz` (the 21 cm line), `source_weight` (the mean of `norm` over groups and frequencies, so
    that dropped sources weigh 0), `channel_weight`) is given — `redshift`, `stack`, `hits`, `offsets`, `stack_weight` and
    `channel` of `skysim.stack_spectra` on `beam`.  The written bits do not depend on `chunk_gb`.  An unstacked directory
    raises ValueError.  Returns the path of the root file."""
    from . import skysim

    formedbeam_params(dict(ha_max=ha_max, envelope_fwhm=envelope_fwhm, weighting=weighting, window=window, parts=parts, stack=stack))
    conf = dict(dict.fromkeys(FORMEDBEAM_STACK_KEYS), **(stack or {}))
    theta, phi, red = skysim.read_positions(cat)
    if stack is not None and red is None:
        raise ValueError("formed_beam: a stack needs the redshifts of the catalogue")
    tel = m.beamtransfer.telescope
    src, nrow, nt = _route_open("formed_beam", m, indir)
    groups = formedbeam_groups(tel, ew=ew, intracyl=intracyl)
    ngroup = groups["group_off"].shape[0] - 1
    if ngroup == 0:
        raise ValueError("formed_beam: no baseline is selected (ew = %s, intracyl = %s)" % (ew, intracyl))
    taper = ringmap_taper(tel, groups, weighting=weighting, window=window)
    scale = np.ascontiguousarray(1.0 / np.asarray(tel.wavelengths, dtype=np.float64))
    env = formedbeam_env(tel.wavelengths, envelope_fwhm)
    freqs = _sim_freqs(tel, None)
    win = formedbeam_windows(tel, theta, phi, nt, ha_max, zmin=zmin, scale_dec=scale_dec)
    tabs = formedbeam_tables(tel.zenith[0], theta)
    nsrc = theta.size
    per_f = 24.0 * nrow * nt + 8.0 * ngroup * nsrc * (parts + 2)
    log = sim_log
    ctx = get_context()
    dev = {k: ctx.to_device(a) for k, a in (("uvals", groups["uvals"]), ("vvals", groups["vvals"]), ("taper", taper),
                                            ("turn", win["turn"]), ("sinth", tabs["sinth"]), ("yc0", tabs["yc0"]),
                                            ("yc1", tabs["yc1"]))} if nsrc else {}
    for fs in _freq_chunks(freqs, chunk_gb, per_f):
        with _StepTimer(log, "read"):
            chunk = _route_read("formed_beam", src, fs, nrow, nt)
        with _StepTimer(log, "formed_beam"):
            if nsrc:
                x_d, w_d = _route_upload(ctx, chunk)
                bm, nm, nm2 = ctx.formed_beam(x_d, groups["group_off"], groups["members"], groups["iu"], groups["iv"], dev["uvals"],
                                              dev["vvals"], ctx.to_device(scale[fs]), env[fs], win["k0"], win["half"], dev["turn"],
                                              dev["sinth"], dev["yc0"], dev["yc1"], w=w_d, taper=dev["taper"], parts=parts)
                data = dict(beam=ctx.to_host(bm), norm=ctx.to_host(nm), norm2=ctx.to_host(nm2))
                del x_d, w_d, bm, nm, nm2
            else:
                data = dict(beam=np.zeros((len(fs), ngroup, parts, 0)), norm=np.zeros((len(fs), ngroup, 0)),
                            norm2=np.zeros((len(fs), ngroup, 0)))
        with _StepTimer(log, "write"):
            _route_write_products(src, fs, "formedbeam", name, data)
    parallel.barrier()
    root = os.path.join(src.directory, "formedbeam_%s.hdf5" % name)
    if parallel.rank0():
        nfreq = int(tel.nfreq)
        beam = np.zeros((nsrc, ngroup, parts, nfreq))
        norm, norm2 = np.zeros((nsrc, ngroup, nfreq)), np.zeros((nsrc, ngroup, nfreq))
        for fi in range(nfreq):
            with storage.File(_product_file(src, fi, "formedbeam", name), "r") as f:
                beam[..., fi] = np.moveaxis(np.asarray(f["beam"][:]), 2, 0)
                norm[..., fi], norm2[..., fi] = np.asarray(f["norm"][:]).T, np.asarray(f["norm2"][:]).T
        freq = np.asarray(tel.frequencies, dtype=np.float64)
        tables = dict(beam=beam[:, :, 0], norm=norm, norm2=norm2, theta=theta, phi=phi, freq=freq, k0=win["k0"], half=win["half"],
                      pol=groups["pol"])
        if parts == 2:
            tables["beam_imag"] = beam[:, :, 1]
        if ew is not None:
            tables["ew"] = np.atleast_1d(np.asarray(ew, dtype=np.float64))
        if red is not None:
            line = float(skysim.LINE_21CM_MHZ if conf["line_mhz"] is None else conf["line_mhz"]) / (1.0 + red)
            sw = norm.mean(axis=(1, 2)) if conf["source_weight"] is None else conf["source_weight"]
            st = skysim.stack_spectra(beam[:, :, 0], freq, line, 2 if conf["halfwidth"] is None else int(conf["halfwidth"]),
                                      source_weight=sw, channel_weight=conf["channel_weight"])
            tables.update(redshift=red, stack=st["stack"], hits=st["hits"], offsets=st["offsets"].astype(np.int64),
                          stack_weight=st["weight"], channel=st["channel"])
        _write_hdf5(root, tables, dict(ha_max=float(ha_max), envelope_fwhm=0.0 if envelope_fwhm is None else float(envelope_fwhm),
                                       weighting=weighting, window=window or "none", intracyl=int(bool(intracyl)),
                                       parts=int(parts), zmin=float(zmin), scale_dec=int(bool(scale_dec)), ntime=nt))
    parallel.barrier()
    return root


# ---- delay power spectra of stacked visibilities with their window function ---------------

DELAYSPEC_WEIGHTINGS = ("mask", "weight")
DELAYSPEC_TAPERS = (None, "hann", "blackman", "blackman-harris")
DELAYSPEC_NORMS = ("window", "inverse")


def delay_spectrum_host(x, w, taper, step, nd, a0, weighting, min_valid, bin_off, dtype=np.float64):
    """The numpy statement of `Context.delay_spectrum` in `dtype`, np.float64 or np.longdouble:
        y_f = T_f omega_f (omega = 1 with weighting "mask", w with "weight", on the samples with w > 0; 0 elsewhere),
        phi_fk = step_f k, taken as phi - rint(phi) into cos and sin of pi (2 .),
        D_a(t) = sum_f y_f x_f exp(2 pi i phi_f,(a - a0)),   W_d(t) = sum_f y_f exp(2 pi i phi_f,d),
        q = sum_t |D_a|^2, h = sum_t |W_d|^2, s1 = sum_t sum_f T_f^2 omega_f, s2 = sum_t sum_f T_f^2 omega_f^2
    over the series of every bin (bin_off (nbin + 1), ascending within [0, nt]) that have at least min_valid kept
    channels; count is their number.  x (nf, nrow, nt) complex, w of that shape or None (ones), taper (nf,) or None
    (ones), step (nf,).  In long double step_f k is exact for |k| < 2^11.  Samples that are not kept enter no arithmetic.
    Returns (q, h (nrow, nbin, nd), s1, s2 (nrow, nbin), count int32)."""
    if dtype not in (np.float64, np.longdouble):
        raise ValueError("delay_spectrum_host: dtype is np.float64 or np.longdouble")
    if weighting not in DELAYSPEC_WEIGHTINGS:
        raise ValueError('delay_spectrum_host: weighting is "mask" or "weight"')
    x = np.asarray(x)
    if x.ndim != 3 or not np.iscomplexobj(x) or (w is not None and np.shape(w) != x.shape):
        raise ValueError("delay_spectrum_host: complex x (nf, nrow, nt) and w of that shape or None expected")
    nf, nrow, nt = x.shape
    nd, a0, min_valid = int(nd), int(a0), int(min_valid)
    step = np.asarray(step, dtype=np.float64)
    off = np.asarray(bin_off, dtype=np.int64).reshape(-1)
    if step.shape != (nf,) or (taper is not None and np.shape(taper) != (nf,)):
        raise ValueError("delay_spectrum_host: step and taper hold one value per frequency")
    if nd < 0 or (nd > 0 and not 0 <= a0 < nd) or min_valid < 1:
        raise ValueError("delay_spectrum_host: nd >= 0, a0 in [0, nd) and min_valid >= 1 expected")
    if off.size < 1 or off[0] < 0 or off[-1] > nt or np.any(np.diff(off) < 0):
        raise ValueError("delay_spectrum_host: bin_off (nbin + 1) must ascend within [0, nt]")
    nbin = off.size - 1
    ctype = np.complex128 if dtype is np.float64 else np.clongdouble
    pi = _ld_pi() if dtype is np.longdouble else np.pi
    T = np.ones(nf, dtype=dtype) if taper is None else np.asarray(taper, dtype=np.float64).astype(dtype)
    with np.errstate(invalid="ignore"):
        kept = np.ones(x.shape, dtype=bool) if w is None else np.asarray(w) > 0
    om = kept.astype(dtype) if (w is None or weighting == "mask") else np.where(kept, np.asarray(w), 0.0).astype(dtype)
    y = np.where(kept, T[:, None, None] * om, 0)
    yx = np.where(kept, y * np.where(kept, x, 0).astype(ctype), 0)
    used = kept.sum(axis=0) >= min_valid   # (nrow, nt)

    def phases(k):
        phi = step.astype(dtype)[:, None] * k.astype(dtype)[None, :]
        ang = pi * (2 * (phi - np.rint(phi)))
        return (np.cos(ang) + 1j * np.sin(ang)).astype(ctype)   # (nf, len k)

    Ea, Ew = phases(np.arange(nd) - a0), phases(np.arange(nd))
    q, h = np.zeros((nrow, nbin, nd), dtype=dtype), np.zeros((nrow, nbin, nd), dtype=dtype)
    s1, s2 = np.zeros((nrow, nbin), dtype=dtype), np.zeros((nrow, nbin), dtype=dtype)
    count = np.zeros((nrow, nbin), dtype=np.int32)
    for r in range(nrow):
        for b in range(nbin):
            ts = np.arange(off[b], off[b + 1])[used[r, off[b] : off[b + 1]]]
            count[r, b] = ts.size
            if ts.size == 0 or nf == 0:
                continue
            D = Ea.T @ yx[:, r, ts]
            W = Ew.T @ y[:, r, ts].astype(ctype)
            q[r, b] = (D.real * D.real + D.imag * D.imag).sum(axis=1)
            h[r, b] = (W.real * W.real + W.imag * W.imag).sum(axis=1)
            s1[r, b] = (T[:, None] * y[:, r, ts]).sum()
            s2[r, b] = (y[:, r, ts] * y[:, r, ts]).sum()
    return q, h, s1, s2, count


def delay_grid(tel, nd=None, oversample=1.0, tau_max=None):
    """The uniform delay grid of `delay_spectrum` for telescope `tel` (or an array of frequencies in MHz): the step
    dtau = 1 / (oversample nf dnu) in microseconds, dnu the median channel spacing as in `delay_classes`; nd delays
    (default nf, or with tau_max the 2 ceil(tau_max / dtau) + 1 that reach it on both sides) centred on a0 = nd // 2;
    step_f = (nu_f - nu_ref) dtau turns per delay step, nu_ref the band centre.  Returns (tau_us (nd,), step (nf,), a0,
    dtau).  Non-finite values and fewer than two frequencies raise ValueError."""
    nu = np.asarray(getattr(tel, "frequencies", tel), dtype=np.float64).reshape(-1)
    if nu.size < 2 or not np.all(np.isfinite(nu)):
        raise ValueError("delay_grid: at least two finite frequencies expected")
    dnu = float(np.median(np.abs(np.diff(nu))))
    oversample = float(oversample)
    if not (np.isfinite(oversample) and oversample > 0 and dnu > 0):
        raise ValueError("delay_grid: a finite oversample > 0 and distinct frequencies expected")
    dtau = 1.0 / (oversample * nu.size * dnu)
    if tau_max is not None:
        tau_max = float(tau_max)
        if not (np.isfinite(tau_max) and tau_max >= 0):
            raise ValueError("delay_grid: tau_max must be finite and >= 0")
        if nd is None:
            nd = 2 * int(np.ceil(tau_max / dtau)) + 1
    nd = nu.size if nd is None else int(nd)
    if nd < 1:
        raise ValueError("delay_grid: nd < 1")
    a0 = nd // 2
    ref = 0.5 * (nu.min() + nu.max())
    return (np.arange(nd) - a0) * dtau, np.ascontiguousarray((nu - ref) * dtau), a0, dtau


def delay_taper(nf, kind=None):
    """The frequency taper of a delay spectrum at the channel centres x = (f + 1/2) / nf (no channel gets weight 0): None
    (ones), "hann", "blackman" or "blackman-harris" (four terms, -92 dB)."""
    nf = int(nf)
    if nf < 1 or kind not in DELAYSPEC_TAPERS:
        raise ValueError('delay_taper: nf >= 1 and kind None, "hann", "blackman" or "blackman-harris" expected')
    coef = {None: (1.0,), "hann": (0.5, -0.5), "blackman": (0.42, -0.5, 0.08),
            "blackman-harris": (0.35875, -0.48829, 0.14128, -0.01168)}[kind]
    x = (np.arange(nf) + 0.5) / nf
    return np.ascontiguousarray(sum(c * np.cos(2.0 * np.pi * k * x) for k, c in enumerate(coef)) + np.zeros(nf))


def delay_normalise(q, h, s, norm="window", ridge=0.0):
    """The delay spectrum from the quadratic sums of `delay_spectrum`: q and h (..., nd) and the noise bias s (...) (s1 or
    s2).  h is the first column of the window matrix F_ab = H_|a - b| of q (real, symmetric, Toeplitz).  norm "window":
    p_a = q_a / sum_b H_|a - b| (every estimate keeps its window, normalised to unit sum); "inverse": p = (F + ridge H_0
    I)^-1 q, the windows undone.  The noise floor is s put through the same operator (the bias of every q_a is s).
    Device tensors go through `Context.toeplitz_solve` (q and the floor as two right-hand sides of one batched call),
    host arrays through `toeplitz_levinson_host`.  Returns (spectrum, noise (..., nd), info (...) int32): info = 0, or the
    code of the Toeplitz solve (nd for H_0 <= 0, as in a bin without data, with "window" too); where info != 0 spectrum
    and noise are NaN."""
    if norm not in DELAYSPEC_NORMS:
        raise ValueError('delay_normalise: norm is "window" or "inverse"')
    ridge = float(ridge)
    if not (np.isfinite(ridge) and ridge >= 0):
        raise ValueError("delay_normalise: ridge not finite or negative")
    on_device = hasattr(q, "data_ptr")
    if tuple(q.shape) != tuple(h.shape) or tuple(s.shape) != tuple(q.shape[:-1]) or len(q.shape) < 1:
        raise ValueError("delay_normalise: q and h (..., nd) and s (...) expected")
    lead, nd = tuple(q.shape[:-1]), int(q.shape[-1])
    if on_device:
        ctx = get_context()
        torch = ctx.torch
        q2, h2, s2 = q.reshape(-1, nd), h.reshape(-1, nd), s.reshape(-1)
        batch = int(q2.shape[0])
        if batch == 0 or nd == 0:
            return torch.zeros_like(q), torch.zeros_like(q), torch.zeros(lead, dtype=torch.int32, device=q.device)
        nan = torch.full_like(q2, float("nan"))
        if norm == "window":
            cum = torch.cumsum(h2, dim=1)   # sum_b H_|a - b| = C_a + C_(nd - 1 - a) - H_0, C the running sum of H
            rows = cum + torch.flip(cum, dims=(1,)) - h2[:, :1]
            info = torch.where(h2[:, 0] > 0, 0, nd).to(torch.int32)
            ok = (info == 0)[:, None]
            safe = torch.where(ok, rows, torch.ones_like(rows))
            p, n = torch.where(ok, q2 / safe, nan), torch.where(ok, s2[:, None] / safe, nan)
        else:
            b = torch.stack([q2, s2[:, None].expand(batch, nd)], dim=1).to(torch.complex128)
            xs, info = ctx.toeplitz_solve(h2.to(torch.complex128), b, ridge=ridge)
            ok = (info == 0)[:, None]
            p, n = torch.where(ok, xs[:, 0].real, nan), torch.where(ok, xs[:, 1].real, nan)
        return p.reshape(lead + (nd,)), n.reshape(lead + (nd,)), info.reshape(lead)
    q2, h2 = np.asarray(q, dtype=np.float64).reshape(-1, nd), np.asarray(h, dtype=np.float64).reshape(-1, nd)
    s2 = np.asarray(s, dtype=np.float64).reshape(-1)
    batch = q2.shape[0]
    p, n = np.full((batch, nd), np.nan), np.full((batch, nd), np.nan)
    info = np.zeros(batch, dtype=np.int32)
    if batch and nd:
        if norm == "window":
            cum = np.cumsum(h2, axis=1)   # sum_b H_|a - b| = C_a + C_(nd - 1 - a) - H_0, C the running sum of H
            rows = cum + cum[:, ::-1] - h2[:, :1]
            info[:] = np.where(h2[:, 0] > 0, 0, nd)
            ok = info == 0
            p[ok], n[ok] = q2[ok] / rows[ok], s2[ok, None] / rows[ok]
        else:
            col = h2.astype(np.complex128)
            col[:, 0] += ridge * col[:, 0].real
            b = np.stack([q2, np.broadcast_to(s2[:, None], (batch, nd))], axis=1)
            xs, info = toeplitz_levinson_host(col, b)
            info = np.asarray(info, dtype=np.int32).reshape(batch)
            ok = info == 0
            p[ok], n[ok] = xs[ok, 0].real, xs[ok, 1].real
    return p.reshape(lead + (nd,)), n.reshape(lead + (nd,)), info.reshape(lead)


DELAYSPECTRUM_DEFAULTS = dict(name="delayspectrum", nd=None, oversample=1.0, tau_max=None, taper="blackman-harris",
                              weighting="mask", norm="window", ridge=0.0, min_valid=None, tbin=None, blen_bins=None)


def delayspectrum_params(d=None):
    """One entry of the pipeline's `delayspectra` list with its defaults filled in; an unknown key raises ValueError, and
    so does a value the steps refuse."""
    out = _conf_filled(d, DELAYSPECTRUM_DEFAULTS, "delayspectra: unknown key(s) %s (known: %s)", show=", ".join)
    if out["taper"] in ("none", "None"):
        out["taper"] = None
    if out["taper"] not in DELAYSPEC_TAPERS or out["weighting"] not in DELAYSPEC_WEIGHTINGS or out["norm"] not in DELAYSPEC_NORMS:
        raise ValueError('delayspectra: taper is None, "hann", "blackman" or "blackman-harris", weighting "mask" or "weight", '
                         'norm "window" or "inverse"')
    out["ridge"], out["oversample"] = float(out["ridge"]), float(out["oversample"])
    if not (np.isfinite(out["ridge"]) and out["ridge"] >= 0 and np.isfinite(out["oversample"]) and out["oversample"] > 0):
        raise ValueError("delayspectra: ridge >= 0 and oversample > 0, both finite, expected")
    for key in ("nd", "min_valid", "tbin"):
        if out[key] is not None:
            out[key] = int(out[key])
            if out[key] < 1:
                raise ValueError("delayspectra: %s < 1" % key)
    if out["tau_max"] is not None and not (np.isfinite(float(out["tau_max"])) and float(out["tau_max"]) >= 0):
        raise ValueError("delayspectra: tau_max must be finite and >= 0")
    return out


def _delayspec_blen_edges(blen, blen_bins):
    """The edges of the baseline-length bins: an int gives that many equal bins over [0, max |b|], an array the edges."""
    if np.ndim(blen_bins) == 0:
        n = int(blen_bins)
        if n < 1:
            raise ValueError("delay_spectrum: blen_bins < 1")
        top = float(blen.max()) if blen.size else 0.0
        return np.linspace(0.0, top if top > 0 else 1.0, n + 1)
    edges = np.asarray(blen_bins, dtype=np.float64).reshape(-1)
    if edges.size < 2 or not np.all(np.isfinite(edges)) or np.any(np.diff(edges) <= 0):
        raise ValueError("delay_spectrum: blen_bins must be a count or at least two ascending finite edges")
    return edges


def delay_spectrum(m, indir, name="delayspectrum", nd=None, oversample=1.0, tau_max=None, taper="blackman-harris",
                   weighting="mask", norm="window", ridge=0.0, min_valid=None, tbin=None, blen_bins=None, chunk_gb=4.0):
    """The delay power spectrum of every row of the stacked Timestream directory `indir` (`Context.delay_spectrum`,
    DESIGN.md section 4.27): the quadratic estimator along frequency with the flags honoured, on the grid
    `delay_grid(tel, nd, oversample, tau_max)` with the taper `delay_taper(nf, taper)`, summed over time bins of `tbin`
    samples (None: the whole directory is one bin) and normalised by `delay_normalise(norm, ridge)`.  weighting "mask"
    uses the flags only, "weight" the weights themselves; a series with fewer than `min_valid` (None: 1) kept channels
    is dropped.  The spectrum needs every frequency of a row at once, so the device takes chunks of rows over all
    frequency files that fit `chunk_gb`; more than one rank raises ValueError, and so does an unstacked directory.
    Writes `delayspectrum_<name>.hdf5` at the root of the directory: `tau` (nd, microseconds), `q`, `window` (= h),
    `spectrum` and `noise` (the normalised s1 for "weight", s2 for "mask") (nrow, nbin, nd), `s1`, `s2`, `count` and
    `info` (nrow, nbin), `bin_off`, `step`, `taper`, `blen` (m) and `horizon` (|b| / c in microseconds) per row, with
    `blen_bins` (a count of equal bins up to the longest baseline, or the edges) `blen_edges`, `wedge` (nblen, nbin, nd),
    the count-weighted mean of `spectrum` over the solved rows of each length bin (NaN where none), and `wedge_hits`
    (nblen, nbin), the series behind it; and the parameters as attributes.  The written bits do not depend on
    `chunk_gb`.  Returns the path of the file."""
    p = delayspectrum_params(dict(name=name, nd=nd, oversample=oversample, tau_max=tau_max, taper=taper, weighting=weighting,
                                  norm=norm, ridge=ridge, min_valid=min_valid, tbin=tbin, blen_bins=blen_bins))
    _delay_one_rank("delay_spectrum")
    tel = m.beamtransfer.telescope
    src, nrow, nt = _route_open("delay_spectrum", m, indir)
    nf = int(tel.nfreq)
    tau, step, a0, dtau = delay_grid(tel, nd=p["nd"], oversample=p["oversample"], tau_max=p["tau_max"])
    nd = int(tau.size)
    tap = delay_taper(nf, p["taper"])
    need = 1 if p["min_valid"] is None else p["min_valid"]
    log = sim_log
    with _StepTimer(log, "read"):
        chunk = _route_read("delay_spectrum", src, range(nf), nrow, nt)
    from ._lib import delayspec_bins

    off = delayspec_bins(nt, p["tbin"])
    nbin = int(off.size) - 1
    ranges = _row_chunks("delay_spectrum", nrow, chunk_gb, 24.0 * nf * nt + 40.0 * nbin * nd + 64.0)
    ctx = get_context()
    out = dict(q=np.empty((nrow, nbin, nd)), window=np.empty((nrow, nbin, nd)), spectrum=np.empty((nrow, nbin, nd)),
               noise=np.empty((nrow, nbin, nd)), s1=np.empty((nrow, nbin)), s2=np.empty((nrow, nbin)),
               count=np.empty((nrow, nbin), dtype=np.int32), info=np.empty((nrow, nbin), dtype=np.int32))
    with _StepTimer(log, "delay_spectrum"):
        tap_d, step_d = ctx.to_device(tap), ctx.to_device(step)
        for r0, r1 in ranges:
            x_d, w_d = _route_upload(ctx, chunk, r0, r1)
            q, h, s1, s2, cnt = ctx.delay_spectrum(x_d, w=w_d, taper=tap_d, step=step_d, nd=nd, a0=a0, weighting=p["weighting"],
                                                   min_valid=need, bins=off)
            sp, ns, info = delay_normalise(q, h, s1 if p["weighting"] == "weight" else s2, norm=p["norm"], ridge=p["ridge"])
            for key, value in (("q", q), ("window", h), ("spectrum", sp), ("noise", ns), ("s1", s1), ("s2", s2), ("count", cnt),
                               ("info", info)):
                out[key][r0:r1] = ctx.to_host(value)
            del x_d, w_d, q, h, s1, s2, cnt, sp, ns, info
    blen = np.sqrt((np.asarray(tel.baselines, dtype=np.float64).reshape(nrow, -1) ** 2).sum(axis=1))
    root = os.path.join(src.directory, "delayspectrum_%s.hdf5" % p["name"])
    with _StepTimer(log, "write"):
        tables = dict(out, tau=tau, bin_off=off, step=step, taper=tap, blen=blen, horizon=blen / DELAY_C)
        if p["blen_bins"] is not None:
            edges = _delayspec_blen_edges(blen, p["blen_bins"])
            which = np.clip(np.searchsorted(edges, blen, side="right") - 1, -1, edges.size - 2)
            which[(blen < edges[0]) | (blen > edges[-1])] = -1
            good = (out["info"] == 0) & (out["count"] > 0)
            wgt = np.where(good, out["count"], 0).astype(np.float64)
            wedge = np.full((edges.size - 1, nbin, nd), np.nan)
            hits = np.zeros((edges.size - 1, nbin), dtype=np.int64)
            for j in range(edges.size - 1):   # in row order: the bits do not depend on the chunk
                rows = np.nonzero(which == j)[0]
                num, den = np.zeros((nbin, nd)), np.zeros(nbin)
                for r in rows:
                    num += wgt[r][:, None] * np.where(good[r][:, None], out["spectrum"][r], 0.0)
                    den += wgt[r]
                wedge[j] = np.where(den[:, None] > 0, num / np.where(den > 0, den, 1.0)[:, None], np.nan)
                hits[j] = den.astype(np.int64)
            tables.update(blen_edges=edges, wedge=wedge, wedge_hits=hits)
        _write_hdf5(root, tables, dict(nd=nd, a0=int(a0), dtau=float(dtau), oversample=p["oversample"], taper=p["taper"] or "none",
                                       weighting=p["weighting"], norm=p["norm"], ridge=p["ridge"], min_valid=int(need),
                                       tbin=-1 if p["tbin"] is None else p["tbin"], ntime=nt))
    return root
