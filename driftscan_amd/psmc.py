"""Monte-Carlo estimators of the Fisher matrix and bias, GPU-backed.

Mirrors ``drift.core.psmc.PSMonteCarlo`` / ``PSMonteCarloAlt`` (drift/core/psmc.py:10-199) and
``drift.core.crosspower.CrossPower`` (drift/core/crosspower.py:8-45): same classes, config properties,
``gen_sample``, ``gen_vecs`` and ``_work_fisher_bias_m``.  They need the KL modes (n^2 per m) and
O(n R + L F R) per batch of R samples, never the ``nbands n^2`` band projections of ``PSExact``.

The samples are drawn on the device by ``dm_psmc_draw``: Philox4x32-10 keyed by ``seed`` with the
counter (mode i, sample s, m, stream), so a draw is a fixed function of (seed, m, s, i, stream) and
the estimate does not depend on how samples are split into calls, how m is batched
(``ps_chunk_gb``) or the number of ranks.  Streams: 0 = PSMonteCarlo's x and CrossPower's x1,
1 = CrossPower's x2, 2 = PSMonteCarloAlt's Z_2 vectors.  ``seed`` is an extension of the reference
(which draws from numpy's global state) for reproducibility.

``fisher_bias_batch`` keeps draws and q on the device for a whole batch of m: draws -> ``dm_qestimate``
-> ``dm_psmc_moments`` (PSMonteCarlo, CrossPower), or draws -> ``dm_psmc_alt`` (PSMonteCarloAlt).  A
subclass that overrides ``gen_sample`` (or ``gen_signs``) with its own host arrays takes the
reference's per-m route through ``_work_fisher_bias_m`` instead.

CrossPower projects the y side of its cross q from x2, so its Fisher estimate
converges to half the exact Fisher matrix; the reference's, whose band terms ignore x2, to the whole.
"""
import numpy as np

from . import config
from .device import get_context
from .psestimation import PSEstimation, _linear_offsets

_MAX_COLS = (1 << 29) - 1   # nblk * R of one dm_qestimate / dm_psmc_alt call
STREAM_X, STREAM_X2, STREAM_ALT = 0, 1, 2


def split_m(n, nchunk):
    """(num, start, end) of n items in nchunk near-equal chunks (caput.mpiutil.split_m)."""
    base, rem = divmod(n, nchunk)
    num = np.array([base + (1 if i < rem else 0) for i in range(nchunk)], dtype=np.int64)
    end = np.cumsum(num)
    return num, end - num, end


class _MCBase(PSEstimation):
    """Batching and mode staging shared by the sampled estimators."""

    nsamples = config.Property(proptype=int, default=500)
    seed = config.Property(proptype=int, default=0)

    def _bytes_per_col(self, n, ndof):
        raise NotImplementedError

    def num_evals_all(self, mi):
        """Number of KL modes of m = mi as the estimators use them (the KL object's threshold, as the reference)."""
        ev = self.kltrans.modes_m(mi, device=True)[0]
        return 0 if ev is None else ev.size

    def _mc_need(self, mi, R):
        """Device bytes of one m at R sample columns: a linear term per column plus the modes and the stored q."""
        bt = self.kltrans.beamtransfer
        n = float(self.num_evals_all(mi))
        nd = float(bt.ndof(mi))
        nq = self.nbands + 1
        return self._bytes_per_col(n, nd) * R + 16.0 * n * nd + 8.0 * nq * self.nsamples

    def _mc_plan(self, ms):
        """(R, batches of ms): R = nsamples unless the largest m alone does not fit the budget at that width; the m are
        batched greedily under ps_chunk_gb and nblk * R below the 2^29 columns of one call."""
        budget = self.ps_chunk_gb * (1 << 30)
        R = max(1, int(self.nsamples))
        if ms:
            big = max(ms, key=lambda mi: self._mc_need(mi, 1))
            fixed = self._mc_need(big, 0)
            per = self._mc_need(big, 1) - fixed
            if fixed + per * R > budget:
                R = max(1, min(R, int((budget - fixed) // per) if budget > fixed else 1))
        batches, cur, used = [], [], 0.0
        for mi in ms:
            need = self._mc_need(mi, R)
            if cur and (used + need > budget or (len(cur) + 1) * R > _MAX_COLS):
                batches.append(cur)
                cur, used = [], 0.0
            cur.append(mi)
            used += need
        if cur:
            batches.append(cur)
        return R, batches

    def _batches(self, ms):
        """Batches of m for accumulate_ms / generate: those of the sampled path (modes and per-column buffers under
        ps_chunk_gb), never the nbands n^2 of PSExact's projections."""
        for batch in self._mc_plan(list(ms))[1]:
            yield batch

    def _stack(self, batch, modes):
        """The device operands of a batch of m with modes: beam_svd, svnum, eigenvectors and eigenvalues back to back."""
        import torch

        ctx = get_context()
        bt = self.kltrans.beamtransfer
        nmodes = np.array([ev.size for ev, _ in modes], dtype=np.int64)
        bsvd = bt._stacked_products(batch, "beam_svd")
        svnum = np.stack([bt._svd_num(mi)[0] for mi in batch])
        ndofs = svnum.sum(axis=1)
        eoff, _ = _linear_offsets(nmodes * ndofs)
        voff, vtot = _linear_offsets(nmodes)
        Vh = np.zeros(max(vtot, 1), dtype=np.float64)
        parts = []
        for k, (ev, E) in enumerate(modes):
            if E.shape[1] != ndofs[k]:
                raise Exception("KL modes of m=%d have length %d, the SVD basis %d" % (batch[k], E.shape[1], ndofs[k]))
            parts.append(ctx.to_device(np.ascontiguousarray(E).ravel()) if isinstance(E, np.ndarray) else E.reshape(-1))
            Vh[voff[k] : voff[k] + nmodes[k]] = ev
        Ed = torch.cat(parts) if len(parts) > 1 else parts[0].contiguous()
        return bsvd, svnum, Ed, eoff, nmodes, ctx.to_device(Vh), voff

    def _modes(self, ms):
        """KL modes (device rows where the mode cache has them) of each m, None for an m without modes."""
        out = []
        for mi in ms:
            ev, E = self.kltrans.modes_m(mi, device=True)
            out.append(None if ev is None or ev.size == 0 else (ev, E))
        return out

    def _draw(self, mi, nsamples, start, stream, kind, power):
        """Draws of one m on the device, (nmodes, nsamples) c128 (a torch tensor), or None without modes."""
        ctx = get_context()
        ev = self.kltrans.modes_m(mi, device=True)[0]
        if ev is None or ev.size == 0:
            return None
        evd = ctx.to_device(np.ascontiguousarray(ev, dtype=np.float64))
        x = ctx.psmc_draw([mi], [ev.size], nsamples, self.seed, stream=stream, kind=kind, power=power, s0=start,
                          evals=evd, evals_off=[0])
        return x.reshape(ev.size, nsamples)


class PSMonteCarlo(_MCBase):
    """Fisher matrix and bias as the covariance and mean of q over simulated data (psmc.py:10-89): Cov(q_a, q_b) = F_ab
    (Padmanabhan and Pen 2003; Dillon et al. 2012).

    nsamples : samples per m (default 500, as the reference)
    seed     : key of the counter-based draws (default 0; an extension of the reference)"""

    def gen_sample(self, mi, nsamples=None, noiseonly=False, start=0, stream=STREAM_X):
        """Random KL data (nmodes, nsamples) c128 of m = mi drawn from the eigenvalue distribution (psmc.py:26-53):
        complex standard normals (E|z|^2 = 1) scaled by (lambda + 1)^1/2, or unscaled with `noiseonly`.  Drawn on the
        device; `start` (first sample index) and `stream` select the draws (extensions of the reference)."""
        nsamples = self.nsamples if nsamples is None else int(nsamples)
        x = self._draw(mi, nsamples, int(start), int(stream), 0, 0 if noiseonly else 1)
        if x is None:
            return np.zeros((0, nsamples), dtype=np.complex128)
        return x.cpu().numpy()

    def _own_draws(self):
        return type(self).gen_sample is PSMonteCarlo.gen_sample

    def _sample(self, mi, n, start, stream):
        """One chunk of samples: the counter-based draws, or what a subclass's own gen_sample (with the reference's
        signature) returns."""
        if self._own_draws():
            return self.gen_sample(mi, n, start=start, stream=stream)
        return self.gen_sample(mi, n)

    def _moments(self, qa):
        mean, cov = get_context().psmc_moments(get_context().to_device(np.ascontiguousarray(qa[np.newaxis])))
        return mean[0].cpu().numpy(), cov[0].cpu().numpy()

    def _work_fisher_bias_m(self, mi):
        """(fisher = cov q, bias = mean q) of one m, the reference's route (psmc.py:55-89): gen_sample per chunk of at
        most ~1000 samples, q_estimator, then the moments on the device."""
        if self.clarray is None:
            self.genbands()
        nb = self.nbands
        if self.num_evals_all(mi) == 0:
            return np.zeros((nb, nb)), np.zeros(nb)
        qa = np.zeros((nb, self.nsamples))
        num, starts, ends = split_m(self.nsamples, (self.nsamples // 1000) + 1)
        for n, s, e in zip(num, starts, ends):
            x = self._sample(mi, int(n), int(s), STREAM_X)
            qa[:, s:e] = self.q_estimator(mi, x)
        mean, cov = self._moments(qa)
        return cov, mean

    def _bytes_per_col(self, n, nd):
        tel = self.telescope
        F, L = tel.nfreq, tel.lmax + 1
        k = 2 if self.crosspower else 1
        # draws, x1 / x2 sky columns (and y), the q of the call, the band partial sums
        return 16.0 * k * (n + nd + L * F) + 8.0 * (self.nbands + 1) * (L / 4.0 + 2.0)

    def fisher_bias_batch(self, ms):
        """[(fisher, bias)] of the given m: per batch of m, the draws, dm_qestimate per chunk of R samples into a
        device-resident q (nblk, nq, nsamples), then dm_psmc_moments."""
        if self.clarray is None:
            self.genbands()
        if not self._own_draws():
            return [self._work_fisher_bias_m(mi) for mi in ms]
        import torch

        ctx = get_context()
        nb, ns = self.nbands, int(self.nsamples)
        cross = bool(self.crosspower)
        nq = nb + 1 if cross else nb
        ms = [int(mi) for mi in ms]
        modes = self._modes(ms)
        out = [(np.zeros((nb, nb)), np.zeros(nb)) for _ in ms]
        idx = [i for i in range(len(ms)) if modes[i] is not None]
        R, batches = self._mc_plan([ms[i] for i in idx])
        pos = iter(idx)
        cl = self._cl_device()[1]
        for batch in batches:
            ii = [next(pos) for _ in batch]
            bsvd, svnum, Ed, eoff, nmodes, Vd, voff = self._stack(batch, [modes[i] for i in ii])
            qall = torch.empty((len(batch), nq, ns), dtype=torch.float64, device=Vd.device)
            for s0 in range(0, ns, R):
                r = min(R, ns - s0)
                x = ctx.psmc_draw(batch, nmodes, r, self.seed, stream=STREAM_X, power=1, s0=s0, evals=Vd, evals_off=voff)
                y = None
                if cross:
                    y = ctx.psmc_draw(batch, nmodes, r, self.seed, stream=STREAM_X2, power=1, s0=s0, evals=Vd,
                                      evals_off=voff)
                q = ctx.qestimate(bsvd, svnum, np.array(batch), cl, Ed, eoff, nmodes, Vd, voff, r, x, voff * r, y=y,
                                  noise=cross, crosspower=cross, zero_mean=bool(self.zero_mean))
                qall[:, :, s0 : s0 + r] = q
                del x, y, q
            mean, cov = ctx.psmc_moments(qall)
            mean, cov = mean.cpu().numpy(), cov.cpu().numpy()
            for k, i in enumerate(ii):
                out[i] = self._result(mean[k], cov[k])
        return out

    def _result(self, mean, cov):
        return cov, mean


class PSMonteCarloAlt(_MCBase):
    """Fisher matrix by a stochastic estimate of the trace (psmc.py:92-199): with Z_2 vectors x (E x x^T = 1),
    F_ab = sum_{i, s} v_a v_b^* / nsamples, v_a = C^-1/2 Q_a C^-1/2 x.  The bias is zero, as in the reference.

    nsamples : Z_2 vectors per m (default 500)
    nswitch  : accepted and unused, as in the reference
    seed     : key of the counter-based draws (default 0; an extension of the reference)"""

    nswitch = config.Property(proptype=int, default=0)

    def gen_signs(self, mi, nsamples=None, start=0):
        """The Z_2 vectors (nmodes, nsamples) of m = mi, +-1 (the reference draws them inside gen_vecs,
        psmc.py:122-125).  Drawn on the device; override to supply other draws."""
        nsamples = self.nsamples if nsamples is None else int(nsamples)
        x = self._draw(mi, nsamples, int(start), STREAM_ALT, 1, 0)
        if x is None:
            return np.zeros((0, nsamples))
        return x.real.cpu().numpy()

    def _own_draws(self):
        return type(self).gen_signs is PSMonteCarloAlt.gen_signs

    def _bytes_per_col(self, n, nd):
        tel = self.telescope
        F, L = tel.nfreq, tel.lmax + 1
        nb = self.nbands
        # draws, x1, x2, the nbands Z (sky) and y1 / v (SVD / KL) columns of the back-projections
        return 16.0 * (n + nd + L * F + nb * (L * F + nd + n)) + 16.0 * nb * nb / 2048.0

    def _alt_call(self, stack, batch, x, R, want_vecs=False):
        bsvd, svnum, Ed, eoff, nmodes, Vd, voff = stack
        return get_context().psmc_alt(bsvd, svnum, np.array(batch), self._cl_device()[1], Ed, eoff, nmodes, Vd, voff, R,
                                      x, voff * R, self.nsamples, want_vecs=want_vecs)

    def _weighted_signs(self, stack, batch, modes, R, start):
        """The draws of a batch weighted by (lambda + 1)^-1/2, block after block on the device: the counter-based draws,
        or a subclass's gen_signs (all nsamples of an m at once) weighted on the host."""
        import torch

        ctx = get_context()
        if self._own_draws():
            nmodes, Vd, voff = stack[4], stack[5], stack[6]
            return ctx.psmc_draw(batch, nmodes, R, self.seed, stream=STREAM_ALT, kind=1, power=-1, s0=start, evals=Vd,
                                 evals_off=voff)
        if start != 0 or R != self.nsamples:
            raise ValueError("PSMonteCarloAlt: a gen_signs override supplies all nsamples draws of an m in one chunk")
        cols = []
        for mi, (ev, _) in zip(batch, modes):
            xv = np.asarray(self.gen_signs(mi, R), dtype=np.complex128)
            cf = (np.asarray(ev, dtype=np.float64) + 1.0) ** -0.5
            cols.append(ctx.to_device(np.ascontiguousarray(cf[:, np.newaxis] * xv).ravel()))
        return torch.cat(cols) if len(cols) > 1 else cols[0]

    def gen_vecs(self, mi):
        """The band vectors v_a (nmodes, nsamples) of m = mi into self.vec_cache (psmc.py:111-161)."""
        if self.clarray is None:
            self.genbands()
        self.vec_cache = []
        md = self._modes([mi])
        if md[0] is None:
            return
        ns = int(self.nsamples)
        stack = self._stack([mi], md)
        x = self._weighted_signs(stack, [mi], md, ns, 0)
        _, vecs = self._alt_call(stack, [mi], x, ns, want_vecs=True)
        n = md[0][0].size
        self.vec_cache = [vecs[a, : n * ns].reshape(n, ns).cpu().numpy() for a in range(self.nbands)]

    def _work_fisher_bias_m(self, mi):
        """(fisher, bias = 0) of one m (psmc.py:163-199)."""
        return self.fisher_bias_batch([mi])[0]

    def fisher_bias_batch(self, ms):
        """[(fisher, zeros)] of the given m: per batch of m and chunk of R samples, the draws, then dm_psmc_alt; the
        chunks' Fisher sums are added in order."""
        if self.clarray is None:
            self.genbands()
        ms = [int(mi) for mi in ms]
        nb, ns = self.nbands, int(self.nsamples)
        modes = self._modes(ms)
        out = [(np.zeros((nb, nb), dtype=np.complex128), np.zeros(nb, dtype=np.complex128)) for _ in ms]
        idx = [i for i in range(len(ms)) if modes[i] is not None]
        R, batches = self._mc_plan([ms[i] for i in idx])
        pos = iter(idx)
        for batch in batches:
            ii = [next(pos) for _ in batch]
            md = [modes[i] for i in ii]
            stack = self._stack(batch, md)
            fsum = None
            for s0 in range(0, ns, R):
                r = min(R, ns - s0)
                f = self._alt_call(stack, batch, self._weighted_signs(stack, batch, md, r, s0), r)
                fsum = f if fsum is None else fsum + f
            fh = fsum.cpu().numpy()
            for k, i in enumerate(ii):
                out[i] = (fh[k], np.zeros(nb, dtype=np.complex128))
        return out


class CrossPower(PSMonteCarlo):
    """Monte-Carlo Fisher matrix and bias of the cross estimate between two independent draws (crosspower.py:8-45):
    fisher = cov[:nb, :nb], bias = cov[-1, :nb] of (q_cross, q_noise)."""

    crosspower = True

    def _work_fisher_bias_m(self, mi):
        if self.clarray is None:
            self.genbands()
        nb = self.nbands
        if self.num_evals_all(mi) == 0:
            return np.zeros((nb, nb)), np.zeros(nb)
        qa = np.zeros((nb + 1, self.nsamples))
        num, starts, ends = split_m(self.nsamples, (self.nsamples // 1000) + 1)
        for n, s, e in zip(num, starts, ends):
            x1 = self._sample(mi, int(n), int(s), STREAM_X)
            x2 = self._sample(mi, int(n), int(s), STREAM_X2)
            qa[:, s:e] = self.q_estimator(mi, x1, x2, noise=True)
        mean, cov = self._moments(qa)
        return self._result(mean, cov)

    def _result(self, mean, cov):
        nb = self.nbands
        return cov[:nb, :nb], cov[-1, :nb]
