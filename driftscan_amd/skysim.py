"""Gaussian skies with the statistics of the model covariances C_l(nu, nu').

The reference makes its simulated skies with ``cora.core.skysim.mkfullsky``; cora is not available, so this module draws
them from the arrays every other stage works from: ``[pol, pol, l, freq, freq]`` as ``skymodel`` or
``KLTransform.signal()`` / ``foreground()`` give them.  The definition:

* the components i = (pol, freq) form one group per polarisation when every cross-polarisation block is zero, one joint
  group otherwise; a polarisation whose block is zero has no group and zero coefficients;
* per group and l, ``T_l`` is the symmetric positive semi-definite square root of ``C_l`` (eigenvalues clipped at 0);
* ``a[r, f, p, l, m] = sum_j T_l[i, j] z_j`` with one Philox4x32-10 block per (component j, l, m, realisation r):
  key = seed, counter ``(p F + f, (l << 16) | m, r, stream)``, complex with E|z|^2 = 1 for m > 0 and real with
  E z^2 = 1 for m = 0; E and B are zero for l < 2 and everything is zero for m > l.

Per-feed gain errors: ``GainModel`` and its numpy statement ``gain_coeff_host``, ``gains_host``
and ``baseline_gains_host``, the oracle of ``gains_device`` / ``Context.ts_gain_apply``.

Point sources are the non-Gaussian skies: ``source_alm`` gives the exact band-limited a_lm of a
catalogue on the device (``dm_source_alm``), ``source_alm_host`` is its numpy statement and oracle.

``draw_alm`` does this on the device (``dm_sky_draw``: the draws are made inside the kernel and multiplied on the matrix
cores); ``groups``, ``covariance_roots(device=False)``, ``draws_host`` and ``correlate_host`` restate it in numpy and need
no GPU.
"""
import numpy as np

from .telescope import T_SIDEREAL

STREAM_SKY_SIGNAL = 16       # clear of psmc.STREAM_X, STREAM_X2, STREAM_ALT = 0, 1, 2
STREAM_SKY_FOREGROUND = 17
STREAM_TS_NOISE = 24         # receiver noise (dm_ts_noise): the low byte of counter word 3, the realisation above it
TS_NOISE_MAX_REAL = 1 << 24
STREAM_TS_GAIN_AMP = 25      # per-feed gain errors (dm_ts_gain_coeff): amplitude and phase components, laid out as the noise
STREAM_TS_GAIN_PHASE = 26
GAIN_BROADBAND = 0xFFFFFFFF  # the frequency word of a gain shared by all channels (freq_corr = "full")
LMAX_LIMIT = 65536           # m and l share one 32-bit counter word


def _check_cv(cv):
    cv = np.asarray(cv, dtype=np.float64)
    if cv.ndim != 5 or cv.shape[0] != cv.shape[1] or cv.shape[3] != cv.shape[4]:
        raise ValueError("need a covariance [pol, pol, l, freq, freq], got shape %s" % (cv.shape,))
    if cv.shape[2] - 1 >= LMAX_LIMIT:
        raise ValueError("lmax = %d is beyond the %d the draw counters can address" % (cv.shape[2] - 1, LMAX_LIMIT - 1))
    return cv


def groups(cv):
    """The groups of jointly drawn components: a list of int arrays of ``j_global = pol * nfreq + freq``."""
    cv = _check_cv(cv)
    npol, nfreq = cv.shape[0], cv.shape[3]
    cross = any(cv[p, q].any() for p in range(npol) for q in range(npol) if p != q)
    if cross:
        return [np.arange(npol * nfreq, dtype=np.int64)]
    return [p * nfreq + np.arange(nfreq, dtype=np.int64) for p in range(npol) if cv[p, p].any()]


def group_covariance(cv, jglobal):
    """(L, n, n) covariance of one group: C[l, (p, f), (q, f')] = cv[p, q, l, f, f']."""
    cv = _check_cv(cv)
    nfreq = cv.shape[3]
    p, f = np.asarray(jglobal) // nfreq, np.asarray(jglobal) % nfreq
    return np.ascontiguousarray(cv[p[:, None], p[None, :], :, f[:, None], f[None, :]].transpose(2, 0, 1))


def covariance_roots(cv, device=True):
    """Per group of ``groups(cv)``, the symmetric roots T (L, n, n) with T_l T_l = C_l.

    device=True: float64 tensors on the GPU, from one batched Hermitian eigendecomposition per group
    (``Context.herm_eig``) and V sqrt(max(lambda, 0)) V^H by the batched ZGEMM.  device=False: numpy arrays from
    ``numpy.linalg.eigh``, the oracle of the tests."""
    cv = _check_cv(cv)
    out = []
    if not device:
        for jg in groups(cv):
            ev, V = np.linalg.eigh(group_covariance(cv, jg))
            T = np.einsum("lik,lk,ljk->lij", V, np.sqrt(np.maximum(ev, 0.0)), V)
            out.append(0.5 * (T + T.transpose(0, 2, 1)))
        return out
    from .device import get_context

    ctx = get_context()
    for jg in groups(cv):
        C = group_covariance(cv, jg)
        L, n = C.shape[0], C.shape[1]
        Cd = ctx.to_device(C.astype(np.complex128))
        ev, W = ctx.herm_eig(Cd, n, n, strideC=n * n, batch=L)      # C = W^H diag(ev) W
        s = ctx.torch.sqrt(ctx.torch.clamp(ev, min=0.0)).contiguous()
        T = ctx.empty((L, n, n), np.complex128)
        ctx.zgemm(W, W, T, n, n, n, 1, n, n, 1, n, conjA=True, kscale=s, batch=L, strideA=n * n, strideB=n * n,
                  strideC=n * n, stride_kscale=n)
        out.append(T.real.contiguous())
        del Cd, W, T
    return out


# ---- numpy restatement of the draws and of the product ----------------------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)


def _philox4x32_10(ctr, key):
    c = [np.asarray(x, dtype=np.uint64) & _M32 for x in ctr]
    k0, k1 = np.uint64(key[0]), np.uint64(key[1])
    for r in range(10):
        if r:
            k0 = (k0 + np.uint64(0x9E3779B9)) & _M32
            k1 = (k1 + np.uint64(0xBB67AE85)) & _M32
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & _M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & _M32]
    return c


def _u53(a, b):
    k = ((a >> np.uint64(5)) << np.uint64(26)) | (b >> np.uint64(6))
    return (k + np.uint64(1)).astype(np.float64) * 2.0**-53


def draws_host(jglobal, L, M=None, nreal=1, seed=0, stream=STREAM_SKY_SIGNAL, first=0):
    """The unit draws z [nreal, n, L, M] of the components ``jglobal`` in numpy (zero for m > l)."""
    M = L if M is None else int(M)
    if L - 1 >= LMAX_LIMIT:
        raise ValueError("lmax beyond the draw counters")
    jg = np.asarray(jglobal, dtype=np.uint64)
    r, j, l, m = np.meshgrid(np.arange(first, first + nreal, dtype=np.uint64), jg, np.arange(L, dtype=np.uint64),
                             np.arange(M, dtype=np.uint64), indexing="ij")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = _philox4x32_10([j, (l << np.uint64(16)) | m, r, np.full_like(j, stream)], (seed & 0xFFFFFFFF, seed >> 32))
    rad = np.sqrt(-np.log(_u53(w[0], w[1])))
    th = 6.283185307179586 * _u53(w[2], w[3])
    z = rad * np.cos(th) + 1j * (rad * np.sin(th))
    z = np.where(m == 0, 1.4142135623730951 * z.real, z)
    return np.where(m <= l, z, 0.0)


def noise_host(sigma, fglobal, ntime, nreal, seed, first=0, stream=STREAM_TS_NOISE):
    """The receiver noise of ``Context.ts_noise`` in numpy: [nreal, nf, npairs, ntime] with ``sigma`` (nf, npairs) (or a
    scalar) times the unit draw of counter ``(pair, fglobal[i], t, ((first + r) << 8) | stream)``."""
    fg = np.asarray(fglobal, dtype=np.uint64).reshape(-1)
    sigma = np.asarray(sigma, dtype=np.float64)
    if sigma.ndim == 0:
        raise ValueError("noise_host: sigma (nf, npairs) expected")
    sigma = np.broadcast_to(sigma, (fg.shape[0], sigma.shape[-1]))
    if first < 0 or first + nreal > TS_NOISE_MAX_REAL:
        raise ValueError("noise_host: realisations beyond the %d the counter word holds" % TS_NOISE_MAX_REAL)
    r, f, p, t = np.meshgrid(np.arange(first, first + nreal, dtype=np.uint64), fg,
                             np.arange(sigma.shape[1], dtype=np.uint64), np.arange(ntime, dtype=np.uint64), indexing="ij")
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    w = _philox4x32_10([p, f, t, (r << np.uint64(8)) | np.uint64(stream)], (seed & 0xFFFFFFFF, seed >> 32))
    rad = np.sqrt(-np.log(_u53(w[0], w[1]))) * sigma[None, :, :, None]
    th = 6.283185307179586 * _u53(w[2], w[3])
    return rad * np.cos(th) + 1j * (rad * np.sin(th))


def correlate_host(T, z):
    """a[..., i, l, m] = sum_j T[l, i, j] z[..., j, l, m] summed in numpy.longdouble (returned as clongdouble):
    T (L, n, n), z [..., n, L, M]."""
    T = np.asarray(T, dtype=np.longdouble)
    z = np.asarray(z)
    re = np.einsum("lij,...jlm->...ilm", T, z.real.astype(np.longdouble))
    im = np.einsum("lij,...jlm->...ilm", T, z.imag.astype(np.longdouble))
    return re + 1j * im



# ---- per-feed gain errors ------------------------------------------------------------------------
class GainModel:
    """Complex gain errors of the feeds, g = (1 + x_amp(t)) exp(i x_phase(t)) per (feed, frequency, realisation).

    Each x_q is a stationary Gaussian process, periodic over the sidereal day, of standard deviation ``sigma_amp`` /
    ``sigma_phase`` (radians) and a Gaussian spectrum of correlation time ``corr_time`` seconds (0: equal weights, white
    for an odd number of samples).  ``freq_corr``: "none" — independent channels; "full" — one broadband gain per feed.
    The gains multiply the sky part of a simulated visibility only: receiver noise is added after them at its usual
    level."""

    def __init__(self, sigma_amp=0.0, sigma_phase=0.0, corr_time=0.0, freq_corr="none", seed=0):
        self.sigma_amp, self.sigma_phase, self.corr_time = float(sigma_amp), float(sigma_phase), float(corr_time)
        self.freq_corr, self.seed = str(freq_corr), int(seed)
        if self.sigma_amp < 0 or self.sigma_phase < 0 or self.corr_time < 0:
            raise ValueError("GainModel: sigma_amp, sigma_phase and corr_time must not be negative")
        if self.freq_corr not in ("none", "full"):
            raise ValueError("GainModel: freq_corr is 'none' or 'full', not %r" % (freq_corr,))

    @classmethod
    def from_config(cls, conf):
        conf = dict(conf)
        unknown = set(conf) - {"sigma_amp", "sigma_phase", "corr_time", "freq_corr", "seed"}
        if unknown:
            raise ValueError("GainModel: unknown keys %s" % sorted(unknown))
        return cls(**conf)

    def __repr__(self):
        return "GainModel(sigma_amp=%r, sigma_phase=%r, corr_time=%r, freq_corr=%r, seed=%r)" % (
            self.sigma_amp, self.sigma_phase, self.corr_time, self.freq_corr, self.seed)

    def kmax(self, ntime):
        """K: (ntime - 1) // 2, capped where s_k = exp(-(2 pi k corr_time / T_SIDEREAL)^2 / 2) drops below 2^-53, i.e. at
        floor(sqrt(106 ln 2) T_SIDEREAL / (2 pi corr_time))."""
        K = (int(ntime) - 1) // 2
        if self.corr_time > 0.0:
            K = min(K, int(np.floor(np.sqrt(106.0 * np.log(2.0)) * T_SIDEREAL / (2.0 * np.pi * self.corr_time))))
        return max(K, 0)

    def weights(self, ntime):
        """c_k, k = 0 .. K: c_k^2 = s_k / sum_j s_j (sum of squares 1, so Var x_q = sigma_q^2)."""
        k = np.arange(self.kmax(ntime) + 1, dtype=np.float64)
        s = np.exp(-0.5 * (2.0 * np.pi * k * self.corr_time / T_SIDEREAL) ** 2)
        return np.sqrt(s / s.sum())

    def correlation(self, ntime, lag):
        """E x(t) x(t + lag) / sigma^2 = sum_k c_k^2 cos(2 pi k lag / ntime), exactly."""
        c = self.weights(ntime)
        return float(np.sum(c**2 * np.cos(2.0 * np.pi * np.arange(c.shape[0]) * lag / ntime)))


# ---- flags of simulated timestreams ---------------------------------------------------------------
STREAM_TS_FLAG = 27          # flag bursts: apart from 0, 1, 2, 16, 17 and 24-26


class FlagModel:
    """Flags of a simulated timestream, weights 0 (flagged) / 1 per (frequency, time sample), the same for every baseline.

    Bursts: a run of ``burst`` samples, cyclic over the day, starts at sample s of global frequency f when
    u(seed, f, s) < p with 1 - (1 - p)^burst = ``fraction``, the probability that a sample is flagged; u is the uniform
    of Philox4x32-10 with key ``seed`` and counter (s, f, 0, 27).  ``windows``: (start, end) in sidereal hours (end <
    start wraps midnight), flagged at all frequencies — the daytime cut.  Host only; the mask of a frequency depends on
    (seed, global frequency) alone, so frequency subsets reproduce the rows of the full call."""

    def __init__(self, fraction=0.0, burst=1, windows=(), seed=0):
        self.fraction, self.burst, self.seed = float(fraction), int(burst), int(seed)
        self.windows = tuple((float(a), float(b)) for a, b in windows)
        if not 0.0 <= self.fraction < 1.0:
            raise ValueError("FlagModel: fraction must lie in [0, 1)")
        if self.burst < 1:
            raise ValueError("FlagModel: burst must be at least 1")
        if any(not (0.0 <= a <= 24.0 and 0.0 <= b <= 24.0) for a, b in self.windows):
            raise ValueError("FlagModel: windows are (start, end) in hours between 0 and 24")

    @classmethod
    def from_config(cls, conf):
        conf = dict(conf)
        unknown = set(conf) - {"fraction", "burst", "windows", "seed"}
        if unknown:
            raise ValueError("FlagModel: unknown keys %s" % sorted(unknown))
        return cls(**conf)

    def __repr__(self):
        return "FlagModel(fraction=%r, burst=%r, windows=%r, seed=%r)" % (self.fraction, self.burst, self.windows, self.seed)

    def start_probability(self):
        """p with 1 - (1 - p)^burst = fraction."""
        return 1.0 - (1.0 - self.fraction) ** (1.0 / self.burst)

    def mask(self, ntime, fglobal):
        """(nf, ntime) float64 of 0 (flagged) / 1 for the global frequency indices ``fglobal``."""
        ntime = int(ntime)
        fg = np.asarray(fglobal, dtype=np.uint64).reshape(-1)
        flagged = np.zeros((fg.shape[0], ntime), dtype=bool)
        if self.fraction > 0.0 and ntime > 0 and fg.shape[0] > 0:
            f, s = np.meshgrid(fg, np.arange(ntime, dtype=np.uint64), indexing="ij")
            seed = self.seed & 0xFFFFFFFFFFFFFFFF
            w = _philox4x32_10([s, f, np.zeros_like(s), np.full_like(s, STREAM_TS_FLAG)], (seed & 0xFFFFFFFF, seed >> 32))
            start = _u53(w[0], w[1]) < self.start_probability()
            for d in range(min(self.burst, ntime)):
                flagged |= np.roll(start, d, axis=1)
        t_hours = 24.0 * np.arange(ntime) / max(ntime, 1)
        for a, b in self.windows:
            cut = (t_hours >= a) & (t_hours < b) if a <= b else (t_hours >= a) | (t_hours < b)
            flagged |= cut[None, :]
        return np.where(flagged, 0.0, 1.0)


STREAM_TS_RFI = 28           # interference bursts: apart from 0, 1, 2, 16, 17 and 24-27


class RFIModel:
    """Interference added to a simulated day, so that a flagger has ground truth.  Host only.

    Bursts are placed as in `FlagModel`: a run of ``burst`` samples, cyclic over the day, starts at sample s of global
    frequency f when u(seed, f, s) < p with 1 - (1 - p)^burst = ``fraction``; u is the uniform of Philox4x32-10 with key
    ``seed`` and counter (s, f, 0, 28).  The same samples are hit in every row of a frequency.  Every sample of a burst
    adds ``amplitude`` x the row's noise sigma x e^{i theta}, theta = 2 pi u of counter (s, f, row + 1, 28): one phase
    per (row, burst); bursts that overlap add up.  A frequency depends on (seed, global frequency) alone, so frequency
    subsets reproduce the rows of the full call."""

    def __init__(self, fraction=0.0, burst=1, amplitude=10.0, seed=0):
        self.fraction, self.burst, self.amplitude, self.seed = float(fraction), int(burst), float(amplitude), int(seed)
        if not 0.0 <= self.fraction < 1.0:
            raise ValueError("RFIModel: fraction must lie in [0, 1)")
        if self.burst < 1:
            raise ValueError("RFIModel: burst must be at least 1")
        if not (np.isfinite(self.amplitude) and self.amplitude >= 0.0):
            raise ValueError("RFIModel: amplitude must be finite and not negative")

    @classmethod
    def from_config(cls, conf):
        conf = dict(conf)
        unknown = set(conf) - {"fraction", "burst", "amplitude", "seed"}
        if unknown:
            raise ValueError("RFIModel: unknown keys %s" % sorted(unknown))
        return cls(**conf)

    def __repr__(self):
        return "RFIModel(fraction=%r, burst=%r, amplitude=%r, seed=%r)" % (self.fraction, self.burst, self.amplitude, self.seed)

    def start_probability(self):
        """p with 1 - (1 - p)^burst = fraction."""
        return 1.0 - (1.0 - self.fraction) ** (1.0 / self.burst)

    def _key(self):
        seed = self.seed & 0xFFFFFFFFFFFFFFFF
        return (seed & 0xFFFFFFFF, seed >> 32)

    def starts(self, ntime, fglobal):
        """(nf, ntime) bool: the samples where a burst starts."""
        fg = np.asarray(fglobal, dtype=np.uint64).reshape(-1)
        if not (self.fraction > 0.0 and ntime > 0 and fg.shape[0] > 0):
            return np.zeros((fg.shape[0], int(ntime)), dtype=bool)
        f, s = np.meshgrid(fg, np.arange(int(ntime), dtype=np.uint64), indexing="ij")
        w = _philox4x32_10([s, f, np.zeros_like(s), np.full_like(s, STREAM_TS_RFI)], self._key())
        return _u53(w[0], w[1]) < self.start_probability()

    def mask(self, ntime, fglobal):
        """(nf, ntime) bool, True where a burst hits: the truth."""
        start = self.starts(ntime, fglobal)
        hit = np.zeros_like(start)
        for d in range(min(self.burst, int(ntime))):
            hit |= np.roll(start, d, axis=1)
        return hit

    def bursts(self, ntime, fglobal, nrow):
        """(nf, nrow, ntime) complex128: what the bursts add to data of unit noise sigma."""
        ntime, nrow = int(ntime), int(nrow)
        fg = np.asarray(fglobal, dtype=np.uint64).reshape(-1)
        start = self.starts(ntime, fg)
        out = np.zeros((fg.shape[0], nrow, ntime), dtype=np.complex128)
        for i, s in zip(*np.nonzero(start)):
            rows = np.arange(1, nrow + 1, dtype=np.uint64)
            w = _philox4x32_10([np.full_like(rows, s), np.full_like(rows, fg[i]), rows, np.full_like(rows, STREAM_TS_RFI)],
                               self._key())
            ph = self.amplitude * np.exp(1j * 6.283185307179586 * _u53(w[0], w[1]))
            for d in range(min(self.burst, ntime)):
                out[i, :, (s + d) % ntime] += ph
        return out


def as_weights(weights, nf, npairs, ntime, fglobal):
    """The `weights` argument of the simulators as a float64 array broadcastable to (nf, npairs, ntime) — (nf, npairs,
    ntime), (nf, 1, ntime) from a FlagModel, a dict of its arguments or an (nf, ntime) array, or (ntime,) — checked."""
    if isinstance(weights, dict):
        weights = FlagModel.from_config(weights)
    if isinstance(weights, FlagModel):
        return weights.mask(ntime, fglobal)[:, None, :]
    if hasattr(weights, "data_ptr"):
        weights = weights.cpu().numpy()
    w = np.asarray(weights, dtype=np.float64)
    if w.shape not in ((nf, npairs, ntime), (nf, ntime), (ntime,)):
        raise ValueError("weights %s are not (nfreq, npairs, ntime), (nfreq, ntime) or (ntime,) = (%d, %d, %d)"
                         % (w.shape, nf, npairs, ntime))
    if w.size and not np.all(np.isfinite(w) & (w >= 0)):
        raise ValueError("weights must be finite and not negative")
    return w[:, None, :] if w.ndim == 2 else w


def as_gains(gains):
    """None, a GainModel, a dict (-> GainModel.from_config) or an explicit array / device tensor, checked."""
    if gains is None or isinstance(gains, GainModel):
        return gains
    if isinstance(gains, dict):
        return GainModel.from_config(gains)
    if hasattr(gains, "data_ptr"):
        if gains.dim() not in (3, 4) or not (gains.is_complex() and gains.element_size() == 16):
            raise ValueError("gains: a complex128 tensor (nf, nfeed, ntime) or (nreal, nf, nfeed, ntime) expected")
        return gains
    gains = np.asarray(gains)
    if gains.ndim not in (3, 4) or gains.dtype != np.complex128:
        raise ValueError("gains: a complex128 array (nf, nfeed, ntime) or (nreal, nf, nfeed, ntime) expected")
    return gains


def _gain_fword(model, fglobal):
    fg = np.asarray(fglobal, dtype=np.int64).reshape(-1)
    if fg.size and fg.min() < 0:
        raise ValueError("gains: negative global frequency index")
    return np.full(fg.shape, GAIN_BROADBAND, dtype=np.uint64) if model.freq_corr == "full" else fg.astype(np.uint64)


def gain_coeff_host(model, nfeed, fglobal, ntime, nreal, first=0, stream=STREAM_TS_GAIN_AMP):
    """The coefficients of ``Context.ts_gain_coeff`` in numpy: [nreal, nf, nfeed, K + 1],
    sigma_q c_k (A_k - i B_k) = sigma_q c_k sqrt(2) conj(z_k) with z_k the unit draw of counter
    (feed, fglobal[i] or 0xFFFFFFFF, k, ((first + r) << 8) | stream), key = the model's seed."""
    if stream not in (STREAM_TS_GAIN_AMP, STREAM_TS_GAIN_PHASE):
        raise ValueError("gain_coeff_host: stream is STREAM_TS_GAIN_AMP or STREAM_TS_GAIN_PHASE")
    if first < 0 or first + nreal > TS_NOISE_MAX_REAL:
        raise ValueError("gain_coeff_host: realisations beyond the %d the counter word holds" % TS_NOISE_MAX_REAL)
    sigma = model.sigma_amp if stream == STREAM_TS_GAIN_AMP else model.sigma_phase
    ck = model.weights(ntime)
    r, f, a, k = np.meshgrid(np.arange(first, first + nreal, dtype=np.uint64), _gain_fword(model, fglobal),
                             np.arange(nfeed, dtype=np.uint64), np.arange(ck.shape[0], dtype=np.uint64), indexing="ij")
    seed = int(model.seed) & 0xFFFFFFFFFFFFFFFF
    w = _philox4x32_10([a, f, k, (r << np.uint64(8)) | np.uint64(stream)], (seed & 0xFFFFFFFF, seed >> 32))
    rad = np.sqrt(-np.log(_u53(w[0], w[1]))) * (sigma * ck * 1.4142135623730951)
    th = 6.283185307179586 * _u53(w[2], w[3])
    return rad * np.cos(th) - 1j * (rad * np.sin(th))


def gain_series_host(coeff, ntime):
    """x(t) = Re sum_k coeff[..., k] e^{2 pi i k t / ntime}: [..., ntime] float64."""
    k = np.arange(coeff.shape[-1])
    ph = np.exp(2j * np.pi * (np.outer(k, np.arange(ntime)) % ntime) / ntime)
    return (coeff @ ph).real


def gains_host(model, nfeed, fglobal, ntime, nreal, first=0):
    """The gains of ``gains_device`` in numpy: [nreal, nf, nfeed, ntime] complex128."""
    xa = gain_series_host(gain_coeff_host(model, nfeed, fglobal, ntime, nreal, first, STREAM_TS_GAIN_AMP), ntime)
    xp = gain_series_host(gain_coeff_host(model, nfeed, fglobal, ntime, nreal, first, STREAM_TS_GAIN_PHASE), ntime)
    return (1.0 + xa) * np.cos(xp) + 1j * ((1.0 + xa) * np.sin(xp))


def baseline_gains_host(g, class_off, members):
    """G[..., c, t] = (1 / n_c) sum_{(i, j) in class c} g[..., i, t] conj(g[..., j, t]) for g [..., nfeed, ntime] and the
    pair table of ``TransitTelescope.redundant_pairs``: what per-feed gains do to a stack of redundant baselines.  The
    members of a class are added one after the other in the table's order."""
    g = np.asarray(g)
    class_off = np.asarray(class_off, dtype=np.int64)
    members = np.asarray(members, dtype=np.int64).reshape(-1, 2)
    n = np.diff(class_off)
    if class_off[0] != 0 or np.any(n <= 0) or class_off[-1] != members.shape[0]:
        raise ValueError("baseline_gains_host: class offsets must start at 0, ascend strictly and end at len(members)")
    if members.size and (members.min() < 0 or members.max() >= g.shape[-2]):
        raise ValueError("baseline_gains_host: a member names a feed the gains do not have")
    G = np.zeros(g.shape[:-2] + (n.shape[0], g.shape[-1]), dtype=g.dtype)
    for c in range(n.shape[0]):
        for i, j in members[class_off[c] : class_off[c + 1]]:
            G[..., c, :] += g[..., i, :] * g[..., j, :].conj()
    return G / n[:, None]


def check_explicit_gains(gains, nreal, nf, nfeed, ntime):
    """Refuse an explicit gain array that is not (nf, nfeed, ntime) or (1 or nreal, nf, nfeed, ntime); only shapes are
    looked at."""
    shape = tuple(int(v) for v in gains.shape)
    if shape[-3:] != (nf, nfeed, ntime) or shape[:-3] not in ((), (1,), (nreal,)):
        raise ValueError("gains: shape %s does not fit (nreal = %d, nf = %d, nfeed = %d, ntime = %d)"
                         % (shape, nreal, nf, nfeed, ntime))


def explicit_gains(gains, nreal, nf, r0, R, sel, nfeed, ntime):
    """The rows of an explicit gain array for realisations r0 .. r0 + R - 1 of a call of `nreal` realisations and `nf`
    frequencies, at the positions `sel` of its frequencies: (1 or R, len(sel), nfeed, ntime), numpy or device as given."""
    check_explicit_gains(gains, nreal, nf, nfeed, ntime)
    g = gains if len(gains.shape) == 4 else gains[None]
    g = g if g.shape[0] == 1 else g[r0 : r0 + R]
    if isinstance(sel, range) and sel.step == 1:
        return g[:, sel.start : sel.stop]             # a view: nothing is copied
    return g[:, list(sel)]


def gain_series_device(model, nfeed, fglobal, ntime, nreal, first=0, stream=STREAM_TS_GAIN_AMP):
    """(coeff, x) on the device: the coefficients (nreal, nf, nfeed, K + 1) of one component (``Context.ts_gain_coeff``)
    and its series (nreal, nf, nfeed, ntime) as the complex numbers sum_k coeff_k e^{2 pi i k t / ntime}, whose real part
    is x(t): one strided-batched ZGEMM against ntime times the conjugate of the table of ``Context.mmode_twiddle``."""
    from .device import get_context

    ctx = get_context()
    fg = np.asarray(fglobal, dtype=np.int64).reshape(-1)
    nf, ntime, nreal, nfeed = int(fg.shape[0]), int(ntime), int(nreal), int(nfeed)
    ck = model.weights(ntime)
    K = ck.shape[0] - 1
    sigma = model.sigma_amp if stream == STREAM_TS_GAIN_AMP else model.sigma_phase
    coeff = ctx.ts_gain_coeff(nreal, fg, nfeed, ck, sigma, model.seed, first, stream, broadband=model.freq_corr == "full")
    x = ctx.empty((nreal, nf, nfeed, ntime), np.complex128)
    rows = nreal * nf * nfeed
    if rows and ntime:
        W = ctx.mmode_twiddle(ntime, K)
        ctx.zgemm(coeff, W, x, rows, ntime, K + 1, rsA=K + 1, csA=1, rsB=1, csB=K + 1, ldc=ntime, conjB=True,
                  alpha=float(ntime))
    return coeff, x


def gains_device(model, nfeed, fglobal, ntime, nreal, first=0, out=None):
    """The gains of `model` on the device: (nreal, nf, nfeed, ntime) c128 — ``gains_host`` restates it.  The series of
    both components come from ``gain_series_device`` and ``Context.ts_gain_compose`` makes g from them.  Working memory:
    two more buffers of g's size."""
    from .device import get_context

    xa = gain_series_device(model, nfeed, fglobal, ntime, nreal, first, STREAM_TS_GAIN_AMP)[1]
    xp = gain_series_device(model, nfeed, fglobal, ntime, nreal, first, STREAM_TS_GAIN_PHASE)[1]
    return get_context().ts_gain_compose(xa, xp, out=out)


# ---- the device path ---------------------------------------------------------------------------------------------------
def _runs(idx):
    """Sorted integers as [(start, count)] of consecutive runs."""
    out = []
    for i in idx:
        if out and out[-1][0] + out[-1][1] == i:
            out[-1][1] += 1
        else:
            out.append([int(i), 1])
    return out


def draw_alm(cv, nreal=1, seed=0, stream=STREAM_SKY_SIGNAL, first=0, mmax=None, freqs=None, to_host=True, roots=None):
    """Realisations ``first .. first + nreal - 1`` of the sky of covariance ``cv``: a_lm [nreal, nfreq_sel, npol, L, M]
    complex128, M = min(mmax, lmax) + 1 (all m by default).

    ``freqs`` (sorted frequency indices) computes only those rows, from the same draws as the full call: a rank of a
    distributed simulation gets its share without communication.  ``roots`` takes ``covariance_roots(cv)`` made
    earlier.  ``to_host=False`` returns the device tensor."""
    cv = _check_cv(cv)
    from .device import get_context

    ctx = get_context()
    npol, L, nfreq = cv.shape[0], cv.shape[2], cv.shape[3]
    M = L if mmax is None else min(int(mmax) + 1, L)
    sel = list(range(nfreq)) if freqs is None else [int(f) for f in freqs]
    if sorted(set(sel)) != sel or (sel and not 0 <= sel[0] <= sel[-1] < nfreq):
        raise ValueError("freqs must be sorted, distinct frequency indices")
    pos = {f: k for k, f in enumerate(sel)}
    nsel = len(sel)
    grp = groups(cv)
    roots = covariance_roots(cv) if roots is None else roots
    out = ctx.empty((int(nreal), nsel, npol, L, M), np.complex128)
    if out.numel() == 0:
        return np.zeros(tuple(out.shape), dtype=np.complex128) if to_host else out
    drawn = set()
    for jg, T in zip(grp, roots):
        p, f = jg // nfreq, jg % nfreq
        drawn.update(int(x) for x in p)
        rowoff = np.array([(pos.get(int(fi), 0) * npol + int(pi)) * L * M for pi, fi in zip(p, f)], dtype=np.int64)
        for row0, nrows in _runs([i for i in range(len(jg)) if int(f[i]) in pos]):
            ctx.sky_draw(T, jg, rowoff, nfreq, row0, nrows, M, seed, stream, first, nreal, out,
                         (nsel * npol * L * M, M, 1))
    for pi in range(npol):   # polarisations without power
        if pi not in drawn:
            out[:, :, pi].zero_()
    return ctx.to_host(out) if to_host else out


def gaussian_sky(cv, nside, nreal=1, seed=0, stream=STREAM_SKY_SIGNAL, first=0, mmax=None, freqs=None,
                 max_bytes=4 << 30):
    """``draw_alm`` followed by ``healpix.sphtrans_inv_sky``: real maps [nreal, freq, pol, pixel].  The coefficients stay
    on the device; a pass is one realisation of as many frequencies as ``max_bytes`` allows the synthesis."""
    from . import healpix

    cv = _check_cv(cv)
    npol, L, nfreq = cv.shape[0], cv.shape[2], cv.shape[3]
    if npol not in (1, 4):
        raise ValueError("gaussian_sky: 1 or 4 polarisations")
    sel = list(range(nfreq)) if freqs is None else [int(f) for f in freqs]
    M = L if mmax is None else min(int(mmax) + 1, L)
    nf = healpix.synth_chunk(len(sel), npol, L, M, nside, max_bytes)
    roots = covariance_roots(cv)
    out = np.empty((int(nreal), len(sel), npol, healpix.npix(nside)))
    for r in range(int(nreal)):
        for f0 in range(0, len(sel), nf):
            a = draw_alm(cv, 1, seed, stream, first + r, mmax, sel[f0 : f0 + nf], to_host=False, roots=roots)
            out[r, f0 : f0 + nf] = healpix.sphtrans_inv_sky(a[0], nside, max_bytes)
            del a
    return out


def write_sky(fname, maps):
    """Write one sky [freq, pol, pixel] as the ``map`` dataset that ``timestream.simulate(maps=[...])`` reads."""
    from . import storage

    maps = np.asarray(maps, dtype=np.float64)
    if maps.ndim != 3:
        raise ValueError("write_sky: one sky [freq, pol, pixel]")
    with storage.File(fname, "w") as f:
        f.create_dataset("map", data=maps)


# ---- point sources ----------------------------------------------------------------------------
SOURCE_CHUNK = 1024          # sources per product of dm_source_alm (SRC_CHUNK of dm_sources.hip): fixes the summation order
_C_LIGHT = 299792458.0       # m / s
_K_BOLTZMANN = 1.380649e-23  # J / K
_CAT_KEYS = ("theta", "phi", "flux", "nu0", "index", "curvature")


def read_catalogue(cat):
    """A catalogue as a dict of float64 arrays: ``theta``, ``phi`` (nsrc, rad), ``flux`` (nsrc, 1 or 4) in Jy at ``nu0``
    (MHz, a scalar or one per source), ``index`` and ``curvature`` (nsrc; the latter 0 when absent), and ``redshift`` (nsrc) only when the catalogue carries it.  ``cat``: such a dict,
    or the name of a file written by `write_catalogue` (`.npz` or HDF5 through `storage.File`)."""
    if isinstance(cat, (str, bytes)) or hasattr(cat, "__fspath__"):
        from . import storage

        with storage.File(cat, "r") as f:
            cat = {k: np.asarray(f[k][:]) for k in _CAT_KEYS + ("redshift",) if k in f}
    missing = [k for k in ("theta", "phi", "flux", "nu0", "index") if k not in cat]
    if missing:
        raise ValueError("source catalogue without %s" % ", ".join(missing))
    theta = np.asarray(cat["theta"], dtype=np.float64).reshape(-1)
    n = theta.size
    flux = np.asarray(cat["flux"], dtype=np.float64)
    flux = flux.reshape(n, 1) if flux.ndim == 1 else flux
    if flux.shape not in ((n, 1), (n, 4)):
        raise ValueError("source catalogue: flux (nsrc, 1 or 4) expected, got %s" % (flux.shape,))
    out = dict(theta=theta, flux=flux)
    for k in ("phi", "nu0", "index", "curvature"):
        v = np.asarray(cat.get(k, 0.0), dtype=np.float64).reshape(-1)
        if v.size not in (1, n):
            raise ValueError("source catalogue: %s needs one value, or one per source" % k)
        out[k] = np.broadcast_to(v, (n,)).copy()
    if n and not (np.all(theta >= 0.0) and np.all(theta <= np.pi)):
        raise ValueError("source catalogue: theta outside [0, pi]")
    if n and not np.all(out["nu0"] > 0.0):
        raise ValueError("source catalogue: nu0 must be positive")
    if cat.get("redshift", None) is not None:   # optional: the objects of a stacking catalogue (`Timestream.catalogue_spectra`)
        red = np.asarray(cat["redshift"], dtype=np.float64).reshape(-1)
        if red.shape != (n,):
            raise ValueError("source catalogue: redshift needs one value per source")
        out["redshift"] = red.copy()
    return out


def write_catalogue(fname, cat):
    """Write a catalogue (see `read_catalogue`) as the file `timestream.simulate(sources=[...])` reads."""
    from . import storage

    cat = read_catalogue(cat)
    with storage.File(fname, "w") as f:
        for k in _CAT_KEYS + (("redshift",) if "redshift" in cat else ()):
            f.create_dataset(k, data=cat[k])


def source_spectra(cat, frequencies):
    """Temperature x solid angle (nf, npol, nsrc) in K sr of the sources at ``frequencies`` (MHz):
    S(nu) = S0 (nu / nu0)^(index + curvature ln(nu / nu0)) in Jy and T Omega = S 1e-26 c^2 / (2 k_B nu^2); every Stokes
    parameter of a source follows the same spectrum."""
    cat = read_catalogue(cat)
    nu = np.asarray(frequencies, dtype=np.float64).reshape(-1)
    x = np.log(nu[:, None] / cat["nu0"][None, :])                                       # (nf, nsrc)
    s = np.exp((cat["index"][None, :] + cat["curvature"][None, :] * x) * x)
    conv = 1e-26 * _C_LIGHT ** 2 / (2.0 * _K_BOLTZMANN * (nu * 1e6) ** 2)               # Jy -> K sr
    return np.ascontiguousarray((conv[:, None] * s)[:, None, :] * cat["flux"].T[None, :, :])


def random_catalogue(n, seed, flux_min=0.1, flux_max=100.0, gamma=2.5, index_mean=-0.7, index_sigma=0.2, pol_frac=0.0,
                     nu0=600.0):
    """A stand-in population of ``n`` sources (like the other sky models here: the shape of a radio-source population, not a
    fitted one): isotropic positions, fluxes in [flux_min, flux_max] Jy at ``nu0`` MHz with dN/dS ~ S^-gamma by inverse
    transform, Gaussian spectral indices.  pol_frac > 0 gives (I, Q, U, V) with linear polarisation pol_frac I at a
    uniform angle and V = 0; pol_frac = 0 gives I alone.  Host numpy, reproducible by ``seed``."""
    n = int(n)
    if not 0.0 < flux_min <= flux_max:
        raise ValueError("random_catalogue: 0 < flux_min <= flux_max expected")
    rng = np.random.default_rng(seed)
    z = rng.uniform(-1.0, 1.0, n)
    phi = rng.uniform(0.0, 2.0 * np.pi, n)
    u = rng.uniform(0.0, 1.0, n)
    if gamma == 1.0:
        s = flux_min * (flux_max / flux_min) ** u
    else:
        a = 1.0 - gamma
        s = (flux_min ** a + u * (flux_max ** a - flux_min ** a)) ** (1.0 / a)
    s = np.clip(s, flux_min, flux_max)
    index = index_mean + index_sigma * rng.standard_normal(n)
    if pol_frac:
        chi = rng.uniform(0.0, np.pi, n)
        flux = np.stack([s, pol_frac * s * np.cos(2.0 * chi), pol_frac * s * np.sin(2.0 * chi), np.zeros(n)], axis=1)
    else:
        flux = s[:, None]
    return dict(theta=np.arccos(z), phi=phi, flux=flux, nu0=np.full(n, float(nu0)), index=index, curvature=np.zeros(n))


def _source_arrays(theta, phi, flux):
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    phi = np.mod(np.asarray(phi, dtype=np.float64).reshape(-1), 2.0 * np.pi)            # [0, 2 pi) on entry
    phi = np.where(phi >= 2.0 * np.pi, 0.0, phi)
    flux = np.asarray(flux, dtype=np.float64)
    if flux.ndim != 3 or flux.shape[1] not in (1, 4):
        raise ValueError("point sources: flux (nf, 1 or 4, nsrc) expected, got %s" % (flux.shape,))
    if not (theta.shape == phi.shape == (flux.shape[2],)):
        raise ValueError("point sources: theta, phi and flux need one entry per source")
    z, sth = np.cos(theta), np.sin(theta)
    if flux.shape[1] == 4:
        bad = np.nonzero((sth == 0.0) & (flux[:, 1:3] != 0.0).any(axis=(0, 1)))[0]
        if bad.size:
            raise ValueError("point sources: source %d lies at a pole (sin theta = 0) and is polarised: Q and U are "
                             "undefined there" % bad[0])
    return z, sth, phi, np.ascontiguousarray(flux)


def _m_range(lmax, mmax, m_range):
    if m_range is not None and mmax is not None:
        raise ValueError("point sources: mmax or m_range, not both")
    m_lo, m_hi = (0, lmax if mmax is None else min(int(mmax), lmax)) if m_range is None else (int(m_range[0]), int(m_range[1]))
    if not 0 <= m_lo <= m_hi <= lmax:
        raise ValueError("point sources: 0 <= m_lo <= m_hi <= lmax expected, got (%d, %d) with lmax %d" % (m_lo, m_hi, lmax))
    return m_lo, m_hi


def source_alm_host(theta, phi, flux, lmax, mmax=None, m_range=None):
    """The a_lm (nf, npol, lmax + 1, nm) of point sources at (theta, phi) with temperature x solid angle ``flux``
    (nf, npol, nsrc), npol = 1 (I -> T) or 4 (I, Q, U, V -> T, E, B, V), m = 0 .. mmax (or m_range, inclusive):

        a^T_lm = sum_s I_s lambda_lm(cos theta_s) e^{-i m phi_s}                      (a^V alike)
        a^E_lm = sum_s e^{-i m phi_s} (W_lm Q_s + i X_lm U_s),   a^B_lm = sum_s e^{-i m phi_s} (W_lm U_s - i X_lm Q_s)

    with `healpix.lambda_lm` / `wx_lm`: the coefficients whose synthesis `healpix.sphtrans_inv_sky_host`, summed against
    the fluxes at the sources, gives sum_pol sum_l [Re(a_l0 b*_l0) + 2 sum_{m > 0} Re(a_lm b*_lm)].  Plain numpy: the oracle
    of `source_alm`, for any input."""
    from . import healpix

    z, sth, phi, flux = _source_arrays(theta, phi, flux)
    lmax = int(lmax)
    m_lo, m_hi = _m_range(lmax, mmax, m_range)
    nf, npol, nsrc = flux.shape
    out = np.zeros((nf, npol, lmax + 1, m_hi - m_lo + 1), dtype=np.complex128)
    if nsrc == 0:
        return out
    off = sth > 0.0                                                  # W and X exist off the poles only
    for m in range(m_lo, m_hi + 1):
        ph = np.cos(m * phi) - 1j * np.sin(m * phi)
        lam = healpix.lambda_lm(lmax, m, z)                          # (L - m, nsrc)
        fp = flux * ph[None, None, :]
        o = out[:, :, m:, m - m_lo]
        o[:, 0] = fp[:, 0] @ lam.T
        if npol == 4:
            o[:, 3] = fp[:, 3] @ lam.T
            W, X = healpix.wx_lm(lmax, m, z[off])
            q, u = fp[:, 1][:, off], fp[:, 2][:, off]
            o[:, 1] = q @ W.T + 1j * (u @ X.T)
            o[:, 2] = u @ W.T - 1j * (q @ X.T)
    return out


def source_alm(cat_or_arrays, lmax, frequencies=None, mmax=None, m_range=None, freqs=None, to_host=True,
               max_bytes=2 << 30):
    """The exact band-limited a_lm of point sources on the device (`dm_source_alm`): (nf, npol, lmax + 1, nm) complex128,
    polarisations T or T, E, B, V, m = 0 .. min(mmax, lmax) or ``m_range = (m_lo, m_hi)`` inclusive — the layout
    `draw_alm` gives per realisation.  No map, no nside: a source sits where the catalogue puts it.

    ``cat_or_arrays``: a catalogue (`read_catalogue`: a dict or a file name) evaluated at ``frequencies`` (MHz) through
    `source_spectra`, or arrays ``(theta, phi, flux)`` with flux (nf, npol, nsrc) in K sr.  ``freqs`` (sorted indices)
    computes those frequency rows only.  ``to_host=False`` returns the device tensor.  ``max_bytes`` bounds the tables
    alive on the device at once and has no influence on the bits of the result."""
    if isinstance(cat_or_arrays, (tuple, list)):
        theta, phi, flux = cat_or_arrays
    else:
        if frequencies is None:
            raise ValueError("source_alm: a catalogue needs the frequencies (MHz) to evaluate its spectra at")
        cat = read_catalogue(cat_or_arrays)
        theta, phi, flux = cat["theta"], cat["phi"], source_spectra(cat, frequencies)
    flux = np.asarray(flux, dtype=np.float64)
    if freqs is not None:
        sel = [int(f) for f in freqs]
        if flux.ndim != 3 or sorted(set(sel)) != sel or (sel and not 0 <= sel[0] <= sel[-1] < flux.shape[0]):
            raise ValueError("freqs must be sorted, distinct frequency indices")
        flux = flux[sel]
    z, sth, phi, flux = _source_arrays(theta, phi, flux)
    lmax = int(lmax)
    m_lo, m_hi = _m_range(lmax, mmax, m_range)
    from .device import get_context

    ctx = get_context()
    out = ctx.source_alm(z, sth, phi, flux, lmax, m_lo, m_hi, max_bytes=max_bytes)
    return ctx.to_host(out) if to_host else out


# ---- coefficients at catalogue positions and their stack --------------------------------------
POINTS_FBLOCK = 8            # frequencies of one call are cut in multiples of this: the blocks of dm_points.hip (8 and 4)
LINE_21CM_MHZ = 1420.40575177


def _point_arrays(theta, phi, npol):
    theta = np.asarray(theta, dtype=np.float64).reshape(-1)
    phi = np.mod(np.asarray(phi, dtype=np.float64).reshape(-1), 2.0 * np.pi)            # [0, 2 pi) on entry
    phi = np.where(phi >= 2.0 * np.pi, 0.0, phi)
    if theta.shape != phi.shape:
        raise ValueError("points: theta and phi need one entry per point")
    if theta.size and not (np.all(theta >= 0.0) and np.all(theta <= np.pi)):
        raise ValueError("points: theta outside [0, pi]")
    z, sth = np.cos(theta), np.sin(theta)
    if npol == 4:
        bad = np.nonzero(sth == 0.0)[0]
        if bad.size:
            raise ValueError("points: point %d lies at a pole (sin theta = 0): Q and U are undefined there" % bad[0])
    return z, sth, phi


def _points_ms(ms, nm, lmax):
    ms = np.arange(nm, dtype=np.int64) if ms is None else np.asarray(ms, dtype=np.int64).reshape(-1)
    if ms.shape != (nm,):
        raise ValueError("points: ms needs one m per column of the coefficients (%d), got %d" % (nm, ms.size))
    if nm and (ms.min() < 0 or ms.max() > lmax or np.unique(ms).size != nm):
        raise ValueError("points: the m of ms must be distinct and within 0 .. lmax = %d" % lmax)
    return ms


def read_positions(cat_or_arrays):
    """(theta, phi, redshift or None) of a stacking catalogue: arrays ``(theta, phi)`` or ``(theta, phi, redshift)``, a
    dict with those keys, or the name of a file that holds them (a file of `write_catalogue` is one).  Fluxes and spectra
    are not needed and not looked at."""
    if isinstance(cat_or_arrays, (tuple, list)):
        if len(cat_or_arrays) not in (2, 3):
            raise ValueError("points: (theta, phi) or (theta, phi, redshift) expected")
        cat = dict(zip(("theta", "phi", "redshift"), cat_or_arrays))
    elif isinstance(cat_or_arrays, (str, bytes)) or hasattr(cat_or_arrays, "__fspath__"):
        from . import storage

        with storage.File(cat_or_arrays, "r") as f:
            cat = {k: np.asarray(f[k][:]) for k in ("theta", "phi", "redshift") if k in f}
    else:
        cat = cat_or_arrays
    if "theta" not in cat or "phi" not in cat:
        raise ValueError("points: a catalogue needs theta and phi")
    theta = np.asarray(cat["theta"], dtype=np.float64).reshape(-1)
    phi = np.asarray(cat["phi"], dtype=np.float64).reshape(-1)
    red = cat.get("redshift", None)
    if red is not None:
        red = np.asarray(red, dtype=np.float64).reshape(-1)
        if red.shape != theta.shape:
            raise ValueError("points: redshift needs one entry per point")
    return theta, phi, red


def alm_at_points_host(alm, theta, phi, ms=None):
    """The coefficients ``alm`` (nf, npol, lmax + 1, nm), npol = 1 (T) or 4 (T, E, B, V), column j holding m = ms[j]
    (default j), evaluated at the points (theta, phi): (npts, npol, nf) float64, polarisations T or T, Q, U, V.  With
    fac = 1 for m = 0 and 2 otherwise

        F^T_m(s) = sum_l a^T_lm lambda_lm(z_s)  (F^V alike)
        F^Q_m(s) = sum_l a^E_lm W_lm + i a^B_lm X_lm,    F^U_m(s) = sum_l a^B_lm W_lm - i a^E_lm X_lm
        value_p(s, f) = sum_m fac_m Re(F^p_m(s) e^{+i m phi_s})

    the value of `healpix.sphtrans_inv_sky_host` with (z, phi) of a point in the place of (ring, pixel), and the adjoint of
    `source_alm_host`.  z = cos(theta), phi reduced to [0, 2 pi), the phase argument the float64 product m * phi.  A
    subset ``ms`` gives a partial sum.  Plain numpy: the oracle of `alm_at_points`, for any input."""
    from . import healpix

    alm = np.asarray(alm, dtype=np.complex128)
    if alm.ndim != 4 or alm.shape[1] not in (1, 4):
        raise ValueError("points: coefficients (nf, 1 or 4, lmax + 1, nm) expected, got %s" % (alm.shape,))
    nf, npol, L, nm = alm.shape
    lmax = L - 1
    ms = _points_ms(ms, nm, lmax)
    z, sth, phi = _point_arrays(theta, phi, npol)
    out = np.zeros((nf, npol, z.size))
    for j, m in enumerate(int(v) for v in ms):
        lam = healpix.lambda_lm(lmax, m, z)                          # (L - m, npts)
        a = alm[:, :, m:, j]
        F = np.zeros((nf, npol, z.size), dtype=np.complex128)
        F[:, 0] = a[:, 0] @ lam
        if npol == 4:
            W, X = healpix.wx_lm(lmax, m, z)
            F[:, 1] = a[:, 1] @ W + 1j * (a[:, 2] @ X)
            F[:, 2] = a[:, 2] @ W - 1j * (a[:, 1] @ X)
            F[:, 3] = a[:, 3] @ lam
        arg = m * phi
        out += (1.0 if m == 0 else 2.0) * (F.real * np.cos(arg) - F.imag * np.sin(arg))
    return np.ascontiguousarray(out.transpose(2, 1, 0))


def alm_at_points(alm, cat_or_arrays, ms=None, to_host=True, max_bytes=2 << 30, out=None, accumulate=False):
    """`alm_at_points_host` on the device (`dm_alm_at_points`: one fused kernel, the recurrence in registers and no table
    in memory): (npts, npol, nf) float64 — a spectrum per object, no map and no nside.  ``alm`` (nf, npol, lmax + 1, nm):
    numpy, or a complex128 device tensor (any strides of a contiguous tensor's view are not followed: it is made
    contiguous).  ``cat_or_arrays``: see `read_positions`.  ``to_host=False`` returns the device tensor; ``out`` (such a
    tensor) with ``accumulate`` adds the values of this call to it.  ``max_bytes`` bounds the coefficients alive on the
    device beyond ``alm`` itself — host coefficients go up in runs of whole blocks of `POINTS_FBLOCK` frequencies — and
    has no influence on the bits, and neither has the set of points of a call."""
    from .device import get_context

    theta, phi, _ = read_positions(cat_or_arrays)
    on_device = bool(getattr(alm, "is_cuda", False))
    if on_device and not (alm.is_complex() and alm.element_size() == 16):
        raise ValueError("alm_at_points: a device tensor must be complex128, got %s" % (alm.dtype,))
    if not on_device:
        alm = np.asarray(alm, dtype=np.complex128)
    if len(alm.shape) != 4 or int(alm.shape[1]) not in (1, 4):
        raise ValueError("points: coefficients (nf, 1 or 4, lmax + 1, nm) expected, got %s" % (tuple(alm.shape),))
    nf, npol, L, nm = [int(v) for v in alm.shape]
    ms = _points_ms(ms, nm, L - 1)
    z, sth, phi = _point_arrays(theta, phi, npol)
    ctx = get_context()
    npts = z.size
    if out is None:
        if accumulate:
            raise ValueError("alm_at_points: accumulate needs the output to add to")
        out = ctx.empty((npts, npol, nf), np.float64)
    if npts and nf:
        if nm == 0:
            if not accumulate:
                out.zero_()
        elif on_device:
            a = alm.contiguous()
            ctx.alm_at_points(z, sth, phi, ms, a, L - 1, nf, npol, (npol * L * nm, L * nm, nm, 1), out=out,
                              accumulate=accumulate, max_bytes=max_bytes)
        else:
            dz, ds, dp = ctx.to_device(z), ctx.to_device(sth), ctx.to_device(phi)
            per_f = 2 * 16 * npol * L * nm                                             # the upload and its re-ordered copy
            step = max(1, int(max_bytes // (POINTS_FBLOCK * per_f))) * POINTS_FBLOCK
            for f0 in range(0, nf, step):
                f1 = min(nf, f0 + step)
                a = ctx.to_device(alm[f0:f1])
                part = out if (f0, f1) == (0, nf) else ctx.empty((npts, npol, f1 - f0), np.float64)
                if part is not out and accumulate:
                    part.copy_(out[:, :, f0:f1])
                ctx.alm_at_points(dz, ds, dp, ms, a, L - 1, f1 - f0, npol, (npol * L * nm, L * nm, nm, 1), out=part,
                                  accumulate=accumulate, max_bytes=max(max_bytes // 2, 1))
                if part is not out:
                    out[:, :, f0:f1] = part
                del a, part
    return ctx.to_host(out) if to_host else out


def stack_spectra(spectra, freqs_mhz, line_mhz, halfwidth, source_weight=None, channel_weight=None):
    """Stack spectra (nsrc, npol, nf) on the channel of each source's line.  ``freqs_mhz`` (nf >= 2, strictly ascending or
    descending) are the channel centres, ``line_mhz`` (nsrc) the observed frequency of the line of every source
    (`LINE_21CM_MHZ` / (1 + redshift) for 21 cm).  The channel of a source is c_s = argmin_f |nu_f - nu_s|; a source
    whose line lies more than half a channel (half the spacing of the two end channels) outside the band is dropped.
    For the offsets k = -K .. K, K = ``halfwidth``, counted along the axis as stored,

        stack[p, k] = sum_s w_s omega_{c_s + k} T[s, p, c_s + k] / sum_s w_s omega_{c_s + k}

    over the kept sources whose channel c_s + k exists and has omega > 0; ``source_weight`` w (nsrc, default 1, >= 0) and
    ``channel_weight`` omega (nf, default 1, >= 0).  Returns a dict: ``stack`` (npol, 2K + 1; 0 where nothing
    contributed), ``hits`` (2K + 1: the number of terms with non-zero weight), ``weight`` (2K + 1: the denominators),
    ``offsets`` (-K .. K), ``channel`` (nsrc: c_s, -1 for dropped sources).  No sub-channel interpolation.  Host numpy: one
    pass over an array the size of the input."""
    T = np.asarray(spectra, dtype=np.float64)
    nu = np.asarray(freqs_mhz, dtype=np.float64).reshape(-1)
    line = np.asarray(line_mhz, dtype=np.float64).reshape(-1)
    K = int(halfwidth)
    if T.ndim != 3 or T.shape[2] != nu.size or T.shape[0] != line.size:
        raise ValueError("stack_spectra: spectra (nsrc, npol, nf) with nf frequencies and nsrc lines expected")
    if K < 0 or nu.size < 2:
        raise ValueError("stack_spectra: halfwidth >= 0 and two frequencies at least expected")
    d = np.diff(nu)
    if not (np.all(d > 0.0) or np.all(d < 0.0)):
        raise ValueError("stack_spectra: frequencies must ascend or descend strictly")
    nsrc, npol, nf = T.shape
    w = np.ones(nsrc) if source_weight is None else np.asarray(source_weight, dtype=np.float64).reshape(-1)
    om = np.ones(nf) if channel_weight is None else np.asarray(channel_weight, dtype=np.float64).reshape(-1)
    if w.shape != (nsrc,) or om.shape != (nf,) or (w < 0.0).any() or (om < 0.0).any():
        raise ValueError("stack_spectra: non-negative weights, one per source and one per channel, expected")
    offsets = np.arange(-K, K + 1)
    if nsrc == 0:
        chan = np.zeros(0, dtype=np.int64)
    else:
        chan = np.argmin(np.abs(nu[None, :] - line[:, None]), axis=1)
        # the band ends half a channel beyond the centres of its end channels
        lo, hi = (0, nf - 1) if d[0] > 0.0 else (nf - 1, 0)
        below = line < nu[lo] - 0.5 * abs(d[0] if lo == 0 else d[-1])
        above = line > nu[hi] + 0.5 * abs(d[-1] if hi == nf - 1 else d[0])
        chan = np.where(below | above | ~np.isfinite(line), -1, chan)
    idx = chan[:, None] + offsets[None, :]                                               # (nsrc, 2K + 1)
    ok = (chan[:, None] >= 0) & (idx >= 0) & (idx < nf)
    idc = np.where(ok, idx, 0)
    wt = np.where(ok, w[:, None] * om[idc], 0.0)                                         # (nsrc, 2K + 1)
    vals = np.take_along_axis(T, np.broadcast_to(idc[:, None, :], (nsrc, npol, offsets.size)), axis=2) if nsrc else \
        np.zeros((0, npol, offsets.size))
    num = np.einsum("sk,spk->pk", wt, np.where(wt[:, None, :] > 0.0, vals, 0.0))
    den = wt.sum(axis=0)
    stack = np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)
    return dict(stack=stack, hits=np.count_nonzero(wt > 0.0, axis=0).astype(np.int64), weight=den, offsets=offsets,
                channel=chan.astype(np.int64))
