// dm_points.hip — spherical-harmonic coefficients evaluated at arbitrary points: the synthesis of dm_synth.hip with the
// rings replaced by a catalogue, and the adjoint of dm_sources.hip.  With fac = 1 for m = 0 and 2 otherwise:
//   F^T_m(s) = sum_l a^T_lm lambda_lm(z_s)                                  (F^V alike)
//   F^Q_m(s) = sum_l a^E_lm W_lm(s) + i a^B_lm X_lm(s),    F^U_m(s) = sum_l a^B_lm W_lm(s) - i a^E_lm X_lm(s)
//   value_p(s, f) = sum_m fac_m Re(F^p_m(s) e^{+i m phi_s})
//
// One fused kernel, no Legendre table in memory (pts_eval_kernel): a lane owns a point and a block of PTS_NFB frequencies,
// walks the m of the call in their order and l upwards inside an m, runs the lambda / W / X recurrence of legendre_column
// (dm_sht.h) in registers and accumulates F_m for its frequencies in registers.  What does not depend on the point is
// made once per call by two small kernels and read by the wave through uniform (scalar) loads:
//   pts_coef_kernel  the square roots of the recurrence per (m, l) and the logarithm of the seed's prefactor per m,
//   pts_pack_kernel  the coefficients of a pass of frequency blocks as [block][m][l - m][frequency in block][polarisation],
//                    one contiguous row per step of the l loop.
//
// What fixes the bits: an output element belongs to one lane, which adds l ascending inside m and m in the order of `ms`;
// a frequency sits in block f / PTS_NFB whatever the pass.  Nothing depends on the other points of the call, on how the
// caller cuts points or frequencies (in multiples of the block), or on max_bytes, which only sets how many frequency
// blocks are packed at once.  No atomics.
#include "dm_sht.h"
#include "dm_kernels.h"
#include "../../include/driftmi.h"

#include <cstdint>

#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr int PTS_TPB = 64;   // points per workgroup: one wave, no cooperation between lanes
template <int NPOL> struct pts_nfb { static constexpr int value = NPOL == 4 ? 4 : 8; };   // frequencies per lane

// coef[(moff[j] + l - m) * 4 + {0, 1, 2, 3}] = a_lm, b_lm of the three-term recurrence (a = sqrt(2m + 3), b = 0 at
// l = m + 1) and n_l, c_lm of W and X (0 where l < 2), in the expressions of legendre_column; logpre[j] its seed
// prefactor.  grid (blocks over l - m, nm).
__global__ __launch_bounds__(256) void pts_coef_kernel(const int* __restrict__ ms, const long long* __restrict__ moff, int lmax,
                                                       double* __restrict__ coef, double* __restrict__ logpre) {
  const int j = blockIdx.y;
  const int m = ms[j];
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > lmax - m) return;
  const int l = m + r;
  double a = 0.0, b = 0.0, nl = 0.0, c = 0.0;
  if (r == 1) a = sqrt(2.0 * m + 3.0);
  if (r >= 2) {
    a = sqrt((4.0 * l * l - 1.0) / ((double)l * l - (double)m * m));
    b = sqrt(((l - 1.0) * (l - 1.0) - (double)m * m) / (4.0 * (l - 1.0) * (l - 1.0) - 1.0));
  }
  if (l >= 2) {
    const double dl = l, dm = m;
    nl = 2.0 * sqrt(1.0 / ((dl - 1.0) * dl * (dl + 1.0) * (dl + 2.0)));
    if (r >= 1) c = sqrt((2.0 * dl + 1.0) / (2.0 * dl - 1.0) * (dl * dl - dm * dm));
  }
  double* o = coef + ((size_t)moff[j] + r) * 4;
  o[0] = a; o[1] = b; o[2] = nl; o[3] = c;
  if (r == 0) {
    double lp = 0.5 * (log(2.0 * m + 1.0) - log(4.0 * kPi));
    for (int k = 1; k <= m; ++k) lp += 0.5 * log((2.0 * k - 1.0) / (2.0 * k));
    logpre[j] = lp;
  }
}

// P[((b * rows + moff[j] + l - m) * NFB + fi) * NPOL + p] = alm[f sf + p sp + l sl + j sm], f = (fb0 + b) NFB + fi (0 beyond
// nf).  grid (blocks over (l - m, fi, p), nm, blocks of the pass).
template <int NPOL, int NFB>
__global__ __launch_bounds__(256) void pts_pack_kernel(const cplx* __restrict__ alm, long long sf, long long sp, long long sl,
                                                       long long sm, const int* __restrict__ ms, const long long* __restrict__ moff,
                                                       long long rows, int lmax, int nf, int fb0, cplx* __restrict__ P) {
  const int j = blockIdx.y, b = blockIdx.z;
  const int m = ms[j];
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (lmax + 1 - m) * NFB * NPOL) return;
  const int r = e / (NFB * NPOL), q = e - r * (NFB * NPOL);
  const int fi = q / NPOL, p = q - fi * NPOL;
  const long long f = (long long)(fb0 + b) * NFB + fi;
  cplx v = make_double2(0.0, 0.0);
  if (f < nf) v = dm_ldg(alm, (size_t)(f * sf + p * sp + (long long)(m + r) * sl + (long long)j * sm));
  dm_stg(P, ((size_t)b * rows + moff[j] + r) * (NFB * NPOL) + q, v);
}

// one row of the l loop: the lane's F_m take a_lm times lambda (T, V) and W, X (Q, U); `a` is uniform over the wave
template <int NPOL, int NFB>
__device__ __forceinline__ void pts_row(const double* __restrict__ a, double lam, double W, double X, double (&Fr)[NFB][NPOL],
                                        double (&Fi)[NFB][NPOL]) {
#pragma unroll
  for (int f = 0; f < NFB; ++f) {
    const double* af = a + f * NPOL * 2;
    Fr[f][0] += af[0] * lam;
    Fi[f][0] += af[1] * lam;
    if constexpr (NPOL == 4) {
      const double er = af[2], ei = af[3], br = af[4], bi = af[5];
      Fr[f][1] += er * W - bi * X;   // Q: a^E W + i a^B X
      Fi[f][1] += ei * W + br * X;
      Fr[f][2] += br * W + ei * X;   // U: a^B W - i a^E X
      Fi[f][2] += bi * W - er * X;
      Fr[f][3] += af[6] * lam;
      Fi[f][3] += af[7] * lam;
    }
  }
}

// out[(s * NPOL + p) * nf + f] (+)= value_p(s, f) for the frequencies of block fb0 + blockIdx.y.  The recurrence is that of
// legendre_column with w = 1: the same seed (exp of the summed logarithms, legendre_scaled_seed where that underflows),
// the same steps and the same `ex` rescaling; its square roots come from pts_coef_kernel, and W and X multiply by one
// reciprocal of sin^2 theta per point where the column divides three times per l.  sin theta = 0 is refused by the entry
// point when NPOL = 4; for NPOL = 1 every m > 0 gives zeros there.
template <int NPOL, int NFB>
__global__ __launch_bounds__(PTS_TPB) void pts_eval_kernel(const double* __restrict__ zs, const double* __restrict__ sths,
                                                           const double* __restrict__ phis, int npts, const int* __restrict__ ms,
                                                           const long long* __restrict__ moff, int nm, long long rows, int lmax,
                                                           const double* __restrict__ coef, const double* __restrict__ logpre,
                                                           const double* __restrict__ P, int nf, int fb0, int accumulate,
                                                           double* __restrict__ out) {
  const int s = blockIdx.x * PTS_TPB + threadIdx.x;
  if (s >= npts) return;
  const double z = zs[s], st = sths[s], ph = phis[s];
  const double s2 = st * st;
  const double is2 = 1.0 / s2;       // (used with NPOL = 4 only, where st > 0)
  const double lst = log(st);
  const double* Pb = P + (size_t)blockIdx.y * rows * (NFB * NPOL * 2);
  double acc[NFB][NPOL];
#pragma unroll
  for (int f = 0; f < NFB; ++f)
#pragma unroll
    for (int p = 0; p < NPOL; ++p) acc[f][p] = 0.0;

  for (int j = 0; j < nm; ++j) {
    const int m = ms[j];
    const double* a = Pb + (size_t)moff[j] * (NFB * NPOL * 2);
    const double* cf = coef + (size_t)moff[j] * 4;
    const double dm = m;
    double lmm = (m > 0) ? exp(logpre[j] + dm * lst) : exp(logpre[j]);
    int ex = 0;
    if (m > 0 && lmm < kDblMin) lmm = legendre_scaled_seed(m, s2, &ex);
    if (m & 1) lmm = -lmm;
    double Fr[NFB][NPOL], Fi[NFB][NPOL];
#pragma unroll
    for (int f = 0; f < NFB; ++f)
#pragma unroll
      for (int p = 0; p < NPOL; ++p) Fr[f][p] = Fi[f][p] = 0.0;
    double pm2 = 0.0, pm1 = lmm;
    {
      // l = m (lambda_{m-1,m} = 0)
      const double lm0 = ldexp(lmm, ex);
      double wv = 0.0, xv = 0.0;
      if (NPOL == 4 && m >= 2) {
        const double l = m, nl = cf[2];
        wv = -nl * (-((l - l * l) * is2 + 0.5 * l * (l - 1.0)) * lm0);
        xv = nl * (l * is2) * ((l - 1.0) * z * lm0);
      }
      pts_row<NPOL, NFB>(a, lm0, wv, xv, Fr, Fi);
    }
    const double mis2 = dm * is2;
    for (int l = m + 1; l <= lmax; ++l) {
      a += NFB * NPOL * 2;
      cf += 4;
      double cur;
      if (l == m + 1) cur = cf[0] * z * pm1;
      else cur = cf[0] * (z * pm1 - cf[1] * pm2);
      if (ex < 0 && fabs(cur) > kTwoP512) { cur *= kTwoM512; pm1 *= kTwoM512; ex += 512; }
      double wv = 0.0, xv = 0.0;
      if (NPOL == 4 && l >= 2) {
        const double dl = l, nl = cf[2], c = cf[3];
        wv = -nl * (-((dl - dm * dm) * is2 + 0.5 * dl * (dl - 1.0)) * cur + c * z * is2 * pm1);
        xv = nl * mis2 * ((dl - 1.0) * z * cur - c * pm1);
      }
      if (NPOL == 4) pts_row<NPOL, NFB>(a, ldexp(cur, ex), ldexp(wv, ex), ldexp(xv, ex), Fr, Fi);
      else pts_row<NPOL, NFB>(a, ldexp(cur, ex), 0.0, 0.0, Fr, Fi);
      pm2 = pm1;
      pm1 = cur;
    }
    double sn, cs;
    sincos(dm * ph, &sn, &cs);
    const double fac = m == 0 ? 1.0 : 2.0;
#pragma unroll
    for (int f = 0; f < NFB; ++f)
#pragma unroll
      for (int p = 0; p < NPOL; ++p) acc[f][p] += fac * (Fr[f][p] * cs - Fi[f][p] * sn);
  }

  const long long f0 = (long long)(fb0 + (int)blockIdx.y) * NFB;
#pragma unroll
  for (int p = 0; p < NPOL; ++p)
#pragma unroll
    for (int f = 0; f < NFB; ++f)
      if (f0 + f < nf) {
        const size_t o = ((size_t)s * NPOL + p) * nf + (size_t)(f0 + f);
        out[o] = accumulate ? out[o] + acc[f][p] : acc[f][p];
      }
}

template <int NPOL>
int pts_run(dm_ctx* ctx, int npts, const double* z, const double* sth, const double* phi, int nm, const int* ms_host, int lmax, int nf,
            const cplx* alm, long long sf, long long sp, long long sl, long long sm, double* out, int accumulate, size_t max_bytes) {
  constexpr int NFB = pts_nfb<NPOL>::value;
  dm_ws_scope ws_scope__(ctx);
  std::vector<int> ms(ms_host, ms_host + nm);
  std::vector<long long> moff(nm);
  long long rows = 0;
  for (int j = 0; j < nm; ++j) { moff[j] = rows; rows += lmax + 1 - ms[j]; }
  const int nfb = (nf + NFB - 1) / NFB;
  const size_t blk_bytes = (size_t)rows * NFB * NPOL * sizeof(cplx);
  const int per_pass = (int)std::max<size_t>(1, std::min<size_t>({(size_t)nfb, (size_t)65535, max_bytes / std::max<size_t>(blk_bytes, 1)}));
  int* d_ms = dm_ws_upload(ctx, ms);
  long long* d_moff = dm_ws_upload(ctx, moff);
  double* coef = dm_ws_alloc_t<double>(ctx, (size_t)rows * 4);
  double* logpre = dm_ws_alloc_t<double>(ctx, (size_t)nm);
  cplx* P = dm_ws_alloc_t<cplx>(ctx, (size_t)per_pass * rows * NFB * NPOL);
  if (!d_ms || !d_moff || !coef || !logpre || !P) return DM_ENOMEM;
  const int lrows = lmax + 1 - *std::min_element(ms.begin(), ms.end());   // the longest column
  DM_PLAUNCH(ctx, DM_PROF_BT_OTHER, pts_coef_kernel, dim3((unsigned)((lrows + 255) / 256), (unsigned)nm), dim3(256), 0, ctx->stream, d_ms,
             d_moff, lmax, coef, logpre);
  DM_HIP(ctx, hipGetLastError());
  for (int fb0 = 0; fb0 < nfb; fb0 += per_pass) {
    const int nb = std::min(per_pass, nfb - fb0);
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (pts_pack_kernel<NPOL, NFB>), dim3((unsigned)((lrows * NFB * NPOL + 255) / 256), (unsigned)nm, (unsigned)nb),
               dim3(256), 0, ctx->stream, alm, sf, sp, sl, sm, d_ms, d_moff, rows, lmax, nf, fb0, P);
    DM_PLAUNCH(ctx, DM_PROF_BT_OTHER, (pts_eval_kernel<NPOL, NFB>), dim3((unsigned)((npts + PTS_TPB - 1) / PTS_TPB), (unsigned)nb),
               dim3(PTS_TPB), 0, ctx->stream, z, sth, phi, npts, d_ms, d_moff, nm, rows, lmax, coef, logpre,
               reinterpret_cast<const double*>(P), nf, fb0, accumulate, out);
    DM_HIP(ctx, hipGetLastError());
  }
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}

}  // namespace

extern "C" int dm_alm_at_points(dm_ctx* ctx, int npts, const double* z_dev, const double* sth_dev, const double* phi_dev, int nm,
                                const int* ms_host, int lmax, int nf, int npol, const void* alm_dev, int64_t stride_f,
                                int64_t stride_p, int64_t stride_l, int64_t stride_m, double* out_dev, int accumulate,
                                size_t max_bytes) {
  if (!ctx) return DM_EARG;
  if (npol != 1 && npol != 4) {
    ctx->err = "dm_alm_at_points: npol = " + std::to_string(npol) + ", 1 (T) or 4 (T, E, B, V) expected";
    return DM_EARG;
  }
  if (npts <= 0 || nf <= 0) {
    ctx->err = "dm_alm_at_points: npts = " + std::to_string(npts) + " and nf = " + std::to_string(nf) + ", one point and one frequency at least expected";
    return DM_EARG;
  }
  DM_ARG(ctx, lmax >= 0 && lmax < 65535 && nm >= 0 && (nm == 0 || ms_host) && z_dev && sth_dev && phi_dev && out_dev);
  DM_ARG(ctx, nm == 0 || alm_dev);
  DM_ARG(ctx, stride_f >= 0 && stride_p >= 0 && stride_l >= 0 && stride_m >= 0);
  DM_ARG(ctx, (size_t)npts * npol <= (size_t)INT64_MAX / sizeof(double) / (size_t)nf);
  {
    std::vector<char> seen((size_t)lmax + 1, 0);
    for (int j = 0; j < nm; ++j) {
      const int m = ms_host[j];
      if (m < 0 || m > lmax) {
        ctx->err = "dm_alm_at_points: ms[" + std::to_string(j) + "] = " + std::to_string(m) + " outside 0 .. lmax = " + std::to_string(lmax);
        return DM_EARG;
      }
      if (seen[m]) {
        ctx->err = "dm_alm_at_points: m = " + std::to_string(m) + " is repeated in ms";
        return DM_EARG;
      }
      seen[m] = 1;
    }
  }
  if (npol == 4) {
    // Q and U have no meaning at a pole, and W and X divide by sin^2 theta
    std::vector<double> sth(npts);
    DM_TRY(dm_download(ctx, sth.data(), sth_dev, sizeof(double) * (size_t)npts));
    for (int s = 0; s < npts; ++s)
      if (!(sth[s] > 0.0)) {
        ctx->err = "dm_alm_at_points: point " + std::to_string(s) + " lies at a pole (sin theta = 0): Q and U are undefined there";
        return DM_EARG;
      }
  }
  if (nm == 0) {
    if (!accumulate) DM_TRY(dm_fill_zero(ctx, out_dev, sizeof(double) * (size_t)npts * npol * nf));
    DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DM_OK;
  }
  const cplx* alm = reinterpret_cast<const cplx*>(alm_dev);
  if (npol == 4)
    return pts_run<4>(ctx, npts, z_dev, sth_dev, phi_dev, nm, ms_host, lmax, nf, alm, stride_f, stride_p, stride_l, stride_m, out_dev,
                      accumulate, max_bytes);
  return pts_run<1>(ctx, npts, z_dev, sth_dev, phi_dev, nm, ms_host, lmax, nf, alm, stride_f, stride_p, stride_l, stride_m, out_dev,
                    accumulate, max_bytes);
}
