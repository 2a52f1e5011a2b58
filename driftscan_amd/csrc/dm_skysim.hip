// dm_skysim.hip — Gaussian sky realisations from the model covariances C_l(nu, nu'): a[r, i, l, m] = sum_j T_l[i, j] z_j
// with T_l the symmetric square root of C_l and z the unit draws of (component j, l, m, realisation r).
//
// Draws: Philox4x32-10 keyed by the 64-bit seed, counter (j_global, (l << 16) | m, r, stream); one block of the
// generator is one complex draw (dm_philox.h), so a draw is a fixed function of (seed, stream, r, j_global, l, m)
// whatever rows, m cut, realisation range or grouping a call asks for.  The draws never exist in memory: a workgroup
// generates those of its (l, chunk of m, realisation) into LDS once and multiplies the rows of T_l into them on
// v_mfma_f64_16x16x4_f64.  Every output element is one accumulator walked through k = 0, 4, 8, ... < n: the summation
// order is set by n alone and two calls give the same bits.
#include "dm_common.h"
#include "dm_philox.h"
#include "../../include/driftmi.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int SD_RG = 64;   // rows of T_l per row group: four 16-row MFMA tiles
constexpr int SD_NMAX = 1024;
constexpr size_t SD_LDS_MAX = 160 * 1024;

struct sky_args {
  const double* T;      // (L, n, n): row stride ld, strideT between multipoles
  const int* jglobal;   // (n) counter word 0 of each component of the group: pol * nfreq + freq
  const int64_t* rowoff;  // (n) offset of each component in out, complex elements
  double* out;
  int64_t strideT, sr, sl, sm;   // out strides of (realisation, l, m), complex elements
  int n, ld, L, M, nfreq, row0, nrows, first;
  uint32_t k0, k1, stream;
};

// row stride of the draws in LDS: the two k rows of a 32-lane ds_read_b64 group fall 32 banks apart
__host__ __device__ constexpr int sd_zs(int C) { return (C % 32 == 16) ? C : C + 16; }

// One workgroup: multipole l = blockIdx.x, real columns [C * blockIdx.y, + C) (complex m in pairs), realisation
// first + blockIdx.z.  CT = C / 16 column sub-tiles; KC columns of T_l are staged per pass.
//   CT = 4: wave w owns column sub-tile w and the four row tiles of a group;  CT = 1: wave w owns row tile w.
template <int CT, int KC>
__global__ __launch_bounds__(256) void sky_draw_kernel(const sky_args a) {
  extern __shared__ __align__(16) unsigned char sd_smem[];
  constexpr int C = 16 * CT, ZS = sd_zs(C), TS = KC + 2, NA = CT == 4 ? 4 : 1;
  const int n = a.n, Kp = (n + 3) & ~3;
  double* zl = reinterpret_cast<double*>(sd_smem);   // Kp x ZS: z[j][real column]
  double* tile = zl + (size_t)Kp * ZS;               // SD_RG x TS
  const int l = blockIdx.x, r = blockIdx.z;
  const int m0 = blockIdx.y * (C / 2);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kq = lane >> 4, cj = lane & 15;
  const int mend = min(a.M, l + 1);                  // coefficients m >= mend of this l are zero
  double* outr = a.out + 2 * ((size_t)r * a.sr + (size_t)l * a.sl);

  if (m0 >= mend) {   // nothing drawn here: the zeros of m > l
    for (int e = threadIdx.x; e < a.nrows * (C / 2); e += 256) {
      const int i = e / (C / 2), m = m0 + e - i * (C / 2);
      if (m < a.M) dm_stg(reinterpret_cast<cplx*>(outr), (size_t)(a.rowoff[a.row0 + i] + (int64_t)m * a.sm), make_double2(0.0, 0.0));
    }
    return;
  }

  // the draws of every component of the group for this chunk of m
  for (int e = threadIdx.x; e < Kp * (C / 2); e += 256) {
    const int j = e / (C / 2), mc = e - j * (C / 2), m = m0 + mc;
    cplx z = make_double2(0.0, 0.0);
    if (j < n && m < mend) {
      uint32_t c[4] = {(uint32_t)a.jglobal[j], ((uint32_t)l << 16) | (uint32_t)m, (uint32_t)a.first + (uint32_t)r, a.stream};
      philox4x32_10(c, a.k0, a.k1);
      z = philox_normal(c, 1.0);
      if (m == 0) {   // real, E z^2 = 1
        z.x *= 1.4142135623730951;
        z.y = 0.0;
      }
    }
    zl[j * ZS + 2 * mc] = z.x;
    zl[j * ZS + 2 * mc + 1] = z.y;
  }

  const double* Tl = a.T + (size_t)l * a.strideT;
  for (int g0 = 0; g0 < a.nrows; g0 += SD_RG) {
    dm_f64x4 acc[NA];
#pragma unroll
    for (int q = 0; q < NA; ++q) acc[q] = dm_f64x4{0.0, 0.0, 0.0, 0.0};
    for (int kc = 0; kc < Kp; kc += KC) {
      const int kn = min(KC, Kp - kc);
      __syncthreads();   // the draws are written / the last pass has read its tile
      for (int e = threadIdx.x; e < SD_RG * KC; e += 256) {
        const int t = e / KC, kk = e - t * KC, i = g0 + t, k = kc + kk;
        tile[t * TS + kk] = (i < a.nrows && k < n) ? dm_ldg(Tl, (size_t)(a.row0 + i) * a.ld + k) : 0.0;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < NA; ++q) {
        const int rt = CT == 4 ? q : wave, ct = CT == 4 ? wave : 0;
        if (g0 + rt * 16 >= a.nrows) continue;
        const double* ta = tile + (rt * 16 + cj) * TS + kq;
        const double* zb = zl + (size_t)(kc + kq) * ZS + ct * 16 + cj;
        for (int k0 = 0; k0 < kn; k0 += 4) acc[q] = dm_mfma(ta[k0], zb[(size_t)k0 * ZS], acc[q]);
      }
    }
#pragma unroll
    for (int q = 0; q < NA; ++q) {
      const int rt = CT == 4 ? q : wave, ct = CT == 4 ? wave : 0;
      const int col = ct * 16 + cj, m = m0 + (col >> 1);
      if (m >= a.M) continue;
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int i = g0 + rt * 16 + kq + 4 * v;
        if (i >= a.nrows) continue;
        const int pol = a.jglobal[a.row0 + i] / a.nfreq;
        const bool zero = m >= mend || (l < 2 && (pol == 1 || pol == 2));   // E and B start at l = 2
        dm_stg(outr, 2 * (size_t)(a.rowoff[a.row0 + i] + (int64_t)m * a.sm) + (col & 1), zero ? 0.0 : acc[q][v]);
      }
    }
  }
}

template <int CT, int KC>
int sky_launch(dm_ctx* ctx, const sky_args& a, int nreal) {
  constexpr int C = 16 * CT;
  const int Kp = (a.n + 3) & ~3;
  const size_t lds = sizeof(double) * ((size_t)Kp * sd_zs(C) + (size_t)SD_RG * (KC + 2));
  if (lds > SD_LDS_MAX) {
    ctx->err = "dm_sky_draw: the draws of a group of this order do not fit the LDS";
    return DM_EARG;
  }
  const auto kernel = sky_draw_kernel<CT, KC>;
  DM_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)SD_LDS_MAX));
  const unsigned nchunk = (unsigned)((2 * (size_t)a.M + C - 1) / C);
  DM_PLAUNCH(ctx, DM_PROF_UTIL, kernel, dim3((unsigned)a.L, nchunk, (unsigned)nreal), dim3(256), lds, ctx->stream, a);
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

}  // namespace

extern "C" int dm_sky_draw(dm_ctx* ctx, int n, int L, int M, const double* T_dev, int ldT, int64_t strideT,
                           const int* jglobal_host, const int64_t* rowoff_host, int nfreq, int row0, int nrows,
                           uint64_t seed, int stream, int first, int nreal, void* out_dev, int64_t stride_real,
                           int64_t stride_l, int64_t stride_m) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, n >= 1 && L >= 1 && M >= 1 && M <= L && T_dev && jglobal_host && rowoff_host && out_dev && nfreq >= 1);
  if (n > SD_NMAX) {
    ctx->err = "dm_sky_draw: group order n = " + std::to_string(n) + " above the supported " + std::to_string(SD_NMAX);
    return DM_EARG;
  }
  if (L > 65536) {
    ctx->err = "dm_sky_draw: lmax >= 65536 does not fit the (l << 16) | m counter word";
    return DM_EARG;
  }
  DM_ARG(ctx, ldT >= n && strideT >= 0 && row0 >= 0 && nrows >= 0 && row0 + nrows <= n && stream >= 0);
  DM_ARG(ctx, first >= 0 && nreal >= 0 && nreal <= 65535 && (int64_t)first + nreal <= (1LL << 32));
  DM_ARG(ctx, stride_real >= 0 && stride_l >= 0 && stride_m >= 1);
  for (int j = 0; j < n; ++j) DM_ARG(ctx, jglobal_host[j] >= 0 && rowoff_host[j] >= 0);
  if (nrows == 0 || nreal == 0) return DM_OK;
  dm_ws_scope ws_scope__(ctx);
  sky_args a;
  a.T = T_dev;
  a.jglobal = dm_ws_upload(ctx, std::vector<int>(jglobal_host, jglobal_host + n));
  a.rowoff = dm_ws_upload(ctx, std::vector<int64_t>(rowoff_host, rowoff_host + n));
  if (!a.jglobal || !a.rowoff) return DM_ENOMEM;
  a.out = reinterpret_cast<double*>(out_dev);
  a.strideT = strideT; a.sr = stride_real; a.sl = stride_l; a.sm = stride_m;
  a.n = n; a.ld = ldT; a.L = L; a.M = M; a.nfreq = nfreq; a.row0 = row0; a.nrows = nrows; a.first = first;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.stream = (uint32_t)stream;
  // 64 real columns per workgroup while the draws of all n components of a chunk stay within 80 KB, 16 above
  if (n <= 128) DM_TRY((sky_launch<4, 64>(ctx, a, nreal)));
  else DM_TRY((sky_launch<1, 32>(ctx, a, nreal)));
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}
