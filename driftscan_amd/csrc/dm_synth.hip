// dm_synth.hip — spherical-harmonic synthesis of real HEALPix maps on the GPU (gfx950).
//
// Replaces: cora.util.hputil.sphtrans_inv_sky as called by the map-makers (drift/pipeline/timestream.py:262, :295, :451).
//
// For every column c = (f, p) and m < Mm = min(M, lmax + 1):
//   1. Legendre   F[c][r][m] = sum_l a[f, p, l, m] lambda_lm(z_r)   (T, V);  F_Q = W a_E + i X a_B,  F_U = W a_B - i X a_E
//                 real x complex grouped GEMMs per (m, Stokes term) against the bt_legendre_kernel tables (MFMA), the
//                 coefficients read in the caller's (f, P, L, M) layout through their strides
//   2. ring       map[c][start_r + j] = sum_m c_m Re(F[c][r][m] exp(i m phi_rj)),  c_0 = 1, c_m = 2
//                 m is folded onto the bin k = m mod nphi_r with the phase c_m exp(i m phi0_r) (phi0_r = 0 or pi / nphi_r:
//                 the argument is reduced exactly), then an inverse DFT of length nphi_r keeps the real part:
//                 belt rings (nphi = 4 nside, a power of two) by the LDS FFT of BT-gen, one workgroup per ring walking
//                 over columns; cap rings (and a belt the FFT does not take) by a direct sum over min(nphi, Mm) bins
//                 against an LDS twiddle table.  Both write float64 pixels coalesced along the ring.
// F is bounded by working through the columns in chunks (kSynthChunkBytes); the tables are built once per call.
#include "dm_common.h"
#include "dm_kernels.h"
#include "dm_sht.h"
#include "../../include/driftmi.h"

#include <algorithm>

namespace {

constexpr size_t kSynthChunkBytes = size_t(1) << 30;   // F of one chunk of columns
constexpr int SY_NC = 4;     // columns per workgroup of the direct ring sum
constexpr int SY_JPT = 2;    // pixels per thread and pass of the direct ring sum
constexpr int SY_KT = 256;   // bins per LDS tile of the direct ring sum
constexpr int SY_NMAX = 8192;  // longest ring of the direct sum: its twiddle table (128 KB) and one bin tile fit the LDS

// B_k = sum over m = k, k + N, ... < Mm of c_m exp(i m phi0) F[m], with phi0 = s pi / N (s = 0 or 1):
// m phi0 = pi ((s m) mod 2N) / N, so sincospi sees an exact argument in [0, 2)
__device__ __forceinline__ cplx synth_bin(const cplx* __restrict__ Fr, int Mm, int N, int s, int k) {
  cplx acc = make_double2(0.0, 0.0);
  for (int m = k; m < Mm; m += N) {
    const cplx f = dm_ldg(Fr, m);
    double sn = 0.0, cs = 1.0;
    if (s) sincospi((double)(m % (2 * N)) / (double)N, &sn, &cs);
    const double c = m == 0 ? 1.0 : 2.0;
    acc.x += c * (f.x * cs - f.y * sn);
    acc.y += c * (f.x * sn + f.y * cs);
  }
  return acc;
}

__device__ __forceinline__ int synth_shift(const ring_geo& g, int r) { return g.phi0[r] != 0.0 ? 1 : 0; }

// Belt rings ring0 .. ring0 + gridDim.y - 1 (N = 4 nside = 2^logn, 8 <= N <= 4096): one workgroup per ring and `cpw`
// columns.  LDS: N + N / 2 complex values, padded as in bt_fused_fft_kernel (48 KB at nside 512).
__global__ __launch_bounds__(256) void sht_synth_fft_kernel(ring_geo g, const cplx* __restrict__ F, int Mm, int ncp,
                                                            int ring0, int cpw, double* __restrict__ maps) {
  constexpr int TPB = 256;
  extern __shared__ __align__(16) unsigned char synth_smem[];
  const int tid = threadIdx.x;
  const int r = ring0 + blockIdx.y;
  const int N = g.nphi[r];
  const int logn = 31 - __clz(N);
  const int sh = max(5, logn - 6);
  auto ph = [&](int a2) { return a2 + (a2 >> sh); };
  const int Np = N + (N >> sh) + 1;
  cplx* X = reinterpret_cast<cplx*>(synth_smem);   // [Np]
  cplx* TW = X + Np;                                  // [N / 2] (padded likewise): exp(+2 pi i k / N)
  for (int k = tid; k < N / 2; k += TPB) {
    double s_, c_;
    sincospi(2.0 * (double)k / (double)N, &s_, &c_);
    TW[ph(k)] = make_double2(c_, s_);
  }
  const int s = synth_shift(g, r);
  const int pix0 = g.start[r];
  const int c_lo = blockIdx.x * cpw, c_hi = min(c_lo + cpw, ncp);
  for (int col = c_lo; col < c_hi; ++col) {
    __syncthreads();   // the previous column's pixels have been read; the twiddles are there
    const cplx* Fr = F + ((size_t)col * g.nring + r) * Mm;
    for (int k = tid; k < N; k += TPB) X[ph((int)(__brev((unsigned)k) >> (32 - logn)))] = synth_bin(Fr, Mm, N, s, k);
    __syncthreads();
    sht_lds_fft<1, TPB>(X, TW, N, logn, sh, Np, tid);
    double* out = maps + (size_t)col * g.npix + pix0;
    for (int j = tid; j < N; j += TPB) out[j] = X[ph(j)].x;
  }
}

// The other rings (list `rings`): one workgroup per (ring, SY_NC columns), a direct sum over the K = min(N, Mm) bins,
// SY_KT of them at a time in LDS next to the N twiddles exp(2 pi i t / N).  A thread owns SY_JPT pixels j per pass and
// walks t = j k mod N by adding j.  LDS: 16 (N + SY_NC SY_KT) bytes.
__global__ __launch_bounds__(256) void sht_synth_dft_kernel(ring_geo g, const cplx* __restrict__ F, int Mm, int ncp,
                                                            const int* __restrict__ rings, double* __restrict__ maps) {
  constexpr int TPB = 256;
  extern __shared__ __align__(16) unsigned char synth_smem[];
  const int tid = threadIdx.x;
  const int r = rings[blockIdx.y];
  const int N = g.nphi[r];
  const int K = min(N, Mm);
  cplx* TW = reinterpret_cast<cplx*>(synth_smem);   // [N]
  cplx* Bs = TW + N;                                   // [SY_NC][SY_KT]
  for (int t = tid; t < N; t += TPB) {
    double s_, c_;
    sincospi(2.0 * (double)t / (double)N, &s_, &c_);
    TW[t] = make_double2(c_, s_);
  }
  const int s = synth_shift(g, r);
  const int c0 = blockIdx.x * SY_NC, nc = min(SY_NC, ncp - c0);
  const size_t pix0 = (size_t)g.start[r];
  for (int j0 = 0; j0 < N; j0 += TPB * SY_JPT) {
    double acc[SY_JPT][SY_NC];
    int jj[SY_JPT];
#pragma unroll
    for (int q = 0; q < SY_JPT; ++q) {
      const int j = j0 + tid + TPB * q;
      jj[q] = j < N ? j : 0;
#pragma unroll
      for (int c = 0; c < SY_NC; ++c) acc[q][c] = 0.0;
    }
    for (int k0 = 0; k0 < K; k0 += SY_KT) {
      __syncthreads();   // twiddles written / the previous tile has been read
      for (int t = tid; t < SY_NC * SY_KT; t += TPB) {
        const int c = t / SY_KT, k = k0 + (t - c * SY_KT);
        Bs[t] = (c < nc && k < K) ? synth_bin(F + ((size_t)(c0 + c) * g.nring + r) * Mm, Mm, N, s, k) : make_double2(0.0, 0.0);
      }
      __syncthreads();
      int idx[SY_JPT];
#pragma unroll
      for (int q = 0; q < SY_JPT; ++q) idx[q] = (int)(((long long)jj[q] * k0) % N);
      const int kend = min(SY_KT, K - k0);
      for (int kk = 0; kk < kend; ++kk) {
        cplx b[SY_NC];
#pragma unroll
        for (int c = 0; c < SY_NC; ++c) b[c] = Bs[c * SY_KT + kk];
#pragma unroll
        for (int q = 0; q < SY_JPT; ++q) {
          const cplx w = TW[idx[q]];
#pragma unroll
          for (int c = 0; c < SY_NC; ++c) acc[q][c] = fma(b[c].x, w.x, fma(-b[c].y, w.y, acc[q][c]));
          idx[q] += jj[q];
          if (idx[q] >= N) idx[q] -= N;
        }
      }
    }
#pragma unroll
    for (int q = 0; q < SY_JPT; ++q) {
      const int j = j0 + tid + TPB * q;
      if (j >= N) continue;
#pragma unroll
      for (int c = 0; c < SY_NC; ++c)
        if (c < nc) maps[(size_t)(c0 + c) * g.npix + pix0 + j] = acc[q][c];
    }
  }
}

}  // namespace

extern "C" {

int dm_sht_synth(dm_ctx* ctx, int nside, const double* ring_cth_host, const double* ring_sth_host, int polarised, int lmax,
                 int M, int ncol, const void* alm_dev, void* maps_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nside > 0 && 4 * nside <= SY_NMAX && ring_cth_host && ring_sth_host && lmax >= 0 && M > 0 && ncol >= 0 &&
                  alm_dev && maps_dev);
  if (ncol == 0) return DM_OK;
  dm_ws_scope ws_scope__(ctx);  // releases on every return path
  geo_host gh;
  DM_TRY(upload_geo(ctx, nside, ring_cth_host, ring_sth_host, gh));
  const int P = polarised ? 4 : 1;
  const int L = lmax + 1;
  const int Mm = std::min(M, L);   // m >= lmax + 1 carries no (l, m)
  const int nring = gh.g.nring, npix = gh.g.npix;
  DM_ARG(ctx, Mm <= 65535 && (size_t)P * L * M <= (size_t)INT32_MAX && (size_t)P * nring * Mm <= (size_t)INT32_MAX);

  // ---- Legendre tables (unweighted) for m < Mm, l = m .. lmax
  std::vector<size_t> loff(Mm);
  size_t ltot = 0;
  for (int m = 0; m < Mm; ++m) { loff[m] = ltot; ltot += (size_t)(L - m) * nring; }
  size_t* d_loff = dm_ws_upload(ctx, loff);
  double* lam = dm_ws_alloc_t<double>(ctx, ltot);
  double* Wt = polarised ? dm_ws_alloc_t<double>(ctx, ltot) : nullptr;
  double* Xt = polarised ? dm_ws_alloc_t<double>(ctx, ltot) : nullptr;
  if (!d_loff || !lam || (polarised && (!Wt || !Xt))) return DM_ENOMEM;
  DM_PLAUNCH(ctx, DM_PROF_BT_OTHER, bt_legendre_kernel, dim3((nring + 63) / 64, Mm), dim3(64), 0, ctx->stream, gh.g, lmax, 0,
             Mm - 1, 1.0, d_loff, lam, Wt, Xt);

  // ---- ring plan: the belt by LDS FFT where N = 4 nside is a power of two in [8, 4096], every other ring by the direct sum
  const int N = 4 * nside;
  int logn = 0;
  while ((1 << logn) < N) ++logn;
  const bool use_fft = nside >= 2 && (N & (N - 1)) == 0 && N <= 4096;
  const int sh = std::max(5, logn - 6);
  const size_t fft_lds = sizeof(cplx) * ((size_t)(N + (N >> sh) + 1) + (N / 2 + ((N / 2) >> sh) + 1));
  std::vector<int> dft_rings;
  int nmax_dft = 0;
  for (int r = 0; r < nring; ++r)
    if (!use_fft || r < nside - 1 || r > 3 * nside - 1) { dft_rings.push_back(r); nmax_dft = std::max(nmax_dft, gh.nphi[r]); }
  int* d_rings = dft_rings.empty() ? nullptr : dm_ws_upload(ctx, dft_rings);
  if (!dft_rings.empty() && !d_rings) return DM_ENOMEM;
  const size_t dft_lds = sizeof(cplx) * ((size_t)nmax_dft + SY_NC * SY_KT);
  if (use_fft)
    DM_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sht_synth_fft_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)fft_lds));
  if (!dft_rings.empty())
    DM_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(sht_synth_dft_kernel),
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)dft_lds));

  // ---- column chunks: F[fl][p][r][m] for nf frequencies at a time
  const size_t per_f = (size_t)P * nring * Mm * sizeof(cplx);
  const int nf_max = (int)std::max<size_t>(1, std::min<size_t>((size_t)ncol, kSynthChunkBytes / per_f));
  cplx* F = dm_ws_alloc_t<cplx>(ctx, (size_t)nf_max * P * nring * Mm);
  if (!F) return DM_ENOMEM;
  const cplx* alm = reinterpret_cast<const cplx*>(alm_dev);
  double* maps = reinterpret_cast<double*>(maps_dev);
  for (int f0 = 0; f0 < ncol; f0 += nf_max) {
    const int nf = std::min(nf_max, ncol - f0);
    const int ncp = nf * P;
    // Legendre products; the second pass accumulates the X terms of Q and U onto the W terms of the first
    for (int pass = 0; pass < (polarised ? 2 : 1); ++pass) {
      std::vector<dm_gemm_desc> g;
      for (int m = 0; m < Mm; ++m) {
        auto add = [&](const double* tab, int pin, int pout, double are, double aim, double beta) {
          dm_gemm_desc d = dm_gemm_make(alm + (((size_t)f0 * P + pin) * L + m) * M + m, P * L * M, M, false, tab + loff[m],
                                        nring, 1, false, F + (size_t)pout * nring * Mm + m, P * nring * Mm, nf, nring, L - m,
                                        are, beta, nullptr, DM_GEMM_B_REAL);
          d.alpha_im = aim;
          d.csc = Mm;
          g.push_back(d);
        };
        if (pass == 0) {
          add(lam, 0, 0, 1.0, 0.0, 0.0);
          if (polarised) {
            add(Wt, 1, 1, 1.0, 0.0, 0.0);   // Q <- W a_E
            add(Wt, 2, 2, 1.0, 0.0, 0.0);   // U <- W a_B
            add(lam, 3, 3, 1.0, 0.0, 0.0);
          }
        } else {
          add(Xt, 2, 1, 0.0, 1.0, 1.0);    // Q += i X a_B
          add(Xt, 1, 2, 0.0, -1.0, 1.0);   // U -= i X a_E
        }
      }
      DM_TRY(dm_gemm_grouped_launch(ctx, g));
    }
    double* mp = maps + (size_t)f0 * P * npix;
    if (use_fft) {
      const int nbelt = 2 * nside + 1;
      const int cpw = std::max(1, std::min(16, (int)(((size_t)ncp * nbelt) / 4096)));
      DM_PLAUNCH(ctx, DM_PROF_BT_RING, sht_synth_fft_kernel, dim3((unsigned)((ncp + cpw - 1) / cpw), (unsigned)nbelt), dim3(256),
                 fft_lds, ctx->stream, gh.g, F, Mm, ncp, nside - 1, cpw, mp);
    }
    if (!dft_rings.empty())
      DM_PLAUNCH(ctx, DM_PROF_BT_RING, sht_synth_dft_kernel, dim3((unsigned)((ncp + SY_NC - 1) / SY_NC), (unsigned)dft_rings.size()),
                 dim3(256), dft_lds, ctx->stream, gh.g, F, Mm, ncp, d_rings, mp);
    DM_HIP(ctx, hipGetLastError());
  }
  return DM_OK;
}

}  // extern "C"
