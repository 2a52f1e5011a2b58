// dm_band.hip — what the band-power estimators share: the projection of KL-basis columns onto the sky and the products
// of the band tables C_a[l] (F x F, real) with the projected columns.
//
// dm_qestimate (dm_qest.hip) folds Z = C_a x2 into y2^H Z, dm_psmc_alt (dm_psmc.hip) stores Z for the back-projection:
// one kernel with two endings.  Every reduction is a fixed-order sum (no atomics).
#include "dm_common.h"
#include "dm_kernels.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int BP_NJ = 4;                  // 16-column MFMA sub-tiles per wave
constexpr int BP_COLS = 4 * 16 * BP_NJ;   // real columns (re / im of a complex column) per workgroup: 256
constexpr int BP_TILE = 4096;             // doubles of the staged table tile (32 KB of LDS)

// (nbands, F*F, L) -> (nbands, L, F*F)
__global__ __launch_bounds__(256) void band_table_transpose_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                                   int FF, int L) {
  __shared__ double t[32][33];
  const size_t band = blockIdx.z;
  const double* src = in + band * (size_t)FF * L;
  double* dst = out + band * (size_t)FF * L;
  const int l0 = blockIdx.x * 32, p0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;   // 32 x 8
  for (int r = ty; r < 32; r += 8) {
    const int p = p0 + r, l = l0 + tx;
    t[r][tx] = (p < FF && l < L) ? src[(size_t)p * L + l] : 0.0;
  }
  __syncthreads();
  for (int r = ty; r < 32; r += 8) {
    const int l = l0 + r, p = p0 + tx;
    if (l < L && p < FF) dst[(size_t)l * FF + p] = t[tx][r];
  }
}

// Z[l, :, n] = C_a[l] X[l, :, n] for every band a and the complex columns n = b R + r of the batch (X laid out
// (nblk, L, F, R) c128), for l >= l0_b.  The complex columns are 2N real columns; Z is an F x F by F x 2N real product on
// v_mfma_f64_16x16x4_f64:
//   A = rows i0..i0+15 of the staged tile (LDS), B = 16 real columns of X, D = Z[i0 + (lane >> 4) + 4 r][col].
// A workgroup owns 256 real columns and a chunk of DM_BAND_LC multipoles and walks every band; the tile of (a, l) is
// staged into LDS once per workgroup in row chunks of at most BP_TILE doubles.  What a lane does with its D values:
//   FOLD:  out[(a * nlc + lc) * N + n] = Re sum_{l in chunk lc, l >= l0_b} sum_f conj(Y[l, f, n]) Z[l, f, n]  (Y laid out as
//          X): Z never leaves the registers.  The sums over the four row groups and over re / im are fixed cross-lane
//          additions; the chunks of l are left to the caller.
//   !FOLD: out[b][a][l][f][n] = Z[l, f, n], 0 for l < l0_b  ((nblk, nbands, L, F, R) c128: each band's slice is laid out
//          as X, so the back-projection reads it without a transpose).
template <bool FOLD>
__global__ __launch_bounds__(256) void band_product_kernel(const double* __restrict__ X, const double* __restrict__ Y,
                                                          const double* __restrict__ tab, const int* __restrict__ l0b,
                                                          double* __restrict__ out, int F, int L, int R, int N,
                                                          int nbands, int nlc) {
  __shared__ double tile[BP_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = blockIdx.y;
  const int lbeg = lc * DM_BAND_LC, lend = min(L, lbeg + DM_BAND_LC);
  const int Fk = (F + 3) & ~3;                                        // contraction length padded to the MFMA's K = 4
  const int FR = max(16, min((F + 15) & ~15, (BP_TILE / Fk) & ~15));  // rows per staged chunk, a multiple of 16
  const int kq = lane >> 4, cj = lane & 15;
  const size_t fstride = 2 * (size_t)R;           // doubles between (l, f) and (l, f + 1)
  const size_t lstride = (size_t)F * fstride;     // doubles between l and l + 1
  const size_t bandstride = (size_t)L * lstride;  // doubles between the blocks of X (the bands of one block in Z)
  // this lane's real column in each sub-tile: offset of its (b, l = 0, f = 0) element in doubles, and its first l
  size_t xbase[BP_NJ], zbase[BP_NJ];
  int lfirst[BP_NJ];
  bool valid[BP_NJ];
#pragma unroll
  for (int j = 0; j < BP_NJ; ++j) {
    const int c = blockIdx.x * BP_COLS + wave * 16 * BP_NJ + j * 16 + cj;   // real column
    valid[j] = c < 2 * N;
    const int n = valid[j] ? c >> 1 : 0, b = n / R, r = n - b * R;
    const size_t col = 2 * (size_t)r + (c & 1);
    xbase[j] = (size_t)b * bandstride + col;
    zbase[j] = (size_t)b * nbands * bandstride + col;   // !FOLD only
    lfirst[j] = valid[j] ? l0b[b] : L;                  // L: masked
  }
  for (int a = 0; a < nbands; ++a) {
    double acc[BP_NJ];
#pragma unroll
    for (int j = 0; j < BP_NJ; ++j) acc[j] = 0.0;
    for (int l = lbeg; l < lend; ++l) {
      const double* T = tab + ((size_t)a * L + l) * F * F;
      for (int r0 = 0; r0 < F; r0 += FR) {
        const int nr = min(FR, F - r0);
        __syncthreads();
        for (int e = threadIdx.x; e < FR * Fk; e += 256) {
          const int i = e / Fk, k = e - i * Fk;
          tile[e] = (i < nr && k < F) ? T[(size_t)(r0 + i) * F + k] : 0.0;
        }
        __syncthreads();
        for (int i0 = 0; i0 < nr; i0 += 16) {
#pragma unroll
          for (int j = 0; j < BP_NJ; ++j) {
            const bool on = l >= lfirst[j];
            const double* xc = X + xbase[j] + (size_t)l * lstride;
            dm_f64x4 z = {0.0, 0.0, 0.0, 0.0};
            for (int k0 = 0; k0 < Fk; k0 += 4) {
              const int k = k0 + kq;
              const double av = tile[(i0 + cj) * Fk + k];
              const double bv = (on && k < F) ? xc[(size_t)k * fstride] : 0.0;
              z = dm_mfma(av, bv, z);
            }
            if constexpr (FOLD) {
              if (on) {
                const double* yc = Y + xbase[j] + (size_t)l * lstride;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                  const int f = r0 + i0 + kq + 4 * q;
                  if (f < r0 + nr) acc[j] += yc[(size_t)f * fstride] * z[q];
                }
              }
            } else if (valid[j]) {
              double* zc = out + zbase[j] + (size_t)a * bandstride + (size_t)l * lstride;
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                const int f = r0 + i0 + kq + 4 * q;
                if (f < r0 + nr) zc[(size_t)f * fstride] = on ? z[q] : 0.0;
              }
            }
          }
        }
      }
    }
    if constexpr (FOLD) {
      // sum over the four row groups (lanes 16 apart), then re + im (neighbouring lanes): fixed order
#pragma unroll
      for (int j = 0; j < BP_NJ; ++j) {
        double v = acc[j];
        v += __shfl_xor(v, 16);
        v += __shfl_xor(v, 32);
        v += __shfl_xor(v, 1);
        const int c = blockIdx.x * BP_COLS + wave * 16 * BP_NJ + j * 16 + cj;
        if (lane < 16 && (cj & 1) == 0 && valid[j]) out[((size_t)a * nlc + lc) * N + (c >> 1)] = v;
      }
    }
  }
}

template <bool FOLD>
void band_product_launch(dm_ctx* ctx, const cplx* x2, const cplx* y2, const double* tab, const int* l0_dev, double* out,
                         int F, int L, int R, int N, int nbands) {
  const int nlc = (L + DM_BAND_LC - 1) / DM_BAND_LC;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, band_product_kernel<FOLD>, dim3((unsigned)((2 * (size_t)N + BP_COLS - 1) / BP_COLS), nlc),
             dim3(256), 0, ctx->stream, reinterpret_cast<const double*>(x2), reinterpret_cast<const double*>(y2), tab,
             l0_dev, out, F, L, R, N, nbands, nlc);
}

}  // namespace

void dm_band_tables(dm_ctx* ctx, const double* cl_bands, double* tab, int nbands, int F, int L) {
  const int FF = F * F;
  DM_PLAUNCH(ctx, DM_PROF_UTIL, band_table_transpose_kernel, dim3((L + 31) / 32, (FF + 31) / 32, nbands), dim3(256), 0,
             ctx->stream, cl_bands, tab, FF, L);
}

void dm_band_qform(dm_ctx* ctx, const cplx* x2, const cplx* y2, const double* tab, const int* l0_dev, double* part, int F,
                   int L, int R, int N, int nbands) {
  band_product_launch<true>(ctx, x2, y2, tab, l0_dev, part, F, L, R, N, nbands);
}

void dm_band_apply(dm_ctx* ctx, const cplx* x2, const double* tab, const int* l0_dev, cplx* z, int F, int L, int R, int N,
                   int nbands) {
  band_product_launch<false>(ctx, x2, nullptr, tab, l0_dev, reinterpret_cast<double*>(z), F, L, R, N, nbands);
}

int dm_band_proj::init(dm_ctx* ctx, int nblk_, int F_, int K_, int P_, int L_, const int* svnum_host, const int* l0_host,
                       const int* nmodes_host, const int64_t* evals_off_host, int R_) {
  DM_ARG(ctx, nblk_ >= 0 && F_ > 0 && K_ > 0 && P_ > 0 && L_ > 0 && R_ > 0 && svnum_host && l0_host && nmodes_host &&
                  evals_off_host);
  DM_ARG(ctx, F_ <= 256 && (int64_t)nblk_ * R_ < (1LL << 29));   // the staged row chunk holds >= 16 rows of <= 256
  nblk = nblk_, F = F_, K = K_, P = P_, L = L_, R = R_;
  svnum = svnum_host, nmodes = nmodes_host, evals_off = evals_off_host;
  ndof.assign(nblk, 0), active.assign(nblk, 0), l0eff.assign(nblk, L), off1.assign(nblk, 0);
  tot1 = totw = 0;
  for (int b = 0; b < nblk; ++b) {
    for (int f = 0; f < F; ++f) ndof[b] += svnum[b * F + f];
    DM_ARG(ctx, svnum[b * F] >= 0 && ndof[b] >= 0);
    active[b] = nmodes[b] > 0 && ndof[b] > 0 && l0_host[b] < L;
    if (active[b]) l0eff[b] = std::max(l0_host[b], 0);
    off1[b] = (int64_t)tot1;
    tot1 += (size_t)ndof[b] * R;
    totw = std::max<size_t>(totw, (size_t)evals_off[b] + std::max(nmodes[b], 0));
  }
  return DM_OK;
}

int dm_band_proj::to_svd(dm_ctx* ctx, const cplx* evecs, const int64_t* evecs_off, const double* w, const int64_t* x_off,
                         int nset, const cplx* const* xin, cplx* const* x1) const {
  std::vector<dm_gemm_desc> g;
  for (int b = 0; b < nblk; ++b) {
    if (!active[b]) continue;
    for (int s = 0; s < nset; ++s)
      g.push_back(dm_gemm_make(evecs + evecs_off[b], 1, ndof[b], true, xin[s] + x_off[b], R, 1, false, x1[s] + off1[b], R,
                               ndof[b], R, nmodes[b], 1.0, 0.0, w ? w + evals_off[b] : nullptr));
  }
  return dm_gemm_grouped_launch(ctx, g);
}

int dm_band_proj::to_sky(dm_ctx* ctx, const cplx* beam, int nset, const cplx* const* x1, cplx* const* x2) const {
  const int PL = P * L;
  const size_t blk = (size_t)L * F * R;   // elements of one block of x2
  std::vector<dm_gemm_desc> g;
  for (int b = 0; b < nblk; ++b) {
    if (!active[b]) continue;
    const int l0 = l0eff[b];
    bool gaps = false;
    for (int f = 0; f < F; ++f) gaps |= svnum[b * F + f] == 0;
    if (gaps)
      for (int s = 0; s < nset; ++s) DM_TRY(dm_fill_zero(ctx, x2[s] + b * blk, sizeof(cplx) * blk));
    int row = 0;
    for (int f = 0; f < F; ++f) {
      const int ns = svnum[b * F + f];
      if (ns > 0) {
        const cplx* Bf = beam + (((size_t)b * F + f) * K) * PL + l0;   // pol 0
        const size_t co = b * blk + ((size_t)l0 * F + f) * R;
        for (int s = 0; s < nset; ++s)
          g.push_back(dm_gemm_make(Bf, 1, PL, true, x1[s] + off1[b] + (size_t)row * R, R, 1, false, x2[s] + co, F * R,
                                   L - l0, R, ns));
      }
      row += ns;
    }
  }
  return dm_gemm_grouped_launch(ctx, g);
}
