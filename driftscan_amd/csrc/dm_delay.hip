// dm_delay.hip — dm_delay_fit, the band-limited weighted least-squares fit along frequency.
//
// One problem per (row, t): with A (nf x r) the basis of the row's class, omega_f = w_f where w_f > 0 and 0 elsewhere,
//   G = sum_f omega_f a_f a_f^T + ridge s I,   s = sum_f omega_f / nf,   G = L L^T,   c = G^-1 sum_f omega_f a_f x_f,
//   model_f = a_f^T c,   v_f = |L^-1 a_f|^2.
// The series x[:, row, t] are strided by nrow nt, so a workgroup takes a tile of TJ consecutive t of one row, reads it
// frequency row by frequency row (TJ contiguous samples each) and stages it transposed in LDS with an odd pitch, as
// rfi_freq_kernel does; x of a sample that is not kept is replaced by 0 on the way in and reaches no arithmetic.  One
// wave works on one series from there on, and every barrier but those around a basis chunk is wave-local.  The basis
// of the row (the same for the whole workgroup) passes through LDS in chunks of DL_FC frequencies, transposed to
// [frequency][vector].
//
// The fixed orders (nothing in them depends on the tile, the launch or the table):
//   G_ij (i >= j)  acc = fma(omega_f, a_fi * a_fj, acc) in ascending f; lane (bi, bj) of an 8 x 8 grid keeps the B x B
//                  block of G in registers, B = 1, 2, 4, 8 for a largest rank up to 8, 16, 32, 64;
//   b_i            acc = fma(a_fi, omega_f * x_f, acc) in ascending f, real and imaginary parts apart; lane = i;
//   s, nvalid      in ascending f;  G_ii += ridge * s when ridge > 0;
//   Cholesky       column by column (left looking), lane = row i: acc = G_ij, acc = fma(-L_ik, L_jk, acc) in ascending
//                  k < j; L_jj = sqrt(acc_j), L_ij = acc_i / L_jj; a pivot acc_j that is not finite or not > 0 ends the
//                  sample with info = j + 1;
//   L y = b        ascending j: y_j = b_j / L_jj, then b_i = fma(-L_ij, y_j, b_i) for i > j;
//   L^T c = y      descending j: c_j = y_j / L_jj, then y_i = fma(-L_ji, c_j, y_i) for i < j;
//   model_f        acc = fma(a_fi, c_i, acc) in ascending i, lane = f;
//   v_f            the forward substitution above on a_f, v = fma(y_j, y_j, v) in ascending j (flagged f of a solved
//                  sample in inpaint mode only).
#include "dm_common.h"
#include "dm_feedpair.h"
#include "dm_stack_table.h"
#include "../../include/driftmi.h"

#include <cfloat>
#include <cmath>

// No implicit contraction in this file: the fused operations of the method are __builtin_fma.
#pragma clang fp contract(off)

#define DM_DELAY_MAX_NF 2048
#define DM_DELAY_MAX_RANK 64
#define DM_DELAY_MAX_BASIS 256

namespace {

constexpr int DL_FC = 16;                      // frequencies of a basis chunk
constexpr int DL_MAX_TJ = 8;                   // series of a tile, at most: 512 threads
constexpr size_t DL_LDS_BYTES = 160 * 1024;
constexpr int DL_CU_WAVES = 32;

// The LDS of a tile: per series ps samples and an rmax x pr matrix, ps and pr odd.
struct dl_layout {
  uint32_t ps, pr, tj, rmax;
  __host__ __device__ size_t xs() const { return 0; }
  __host__ __device__ size_t ws() const { return (size_t)16 * tj * ps; }
  __host__ __device__ size_t g() const { return ws() + (size_t)8 * tj * ps; }
  __host__ __device__ size_t c() const { return (g() + (size_t)8 * tj * rmax * pr + 15) & ~(size_t)15; }
  __host__ __device__ size_t chunk() const { return c() + (size_t)16 * tj * rmax; }
  __host__ __device__ size_t bytes() const { return chunk() + (size_t)8 * DL_FC * pr; }
};

inline dl_layout delay_layout(int nf, int rmax, int tj) {
  dl_layout L;
  L.ps = (uint32_t)nf | 1u;
  L.pr = (uint32_t)rmax | 1u;
  L.tj = (uint32_t)tj;
  L.rmax = (uint32_t)rmax;
  return L;
}

// the series of a tile for nf frequencies and a largest rank rmax: the TJ that puts most waves on a CU, the larger of
// two that tie (more series share a basis chunk); 0: no tile fits
inline int delay_tile(int nf, int rmax) {
  if (nf < 1 || nf > DM_DELAY_MAX_NF || rmax < 1 || rmax > DM_DELAY_MAX_RANK) return 0;
  int best = 0;
  size_t best_waves = 0;
  for (int tj = 1; tj <= DL_MAX_TJ; ++tj) {
    const size_t b = delay_layout(nf, rmax, tj).bytes();
    if (b > DL_LDS_BYTES) break;
    size_t groups = DL_LDS_BYTES / b;
    if (groups * tj > (size_t)DL_CU_WAVES) groups = DL_CU_WAVES / tj;
    if (groups * tj >= best_waves) {
      best_waves = groups * tj;
      best = tj;
    }
  }
  return best;
}

struct dl_table {
  unsigned char rank[DM_DELAY_MAX_BASIS];
  uint32_t off[DM_DELAY_MAX_BASIS];   // the vectors before basis k
};

// Wave-local barrier: the LDS operations of a wave complete in order.
__device__ __forceinline__ void dl_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ bool dl_pos_finite(double v) { return v > 0.0 && v <= DBL_MAX; }

template <int B, bool HAS_W>
__global__ __launch_bounds__(64 * DL_MAX_TJ) void delay_fit_kernel(const cplx* x, const double* w, cplx* xout, double* wout,
                                                                  int* __restrict__ info, const double* __restrict__ basis,
                                                                  const int* __restrict__ basis_of, const dl_table tb,
                                                                  uint32_t nbasis, uint32_t nf, uint32_t nrow, uint32_t nt,
                                                                  uint32_t ntile, int mode, double ridge, int min_valid,
                                                                  const dl_layout L) {
  extern __shared__ cplx dl_lds[];
  unsigned char* lds = reinterpret_cast<unsigned char*>(dl_lds);
  const uint32_t ps = L.ps, pr = L.pr, TJ = L.tj, T = 64 * TJ;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = blockIdx.x % ntile, row = blockIdx.x / ntile, jt0 = tile * TJ;
  const int kb = basis_of[row];
  const bool bad_class = kb < 0 || kb >= (int)nbasis;
  const uint32_t r = bad_class ? 0u : (uint32_t)tb.rank[kb];   // the same for the whole workgroup; r <= L.rmax
  const double* A = basis + (bad_class ? (size_t)0 : (size_t)tb.off[kb] * nf);
  // ---- the tile comes in: thread = (frequency row fr, series tj)
  const uint32_t tj = tid % TJ, fr = tid / TJ;
  const bool mine_in = jt0 + tj < nt;
  {
    cplx* xs = reinterpret_cast<cplx*>(lds + L.xs()) + (size_t)tj * ps;
    double* wsm = reinterpret_cast<double*>(lds + L.ws()) + (size_t)tj * ps;
    for (uint32_t k = fr; k < nf; k += 64) {
      cplx v = make_double2(0.0, 0.0);
      double wk = 0.0;
      if (mine_in) {   // a series past nt is staged as flagged throughout
        const size_t idx = ((size_t)k * nrow + row) * nt + jt0 + tj;
        wk = 1.0;
        if constexpr (HAS_W) wk = dm_ldg(w, idx);
        if (wk > 0.0)
          v = dm_ldg(x, idx);
        else
          wk = 0.0;
      }
      xs[k] = v;
      wsm[k] = wk;
    }
  }
  // ---- one wave, one series
  const bool active = jt0 + wave < nt;
  cplx* xs = reinterpret_cast<cplx*>(lds + L.xs()) + (size_t)wave * ps;
  double* wsm = reinterpret_cast<double*>(lds + L.ws()) + (size_t)wave * ps;
  double* G = reinterpret_cast<double*>(lds + L.g()) + (size_t)wave * L.rmax * pr;
  cplx* cs = reinterpret_cast<cplx*>(lds + L.c()) + (size_t)wave * L.rmax;
  double* ch = reinterpret_cast<double*>(lds + L.chunk());
  // 1. G, b, s and nvalid in ascending f
  double acc[B][B];
#pragma unroll
  for (int a = 0; a < B; ++a)
#pragma unroll
    for (int b = 0; b < B; ++b) acc[a][b] = 0.0;
  double bre = 0.0, bim = 0.0, s = 0.0;
  int nvalid = 0;
  const uint32_t bi = lane >> 3, bj = lane & 7u;
  for (uint32_t f0 = 0; f0 < nf && r > 0; f0 += DL_FC) {
    __syncthreads();   // the chunk before is read no more (and, the first time, the tile is in)
    for (uint32_t e = tid; e < r * DL_FC; e += T) {
      const uint32_t i = e / DL_FC, fl = e % DL_FC;
      ch[fl * pr + i] = f0 + fl < nf ? dm_ldg(A, (size_t)i * nf + f0 + fl) : 0.0;
    }
    __syncthreads();
    if (!active) continue;
    const uint32_t nfc = nf - f0 < (uint32_t)DL_FC ? nf - f0 : (uint32_t)DL_FC;
    for (uint32_t fl = 0; fl < nfc; ++fl) {
      const double om = wsm[f0 + fl];
      const cplx xv = xs[f0 + fl];
      const double* af = ch + fl * pr;
      s += om;
      nvalid += om > 0.0 ? 1 : 0;
      if (bi >= bj) {
        double ai[B], aj[B];
#pragma unroll
        for (int a = 0; a < B; ++a) {
          ai[a] = bi * B + a < r ? af[bi * B + a] : 0.0;
          aj[a] = bj * B + a < r ? af[bj * B + a] : 0.0;
        }
#pragma unroll
        for (int a = 0; a < B; ++a)
#pragma unroll
          for (int b = 0; b < B; ++b) acc[a][b] = __builtin_fma(om, ai[a] * aj[b], acc[a][b]);
      }
      if (lane < r) {
        const double a = af[lane];
        bre = __builtin_fma(a, om * xv.x, bre);
        bim = __builtin_fma(a, om * xv.y, bim);
      }
    }
  }
  if (r == 0) __syncthreads();   // the tile is in
  int inf = bad_class ? -2 : 0;
  if (active && !bad_class) {
    if (bi >= bj) {
#pragma unroll
      for (int a = 0; a < B; ++a)
#pragma unroll
        for (int b = 0; b < B; ++b) {
          const uint32_t i = bi * B + a, j = bj * B + b;
          if (i < r && j <= i) G[i * pr + j] = acc[a][b];
        }
    }
    const int need = min_valid <= 0 ? (int)r : min_valid;
    if (nvalid < need || nvalid == 0) inf = -1;
    dl_wave_sync();
    if (inf == 0) {
      s = s / (double)nf;
      if (ridge > 0.0 && lane < r) G[lane * pr + lane] += ridge * s;
      dl_wave_sync();
      // 2. Cholesky, in place in the lower triangle
      for (uint32_t j = 0; j < r; ++j) {
        double a = 0.0;
        if (lane >= j && lane < r) {
          a = G[lane * pr + j];
          for (uint32_t k = 0; k < j; ++k) a = __builtin_fma(-G[lane * pr + k], G[j * pr + k], a);
        }
        const double d = __shfl(a, (int)j, 64);
        if (!dl_pos_finite(d)) {
          inf = (int)j + 1;
          break;
        }
        const double ljj = sqrt(d);
        if (lane == j)
          G[j * pr + j] = ljj;
        else if (lane > j && lane < r)
          G[lane * pr + j] = a / ljj;
        dl_wave_sync();
      }
    }
    if (inf == 0) {
      // 3. L y = b, L^T c = y
      for (uint32_t j = 0; j < r; ++j) {
        const double ljj = G[j * pr + j];
        const double yre = __shfl(bre, (int)j, 64) / ljj, yim = __shfl(bim, (int)j, 64) / ljj;
        if (lane == j) {
          bre = yre;
          bim = yim;
        } else if (lane > j && lane < r) {
          const double l = G[lane * pr + j];
          bre = __builtin_fma(-l, yre, bre);
          bim = __builtin_fma(-l, yim, bim);
        }
      }
      for (uint32_t j = r; j > 0; --j) {
        const uint32_t q = j - 1;
        const double lqq = G[q * pr + q];
        const double cre = __shfl(bre, (int)q, 64) / lqq, cim = __shfl(bim, (int)q, 64) / lqq;
        if (lane == q) {
          bre = cre;
          bim = cim;
        } else if (lane < q) {
          const double l = G[q * pr + lane];
          bre = __builtin_fma(-l, cre, bre);
          bim = __builtin_fma(-l, cim, bim);
        }
      }
      if (lane < r) cs[lane] = make_double2(bre, bim);
      dl_wave_sync();
      // 4. the model, lane = f
      for (uint32_t f = lane; f < nf; f += 64) {
        double mre = 0.0, mim = 0.0;
        for (uint32_t i = 0; i < r; ++i) {
          const double a = dm_ldg(A, (size_t)i * nf + f);
          const cplx c = cs[i];
          mre = __builtin_fma(a, c.x, mre);
          mim = __builtin_fma(a, c.y, mim);
        }
        const bool kept = wsm[f] > 0.0;
        if (mode == 0) {
          xs[f] = make_double2(mre, mim);
        } else if (mode == 1) {
          if (kept) {
            const cplx v = xs[f];
            xs[f] = make_double2(v.x - mre, v.y - mim);
          }
        } else if (!kept) {
          xs[f] = make_double2(mre, mim);
        }
      }
      dl_wave_sync();
      // 5. the weight of a filled sample
      if (mode == 2) {
        for (uint32_t f = 0; f < nf; ++f) {
          if (wsm[f] > 0.0) continue;   // the same for the whole wave; a fill weight is written behind the walk
          double z = lane < r ? dm_ldg(A, (size_t)lane * nf + f) : 0.0, v = 0.0;
          for (uint32_t j = 0; j < r; ++j) {
            const double yj = __shfl(z, (int)j, 64) / G[j * pr + j];
            v = __builtin_fma(yj, yj, v);
            if (lane > j && lane < r) z = __builtin_fma(-G[lane * pr + j], yj, z);
          }
          if (lane == 0) wsm[f] = dl_pos_finite(v) ? 1.0 / v : 0.0;
          dl_wave_sync();
        }
      }
    }
  }
  if (active && inf != 0 && mode == 0) {   // not solved: no model
    for (uint32_t f = lane; f < nf; f += 64) xs[f] = make_double2(0.0, 0.0);
  }
  if (active && lane == 0) info[(size_t)row * nt + jt0 + wave] = inf;
  __syncthreads();
  // ---- the tile leaves as it came
  if (mine_in) {
    const cplx* xo = reinterpret_cast<const cplx*>(lds + L.xs()) + (size_t)tj * ps;
    const double* wo = reinterpret_cast<const double*>(lds + L.ws()) + (size_t)tj * ps;
    for (uint32_t k = fr; k < nf; k += 64) {
      const size_t idx = ((size_t)k * nrow + row) * nt + jt0 + tj;
      dm_stg(xout, idx, xo[k]);
      dm_stg(wout, idx, wo[k]);
    }
  }
}

}  // namespace

extern "C" int dm_delay_max_nf(void) { return DM_DELAY_MAX_NF; }
extern "C" int dm_delay_max_rank(void) { return DM_DELAY_MAX_RANK; }
extern "C" int dm_delay_tile(int nf, int max_rank) { return delay_tile(nf, max_rank); }

extern "C" int dm_delay_fit(dm_ctx* ctx, int nf, int nrow, int nt, int mode, double ridge, int min_valid, int nbasis,
                            const int* rank_host, const double* basis_dev, const int* basis_of_dev, const void* x_dev,
                            const double* w_dev, void* xout_dev, double* wout_dev, int* info_dev) {
  static const char* who = "dm_delay_fit";
  if (!ctx) return DM_EARG;
  if (nf < 0 || nrow < 0 || nt < 0 || nbasis < 0) return dm_refuse(ctx, who, "negative size");
  if (mode < 0 || mode > 2) return dm_refuse(ctx, who, "mode is 0 (model), 1 (filter) or 2 (inpaint)");
  if (!std::isfinite(ridge) || ridge < 0.0) return dm_refuse(ctx, who, "ridge not finite or negative");
  const uint64_t nel = (uint64_t)nf * nrow * nt;
  if (nel == 0) return DM_OK;
  if (nf > DM_DELAY_MAX_NF) return dm_refuse(ctx, who, "nf > " + std::to_string(DM_DELAY_MAX_NF));
  if (nbasis < 1) return dm_refuse(ctx, who, "nbasis < 1 with work to do");
  if (nbasis > DM_DELAY_MAX_BASIS) return dm_refuse(ctx, who, "nbasis > " + std::to_string(DM_DELAY_MAX_BASIS));
  if (!rank_host || !basis_dev || !basis_of_dev || !x_dev || !xout_dev || !wout_dev || !info_dev)
    return dm_refuse(ctx, who, "null rank, basis, basis_of, x, x_out, w_out or info with work to do");
  dl_table tb;
  int rmax = 0;
  uint64_t nvec = 0;
  for (int k = 0; k < DM_DELAY_MAX_BASIS; ++k) {
    tb.rank[k] = 0;
    tb.off[k] = 0;
  }
  for (int k = 0; k < nbasis; ++k) {
    const int rk = rank_host[k];
    if (rk < 1 || rk > nf || rk > DM_DELAY_MAX_RANK)
      return dm_refuse(ctx, who, "rank of basis " + std::to_string(k) + " is < 1, > nf or > " + std::to_string(DM_DELAY_MAX_RANK));
    tb.rank[k] = (unsigned char)rk;
    tb.off[k] = (uint32_t)nvec;
    nvec += (uint64_t)rk;
    rmax = rk > rmax ? rk : rmax;
  }
  {
    const dm_span in[4] = {{x_dev, 16 * nel, "x"},
                           {w_dev, w_dev ? 8 * nel : 0, "w"},
                           {basis_dev, 8 * nvec * nf, "basis"},
                           {basis_of_dev, 4 * (uint64_t)nrow, "basis_of"}};
    const dm_span out[3] = {{xout_dev, 16 * nel, "x_out"}, {wout_dev, 8 * nel, "w_out"}, {info_dev, 4 * (uint64_t)nrow * nt, "info"}};
    for (int o = 0; o < 3; ++o)
      for (int i = 0; i < 4 + o; ++i) {
        const dm_span& other = i < 4 ? in[i] : out[i - 4];
        if ((o == 0 && i == 0 && xout_dev == x_dev) || (o == 1 && i == 1 && wout_dev == w_dev)) continue;   // in place
        if (dm_spans_overlap((uint64_t)out[o].p, out[o].bytes, 0, (uint64_t)other.p, other.bytes, 0, 1))
          return dm_refuse(ctx, who, std::string(out[o].name) + " shares an element with " + other.name +
                                         " (x_out may be x and w_out may be w)");
      }
  }
  const int tj = delay_tile(nf, rmax);
  if (tj < 1) return dm_refuse(ctx, who, "no tile for this nf and rank");
  const dl_layout L = delay_layout(nf, rmax, tj);
  const size_t lds = L.bytes();
  const uint32_t ntile = ((uint32_t)nt + L.tj - 1) / L.tj;
  const uint64_t nblocks = (uint64_t)nrow * ntile;
  if (nblocks >= (1ull << 31)) return dm_refuse(ctx, who, "too many workgroups for one launch");
  DM_HIP(ctx, hipSetDevice(ctx->device));
  const cplx* x = static_cast<const cplx*>(x_dev);
  cplx* xo = static_cast<cplx*>(xout_dev);
  const dim3 grid((unsigned)nblocks), block(64 * L.tj);
#define DL_LAUNCH(B, HAS_W)                                                                                                 \
  do {                                                                                                                      \
    if (int rc = dm_lds_attr(ctx, delay_fit_kernel<B, HAS_W>, lds)) return rc;                                              \
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (delay_fit_kernel<B, HAS_W>), grid, block, lds, ctx->stream, x, w_dev, xo, wout_dev,      \
               info_dev, basis_dev, basis_of_dev, tb, (uint32_t)nbasis, (uint32_t)nf, (uint32_t)nrow, (uint32_t)nt, ntile,  \
               mode, ridge, min_valid, L);                                                                                  \
  } while (0)
#define DL_LAUNCH_W(B)     \
  do {                     \
    if (w_dev)             \
      DL_LAUNCH(B, true);  \
    else                   \
      DL_LAUNCH(B, false); \
  } while (0)
  if (rmax <= 8)
    DL_LAUNCH_W(1);
  else if (rmax <= 16)
    DL_LAUNCH_W(2);
  else if (rmax <= 32)
    DL_LAUNCH_W(4);
  else
    DL_LAUNCH_W(8);
#undef DL_LAUNCH_W
#undef DL_LAUNCH
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}
