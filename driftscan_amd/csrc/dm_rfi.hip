// dm_rfi.hip — RFI flagging of one day's data along time: dm_rfi_flag runs an iterated
// SumThreshold in the AOFlagger style on every (frequency, row) series, cut into balanced segments, and writes the
// weights of the day with the flagged samples at 0.
//
// A workgroup of 4 waves takes one (frequency, row, segment) of n <= DM_RFI_MAX_SEGMENT samples.  Thread t owns the
// samples t, t + 256, ...: it stages their x (16 bytes per lane, contiguous across the lanes) and input flags in LDS
// once and keeps their w in registers, so every element of x and w comes from HBM once per call and only w_out and the
// small outputs are written.  A flagged sample is staged as x = 0, so that its value, NaN included, reaches nothing.  All
// iterations run on the LDS copy: the background (a Gaussian-weighted mean over the unflagged neighbours, one FMA per
// component and term in ascending order), the amplitude of the residual, the median, and the window passes.  The median
// is an exact order statistic: a radix select over the 8 bytes of the bit patterns of the non-negative amplitudes, most
// significant first, with a histogram of 256 integer LDS counters and a block scan per byte.  No floating-point atomics
// anywhere; the integer counters of the histogram, of nflag and of the occupancy sum to the same value in any order.
// Window sums are direct sums in ascending order, one thread per window start.  Nothing depends on the row, the
// frequency or the batch: a row has the same bits in w_out and noise alone and in any batch.
//
// The occupancy step: the row kernel counts, per (frequency, sample), the rows whose sample is input flagged and the
// rows where detection flagged it anew, with integer atomics; the second kernel (lane = sample, contiguous across the
// lanes) decides every column from these two integers and zeroes the columns that are hit in every row.
#include "dm_common.h"
#include "dm_rfi_table.h"
#include "dm_stack_table.h"
#include "../../include/driftmi.h"

// No implicit contraction in this file (as dm_sidereal.hip): the fused operations of the method are __builtin_fma.
#pragma clang fp contract(off)

namespace {

constexpr int RFI_THREADS = 256, RFI_WAVES = RFI_THREADS / 64, RFI_SPT = DM_RFI_MAX_SEGMENT / RFI_THREADS;

// the sum of v over the workgroup, to every thread; red holds RFI_WAVES ints
__device__ __forceinline__ int rfi_block_sum(int v, int* red, uint32_t lane, uint32_t wave) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();   // red may still be read from the call before
  if (lane == 0) red[wave] = v;
  __syncthreads();
  int s = 0;
#pragma unroll
  for (int i = 0; i < RFI_WAVES; ++i) s += red[i];
  return s;
}

template <bool HAS_W>
__global__ __launch_bounds__(RFI_THREADS) void rfi_row_kernel(const cplx* __restrict__ x, const double* w, double* w_out,
                                                              double* __restrict__ noise, int* __restrict__ nflag,
                                                              int* __restrict__ occ, int* __restrict__ nin_flagged,
                                                              const dm_rfi_tables tb, uint32_t nrow, uint32_t nt,
                                                              uint32_t nseg, uint32_t pitch) {
  extern __shared__ cplx rfi_lds[];
  cplx* xs = rfi_lds;                                             // [pitch]
  double* amp = reinterpret_cast<double*>(xs + pitch);            // [pitch] |x - background|
  unsigned char* fI = reinterpret_cast<unsigned char*>(amp + pitch);   // [pitch] input flags
  unsigned char* fB = fI + pitch;                                 // [pitch] the fit-exclusion set
  unsigned char* fD = fB + pitch;                                 // [pitch] detection: 1 in D, 2 joins D after this pass
  int* hist = reinterpret_cast<int*>(fD + pitch);                 // [256]
  int* red = hist + 256;                                          // [RFI_WAVES]
  int* sel = red + RFI_WAVES;                                     // [2] the selected byte and the rank inside it
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t seg = blockIdx.x % nseg, cell = blockIdx.x / nseg, f = cell / nrow;
  const uint32_t j0 = (uint32_t)(((uint64_t)seg * nt) / nseg), j1 = (uint32_t)(((uint64_t)(seg + 1) * nt) / nseg);
  const uint32_t n = j1 - j0;                                     // 1 <= n <= segment <= pitch
  const size_t base = (size_t)cell * nt + j0;
  double wv[RFI_SPT];
#pragma unroll
  for (int u = 0; u < RFI_SPT; ++u) {
    const uint32_t j = tid + RFI_THREADS * u;
    wv[u] = 1.0;
    if (j < n) {
      cplx v = dm_ldg(x, base + j);
      bool ok = true;
      if constexpr (HAS_W) {
        wv[u] = dm_ldg(w, base + j);
        ok = wv[u] > 0.0;
      }
      if (!ok) v = make_double2(0.0, 0.0);
      xs[j] = v;
      fI[j] = ok ? 0 : 1;
      fB[j] = ok ? 0 : 1;
      fD[j] = ok ? 0 : 1;
    }
  }
  __syncthreads();
  const int H = tb.H;
  double med = 0.0;
  bool all_flagged = false;
  for (int it = 0; it < tb.niter; ++it) {
    // 1. the samples outside B
    int mine = 0;
#pragma unroll
    for (int u = 0; u < RFI_SPT; ++u) {
      const uint32_t j = tid + RFI_THREADS * u;
      if (j < n && !fB[j]) ++mine;
    }
    const int c = rfi_block_sum(mine, red, lane, wave);
    if (c < tb.min_good) {   // the same for the whole workgroup
      all_flagged = true;
      med = 0.0;
      break;
    }
    // 2. background and amplitude of every sample outside I; D restarts from I and the unjudgeable samples
#pragma unroll 1
    for (int u = 0; u < RFI_SPT; ++u) {
      const uint32_t j = tid + RFI_THREADS * u;
      if (j >= n) break;
      double a = 0.0;
      unsigned char d = 1;
      if (!fI[j]) {
        double sx = 0.0, sy = 0.0, sg = 0.0;
        int used = 0;
        for (int dd = -H; dd <= H; ++dd) {   // dd is the same for every lane: g comes from the kernel arguments
          const int k = (int)j + dd;
          if (k < 0 || k >= (int)n || fB[k]) continue;
          const double g = tb.g[dd < 0 ? -dd : dd];
          const cplx v = xs[k];
          sx = __builtin_fma(g, v.x, sx);
          sy = __builtin_fma(g, v.y, sy);
          sg += g;
          ++used;
        }
        if (used > 0) {
          const cplx v = xs[j];
          const double rx = v.x - sx / sg, ry = v.y - sy / sg;
          a = sqrt(rx * rx + ry * ry);
          d = 0;
        }
      }
      amp[j] = a;
      fD[j] = d;
    }
    __syncthreads();
    // 3. the lower median of the amplitudes outside B: rank (c - 1) / 2 of c, by bytes from the most significant
    {
      unsigned long long key[RFI_SPT];
      uint32_t live = 0;
#pragma unroll
      for (int u = 0; u < RFI_SPT; ++u) {
        const uint32_t j = tid + RFI_THREADS * u;
        key[u] = 0;
        if (j < n && !fB[j]) {
          key[u] = (unsigned long long)__double_as_longlong(amp[j]);
          live |= 1u << u;
        }
      }
      unsigned long long prefix = 0;
      int rank = (c - 1) / 2;
      for (int p = 7; p >= 0; --p) {
        hist[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < RFI_SPT; ++u)
          if ((live >> u) & 1u) {
            if (p == 7 || (key[u] >> (8 * (p + 1))) == prefix) atomicAdd(&hist[(key[u] >> (8 * p)) & 255ull], 1);
          }
        __syncthreads();
        const int v = hist[tid];
        int incl = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
          const int t = __shfl_up(incl, o, 64);
          if ((int)lane >= o) incl += t;
        }
        if (lane == 63) red[wave] = incl;
        __syncthreads();
        int excl = incl - v;
        for (uint32_t i = 0; i < wave; ++i) excl += red[i];
        if (v > 0 && excl <= rank && rank < excl + v) {   // exactly one thread
          sel[0] = (int)tid;
          sel[1] = rank - excl;
        }
        __syncthreads();
        prefix = (prefix << 8) | (unsigned long long)sel[0];
        rank = sel[1];
      }
      med = __longlong_as_double((long long)prefix);
    }
    // 4. the window passes, each against D as it stood at the start of the pass
    for (int i = 0; i < tb.nwin; ++i) {
      const uint32_t M = (uint32_t)tb.window[i];
      if (M > n) break;
      const double thr = med * tb.t[it][i];
      for (uint32_t j = tid; j + M <= n; j += RFI_THREADS) {
        int cnt = 0;
        double S = 0.0;
        for (uint32_t k = j; k < j + M; ++k)
          if (fD[k] != 1) {
            ++cnt;
            S += amp[k];
          }
        if (cnt >= 1 && S > (double)cnt * thr)
          for (uint32_t k = j; k < j + M; ++k)
            if (fD[k] != 1) fD[k] = 2;
      }
      __syncthreads();
#pragma unroll
      for (int u = 0; u < RFI_SPT; ++u) {
        const uint32_t j = tid + RFI_THREADS * u;
        if (j < n && fD[j] == 2) fD[j] = 1;
      }
      __syncthreads();
    }
    // 5. B of the next iteration
#pragma unroll
    for (int u = 0; u < RFI_SPT; ++u) {
      const uint32_t j = tid + RFI_THREADS * u;
      if (j < n) fB[j] = fD[j];
    }
    __syncthreads();
  }
  int fresh = 0;
#pragma unroll
  for (int u = 0; u < RFI_SPT; ++u) {
    const uint32_t j = tid + RFI_THREADS * u;
    if (j < n) {
      const bool in = fI[j] != 0, flagged = all_flagged || fB[j] != 0;
      dm_stg(w_out, base + j, flagged ? 0.0 : wv[u]);
      if (in) atomicAdd(&nin_flagged[(size_t)f * nt + j0 + j], 1);
      if (flagged && !in) {
        atomicAdd(&occ[(size_t)f * nt + j0 + j], 1);
        ++fresh;
      }
    }
  }
  fresh = rfi_block_sum(fresh, red, lane, wave);
  if (tid == 0) {
    if (fresh > 0) atomicAdd(&nflag[cell], fresh);
    dm_stg(noise, (size_t)cell * nseg + seg, all_flagged ? 0.0 : med / DM_RFI_SQRT_LN2);
  }
}

// lane = sample: a column (f, j) with n_new > row_share n_in is flagged in the rows r0 .. r1 - 1 of this workgroup
__global__ __launch_bounds__(RFI_THREADS) void rfi_occupancy_kernel(double* __restrict__ w_out, const int* __restrict__ occ,
                                                                    const int* __restrict__ nin_flagged, uint32_t nrow,
                                                                    uint32_t nt, uint32_t rows_per, double row_share) {
  const uint32_t j = blockIdx.x * RFI_THREADS + threadIdx.x, f = blockIdx.y;
  if (j >= nt) return;
  const int n_in = (int)nrow - nin_flagged[(size_t)f * nt + j], n_new = occ[(size_t)f * nt + j];
  if (!(n_in > 0 && (double)n_new > row_share * (double)n_in)) return;
  const uint32_t r0 = blockIdx.z * rows_per, r1 = r0 + rows_per < nrow ? r0 + rows_per : nrow;
  for (uint32_t r = r0; r < r1; ++r) dm_stg(w_out, ((size_t)f * nrow + r) * nt + j, 0.0);
}

int rfi_refuse(dm_ctx* ctx, const std::string& what) {
  ctx->err = "dm_rfi_flag: " + what;
  return DM_EARG;
}

}  // namespace

extern "C" int dm_rfi_max_segment(void) { return DM_RFI_MAX_SEGMENT; }

extern "C" int dm_rfi_flag(dm_ctx* ctx, int nf, int nrow, int nt, int segment, double kernel_sigma, int nwin,
                           const int* windows_host, double chi1, double rho, int niter, double base, int min_good,
                           double row_share, const void* x_dev, const double* w_dev, double* wout_dev, double* noise_dev,
                           int* nflag_dev, int* occupancy_dev) {
  if (!ctx) return DM_EARG;
  if (nf < 0 || nrow < 0 || nt < 0) return rfi_refuse(ctx, "negative size");
  const std::string bad = dm_rfi_check(nt, segment, kernel_sigma, nwin, windows_host, chi1, rho, niter, base, min_good, row_share);
  if (!bad.empty()) return rfi_refuse(ctx, bad);
  const uint64_t nel = (uint64_t)nf * nrow * nt;
  if (nel == 0) return DM_OK;
  const uint32_t nseg = (uint32_t)(((int64_t)nt + segment - 1) / segment);
  if (!x_dev || !wout_dev || !noise_dev || !nflag_dev || !occupancy_dev)
    return rfi_refuse(ctx, "null x, w_out, noise, nflag or occupancy with work to do");
  {
    const uint64_t ip[2] = {(uint64_t)x_dev, (uint64_t)w_dev}, ib[2] = {16 * nel, w_dev ? 8 * nel : 0};
    const uint64_t op[4] = {(uint64_t)wout_dev, (uint64_t)noise_dev, (uint64_t)nflag_dev, (uint64_t)occupancy_dev};
    const uint64_t ob[4] = {8 * nel, 8 * (uint64_t)nf * nrow * nseg, 4 * (uint64_t)nf * nrow, 4 * (uint64_t)nf * nt};
    for (int o = 0; o < 4; ++o) {
      for (int i = 0; i < 2; ++i) {
        if (o == 0 && i == 1 && op[o] == ip[i]) continue;   // w_out may be w itself
        if (dm_spans_overlap(ip[i], ib[i], 0, op[o], ob[o], 0, 1))
          return rfi_refuse(ctx, "an output shares an element with x or w (w_out may be w itself)");
      }
      for (int p = 0; p < o; ++p)
        if (dm_spans_overlap(op[p], ob[p], 0, op[o], ob[o], 0, 1)) return rfi_refuse(ctx, "two outputs share an element");
    }
  }
  const uint64_t nblocks = (uint64_t)nf * nrow * nseg;
  if (nblocks >= (1ull << 31) || nf > 65535) return rfi_refuse(ctx, "too many workgroups for one launch");
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_rfi_tables tb;
  dm_rfi_make_tables(kernel_sigma, nwin, windows_host, chi1, rho, niter, base, min_good, &tb);
  dm_ws_scope ws(ctx);
  int* nin_flagged = dm_ws_alloc_t<int>(ctx, (size_t)nf * nt);
  if (!nin_flagged) return DM_ENOMEM;
  DM_HIP(ctx, hipMemsetAsync(nin_flagged, 0, 4 * (size_t)nf * nt, ctx->stream));
  DM_HIP(ctx, hipMemsetAsync(occupancy_dev, 0, 4 * (size_t)nf * nt, ctx->stream));
  DM_HIP(ctx, hipMemsetAsync(nflag_dev, 0, 4 * (size_t)nf * nrow, ctx->stream));
  // the longest balanced segment is ceil(nt / nseg) <= segment; the byte arrays keep the integers behind them aligned
  uint32_t pitch = (uint32_t)(((int64_t)nt + nseg - 1) / nseg);
  pitch = (pitch + 15u) & ~15u;
  const size_t lds = (size_t)pitch * (16 + 8 + 3) + (256 + RFI_WAVES + 2) * sizeof(int);
  const cplx* x = static_cast<const cplx*>(x_dev);
  if (w_dev)
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (rfi_row_kernel<true>), dim3((unsigned)nblocks), dim3(RFI_THREADS), lds, ctx->stream, x,
               w_dev, wout_dev, noise_dev, nflag_dev, occupancy_dev, nin_flagged, tb, (uint32_t)nrow, (uint32_t)nt, nseg,
               pitch);
  else
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (rfi_row_kernel<false>), dim3((unsigned)nblocks), dim3(RFI_THREADS), lds, ctx->stream, x,
               w_dev, wout_dev, noise_dev, nflag_dev, occupancy_dev, nin_flagged, tb, (uint32_t)nrow, (uint32_t)nt, nseg,
               pitch);
  DM_HIP(ctx, hipGetLastError());
  if (row_share < 1.0) {
    uint32_t rows_per = 256, nz = ((uint32_t)nrow + rows_per - 1) / rows_per;
    if (nz > 65535u) {
      nz = 65535u;
      rows_per = ((uint32_t)nrow + nz - 1) / nz;
      nz = ((uint32_t)nrow + rows_per - 1) / rows_per;
    }
    DM_PLAUNCH(ctx, DM_PROF_UTIL, rfi_occupancy_kernel, dim3(((unsigned)nt + RFI_THREADS - 1) / RFI_THREADS, (unsigned)nf, nz),
               dim3(RFI_THREADS), 0, ctx->stream, wout_dev, occupancy_dev, nin_flagged, (uint32_t)nrow, (uint32_t)nt,
               rows_per, row_share);
    DM_HIP(ctx, hipGetLastError());
  }
  return DM_OK;
}
