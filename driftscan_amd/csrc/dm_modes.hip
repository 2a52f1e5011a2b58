// dm_modes.hip — the data side of the m-mode chain: block-apply of stored product blocks to a few vectors, and the
// twiddle table of the time -> m transform.
//
// dm_blockvec_grouped: y_p = alpha_p op(A_p) x_p for a ragged list of problems with a SMALL number R of right-hand sides
// (R <= 8).  Every element of A is read once with a 16-byte load; the kernel is bound by that stream, not by arithmetic
// (8 R flops per 16 bytes), so it runs on the fp64 VALU and spends its registers on loads in flight.  Two forms, picked
// per problem from its strides:
//   dot  (A contiguous along K, or no unit stride at all): a wave owns BV_RW rows per pass, lanes run along K with R
//        accumulators per row, and the 2 R BV_RW partial sums of a lane meet in ONE transposing butterfly over the wave;
//   axpy (A contiguous along M): a lane owns one row, the four waves of the workgroup take every fourth k and wave 0 adds
//        their partial sums in a fixed order.
// x is staged in LDS in chunks of BV_KC rows of K, laid out [r][k] so that neighbouring lanes read neighbouring words.
// One output element is produced by one wave (dot) or the four waves of one workgroup (axpy) in an order that depends on
// (K, strides, R) only: no atomics, and the result of a problem does not depend on what else is in the batch.
#include "dm_common.h"
#include "../../include/driftmi.h"

namespace {

constexpr int BV_KC = 256;     // rows of x per LDS chunk (R * 4 KiB)
constexpr int BV_RW = 4;       // rows per wave and pass in the dot form
constexpr int BV_DOT_ROWS = 4 * BV_RW;
constexpr int BV_DOT_GROUPS = 4;   // passes per workgroup when x fits one chunk (K <= BV_KC): x is staged once for 64 rows
constexpr int BV_AXPY_ROWS = 64;

struct bv_desc {
  const cplx* A;
  const cplx* x;
  cplx* y;
  long long rsA, csA, rsB, csB, ldc;
  int M, K;
  int conjA, conjB;
  int axpy;
  int groups;
  double alpha;
};
struct bv_item { int desc; int row0; };

constexpr int bv_pow2(int n) { return n <= 1 ? 1 : 2 * bv_pow2((n + 1) / 2); }

// Sum N values per lane over the 64 lanes of a wave in N - 1 + log2(64 / N) shuffles instead of 6 N: at offset O the
// lanes with bit O set keep the upper half of the values and hand the lower half over (and the other way round), so the
// number of live values halves with every step; once one is left the usual butterfly finishes.  Afterwards value number
// lane >> (6 - log2 N) is complete in v[0].  The order of the additions is fixed by N alone.
template <int N, int O>
__device__ __forceinline__ void bv_wave_reduce(double* v, int lane) {
  if constexpr (N > 1) {
    const bool up = (lane & O) != 0;
#pragma unroll
    for (int j = 0; j < N / 2; ++j) {
      const double send = up ? v[j] : v[j + N / 2];
      const double keep = up ? v[j + N / 2] : v[j];
      v[j] = keep + __shfl_xor(send, O, 64);
    }
    bv_wave_reduce<N / 2, O / 2>(v, lane);
  } else {
#pragma unroll
    for (int o = O; o > 0; o >>= 1) v[0] += __shfl_xor(v[0], o, 64);
  }
}

template <int R>
__device__ __forceinline__ void bv_stage_x(cplx* xs, const bv_desc& d, int k0, int kc, int tid, double sb) {
  for (int i = tid; i < kc * R; i += 256) {
    const int kk = i / R, r = i - kk * R;
    cplx v = dm_ldg(d.x, (size_t)(k0 + kk) * d.rsB + (size_t)r * d.csB);
    v.y *= sb;
    xs[r * BV_KC + kk] = v;
  }
}

template <int R>
__global__ __launch_bounds__(256) void blockvec_kernel(const bv_desc* __restrict__ dd, const bv_item* __restrict__ items) {
  __shared__ cplx xs[R * BV_KC];
  const bv_item it = items[blockIdx.x];
  const bv_desc d = dd[it.desc];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double sa = d.conjA ? -1.0 : 1.0, sb = d.conjB ? -1.0 : 1.0;

  if (d.axpy) {
    // 64 rows per workgroup, a lane per row; the four waves take every fourth k and their partial sums are added in the
    // order 0, 1, 2, 3 by wave 0 (through the LDS that held x)
    const int row = it.row0 + lane;
    const bool live = row < d.M;
    const cplx* Ar = d.A + (size_t)(live ? row : d.M - 1) * d.rsA;   // idle lanes re-read the last row, store nothing
    cplx acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = make_double2(0.0, 0.0);
    for (int k0 = 0; k0 < d.K; k0 += BV_KC) {
      const int kc = min(BV_KC, d.K - k0);
      __syncthreads();
      bv_stage_x<R>(xs, d, k0, kc, tid, sb);
      __syncthreads();
#pragma unroll 8
      for (int kk = wave; kk < kc; kk += 4) {
        cplx a = dm_ldg(Ar, (size_t)(k0 + kk) * d.csA);
        a.y *= sa;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const cplx xv = xs[r * BV_KC + kk];
          acc[r].x = fma(a.x, xv.x, fma(-a.y, xv.y, acc[r].x));
          acc[r].y = fma(a.x, xv.y, fma(a.y, xv.x, acc[r].y));
        }
      }
    }
    __syncthreads();
    if (wave > 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) xs[((wave - 1) * R + r) * 64 + lane] = acc[r];   // 3 R 64 <= R BV_KC
    }
    __syncthreads();
    if (wave == 0 && live) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        cplx t = acc[r];
#pragma unroll
        for (int w = 0; w < 3; ++w) t = cadd(t, xs[(w * R + r) * 64 + lane]);
        dm_stg(d.y, (size_t)row * d.ldc + r, cscale(t, d.alpha));
      }
    }
    return;
  }

  // dot form: the accumulators of a pass are one flat array v[((i R) + r) 2 + re/im], padded to a power of two
  constexpr int NV = bv_pow2(BV_RW * R * 2);
  constexpr int LANES_PER_VALUE = 64 / NV;
  for (int g = 0; g < d.groups; ++g) {
    const int rbase = it.row0 + (g * 4 + wave) * BV_RW;
    if (g > 0 && it.row0 + g * BV_DOT_ROWS >= d.M) break;   // (uniform over the workgroup; groups > 1 only with K <= BV_KC)
    const cplx* Ar[BV_RW];
#pragma unroll
    for (int i = 0; i < BV_RW; ++i) Ar[i] = d.A + (size_t)min(rbase + i, d.M - 1) * d.rsA;
    double v[NV];
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.0;
    for (int k0 = 0; k0 < d.K; k0 += BV_KC) {
      const int kc = min(BV_KC, d.K - k0);
      if (g == 0) {   // later passes re-use the one chunk there is
        __syncthreads();
        bv_stage_x<R>(xs, d, k0, kc, tid, sb);
        __syncthreads();
      }
      for (int kk = lane; kk < kc; kk += 64) {
        cplx a[BV_RW];
#pragma unroll
        for (int i = 0; i < BV_RW; ++i) {
          a[i] = dm_ldg(Ar[i], (size_t)(k0 + kk) * d.csA);
          a[i].y *= sa;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const cplx xv = xs[r * BV_KC + kk];
#pragma unroll
          for (int i = 0; i < BV_RW; ++i) {
            double& re = v[(i * R + r) * 2];
            double& im = v[(i * R + r) * 2 + 1];
            re = fma(a[i].x, xv.x, fma(-a[i].y, xv.y, re));
            im = fma(a[i].x, xv.y, fma(a[i].y, xv.x, im));
          }
        }
      }
    }
    bv_wave_reduce<NV, 32>(v, lane);
    const int idx = lane / LANES_PER_VALUE;
    if ((lane % LANES_PER_VALUE) == 0 && idx < BV_RW * R * 2) {
      const int i = idx / (2 * R), r = (idx >> 1) % R, c = idx & 1;
      const int row = rbase + i;
      if (row < d.M) dm_stg(reinterpret_cast<double*>(d.y), ((size_t)row * d.ldc + r) * 2 + c, v[0] * d.alpha);
    }
  }
}

// W[t, m] = exp(-2 pi i ((m t) mod ntime) / ntime) / ntime: the phase is reduced in integers, sincospi sees an exact
// multiple of 1 / ntime in [0, 2)
__global__ __launch_bounds__(256) void mmode_twiddle_kernel(int ntime, int nm, cplx* __restrict__ W) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)ntime * nm) return;
  const long long t = idx / nm, m = idx - t * nm;
  const long long q = (m * t) % ntime;
  double s_, c_;
  sincospi(2.0 * (double)q / (double)ntime, &s_, &c_);
  const double inv = 1.0 / (double)ntime;
  dm_stg(W, (size_t)idx, make_double2(c_ * inv, -s_ * inv));
}

template <int R>
void bv_launch(dm_ctx* ctx, size_t nitems, const bv_desc* dd, const bv_item* di) {
  hipLaunchKernelGGL((blockvec_kernel<R>), dim3((unsigned)nitems), dim3(256), 0, ctx->stream, dd, di);
}

}  // namespace

extern "C" {

int dm_blockvec_grouped(dm_ctx* ctx, int nprob, const dm_zgemm_problem* probs_host) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, nprob >= 0 && (nprob == 0 || probs_host != nullptr));
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws(ctx);
  std::vector<bv_desc> descs;
  std::vector<bv_item> items;
  int R = 0;
  double bytes = 0.0;
  for (int p = 0; p < nprob; ++p) {
    const dm_zgemm_problem& q = probs_host[p];
    DM_ARG(ctx, q.M >= 0 && q.K >= 0 && q.N >= 1 && q.N <= 8);
    DM_ARG(ctx, R == 0 || q.N == R);
    DM_ARG(ctx, q.beta == 0.0 && q.ldc >= q.N);
    R = q.N;
    if (q.M == 0 || q.K == 0) continue;   // skipped: nothing is written
    DM_ARG(ctx, q.A != nullptr && q.B != nullptr && q.C != nullptr);
    bv_desc d;
    d.A = static_cast<const cplx*>(q.A); d.x = static_cast<const cplx*>(q.B); d.y = static_cast<cplx*>(q.C);
    d.rsA = q.rsA; d.csA = q.csA; d.rsB = q.rsB; d.csB = q.csB; d.ldc = q.ldc;
    d.M = q.M; d.K = q.K; d.conjA = q.conjA != 0; d.conjB = q.conjB != 0;
    d.axpy = (q.rsA == 1 && q.csA != 1) ? 1 : 0;
    d.groups = (!d.axpy && q.K <= BV_KC) ? BV_DOT_GROUPS : 1;
    d.alpha = q.alpha;
    const int rows = d.axpy ? BV_AXPY_ROWS : BV_DOT_ROWS * d.groups;
    for (int r0 = 0; r0 < q.M; r0 += rows) items.push_back(bv_item{(int)descs.size(), r0});
    descs.push_back(d);
    bytes += 16.0 * (double)q.M * (double)q.K;
  }
  if (items.empty()) return DM_OK;
  const bv_desc* dd = dm_ws_upload(ctx, descs);
  const bv_item* di = dm_ws_upload(ctx, items);
  if (!dd || !di) return DM_ENOMEM;
  {
    dm_prof_scope ps(ctx, DM_PROF_BLOCKVEC, bytes);
    switch (R) {
      case 1: bv_launch<1>(ctx, items.size(), dd, di); break;
      case 2: bv_launch<2>(ctx, items.size(), dd, di); break;
      case 3: bv_launch<3>(ctx, items.size(), dd, di); break;
      case 4: bv_launch<4>(ctx, items.size(), dd, di); break;
      case 5: bv_launch<5>(ctx, items.size(), dd, di); break;
      case 6: bv_launch<6>(ctx, items.size(), dd, di); break;
      case 7: bv_launch<7>(ctx, items.size(), dd, di); break;
      default: bv_launch<8>(ctx, items.size(), dd, di); break;
    }
  }
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

int dm_mmode_twiddle(dm_ctx* ctx, int ntime, int mmax, void* W_dev) {
  if (!ctx) return DM_EARG;
  DM_ARG(ctx, ntime >= 1 && mmax >= 0 && W_dev != nullptr);
  DM_HIP(ctx, hipSetDevice(ctx->device));
  const long long n = (long long)ntime * (mmax + 1);
  DM_PLAUNCH(ctx, DM_PROF_UTIL, mmode_twiddle_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ntime,
             mmax + 1, static_cast<cplx*>(W_dev));
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

}  // extern "C"
