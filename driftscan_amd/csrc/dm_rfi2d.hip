// dm_rfi2d.hip — the two RFI steps beside dm_rfi_flag: dm_rfi_flag_freq, the method of section
// 4.20 with the series taken along frequency, and dm_rfi_dilate, the scale-invariant rank operator in exact integers
// along time or frequency.
//
// dm_rfi_flag_freq.  The series x[:, row, j] are strided by nrow nt, so a workgroup takes a tile of TJ consecutive j of
// one row and one frequency segment: it reads the tile frequency row by frequency row (TJ 16-byte samples, contiguous)
// and stages it transposed in LDS.  Up to 256 samples a wave works alone on its series: lane l owns the samples l,
// l + 64, ..., and every barrier of the method is wave-local (LDS operations of one wave complete in order).  Longer
// segments leave room for one workgroup per CU only, and the method waits on LDS most of the time, so W = 16 / TJ waves
// share a series and the barriers are the workgroup's: every series of the tile then walks through the same barriers,
// and one that runs out of samples computes on and is dropped at the end.  The arithmetic is that of rfi_row_kernel
// term by term: the background in ascending d with one FMA per component and term, the window sums in ascending k, the
// median as an exact radix select over the bytes of the amplitudes.  The outputs are therefore the bits dm_rfi_flag
// gives on a transposed copy.  The flags go back through LDS and leave as they came, TJ samples per frequency row.  TJ
// follows the segment length (35 bytes of LDS per sample and series).  Against rfi_row_kernel a select round has two
// barriers instead of three (two sets of counters used in turn) and a window pass one instead of two (the samples a
// pass flags carry the number of the pass, and count as flagged from the next pass on).
//
// dm_rfi_dilate.  psi_i = 0 (missing), 65536 - kappa (flagged) or -kappa (else); P the prefix sums; sample j is flagged
// iff max_{b > j} P_b >= min_{a <= j} P_a.  |P| <= 65536 n and n <= 16384, so 32-bit integers hold every sum.  Along
// time a workgroup takes one series: sample classes in LDS, a chunk of consecutive samples per thread, one block scan
// for the chunk carries, a forward walk that leaves the prefix minima in LDS and a backward walk that decides.  Along
// frequency lane = j: a forward walk over f leaves the prefix minimum and the class of every sample in a workspace
// word, the backward walk decides.  Both copy w to w_out on the way in and write zeros over the new flags only.
#include "dm_common.h"
#include "dm_feedpair.h"
#include "dm_rfi_table.h"
#include "dm_stack_table.h"
#include "../../include/driftmi.h"

#include <climits>

// No implicit contraction in this file (as dm_rfi.hip): the fused operations of the method are __builtin_fma.
#pragma clang fp contract(off)

#define DM_RFI_DILATE_MAX_TIME 16384
#define DM_RFI_DILATE_MAX_FREQ DM_RFI_MAX_SEGMENT
static_assert(65536ll * DM_RFI_DILATE_MAX_TIME < (1ll << 31) && 65536ll * DM_RFI_DILATE_MAX_FREQ < (1ll << 28),
              "32-bit prefix sums, and 4 P + class in a 32-bit word along frequency");

namespace {

constexpr int RF_MAX_W = 8, RF_MAX_THREADS = 1024, RF_THREADS = 256, RF_WAVES = RF_THREADS / 64;
constexpr int RD_FREQ_THREADS = 64;                 // one wave per workgroup: short rows still spread over the CUs
constexpr uint64_t RD_FREQ_WORDS = 128ull << 20;   // workspace words of one launch along frequency (512 MB)
constexpr size_t RF_LDS_BYTES = 160 * 1024;
constexpr int RF_ONE_WAVE = 256;

// the TJ of a longest segment of n samples; 0: no such segment
inline int rfi_freq_tile(int n) { return n < 1 || n > DM_RFI_MAX_SEGMENT ? 0 : n <= 512 ? 8 : n <= 1024 ? 4 : 2; }

// the waves that work on one series: one up to RF_ONE_WAVE samples (several workgroups then fit a CU), else as many as
// make a workgroup of RF_MAX_THREADS threads with the tile's series
inline uint32_t rfi_freq_waves(int n, int tj) { return n <= RF_ONE_WAVE || tj < 1 ? 1u : (uint32_t)(RF_MAX_THREADS / 64 / tj); }

// The LDS of a tile: per series ps samples (ps odd: the transposed stores of a frequency row fall into different banks).
struct rf_layout {
  uint32_t ps, tj, w;   // samples per series, series per tile, waves per series
  __host__ __device__ size_t xs() const { return 0; }
  __host__ __device__ size_t amp() const { return (size_t)16 * tj * ps; }
  __host__ __device__ size_t wv() const { return amp() + (size_t)8 * tj * ps; }
  __host__ __device__ size_t flags() const { return wv() + (size_t)8 * tj * ps; }
  __host__ __device__ size_t hist() const { return (flags() + (size_t)3 * tj * ps + 15) & ~(size_t)15; }
  __host__ __device__ size_t red() const { return hist() + (size_t)4 * 512 * tj; }
  __host__ __device__ size_t sel() const { return red() + (size_t)4 * RF_MAX_W * tj; }
  __host__ __device__ size_t bytes() const { return sel() + (size_t)4 * 2 * tj; }
};

// Wave-local barrier: the LDS operations of a wave complete in order, so keeping the compiler from moving accesses
// across this point is all that is needed.
__device__ __forceinline__ void rf_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ int rf_wave_sum(int v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

template <bool TEAM>
__device__ __forceinline__ void rf_sync() {
  if constexpr (TEAM)
    __syncthreads();
  else
    rf_wave_sync();
}

// the sum of v over the W waves of a series, to all of them; red holds RF_MAX_W ints of this series
template <bool TEAM>
__device__ __forceinline__ int rf_team_sum(int v, int* red, uint32_t lane, uint32_t tw, uint32_t W) {
  v = rf_wave_sum(v);
  if constexpr (!TEAM) return v;
  __syncthreads();   // red may still be read from the call before
  if (lane == 0) red[tw] = v;
  __syncthreads();
  int s = 0;
  for (uint32_t i = 0; i < W; ++i) s += red[i];
  return s;
}

// TEAM = false: one wave per series, every barrier wave-local, a series that runs out of samples stops.  TEAM = true:
// W waves per series and workgroup barriers, so every series of the tile walks through the same barriers: one that runs
// out of samples (or lies past nt) goes on computing and its results are dropped.
template <bool HAS_W, bool TEAM>
__global__ __launch_bounds__(RF_MAX_THREADS) void rfi_freq_kernel(const cplx* __restrict__ x, const double* w, double* w_out,
                                                                  double* __restrict__ noise, int* __restrict__ nflag,
                                                                  int* __restrict__ occ, int* __restrict__ nin_flagged,
                                                                  const dm_rfi_tables tb, uint32_t nf, uint32_t nrow,
                                                                  uint32_t nt, uint32_t nseg, uint32_t ntile,
                                                                  const rf_layout L) {
  extern __shared__ cplx rf_lds[];
  unsigned char* lds = reinterpret_cast<unsigned char*>(rf_lds);
  const uint32_t ps = L.ps, TJ = L.tj, W = TEAM ? L.w : 1u, T = 64 * W;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t tile = blockIdx.x % ntile, rest = blockIdx.x / ntile, row = rest % nrow, seg = rest / nrow;
  const uint32_t f0 = (uint32_t)(((uint64_t)seg * nf) / nseg), f1 = (uint32_t)(((uint64_t)(seg + 1) * nf) / nseg);
  const uint32_t n = f1 - f0;                                     // 1 <= n <= segment, n <= ps
  const uint32_t jt0 = tile * TJ;
  // ---- the tile comes in: thread = (frequency row fr, series tj), TJ samples of a frequency row are contiguous
  const uint32_t tj = tid % TJ, fr = tid / TJ;
  const bool mine_in = jt0 + tj < nt;
  {
    cplx* xs = reinterpret_cast<cplx*>(lds + L.xs()) + (size_t)tj * ps;
    double* ws = reinterpret_cast<double*>(lds + L.wv()) + (size_t)tj * ps;
    unsigned char* fI = lds + L.flags() + (size_t)tj * ps;
    unsigned char* fB = fI + (size_t)TJ * ps;
    unsigned char* fD = fB + (size_t)TJ * ps;
    for (uint32_t k = fr; k < n; k += T) {
      cplx v = make_double2(0.0, 0.0);
      bool ok = false;
      double wk = 0.0;
      if (mine_in) {   // a series past nt is staged as flagged throughout: TEAM walks through it, nothing leaves it
        const size_t idx = ((size_t)(f0 + k) * nrow + row) * nt + jt0 + tj;
        v = dm_ldg(x, idx);
        ok = true;
        wk = 1.0;
        if constexpr (HAS_W) {
          wk = dm_ldg(w, idx);
          ok = wk > 0.0;
        }
        if (!ok) v = make_double2(0.0, 0.0);
      }
      xs[k] = v;
      ws[k] = wk;
      fI[k] = ok ? 0 : 1;
      fB[k] = ok ? 0 : 1;
      fD[k] = ok ? 0 : 1;
    }
  }
  __syncthreads();
  // ---- W waves, one series
  const uint32_t team = wave / W, tw = wave % W, ts = tw * 64 + lane;
  const bool active = jt0 + team < nt;
  if (TEAM || active) {
    const cplx* xs = reinterpret_cast<const cplx*>(lds + L.xs()) + (size_t)team * ps;
    double* amp = reinterpret_cast<double*>(lds + L.amp()) + (size_t)team * ps;
    unsigned char* fI = lds + L.flags() + (size_t)team * ps;
    unsigned char* fB = fI + (size_t)TJ * ps;
    unsigned char* fD = fB + (size_t)TJ * ps;
    int* hist = reinterpret_cast<int*>(lds + L.hist()) + 512 * team;   // two sets of 256 counters, used in turn
    int* red = reinterpret_cast<int*>(lds + L.red()) + RF_MAX_W * team;
    int* sel = reinterpret_cast<int*>(lds + L.sel()) + 2 * team;
    const int H = tb.H;
    double med = 0.0;
    bool all_flagged = false;
    for (int it = 0; it < tb.niter; ++it) {
      // 1. the samples outside B
      int good = 0;
      for (uint32_t j = ts; j < n; j += T)
        if (!fB[j]) ++good;
      const int c = rf_team_sum<TEAM>(good, red, lane, tw, W);
      if (c < tb.min_good) {   // the same for the whole series
        all_flagged = true;
        if constexpr (!TEAM) break;
      }
      // 2. background and amplitude of every sample outside I; D restarts from I and the unjudgeable samples
      for (uint32_t j = ts; j < n; j += T) {
        double a = 0.0;
        unsigned char d = 1;
        if (!fI[j]) {
          double sx = 0.0, sy = 0.0, sg = 0.0;
          int used = 0;
          for (int dd = -H; dd <= H; ++dd) {
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
      for (uint32_t b = ts; b < 512; b += T) hist[b] = 0;
      rf_sync<TEAM>();
      // 3. the lower median of the amplitudes outside B: rank (c - 1) / 2 of c, by bytes from the most significant
      {
        unsigned long long prefix = 0;
        int rank = (c - 1) / 2;
        for (int p = 7; p >= 0; --p) {
          int* h = hist + 256 * (p & 1);   // zeroed: before the loop, or during the pass before the last one
          for (uint32_t j = ts; j < n; j += T)
            if (!fB[j]) {
              const unsigned long long key = (unsigned long long)__double_as_longlong(amp[j]);
              if (p == 7 || (key >> (8 * (p + 1))) == prefix) atomicAdd(&h[(key >> (8 * p)) & 255ull], 1);
            }
          rf_sync<TEAM>();
          if (tw == 0) {   // the first wave of the series scans the 256 counters, four to a lane, and zeroes them
            int v[4], s = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              v[b] = h[4 * lane + b];
              h[4 * lane + b] = 0;
              s += v[b];
            }
            int incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
              const int t = __shfl_up(incl, o, 64);
              if ((int)lane >= o) incl += t;
            }
            int e = incl - s;
#pragma unroll
            for (int b = 0; b < 4; ++b) {
              if (v[b] > 0 && e <= rank && rank < e + v[b]) {   // exactly one counter of one lane
                sel[0] = 4 * (int)lane + b;
                sel[1] = rank - e;
              }
              e += v[b];
            }
          }
          rf_sync<TEAM>();   // sel is read here and written again only behind the next barrier
          prefix = (prefix << 8) | (unsigned long long)(sel[0] & 255);
          rank = sel[1];
        }
        med = __longlong_as_double((long long)prefix);
      }
      // 4. the window passes, each against D as it stood at the start of the pass
      for (int i = 0; i < tb.nwin; ++i) {
        const uint32_t M = (uint32_t)tb.window[i];
        if (M > n) break;
        const double thr = med * tb.t[it][i];
        // a sample that pass i' flags is marked 2 + i': in D for every later pass, outside D for the rest of its own
        const unsigned char mark = (unsigned char)(2 + i);
        for (uint32_t j = ts; j + M <= n; j += T) {
          int cnt = 0;
          double S = 0.0;
          for (uint32_t k = j; k < j + M; ++k) {
            const unsigned char d = fD[k];
            if (d == 0 || d == mark) {
              ++cnt;
              S += amp[k];
            }
          }
          if (cnt >= 1 && S > (double)cnt * thr)
            for (uint32_t k = j; k < j + M; ++k)
              if (fD[k] == 0) fD[k] = mark;
        }
        rf_sync<TEAM>();
      }
      // 5. B of the next iteration
      for (uint32_t j = ts; j < n; j += T) fB[j] = fD[j] != 0 ? 1 : 0;
      rf_sync<TEAM>();
    }
    int fresh = 0;
    for (uint32_t j = ts; j < n; j += T) {
      const bool flagged = all_flagged || fB[j] != 0;
      fB[j] = flagged ? 1 : 0;
      if (flagged && !fI[j]) ++fresh;
    }
    fresh = rf_team_sum<TEAM>(fresh, red, lane, tw, W);
    if (ts == 0 && active) {
      if (fresh > 0) atomicAdd(&nflag[(size_t)row * nt + jt0 + team], fresh);
      dm_stg(noise, ((size_t)seg * nrow + row) * nt + jt0 + team, all_flagged ? 0.0 : med / DM_RFI_SQRT_LN2);
    }
  }
  __syncthreads();
  // ---- the tile leaves as it came
  if (mine_in) {
    const double* ws = reinterpret_cast<const double*>(lds + L.wv()) + (size_t)tj * ps;
    const unsigned char* fI = lds + L.flags() + (size_t)tj * ps;
    const unsigned char* fB = fI + (size_t)TJ * ps;
    for (uint32_t k = fr; k < n; k += T) {
      const size_t idx = ((size_t)(f0 + k) * nrow + row) * nt + jt0 + tj, col = (size_t)(f0 + k) * nt + jt0 + tj;
      const bool in = fI[k] != 0, flagged = fB[k] != 0;
      dm_stg(w_out, idx, flagged ? 0.0 : ws[k]);
      if (in) atomicAdd(&nin_flagged[col], 1);
      if (flagged && !in) atomicAdd(&occ[col], 1);
    }
  }
}

// lane = sample (as the column kernel of dm_rfi.hip): a column (f, j) with n_new > row_share n_in is flagged in the rows
// r0 .. r1 - 1 of this workgroup
__global__ __launch_bounds__(RF_THREADS) void rfi2d_occupancy_kernel(double* __restrict__ w_out, const int* __restrict__ occ,
                                                                     const int* __restrict__ nin_flagged, uint32_t nrow,
                                                                     uint32_t nt, uint32_t rows_per, double row_share) {
  const uint32_t j = blockIdx.x * RF_THREADS + threadIdx.x, f = blockIdx.y;
  if (j >= nt) return;
  const int n_in = (int)nrow - nin_flagged[(size_t)f * nt + j], n_new = occ[(size_t)f * nt + j];
  if (!(n_in > 0 && (double)n_new > row_share * (double)n_in)) return;
  const uint32_t r0 = blockIdx.z * rows_per, r1 = r0 + rows_per < nrow ? r0 + rows_per : nrow;
  for (uint32_t r = r0; r < r1; ++r) dm_stg(w_out, ((size_t)f * nrow + r) * nt + j, 0.0);
}

// ---- dilation --------------------------------------------------------------------------------------------------------
// the class of a sample: 0 missing, 1 flagged, 2 neither
__device__ __forceinline__ int rd_class(const double* w, const double* ref, size_t idx) {
  if (ref && !(dm_ldg(ref, idx) > 0.0)) return 0;
  return dm_ldg(w, idx) > 0.0 ? 2 : 1;
}
__device__ __forceinline__ int rd_psi(int cls, int kappa) { return cls == 0 ? 0 : cls == 1 ? 65536 - kappa : -kappa; }

// One workgroup, one contiguous series of n <= DM_RFI_DILATE_MAX_TIME samples; thread t owns the chunk [t C, (t + 1) C),
// C odd (its walks through the 32-bit minima then fall into different banks).
__global__ __launch_bounds__(RF_THREADS) void rfi_dilate_time_kernel(const double* w, const double* __restrict__ ref,
                                                                     double* w_out, int* __restrict__ nadded, uint32_t n,
                                                                     uint32_t C, int kappa) {
  extern __shared__ cplx rf_lds[];
  int* pmin = reinterpret_cast<int*>(rf_lds);                               // [RF_THREADS C]
  unsigned char* cls = reinterpret_cast<unsigned char*>(pmin + RF_THREADS * C);   // [RF_THREADS C]
  __shared__ int carry[3][RF_WAVES];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const size_t base = (size_t)blockIdx.x * n;
  const bool copy = w_out != w;
  for (uint32_t j = tid; j < n; j += RF_THREADS) {
    cls[j] = (unsigned char)rd_class(w, ref, base + j);
    if (copy) dm_stg(w_out, base + j, dm_ldg(w, base + j));
  }
  __syncthreads();
  const uint32_t j0 = tid * C < n ? tid * C : n, j1 = j0 + C < n ? j0 + C : n;
  // the chunk alone, relative to its start: sum, min of P_a (a in the chunk), max of P_b (b - 1 in the chunk)
  int sum = 0, cmin = INT_MAX, cmax = INT_MIN;
  for (uint32_t j = j0; j < j1; ++j) {
    cmin = sum < cmin ? sum : cmin;
    sum += rd_psi(cls[j], kappa);
    cmax = sum > cmax ? sum : cmax;
  }
  // P at the start of every chunk
  int incl = sum;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(incl, o, 64);
    if ((int)lane >= o) incl += t;
  }
  if (lane == 63) carry[0][wave] = incl;
  __syncthreads();
  int start = incl - sum;
  for (uint32_t i = 0; i < wave; ++i) start += carry[0][i];
  // the minimum of P over the chunks before, the maximum over the chunks after
  const bool some = j1 > j0;
  int lo = some ? start + cmin : INT_MAX, hi = some ? start + cmax : INT_MIN;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int a = __shfl_up(lo, o, 64), b = __shfl_down(hi, o, 64);
    if ((int)lane >= o) lo = a < lo ? a : lo;
    if ((int)lane + o < 64) hi = b > hi ? b : hi;
  }
  if (lane == 63) carry[1][wave] = lo;
  if (lane == 0) carry[2][wave] = hi;
  int before = __shfl_up(lo, 1, 64), after = __shfl_down(hi, 1, 64);
  if (lane == 0) before = INT_MAX;
  if (lane == 63) after = INT_MIN;
  __syncthreads();
  for (uint32_t i = 0; i < RF_WAVES; ++i) {
    if (i < wave) before = carry[1][i] < before ? carry[1][i] : before;
    if (i > wave) after = carry[2][i] > after ? carry[2][i] : after;
  }
  // forward: min_{a <= j} P_a; backward: max_{b > j} P_b and the decision
  int p = start, run = before;
  for (uint32_t j = j0; j < j1; ++j) {
    run = p < run ? p : run;
    pmin[j] = run;
    p += rd_psi(cls[j], kappa);
  }
  int added = 0;
  run = after;
  for (uint32_t j = j1; j > j0; --j) {
    run = p > run ? p : run;   // p = P_j, the prefix sum behind sample j - 1
    const int c = cls[j - 1];
    if (c == 2 && run >= pmin[j - 1]) {
      cls[j - 1] = 3;   // newly flagged
      ++added;
    }
    p -= rd_psi(c, kappa);
  }
  added = rf_wave_sum(added);
  __syncthreads();   // carry[0] is read no more
  if (lane == 0) carry[0][wave] = added;
  // the zeros go out through the threads that copied these samples
  for (uint32_t j = tid; j < n; j += RF_THREADS)
    if (cls[j] == 3) dm_stg(w_out, base + j, 0.0);
  __syncthreads();
  if (tid == 0) {
    int s = 0;
    for (int i = 0; i < RF_WAVES; ++i) s += carry[0][i];
    nadded[blockIdx.x] = s;
  }
}

// lane = j, a walk over the nf samples of the series (row r0 + blockIdx.y, j); word (f, blockIdx.y, j) of `scratch` keeps
// 4 min_{a <= f} P_a + class between the two walks.
__global__ __launch_bounds__(RD_FREQ_THREADS) void rfi_dilate_freq_kernel(const double* w, const double* __restrict__ ref,
                                                                     double* w_out, int* __restrict__ nadded,
                                                                     int* __restrict__ scratch, uint32_t nf, uint32_t nrow,
                                                                     uint32_t nt, uint32_t r0, uint32_t rows, int kappa) {
  const uint32_t j = blockIdx.x * RD_FREQ_THREADS + threadIdx.x, rb = blockIdx.y, row = r0 + rb;
  if (j >= nt) return;
  const bool copy = w_out != w;
  int p = 0, run = INT_MAX;
#pragma unroll 4
  for (uint32_t f = 0; f < nf; ++f) {
    const size_t idx = ((size_t)f * nrow + row) * nt + j;
    const int c = rd_class(w, ref, idx);
    if (copy) dm_stg(w_out, idx, dm_ldg(w, idx));
    run = p < run ? p : run;
    scratch[((size_t)f * rows + rb) * nt + j] = run * 4 + c;
    p += rd_psi(c, kappa);
  }
  int added = 0;
  run = INT_MIN;
#pragma unroll 4
  for (uint32_t f = nf; f > 0; --f) {
    run = p > run ? p : run;   // p = P_f
    const int word = scratch[((size_t)(f - 1) * rows + rb) * nt + j], c = word & 3, lo = (word - c) / 4;
    if (c == 2 && run >= lo) {
      dm_stg(w_out, ((size_t)(f - 1) * nrow + row) * nt + j, 0.0);
      ++added;
    }
    p -= rd_psi(c, kappa);
  }
  nadded[(size_t)row * nt + j] = added;
}

}  // namespace

extern "C" int dm_rfi_freq_tile(int segment_len) { return rfi_freq_tile(segment_len); }

extern "C" int dm_rfi_flag_freq(dm_ctx* ctx, int nf, int nrow, int nt, int segment, double kernel_sigma, int nwin,
                                const int* windows_host, double chi1, double rho, int niter, double base, int min_good,
                                double row_share, const void* x_dev, const double* w_dev, double* wout_dev,
                                double* noise_dev, int* nflag_dev, int* occupancy_dev) {
  static const char* who = "dm_rfi_flag_freq";
  if (!ctx) return DM_EARG;
  if (nf < 0 || nrow < 0 || nt < 0) return dm_refuse(ctx, who, "negative size");
  const std::string bad = dm_rfi_check(nf, segment, kernel_sigma, nwin, windows_host, chi1, rho, niter, base, min_good, row_share);
  if (!bad.empty()) return dm_refuse(ctx, who, bad);
  const uint64_t nel = (uint64_t)nf * nrow * nt;
  if (nel == 0) return DM_OK;
  const uint32_t nseg = (uint32_t)(((int64_t)nf + segment - 1) / segment);
  if (!x_dev || !wout_dev || !noise_dev || !nflag_dev || !occupancy_dev)
    return dm_refuse(ctx, who, "null x, w_out, noise, nflag or occupancy with work to do");
  {
    const uint64_t ip[2] = {(uint64_t)x_dev, (uint64_t)w_dev}, ib[2] = {16 * nel, w_dev ? 8 * nel : 0};
    const uint64_t op[4] = {(uint64_t)wout_dev, (uint64_t)noise_dev, (uint64_t)nflag_dev, (uint64_t)occupancy_dev};
    const uint64_t ob[4] = {8 * nel, 8 * (uint64_t)nseg * nrow * nt, 4 * (uint64_t)nrow * nt, 4 * (uint64_t)nf * nt};
    for (int o = 0; o < 4; ++o) {
      for (int i = 0; i < 2; ++i) {
        if (o == 0 && i == 1 && op[o] == ip[i]) continue;   // w_out may be w itself
        if (dm_spans_overlap(ip[i], ib[i], 0, op[o], ob[o], 0, 1))
          return dm_refuse(ctx, who, "an output shares an element with x or w (w_out may be w itself)");
      }
      for (int p = 0; p < o; ++p)
        if (dm_spans_overlap(op[p], ob[p], 0, op[o], ob[o], 0, 1)) return dm_refuse(ctx, who, "two outputs share an element");
    }
  }
  const uint32_t longest = (uint32_t)(((int64_t)nf + nseg - 1) / nseg);   // of the balanced segments, <= segment
  rf_layout L;
  L.tj = (uint32_t)rfi_freq_tile((int)longest);
  L.ps = longest | 1u;
  L.w = rfi_freq_waves((int)longest, (int)L.tj);
  const size_t lds = L.bytes();
  if (L.tj == 0 || lds > RF_LDS_BYTES) return dm_refuse(ctx, who, "no tile for this segment length");
  const uint32_t ntile = ((uint32_t)nt + L.tj - 1) / L.tj;
  const uint64_t nblocks = (uint64_t)nseg * nrow * ntile;
  if (nblocks >= (1ull << 31) || nf > 65535) return dm_refuse(ctx, who, "too many workgroups for one launch");
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_rfi_tables tb;
  dm_rfi_make_tables(kernel_sigma, nwin, windows_host, chi1, rho, niter, base, min_good, &tb);
  dm_ws_scope ws(ctx);
  int* nin_flagged = dm_ws_alloc_t<int>(ctx, (size_t)nf * nt);
  if (!nin_flagged) return DM_ENOMEM;
  DM_HIP(ctx, hipMemsetAsync(nin_flagged, 0, 4 * (size_t)nf * nt, ctx->stream));
  DM_HIP(ctx, hipMemsetAsync(occupancy_dev, 0, 4 * (size_t)nf * nt, ctx->stream));
  DM_HIP(ctx, hipMemsetAsync(nflag_dev, 0, 4 * (size_t)nrow * nt, ctx->stream));
  const cplx* x = static_cast<const cplx*>(x_dev);
  const dim3 grid((unsigned)nblocks), block(64 * L.tj * L.w);
#define RF_LAUNCH(HAS_W, TEAM)                                                                                              \
  do {                                                                                                                      \
    if (int rc = dm_lds_attr(ctx, rfi_freq_kernel<HAS_W, TEAM>, lds)) return rc;                                            \
    DM_PLAUNCH(ctx, DM_PROF_UTIL, (rfi_freq_kernel<HAS_W, TEAM>), grid, block, lds, ctx->stream, x, w_dev, wout_dev,        \
               noise_dev, nflag_dev, occupancy_dev, nin_flagged, tb, (uint32_t)nf, (uint32_t)nrow, (uint32_t)nt, nseg,      \
               ntile, L);                                                                                                   \
  } while (0)
  if (L.w > 1) {
    if (w_dev)
      RF_LAUNCH(true, true);
    else
      RF_LAUNCH(false, true);
  } else {
    if (w_dev)
      RF_LAUNCH(true, false);
    else
      RF_LAUNCH(false, false);
  }
#undef RF_LAUNCH
  DM_HIP(ctx, hipGetLastError());
  if (row_share < 1.0) {
    uint32_t rows_per = 256, nz = ((uint32_t)nrow + rows_per - 1) / rows_per;
    if (nz > 65535u) {
      nz = 65535u;
      rows_per = ((uint32_t)nrow + nz - 1) / nz;
      nz = ((uint32_t)nrow + rows_per - 1) / rows_per;
    }
    DM_PLAUNCH(ctx, DM_PROF_UTIL, rfi2d_occupancy_kernel, dim3(((unsigned)nt + RF_THREADS - 1) / RF_THREADS, (unsigned)nf, nz),
               dim3(RF_THREADS), 0, ctx->stream, wout_dev, occupancy_dev, nin_flagged, (uint32_t)nrow, (uint32_t)nt, rows_per,
               row_share);
    DM_HIP(ctx, hipGetLastError());
  }
  return DM_OK;
}

extern "C" int dm_rfi_dilate_max_length(int axis) {
  return axis == 0 ? DM_RFI_DILATE_MAX_TIME : axis == 1 ? DM_RFI_DILATE_MAX_FREQ : 0;
}

extern "C" int dm_rfi_dilate(dm_ctx* ctx, int nf, int nrow, int nt, int axis, double eta, const double* w_dev,
                             const double* wref_dev, double* wout_dev, int* nadded_dev) {
  static const char* who = "dm_rfi_dilate";
  if (!ctx) return DM_EARG;
  if (nf < 0 || nrow < 0 || nt < 0) return dm_refuse(ctx, who, "negative size");
  if (axis != 0 && axis != 1) return dm_refuse(ctx, who, "axis is 0 (time) or 1 (frequency)");
  if (!std::isfinite(eta) || !(eta >= 0.0 && eta < 1.0)) return dm_refuse(ctx, who, "eta not finite or outside [0, 1)");
  const double kd = std::rint((1.0 - eta) * 65536.0);
  if (kd < 1.0) return dm_refuse(ctx, who, "kappa = rint((1 - eta) 65536) < 1");
  const int kappa = (int)kd;
  const int len = axis == 0 ? nt : nf;
  if (len > dm_rfi_dilate_max_length(axis))
    return dm_refuse(ctx, who, "series longer than " + std::to_string(dm_rfi_dilate_max_length(axis)));
  const uint64_t nel = (uint64_t)nf * nrow * nt;
  if (nel == 0) return DM_OK;
  if (!w_dev || !wout_dev || !nadded_dev) return dm_refuse(ctx, who, "null w, w_out or nadded with work to do");
  {
    const uint64_t nser = axis == 0 ? (uint64_t)nf * nrow : (uint64_t)nrow * nt;
    const uint64_t ip[2] = {(uint64_t)w_dev, (uint64_t)wref_dev}, ib[2] = {8 * nel, wref_dev ? 8 * nel : 0};
    const uint64_t op[2] = {(uint64_t)wout_dev, (uint64_t)nadded_dev}, ob[2] = {8 * nel, 4 * nser};
    for (int o = 0; o < 2; ++o)
      for (int i = 0; i < 2; ++i) {
        if (o == 0 && i == 0 && op[o] == ip[i]) continue;   // w_out may be w itself
        if (dm_spans_overlap(ip[i], ib[i], 0, op[o], ob[o], 0, 1))
          return dm_refuse(ctx, who, "an output shares an element with w or w_ref (w_out may be w itself)");
      }
    if (dm_spans_overlap(op[0], ob[0], 0, op[1], ob[1], 0, 1)) return dm_refuse(ctx, who, "two outputs share an element");
  }
  DM_HIP(ctx, hipSetDevice(ctx->device));
  if (axis == 0) {
    const uint64_t nser = (uint64_t)nf * nrow;
    if (nser >= (1ull << 31)) return dm_refuse(ctx, who, "too many workgroups for one launch");
    const uint32_t C = (((uint32_t)nt + RF_THREADS - 1) / RF_THREADS) | 1u;
    const size_t lds = (size_t)RF_THREADS * C * 5;
    if (int rc = dm_lds_attr(ctx, rfi_dilate_time_kernel, lds)) return rc;
    DM_PLAUNCH(ctx, DM_PROF_UTIL, rfi_dilate_time_kernel, dim3((unsigned)nser), dim3(RF_THREADS), lds, ctx->stream, w_dev,
               wref_dev, wout_dev, nadded_dev, (uint32_t)nt, C, kappa);
    DM_HIP(ctx, hipGetLastError());
    return DM_OK;
  }
  // along frequency: rows in batches that bound the workspace
  const uint64_t per_row = (uint64_t)nf * nt;
  uint64_t rows = RD_FREQ_WORDS / per_row;
  rows = rows < 1 ? 1 : rows > 65535 ? 65535 : rows;
  if (rows > (uint64_t)nrow) rows = (uint64_t)nrow;
  dm_ws_scope ws(ctx);
  int* scratch = dm_ws_alloc_t<int>(ctx, (size_t)(per_row * rows));
  if (!scratch) return DM_ENOMEM;
  for (uint64_t r0 = 0; r0 < (uint64_t)nrow; r0 += rows) {
    const uint32_t nr = (uint32_t)((uint64_t)nrow - r0 < rows ? (uint64_t)nrow - r0 : rows);
    DM_PLAUNCH(ctx, DM_PROF_UTIL, rfi_dilate_freq_kernel, dim3(((unsigned)nt + RD_FREQ_THREADS - 1) / RD_FREQ_THREADS, nr),
               dim3(RD_FREQ_THREADS), 0, ctx->stream, w_dev, wref_dev, wout_dev, nadded_dev, scratch, (uint32_t)nf, (uint32_t)nrow, (uint32_t)nt,
               (uint32_t)r0, (uint32_t)rows, kappa);
    DM_HIP(ctx, hipGetLastError());
  }
  return DM_OK;
}
