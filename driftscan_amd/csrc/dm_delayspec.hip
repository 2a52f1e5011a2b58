// dm_delayspec.hip — dm_delay_spectrum, the delay power spectrum of stacked visibilities with its window function
// (DESIGN.md section 4.27).  No counterpart in the reference.
//
// For row r, sample t, frequency f, delay a = 0 .. nd - 1 and lag d = 0 .. nd - 1:
//   kept_f(t) = w_f(t) > 0,   omega_f = 1 (weighting 0) or w_f (weighting 1) where kept and 0 elsewhere,   y_f = T_f omega_f,
//   phi_fk = step_f k  (one rounded product),   (S, C)_fk = sincospi(2 (phi_fk - rint(phi_fk)))  (the reduction is exact),
//   D_a(t) = sum_f y_f x_f (C + i S)_f,(a - a0),   W_d(t) = sum_f y_f (C + i S)_f,d,
//   q[r, b, a] = sum_t |D_a(t)|^2,   h[r, b, d] = sum_t |W_d(t)|^2,   s1 = sum_t sum_f T_f y_f,   s2 = sum_t sum_f y_f y_f,
// the sums over t over the used series of bin b: those of its samples with at least min_valid kept channels.
//
// Two real products with K = nf on v_mfma_f64_16x16x4_f64: rows are delays (lags), columns samples.  One workgroup of
// eight waves takes one row, one segment of a bin and DS_ND = 128 delays; wave w owns the 16 delays e0 + 16 w.  The
// segment is walked in tiles of DS_TT = 64 samples, each tile through the frequencies in chunks of DS_KC = 16: the chunk
// is staged in LDS as the planes Re (y x), Im (y x) and y (the weighting and the taper happen on the way in: no weighted
// copy exists in memory), the next chunk's samples are in flight in registers meanwhile, each lane produces the cos /
// sin of its own A elements (frequency kq = lane >> 4 of each group of four, delay lane & 15) once per chunk, and every
// accumulator takes its MFMAs of the chunk back to back.  After the last chunk of a tile the squared magnitudes of the
// accumulators are added to per-lane sums and the accumulators start again from 0: the transformed cube never exists.
//
// The fixed orders, functions of nf and of the bin's sample range [b0, b1) alone:
//   * D_a(t) and W_d(t) are one accumulator each for the real and the imaginary part, walked through the frequencies in
//     ascending order four at a time (per four: the cos product, then the sin product) from f = 0; an nf that is no
//     multiple of four ends with frequencies of weight 0.
//   * A bin of L = b1 - b0 samples is cut into n = min(DS_SEGS, ceil(L / DS_SEG_MIN)) segments of
//     DS_TT ceil(ceil(L / n) / DS_TT) samples from b0 on (the last one short).  Within a segment that starts at s0, lane
//     column j = 0 .. 15 sums |.|^2 = re re + im im (two rounded products, one sum) of the samples s0 + j, s0 + j + 16, ...
//     in ascending order (dropped series and samples past the end add +0); the 16 columns are then combined by the
//     butterfly (j ^ 8, j ^ 4, j ^ 2, j ^ 1).  A bin of one segment is written straight to the outputs; the partial sums
//     of the others go to scratch memory (n (2 nd + 2) doubles per row, n <= DS_SEGS) and a second kernel adds them in
//     ascending segment order.
//   * s1 and s2: column j = 0 .. 63 of a segment sums its samples s0 + j, s0 + j + 64, ... each over ascending f, the 64
//     columns are combined by the butterfly (32, 16, 8, 4, 2, 1), the segments as above.
// The bits of (row, bin, .) therefore depend on nothing else in the launch: not on the other rows or bins, not on nd or
// the delay block (so a launch with a smaller nd gives a prefix of h, and of q when a0 is the same), not on which of h,
// s1, s2 and count are null.  No phase table, no atomics.
#include "dm_common.h"
#include "dm_feedpair.h"
#include "dm_stack_table.h"
#include "../../include/driftmi.h"

#include <cmath>

// No implicit contraction in this file: phi, y and y x are rounded products, and so are the squares of the epilogue.
#pragma clang fp contract(off)

namespace {

constexpr int DS_TT = 64;             // samples of a staged tile
constexpr int DS_ND = 128;            // delays of a workgroup: 16 per wave
constexpr int DS_KC = 16;             // frequencies of a staged chunk
constexpr int DS_XS = DS_TT + 16;     // row pitch of a staged plane: the two frequency rows of a 32-lane ds_read_b64 group
                                      // fall 32 banks apart
constexpr int DS_THREADS = 512;
constexpr int DS_SI = DS_KC / (DS_THREADS / DS_TT);   // frequencies a thread stages per chunk
constexpr int DS_SEG_MIN = 128;       // a bin is split only into segments of at least this many samples
constexpr int DS_SEGS = 4;            // and into at most this many
constexpr int DS_MAX_NF = 16384;
constexpr int DS_MAX_ND = 2048;       // step_f k is exact in a 64-bit significand for |k| < 2^11

struct ds_seg {
  int t0, t1;   // the samples of the segment
  int bin;
  int slot;     // of the partial sums in scratch memory, or -1: the segment is its bin and goes to the outputs
};

struct ds_bin {
  int slot0, nseg;
};

struct ds_args {
  const cplx* x;
  const double* w;              // or null
  const double* taper;          // or null
  const double* step;
  const unsigned char* valid;   // (nrow, nt): the series is used; null: every series is
  const ds_seg* segs;
  const ds_bin* bins;
  double *q, *h, *s1, *s2;      // h, s1, s2 or null
  int* count;                   // or null
  double *pq, *ph, *ps1, *ps2;  // the partial sums: (nslot, nrow, nd) and (nslot, nrow)
  int* pcount;
  uint32_t nf, nrow, nt, nd, nbin, nseg, ndb;
  int a0, weighting, min_valid;
};

// valid[row, t] = the series has at least min_valid kept channels
__global__ __launch_bounds__(256) void delayspec_valid_kernel(const ds_args a, unsigned char* valid) {
  const uint32_t t = blockIdx.x * 256u + threadIdx.x, row = blockIdx.y;
  if (t >= a.nt) return;
  int n = 0;
  for (uint32_t f = 0; f < a.nf; ++f) n += dm_ldg(a.w, ((size_t)f * a.nrow + row) * a.nt + t) > 0.0 ? 1 : 0;
  valid[(size_t)row * a.nt + t] = n >= a.min_valid ? 1 : 0;
}

template <bool WIN>
__global__ __launch_bounds__(DS_THREADS) void delayspec_kernel(const ds_args a) {
  __shared__ double xr[DS_KC * DS_XS], xi[DS_KC * DS_XS], xy[DS_KC * DS_XS];
  __shared__ double sk[DS_KC], tk[DS_KC];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t r = (uint32_t)dm_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const uint32_t db = r % a.ndb;   // the delay blocks of one (row, segment) are neighbours: they stage the same samples
  r /= a.ndb;
  const uint32_t si = r % a.nseg, row = r / a.nseg;
  const ds_seg seg = a.segs[si];
  const uint32_t t0 = (uint32_t)seg.t0, t1 = (uint32_t)seg.t1;
  const uint32_t e0 = db * DS_ND + wave * 16;
  const uint32_t cj = lane & 15u, kq = lane >> 4;
  const bool wave_on = e0 < a.nd;                                    // uniform in the wave
  const double ka = (double)((int)(e0 + cj) - a.a0), kw = (double)(e0 + cj);
  const uint32_t nkc = (a.nf + DS_KC - 1) / DS_KC, ntile = (t1 - t0 + DS_TT - 1) / DS_TT, nit = nkc * ntile;
  // staging: thread = (sample st, frequencies sf + 8 i of the chunk)
  const uint32_t st = tid & (DS_TT - 1), sf = tid / DS_TT;
  cplx pv[DS_SI];
  double pw[DS_SI];
  typedef const unsigned char __attribute__((address_space(1)))* gbyte_c;   // a global load, as dm_ldg
  auto used = [&](uint32_t t) { return t < t1 && (!a.valid || ((gbyte_c)a.valid)[(size_t)row * a.nt + t] != 0); };
  auto fetch = [&](uint32_t it) {
    const uint32_t tile = it / nkc, kc = (it - tile * nkc) * DS_KC;
    const uint32_t t = t0 + tile * DS_TT + st;
    const bool on = used(t);
#pragma unroll
    for (int i = 0; i < DS_SI; ++i) {
      const uint32_t f = kc + sf + (uint32_t)(DS_THREADS / DS_TT) * i;
      pv[i] = make_double2(0.0, 0.0);
      pw[i] = 0.0;   // a frequency past nf, a sample past the segment and a dropped series are staged as not kept
      if (f < a.nf && on) {
        const size_t idx = ((size_t)f * a.nrow + row) * a.nt + t;
        pw[i] = a.w ? dm_ldg(a.w, idx) : 1.0;
        pv[i] = dm_ldg(a.x, idx);
      }
    }
  };
  dm_f64x4 are[DS_TT / 16], aim[DS_TT / 16], wre[DS_TT / 16], wim[DS_TT / 16];
  const dm_f64x4 zero4 = dm_f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int tt = 0; tt < DS_TT / 16; ++tt) are[tt] = aim[tt] = wre[tt] = wim[tt] = zero4;
  dm_f64x4 P = zero4, H = zero4;
  double S1 = 0.0, S2 = 0.0;
  int cnt = 0;
  fetch(0);
  for (uint32_t it = 0; it < nit; ++it) {
    const uint32_t tile = it / nkc, kci = it - tile * nkc, kc = kci * DS_KC;
    __syncthreads();   // the chunk before is read no more
#pragma unroll
    for (int i = 0; i < DS_SI; ++i) {
      const uint32_t k = sf + (uint32_t)(DS_THREADS / DS_TT) * i, f = kc + k;
      const double tf = f < a.nf ? (a.taper ? dm_ldg(a.taper, f) : 1.0) : 0.0;
      const bool kept = pw[i] > 0.0;   // false for 0, negatives and NaN
      const double y = kept ? (a.weighting ? tf * pw[i] : tf) : 0.0;
      xr[k * DS_XS + st] = kept ? y * pv[i].x : 0.0;
      xi[k * DS_XS + st] = kept ? y * pv[i].y : 0.0;
      xy[k * DS_XS + st] = y;
    }
    if (tid < (uint32_t)DS_KC) {
      const uint32_t f = kc + tid;
      sk[tid] = f < a.nf ? dm_ldg(a.step, f) : 0.0;
      tk[tid] = f < a.nf ? (a.taper ? dm_ldg(a.taper, f) : 1.0) : 0.0;
    }
    __syncthreads();
    if (it + 1 < nit) fetch(it + 1);   // in flight behind the MFMAs of this chunk
    const uint32_t nk = a.nf - kc < (uint32_t)DS_KC ? a.nf - kc : (uint32_t)DS_KC, nq = (nk + 3) / 4;
    if (db == 0 && tid < (uint32_t)DS_TT) {
      if (kci == 0 && used(t0 + tile * DS_TT + tid)) ++cnt;
      for (uint32_t k = 0; k < nk; ++k) {
        const double y = xy[k * DS_XS + tid];
        S1 += tk[k] * y;
        S2 += y * y;
      }
    }
    if (wave_on) {
      const uint32_t tleft = t1 - (t0 + tile * DS_TT), ntt = tleft >= (uint32_t)DS_TT ? DS_TT / 16 : (tleft + 15) / 16;
      double cs[DS_KC / 4], sn[DS_KC / 4], cw[DS_KC / 4], sw[DS_KC / 4];
#pragma unroll
      for (int q = 0; q < DS_KC / 4; ++q) {
        const double s = sk[4 * q + kq];
        const double pa = s * ka;
        sincospi(2.0 * (pa - rint(pa)), &sn[q], &cs[q]);   // exact: |phi - rint(phi)| <= 1/2
        if constexpr (WIN) {
          const double pl = s * kw;
          sincospi(2.0 * (pl - rint(pl)), &sw[q], &cw[q]);
        }
      }
#pragma unroll
      for (int tt = 0; tt < DS_TT / 16; ++tt) {
        if ((uint32_t)tt < ntt) {
          double br[DS_KC / 4], bi[DS_KC / 4], by[DS_KC / 4];
#pragma unroll
          for (int q = 0; q < DS_KC / 4; ++q) {
            br[q] = xr[(4 * q + kq) * DS_XS + tt * 16 + cj];
            bi[q] = xi[(4 * q + kq) * DS_XS + tt * 16 + cj];
            if constexpr (WIN) by[q] = xy[(4 * q + kq) * DS_XS + tt * 16 + cj];
          }
#pragma unroll
          for (int q = 0; q < DS_KC / 4; ++q) {
            if ((uint32_t)q < nq) {
              are[tt] = dm_mfma(cs[q], br[q], are[tt]);
              are[tt] = dm_mfma(-sn[q], bi[q], are[tt]);
            }
          }
#pragma unroll
          for (int q = 0; q < DS_KC / 4; ++q) {
            if ((uint32_t)q < nq) {
              aim[tt] = dm_mfma(cs[q], bi[q], aim[tt]);
              aim[tt] = dm_mfma(sn[q], br[q], aim[tt]);
            }
          }
          if constexpr (WIN) {
#pragma unroll
            for (int q = 0; q < DS_KC / 4; ++q) {
              if ((uint32_t)q < nq) wre[tt] = dm_mfma(cw[q], by[q], wre[tt]);
            }
#pragma unroll
            for (int q = 0; q < DS_KC / 4; ++q) {
              if ((uint32_t)q < nq) wim[tt] = dm_mfma(sw[q], by[q], wim[tt]);
            }
          }
        }
      }
      if (kci + 1 == nkc) {   // the tile is complete: square, add, start again (a column tile that took no MFMA adds +0)
#pragma unroll
        for (int tt = 0; tt < DS_TT / 16; ++tt) {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const double pr = are[tt][e] * are[tt][e], pi = aim[tt][e] * aim[tt][e];
            P[e] += pr + pi;
            if constexpr (WIN) {
              const double hr = wre[tt][e] * wre[tt][e], hi = wim[tt][e] * wim[tt][e];
              H[e] += hr + hi;
            }
          }
          are[tt] = aim[tt] = zero4;
          if constexpr (WIN) wre[tt] = wim[tt] = zero4;
        }
      }
    }
  }
  // ---- the epilogue: the columns of a segment combined in a fixed order, the stores
  const bool direct = seg.slot < 0;
  if (db == 0 && wave == 0) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      S1 += __shfl_xor(S1, m);
      S2 += __shfl_xor(S2, m);
      cnt += __shfl_xor(cnt, m);
    }
    if (lane == 0) {
      const size_t o = direct ? (size_t)row * a.nbin + (uint32_t)seg.bin : (size_t)seg.slot * a.nrow + row;
      if (a.s1) dm_stg(direct ? a.s1 : a.ps1, o, S1);
      if (a.s2) dm_stg(direct ? a.s2 : a.ps2, o, S2);
      if (a.count) (direct ? a.count : a.pcount)[o] = cnt;
    }
  }
  if (!wave_on) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
#pragma unroll
    for (int m = 8; m >= 1; m >>= 1) {
      P[e] += __shfl_xor(P[e], m);
      if constexpr (WIN) H[e] += __shfl_xor(H[e], m);
    }
  }
  if (cj == 0) {
    const size_t o = (direct ? (size_t)row * a.nbin + (uint32_t)seg.bin : (size_t)seg.slot * a.nrow + row) * a.nd;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const uint32_t d = e0 + kq + 4u * e;
      if (d >= a.nd) continue;
      dm_stg(direct ? a.q : a.pq, o + d, P[e]);
      if constexpr (WIN) dm_stg(direct ? a.h : a.ph, o + d, H[e]);
    }
  }
}

// the second pass: the bins that were split are the sums of their segments in ascending order, the empty bins are zeros
__global__ __launch_bounds__(256) void delayspec_combine_kernel(const ds_args a) {
  const uint32_t d = blockIdx.x * 256u + threadIdx.x, b = blockIdx.y, row = blockIdx.z;
  const ds_bin bin = a.bins[b];
  if (bin.nseg == 1) return;
  const size_t ob = (size_t)row * a.nbin + b;
  if (d < a.nd) {
    double sq = 0.0, sh = 0.0;
    for (int s = 0; s < bin.nseg; ++s) {
      const size_t p = ((size_t)(bin.slot0 + s) * a.nrow + row) * a.nd + d;
      sq = s ? sq + dm_ldg(a.pq, p) : dm_ldg(a.pq, p);
      if (a.h) sh = s ? sh + dm_ldg(a.ph, p) : dm_ldg(a.ph, p);
    }
    dm_stg(a.q, ob * a.nd + d, sq);
    if (a.h) dm_stg(a.h, ob * a.nd + d, sh);
  }
  if (d == 0) {
    double v1 = 0.0, v2 = 0.0;
    int n = 0;
    for (int s = 0; s < bin.nseg; ++s) {
      const size_t p = (size_t)(bin.slot0 + s) * a.nrow + row;
      if (a.s1) v1 = s ? v1 + dm_ldg(a.ps1, p) : dm_ldg(a.ps1, p);
      if (a.s2) v2 = s ? v2 + dm_ldg(a.ps2, p) : dm_ldg(a.ps2, p);
      if (a.count) n += a.pcount[p];
    }
    if (a.s1) dm_stg(a.s1, ob, v1);
    if (a.s2) dm_stg(a.s2, ob, v2);
    if (a.count) a.count[ob] = n;
  }
}

}  // namespace

extern "C" int dm_delayspec_max_nf(void) { return DS_MAX_NF; }
extern "C" int dm_delayspec_max_nd(void) { return DS_MAX_ND; }

extern "C" int dm_delayspec_segments(int nsamples, int* length) {
  if (nsamples <= 0) {
    if (length) *length = 0;
    return 0;
  }
  int n = (nsamples + DS_SEG_MIN - 1) / DS_SEG_MIN;
  if (n > DS_SEGS) n = DS_SEGS;
  const int len = DS_TT * (((nsamples + n - 1) / n + DS_TT - 1) / DS_TT);
  if (length) *length = len;
  return (nsamples + len - 1) / len;
}

extern "C" int dm_delay_spectrum(dm_ctx* ctx, int nf, int nrow, int nt, int nd, int a0, int weighting, int min_valid,
                                 const double* taper_dev, const double* step_dev, int nbin, const int* bin_off_host,
                                 const void* x_dev, const double* w_dev, double* q_dev, double* h_dev, double* s1_dev,
                                 double* s2_dev, int* count_dev) {
  static const char* who = "dm_delay_spectrum";
  if (!ctx) return DM_EARG;
  if (nf < 0 || nrow < 0 || nt < 0 || nd < 0 || nbin < 0) return dm_refuse(ctx, who, "negative size");
  if (weighting != 0 && weighting != 1) return dm_refuse(ctx, who, "weighting is 0 (the mask) or 1 (the weights)");
  if (nf > DS_MAX_NF) return dm_refuse(ctx, who, "nf > dm_delayspec_max_nf()");
  if (nd > DS_MAX_ND) return dm_refuse(ctx, who, "nd > dm_delayspec_max_nd()");
  if (min_valid < 1) return dm_refuse(ctx, who, "min_valid < 1");
  if (nd > 0 && (a0 < 0 || a0 >= nd)) return dm_refuse(ctx, who, "a0 is outside [0, nd)");
  if (nf == 0 || nrow == 0 || nt == 0 || nbin == 0 || nd == 0) return DM_OK;
  if (!x_dev || !step_dev || !bin_off_host || !q_dev) return dm_refuse(ctx, who, "null x, step, bin_off or q with work to do");
  if (bin_off_host[0] < 0 || bin_off_host[nbin] > nt) return dm_refuse(ctx, who, "bin_off leaves [0, nt]");
  for (int b = 0; b < nbin; ++b)
    if (bin_off_host[b + 1] < bin_off_host[b]) return dm_refuse(ctx, who, "bin_off decreases at bin " + std::to_string(b));
  const uint64_t nx = (uint64_t)nf * nrow * nt, no = (uint64_t)nrow * nbin;
  {
    const dm_span in[4] = {{x_dev, 16 * nx, "x"},
                           {w_dev, w_dev ? 8 * nx : 0, "w"},
                           {taper_dev, taper_dev ? 8 * (uint64_t)nf : 0, "taper"},
                           {step_dev, 8 * (uint64_t)nf, "step"}};
    const dm_span out[5] = {{q_dev, 8 * no * nd, "q"},
                            {h_dev, h_dev ? 8 * no * nd : 0, "h"},
                            {s1_dev, s1_dev ? 8 * no : 0, "s1"},
                            {s2_dev, s2_dev ? 8 * no : 0, "s2"},
                            {count_dev, count_dev ? 4 * no : 0, "count"}};
    const std::string shared = dm_spans_shared(in, 4, out, 5);
    if (!shared.empty()) return dm_refuse(ctx, who, shared);
  }
  // the segments: a function of the bins alone
  std::vector<ds_seg> segs;
  std::vector<ds_bin> bins((size_t)nbin);
  int nslot = 0;
  bool combine = false;
  const bool none_used = !w_dev && nf < min_valid;   // without weights every series has nf kept channels
  for (int b = 0; b < nbin; ++b) {
    const int b0 = bin_off_host[b], L = none_used ? 0 : bin_off_host[b + 1] - b0;
    int len = 0;
    const int n = dm_delayspec_segments(L, &len);
    bins[(size_t)b] = ds_bin{nslot, n};
    for (int s = 0; s < n; ++s) {
      const int s0 = b0 + s * len, s1 = s0 + len < b0 + L ? s0 + len : b0 + L;
      segs.push_back(ds_seg{s0, s1, b, n == 1 ? -1 : nslot + s});
    }
    if (n != 1) combine = true;
    if (n > 1) nslot += n;
  }
  ds_args a;
  a.ndb = ((uint32_t)nd + DS_ND - 1) / DS_ND;
  a.nseg = (uint32_t)segs.size();
  const uint64_t nblocks = (uint64_t)nrow * a.nseg * a.ndb;
  if (nblocks >= (1ull << 31) || nrow > 65535 || nbin > 65535)
    return dm_refuse(ctx, who, "too many workgroups for one launch (nrow, nbin <= 65535)");
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws_scope__(ctx);
  a.segs = dm_ws_upload(ctx, segs);
  a.bins = dm_ws_upload(ctx, bins);
  if (!a.segs || !a.bins) return DM_ENOMEM;
  a.pq = a.ph = a.ps1 = a.ps2 = nullptr;
  a.pcount = nullptr;
  if (nslot > 0) {
    const size_t np = (size_t)nslot * nrow;
    a.pq = dm_ws_alloc_t<double>(ctx, np * nd);
    a.ph = h_dev ? dm_ws_alloc_t<double>(ctx, np * nd) : nullptr;
    a.ps1 = dm_ws_alloc_t<double>(ctx, np);
    a.ps2 = dm_ws_alloc_t<double>(ctx, np);
    a.pcount = dm_ws_alloc_t<int>(ctx, np);
    if (!a.pq || (h_dev && !a.ph) || !a.ps1 || !a.ps2 || !a.pcount) return DM_ENOMEM;
  }
  unsigned char* valid = nullptr;
  if (w_dev) {
    valid = dm_ws_alloc_t<unsigned char>(ctx, (size_t)nrow * nt);
    if (!valid) return DM_ENOMEM;
  }
  a.x = static_cast<const cplx*>(x_dev);
  a.w = w_dev;
  a.taper = taper_dev;
  a.step = step_dev;
  a.valid = valid;
  a.q = q_dev; a.h = h_dev; a.s1 = s1_dev; a.s2 = s2_dev; a.count = count_dev;
  a.nf = (uint32_t)nf; a.nrow = (uint32_t)nrow; a.nt = (uint32_t)nt; a.nd = (uint32_t)nd; a.nbin = (uint32_t)nbin;
  a.a0 = a0; a.weighting = weighting; a.min_valid = min_valid;
  if (valid && a.nseg > 0) {
    const dim3 grid(((unsigned)nt + 255u) / 256u, (unsigned)nrow);
    DM_PLAUNCH(ctx, DM_PROF_UTIL, delayspec_valid_kernel, grid, dim3(256), 0, ctx->stream, a, valid);
    DM_HIP(ctx, hipGetLastError());
  }
  if (a.nseg > 0) {
    uint64_t used = 0;
    for (const ds_seg& s : segs) used += (uint64_t)(s.t1 - s.t0);
    const double flops = (h_dev ? 12.0 : 8.0) * (double)nf * nd * nrow * (double)used;
    const dim3 grid((unsigned)nblocks), block(DS_THREADS);
    {
      dm_prof_scope ps(ctx, DM_PROF_UTIL, flops);
      if (h_dev)
        hipLaunchKernelGGL(delayspec_kernel<true>, grid, block, 0, ctx->stream, a);
      else
        hipLaunchKernelGGL(delayspec_kernel<false>, grid, block, 0, ctx->stream, a);
    }
    DM_HIP(ctx, hipGetLastError());
  }
  if (combine) {
    const dim3 grid(((unsigned)nd + 255u) / 256u, (unsigned)nbin, (unsigned)nrow);
    DM_PLAUNCH(ctx, DM_PROF_UTIL, delayspec_combine_kernel, grid, dim3(256), 0, ctx->stream, a);
    DM_HIP(ctx, hipGetLastError());
  }
  return DM_OK;
}
