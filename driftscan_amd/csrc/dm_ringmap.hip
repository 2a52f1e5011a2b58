// dm_ringmap.hip — dm_ringmap, the north-south beamformer of stacked visibilities.
//
// For frequency f, group g (a list of rows of vis), elevation s_e and sample t:
//   x_b(t) = T_b w_b(t) where w_b(t) > 0 and 0 elsewhere,   D(t) = sum_b x_b(t),   D2(t) = sum_b T_b x_b(t),
//   tau_be = (scale_f v_b) s_e,   phi_be = tau_be - rint(tau_be)  (exact),   (S, C)_be = sincospi(2 phi_be),
//   map[0](e, t) = sum_b (C_be Re X_b(t) + S_be Im X_b(t)) / D(t),   X_b(t) = x_b(t) V_b(t),
//   map[1](e, t) = sum_b (C_be Im X_b(t) - S_be Re X_b(t)) / D(t).
// A real product with K = 2 nb on v_mfma_f64_16x16x4_f64: rows are elevations, columns samples.  One workgroup of eight
// waves takes RM_EL = 128 elevations x RM_TT = 128 samples of one (f, g); wave w owns the 16 elevations e0 + 16 w and
// all eight 16-sample column tiles.  The members pass through LDS in chunks of RM_KC = 16: the chunk is staged as the
// planes Re X, Im X and x (the weighting happens on the way in: no weighted copy exists in memory), the next chunk's
// samples are already in flight in registers while this one is multiplied, each lane produces the cos / sin of its own
// A element (member kq = lane >> 4 of each group of four, elevation lane & 15) once per chunk, and every accumulator
// then takes its MFMAs of the chunk back to back.  With parts = 2 the second accumulator set reads the same staged
// tile and the same cos / sin.  D and D2 are summed from the staged x plane by the first 128 threads, the division is
// the epilogue.  No table in memory, no atomics.
//
// The fixed orders: an output element is one accumulator walked through the members of its group in list order, four
// at a time (cos then sin of each four), from the first member of the group; a group whose size is no multiple of four
// ends with members of weight 0.  D and D2 are sequential sums in list order.  None of it depends on the tile, on the
// other groups, frequencies, elevations or samples of the launch.
#include "dm_common.h"
#include "dm_feedpair.h"
#include "dm_stack_table.h"
#include "../../include/driftmi.h"

#include <cmath>

// No implicit contraction in this file: tau, x and X are rounded products.
#pragma clang fp contract(off)

namespace {

constexpr int RM_TT = 128;            // samples of a workgroup
constexpr int RM_EL = 128;            // elevations of a workgroup: 16 per wave
constexpr int RM_KC = 16;             // members of a staged chunk
constexpr int RM_XS = RM_TT + 16;     // row pitch of a staged plane: the two member rows of a 32-lane ds_read_b64 group
                                      // fall 32 banks apart
constexpr int RM_THREADS = 512;
constexpr int RM_SI = RM_KC / (RM_THREADS / RM_TT);   // members a thread stages per chunk

struct rm_args {
  const cplx* vis;
  const double* w;        // or null
  const int* group_off;   // device copies of the host tables
  const int* members;
  const double* v;
  const double* taper;    // or null
  const double* scale;
  const double* sinza;
  double* map;
  double* norm;           // or null
  double* norm2;          // or null
  uint32_t nf, nrow, nt, ngroup, nel, neb, ntb;
};

template <int PARTS>
__global__ __launch_bounds__(RM_THREADS) void ringmap_kernel(const rm_args a) {
  __shared__ double xr[RM_KC * RM_XS], xi[RM_KC * RM_XS], xw[RM_KC * RM_XS];
  __shared__ double vk[RM_KC], tk[RM_KC], dsum[RM_TT];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  uint32_t r = (uint32_t)dm_xcd_remap((int)blockIdx.x, (int)gridDim.x);
  const uint32_t eb = r % a.neb;   // elevation blocks of one (f, g, sample block) are neighbours: they stage the same rows
  r /= a.neb;
  const uint32_t tb = r % a.ntb;
  r /= a.ntb;
  const uint32_t g = r % a.ngroup, f = r / a.ngroup;
  const uint32_t m0 = (uint32_t)a.group_off[g], nb = (uint32_t)a.group_off[g + 1] - m0;
  const uint32_t t0 = tb * RM_TT, e0 = eb * RM_EL + wave * 16;
  const uint32_t cj = lane & 15u, kq = lane >> 4;
  const bool wave_on = e0 < a.nel;                                   // uniform in the wave
  const uint32_t tleft = a.nt - t0, ntt = tleft >= (uint32_t)RM_TT ? RM_TT / 16 : (tleft + 15) / 16;
  const double se = e0 + cj < a.nel ? dm_ldg(a.sinza, e0 + cj) : 0.0;
  const double scale = dm_ldg(a.scale, f);
  // staging: thread = (sample st, members sk + 4 i of the chunk)
  const uint32_t st = tid & (RM_TT - 1), sk = tid / RM_TT;
  const bool t_in = t0 + st < a.nt;
  cplx pv[RM_SI];
  double pw[RM_SI];
  auto fetch = [&](uint32_t kc) {
#pragma unroll
    for (int i = 0; i < RM_SI; ++i) {
      const uint32_t m = kc + sk + 4u * i;
      pv[i] = make_double2(0.0, 0.0);
      pw[i] = 0.0;   // a member past the group and a sample past nt are staged as not kept
      if (m < nb && t_in) {
        const size_t idx = ((size_t)f * a.nrow + (size_t)a.members[m0 + m]) * a.nt + t0 + st;
        pw[i] = a.w ? dm_ldg(a.w, idx) : 1.0;
        pv[i] = dm_ldg(a.vis, idx);
      }
    }
  };
  dm_f64x4 acc[PARTS][RM_TT / 16];
#pragma unroll
  for (int p = 0; p < PARTS; ++p)
#pragma unroll
    for (int tt = 0; tt < RM_TT / 16; ++tt) acc[p][tt] = dm_f64x4{0.0, 0.0, 0.0, 0.0};
  double D = 0.0, D2 = 0.0;
  if (nb > 0) fetch(0);
  for (uint32_t kc = 0; kc < nb; kc += RM_KC) {
    __syncthreads();   // the chunk before is read no more
#pragma unroll
    for (int i = 0; i < RM_SI; ++i) {
      const uint32_t k = sk + 4u * i, m = kc + k;
      const double tb_ = m < nb ? (a.taper ? dm_ldg(a.taper, (size_t)m0 + m) : 1.0) : 0.0;
      const bool kept = pw[i] > 0.0;   // false for 0, negatives and NaN
      const double x = kept ? tb_ * pw[i] : 0.0;
      xr[k * RM_XS + st] = kept ? x * pv[i].x : 0.0;
      xi[k * RM_XS + st] = kept ? x * pv[i].y : 0.0;
      xw[k * RM_XS + st] = x;
    }
    if (tid < (uint32_t)RM_KC) {
      const uint32_t m = kc + tid;
      vk[tid] = m < nb ? scale * dm_ldg(a.v, (size_t)m0 + m) : 0.0;
      tk[tid] = m < nb ? (a.taper ? dm_ldg(a.taper, (size_t)m0 + m) : 1.0) : 0.0;
    }
    __syncthreads();
    if (kc + RM_KC < nb) fetch(kc + RM_KC);   // in flight behind the MFMAs of this chunk
    const uint32_t nk = nb - kc < (uint32_t)RM_KC ? nb - kc : (uint32_t)RM_KC, nq = (nk + 3) / 4;
    if (tid < (uint32_t)RM_TT) {
      for (uint32_t k = 0; k < nk; ++k) {
        const double x = xw[k * RM_XS + tid];
        D += x;
        D2 += tk[k] * x;
      }
    }
    if (wave_on) {
      double cs[RM_KC / 4], sn[RM_KC / 4];
#pragma unroll
      for (int q = 0; q < RM_KC / 4; ++q) {
        const double tau = vk[4 * q + kq] * se;
        sincospi(2.0 * (tau - rint(tau)), &sn[q], &cs[q]);   // exact: |tau - rint(tau)| <= 1/2
      }
#pragma unroll
      for (int tt = 0; tt < RM_TT / 16; ++tt) {
        if ((uint32_t)tt < ntt) {
          double br[RM_KC / 4], bi[RM_KC / 4];
#pragma unroll
          for (int q = 0; q < RM_KC / 4; ++q) {
            br[q] = xr[(4 * q + kq) * RM_XS + tt * 16 + cj];
            bi[q] = xi[(4 * q + kq) * RM_XS + tt * 16 + cj];
          }
#pragma unroll
          for (int q = 0; q < RM_KC / 4; ++q) {
            if ((uint32_t)q < nq) {
              acc[0][tt] = dm_mfma(cs[q], br[q], acc[0][tt]);
              acc[0][tt] = dm_mfma(sn[q], bi[q], acc[0][tt]);
            }
          }
          if constexpr (PARTS == 2) {
#pragma unroll
            for (int q = 0; q < RM_KC / 4; ++q) {
              if ((uint32_t)q < nq) {
                acc[1][tt] = dm_mfma(cs[q], bi[q], acc[1][tt]);
                acc[1][tt] = dm_mfma(-sn[q], br[q], acc[1][tt]);
              }
            }
          }
        }
      }
    }
  }
  // ---- the epilogue: D to every wave, the division, the stores
  if (tid < (uint32_t)RM_TT) dsum[tid] = D;
  __syncthreads();
  if (eb == 0 && tid < (uint32_t)RM_TT && t_in) {
    const size_t o = ((size_t)f * a.ngroup + g) * a.nt + t0 + tid;
    if (a.norm) dm_stg(a.norm, o, D == 0.0 ? 0.0 : D);
    if (a.norm2) dm_stg(a.norm2, o, D == 0.0 ? 0.0 : D2);
  }
  if (!wave_on) return;
#pragma unroll
  for (int tt = 0; tt < RM_TT / 16; ++tt) {
    const uint32_t t = t0 + tt * 16 + cj;
    if ((uint32_t)tt >= ntt || t >= a.nt) continue;
    const double d = dsum[tt * 16 + cj];
#pragma unroll
    for (int p = 0; p < PARTS; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t e = e0 + kq + 4u * q;
        if (e >= a.nel) continue;
        const size_t o = ((((size_t)f * a.ngroup + g) * PARTS + p) * a.nel + e) * a.nt + t;
        dm_stg(a.map, o, d == 0.0 ? 0.0 : acc[p][tt][q] / d);
      }
  }
}

}  // namespace

extern "C" int dm_ringmap(dm_ctx* ctx, int nf, int nrow, int nt, int ngroup, const int* group_off_host,
                          const int* members_host, const double* v_dev, const double* taper_dev, const double* scale_dev,
                          int nel, const double* sinza_dev, int parts, const void* vis_dev, const double* w_dev,
                          double* map_dev, double* norm_dev, double* norm2_dev) {
  static const char* who = "dm_ringmap";
  if (!ctx) return DM_EARG;
  if (nf < 0 || nrow < 0 || nt < 0 || ngroup < 0 || nel < 0) return dm_refuse(ctx, who, "negative size");
  if (parts != 1 && parts != 2) return dm_refuse(ctx, who, "parts is 1 (real part) or 2 (real and imaginary part)");
  if (nf == 0 || nt == 0 || ngroup == 0 || nel == 0) return DM_OK;
  if (!group_off_host || !scale_dev || !sinza_dev || !map_dev)
    return dm_refuse(ctx, who, "null group_off, scale, sinza or map with work to do");
  if (group_off_host[0] < 0) return dm_refuse(ctx, who, "group_off[0] < 0");
  for (int g = 0; g < ngroup; ++g)
    if (group_off_host[g + 1] < group_off_host[g]) return dm_refuse(ctx, who, "group_off decreases at group " + std::to_string(g));
  const int nmem = group_off_host[ngroup];
  if (nmem > 0 && (!members_host || !v_dev || !vis_dev)) return dm_refuse(ctx, who, "null members, v or vis with members listed");
  for (int m = group_off_host[0]; m < nmem; ++m)
    if (members_host[m] < 0 || members_host[m] >= nrow)
      return dm_refuse(ctx, who, "member " + std::to_string(m) + " is outside [0, nrow)");
  const uint64_t nvis = (uint64_t)nf * nrow * nt, nnorm = (uint64_t)nf * ngroup * nt;
  {
    const dm_span in[6] = {{vis_dev, 16 * nvis, "vis"},
                           {w_dev, w_dev ? 8 * nvis : 0, "w"},
                           {v_dev, 8 * (uint64_t)nmem, "v"},
                           {taper_dev, taper_dev ? 8 * (uint64_t)nmem : 0, "taper"},
                           {scale_dev, 8 * (uint64_t)nf, "scale"},
                           {sinza_dev, 8 * (uint64_t)nel, "sinza"}};
    const dm_span out[3] = {{map_dev, 8 * nnorm * parts * nel, "map"},
                            {norm_dev, norm_dev ? 8 * nnorm : 0, "norm"},
                            {norm2_dev, norm2_dev ? 8 * nnorm : 0, "norm2"}};
    const std::string shared = dm_spans_shared(in, 6, out, 3);
    if (!shared.empty()) return dm_refuse(ctx, who, shared);
  }
  rm_args a;
  a.neb = ((uint32_t)nel + RM_EL - 1) / RM_EL;
  a.ntb = ((uint32_t)nt + RM_TT - 1) / RM_TT;
  const uint64_t nblocks = (uint64_t)nf * ngroup * a.neb * a.ntb;
  if (nblocks >= (1ull << 31)) return dm_refuse(ctx, who, "too many workgroups for one launch");
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws_scope__(ctx);
  a.group_off = dm_ws_upload(ctx, std::vector<int>(group_off_host, group_off_host + ngroup + 1));
  a.members = dm_ws_upload(ctx, std::vector<int>(members_host ? members_host : group_off_host,
                                                 members_host ? members_host + nmem : group_off_host));
  if (!a.group_off || !a.members) return DM_ENOMEM;
  a.vis = static_cast<const cplx*>(vis_dev);
  a.w = w_dev;
  a.v = v_dev;
  a.taper = taper_dev;
  a.scale = scale_dev;
  a.sinza = sinza_dev;
  a.map = map_dev;
  a.norm = norm_dev;
  a.norm2 = norm2_dev;
  a.nf = (uint32_t)nf; a.nrow = (uint32_t)nrow; a.nt = (uint32_t)nt; a.ngroup = (uint32_t)ngroup; a.nel = (uint32_t)nel;
  const dim3 grid((unsigned)nblocks), block(RM_THREADS);
  const double flops = 4.0 * parts * (double)nf * nmem * nel * nt;
  {
    dm_prof_scope ps(ctx, DM_PROF_UTIL, flops);
    if (parts == 1)
      hipLaunchKernelGGL(ringmap_kernel<1>, grid, block, 0, ctx->stream, a);
    else
      hipLaunchKernelGGL(ringmap_kernel<2>, grid, block, 0, ctx->stream, a);
  }
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}
