// dm_formedbeam.hip — dm_formed_beam, tracking beams on catalogue positions from stacked visibilities (DESIGN.md
// section 4.26).
//
// For frequency f, group p (a list of rows of vis with east-west and north-south separations u_b, v_b), source s with
// the window k = k0_s + j (mod nt), j = -H_s .. H_s:
//   D      = turn_s - k / nt, reduced to [-1/2, 1/2];  (sd, cd) = sincospi(2 D)
//   x      = sinth_s sd,   y = yc0_s - yc1_s cd,   A = exp(-(env_f (x x)))   (env_f = 0: A = 1)
//   x_b(k) = T_b w_b(k) where w_b(k) > 0, else 0,   X_b(k) = x_b(k) V_b(k)
//   phi_u  = frac((scale_f u_b) x),  phi_v = frac((scale_f v_b) y),  frac(t) = t - rint(t)  (exact)
//   num    = sum_k sum_b A Re(X_b(k) conj(E(phi_u) E(phi_v))),  E(phi) = exp(2 pi i phi) from sincospi(2 phi)
//   D      = sum_k A sum_b x_b(k),   D2 = sum_k A A sum_b x_b(k),   beam = num / D  (all three 0 where D = 0).
//
// A workgroup of four waves owns one (f, p) and 64 neighbouring sources of the catalogue sorted by k0: lane l of every
// wave is source l of the block.  The workgroup walks the union of the block's windows in sample order, in the tiles
// of FB_KT = 4 samples [4 i, min(4 i + 4, nt)) of the absolute sample index, and per tile through the members of the
// group in chunks of FB_MC = 256; a (chunk x tile) of X and x is staged in LDS once (the weighting happens on the way
// in: no weighted copy exists in memory) and serves the 64 sources.  Wave w takes members [64 w, 64 w + 64) of every
// chunk.  Two paths, chosen per group by the number of distinct u among its members:
//   factorised (at most FB_NU = 8 distinct u): A E(phi_u) of the tile's samples and the group's distinct u are made once
//     per tile into LDS; E(phi_v) is made in registers when the v index of the member differs from the one before it in
//     the wave's run; a member costs one complex multiply and one complex multiply-add;
//   direct (more distinct u): one sincospi(2 (phi_u + phi_v)) per member.
// No table in memory, no atomics on floating point.
//
// The fixed order of a (f, p, s): four partial sums, one per wave, each a sequential fma chain over
//   tiles of the window in window order > chunks of 256 members > samples of the tile > the wave's 64 members in list order
// (Re X P_re then Im X P_im per member), added as ((w0 + w1) + w2) + w3.  D and D2 alike, with the sum of x over the
// wave's 64 members of a (chunk, sample) taken as: lane i of 16 adds members i, i + 16, i + 32, i + 48 in turn, then the
// xor butterfly 8, 4, 2, 1.  The tiles are those of the absolute sample index, so the order depends on the source's own
// window and the group's member list only: not on the other sources, their order, or the launch.
#include "dm_common.h"
#include "dm_feedpair.h"
#include "dm_stack_table.h"
#include "../../include/driftmi.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <numeric>

// No implicit contraction in this file: the phases are rounded products; every fma below is written out.
#pragma clang fp contract(off)

namespace {

constexpr int FB_SB = 64;        // sources of a workgroup: one per lane
constexpr int FB_W = 4;          // waves of a workgroup
constexpr int FB_MC = 256;       // members of a staged chunk: 64 per wave
constexpr int FB_KT = 4;         // samples of a staged tile
constexpr int FB_NU = 8;         // distinct u up to which a group takes the factorised path
constexpr int FB_THREADS = FB_SB * FB_W;
static_assert(FB_KT == FB_W, "wave w makes the u phasors of sample w of a tile");

struct fb_args {
  const cplx* vis;
  const double* w;         // or null
  const double* taper;     // or null
  const int* group_off;    // device copies of the host tables
  const int* members;
  const int* iu;           // per member: index into uvals
  const int* iv;           // per member: index into vvals
  const int* lu;           // per member: index into the group's own list of distinct u
  const int* gu_off;       // per group: its distinct u, gu[gu_off[p] .. gu_off[p + 1]) indices into uvals
  const int* gu;
  const int* perm;         // the sources in the order of k0
  const int* k0;
  const int* half;
  const double* uvals;
  const double* vvals;
  const double* scale;
  const double* env;
  const double* turn;
  const double* sinth;
  const double* yc0;
  const double* yc1;
  double* beam;
  double* norm;            // or null
  double* norm2;           // or null
  int nf, nrow, nt, ngroup, nsrc, nsb;
};

template <int PARTS>
__global__ __launch_bounds__(FB_THREADS) void formed_beam_kernel(const fb_args a) {
  __shared__ double2 xs[FB_MC * FB_KT];            // X of the staged (chunk, tile); the partial sums at the end
  __shared__ double xw[FB_MC * FB_KT];             // x of it
  __shared__ double2 eu[FB_KT * FB_NU * FB_SB];    // A E(phi_u) per (sample of the tile, distinct u, source)
  __shared__ double msu[FB_MC], msv[FB_MC];        // scale u_b, scale v_b of the chunk
  __shared__ int2 mli[FB_MC];                      // (index of u in the group's list, index of v) of the chunk
  __shared__ int kr[2];
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int r = (int)blockIdx.x;
  const int sb = r % a.nsb;
  r /= a.nsb;
  const int p = r % a.ngroup, f = r / a.ngroup;
  const int si = sb * FB_SB + lane;
  const bool valid = si < a.nsrc;
  const int s = valid ? a.perm[si] : 0;
  const int k0 = valid ? a.k0[s] : 0, H = valid ? a.half[s] : -1;
  const double turn = valid ? dm_ldg(a.turn, s) : 0.0, sth = valid ? dm_ldg(a.sinth, s) : 0.0;
  const double c0 = valid ? dm_ldg(a.yc0, s) : 0.0, c1 = valid ? dm_ldg(a.yc1, s) : 0.0;
  if (tid == 0) {
    kr[0] = INT_MAX;
    kr[1] = INT_MIN;
  }
  __syncthreads();
  if (wave == 0 && H >= 0) {
    atomicMin(&kr[0], k0 - H);
    atomicMax(&kr[1], k0 + H);
  }
  __syncthreads();
  const int Kmin = kr[0], Kmax = kr[1];
  const int m0 = a.group_off[p], nb = a.group_off[p + 1] - m0;
  const int gu0 = a.gu_off[p], nug = a.gu_off[p + 1] - gu0;
  const bool fact = nug <= FB_NU;   // uniform in the launch for this group
  const double scale = dm_ldg(a.scale, f), env = dm_ldg(a.env, f);
  const int nt = a.nt;
  double acc_re = 0.0, acc_im = 0.0, D = 0.0, D2 = 0.0;
  if (Kmin <= Kmax && nb > 0) {
    // the tile that holds the first sample: kabs in [0, nt), Kt the unwrapped coordinate of the tile's first sample
    const int kabs0 = ((Kmin % nt) + nt) % nt;
    int Kt = Kmin - kabs0 % FB_KT;
    while (Kt <= Kmax) {
      const int a0 = ((Kt % nt) + nt) % nt;
      const int len = nt - a0 < FB_KT ? nt - a0 : FB_KT;
      // this lane's geometry at the samples of the tile
      double xk[FB_KT], yk[FB_KT], Ak[FB_KT];
      bool any_on[FB_KT];
#pragma unroll
      for (int kk = 0; kk < FB_KT; ++kk) {
        const int K = Kt + kk;
        const bool on = kk < len && H >= 0 && K >= k0 - H && K <= k0 + H;
        double d = turn - (double)(a0 + kk) / (double)nt;
        d -= rint(d);
        double sd, cd;
        sincospi(2.0 * d, &sd, &cd);
        const double x = sth * sd;
        const double y = c0 - c1 * cd;
        const double A = env == 0.0 ? 1.0 : exp(-(env * (x * x)));
        xk[kk] = x;
        yk[kk] = y;
        Ak[kk] = on ? A : 0.0;   // a sample outside the window adds exact zeros
        any_on[kk] = __any(on) != 0;
      }
      for (int cm = 0; cm < nb; cm += FB_MC) {
        __syncthreads();   // the chunk before, and with cm = 0 the tile before, are read no more
        if (cm == 0 && fact) {
#pragma unroll
          for (int kk = 0; kk < FB_KT; ++kk) {
            if (kk == wave && any_on[kk]) {
              for (int j = 0; j < nug; ++j) {
                const double su = scale * dm_ldg(a.uvals, (size_t)a.gu[gu0 + j]);
                const double tau = su * xk[kk];
                double sn, cs;
                sincospi(2.0 * (tau - rint(tau)), &sn, &cs);
                eu[(kk * FB_NU + j) * FB_SB + lane] = make_double2(Ak[kk] * cs, Ak[kk] * sn);
              }
            }
          }
        }
        {
          const int kk = tid & (FB_KT - 1);
#pragma unroll
          for (int i = 0; i < FB_MC * FB_KT / FB_THREADS; ++i) {
            const int ml = (tid >> 2) + (FB_THREADS / FB_KT) * i, m = cm + ml;
            double2 X = make_double2(0.0, 0.0);
            double x = 0.0;   // a member past the group and a sample past the tile are staged as not kept
            if (m < nb && kk < len) {
              const size_t idx = ((size_t)f * a.nrow + (size_t)a.members[m0 + m]) * nt + a0 + kk;
              const double wv = a.w ? dm_ldg(a.w, idx) : 1.0;
              if (wv > 0.0) {   // false for 0, negatives and NaN: such a sample is not read
                x = (a.taper ? dm_ldg(a.taper, (size_t)m0 + m) : 1.0) * wv;
                const cplx V = dm_ldg(a.vis, idx);
                X = make_double2(x * V.x, x * V.y);
              }
            }
            xs[ml * FB_KT + kk] = X;
            xw[ml * FB_KT + kk] = x;
          }
          if (tid < FB_MC && cm + tid < nb) {
            const int iu = a.iu[m0 + cm + tid], iv = a.iv[m0 + cm + tid];
            msu[tid] = scale * dm_ldg(a.uvals, (size_t)iu);
            msv[tid] = scale * dm_ldg(a.vvals, (size_t)iv);
            mli[tid] = make_int2(a.lu[m0 + cm + tid], iv);
          }
        }
        __syncthreads();
        const int nbc = nb - cm < FB_MC ? nb - cm : FB_MC;
        const int mb = wave * (FB_MC / FB_W), me = mb + FB_MC / FB_W < nbc ? mb + FB_MC / FB_W : nbc;
        if (mb >= me) continue;   // uniform in the wave; the barriers above are reached by the next round
        // sum of x over the wave's members, per sample: lane = (sample lane >> 4, i = lane & 15)
        double sx = 0.0;
#pragma unroll
        for (int q = 0; q < FB_MC / FB_W / 16; ++q) sx += xw[(mb + (lane & 15) + 16 * q) * FB_KT + (lane >> 4)];
        sx += __shfl_xor(sx, 8);
        sx += __shfl_xor(sx, 4);
        sx += __shfl_xor(sx, 2);
        sx += __shfl_xor(sx, 1);
#pragma unroll
        for (int kk = 0; kk < FB_KT; ++kk) {
          const double xsum = __shfl(sx, kk * 16);
          if (!any_on[kk]) continue;
          D = fma(Ak[kk], xsum, D);
          D2 = fma(Ak[kk] * Ak[kk], xsum, D2);
          const double x = xk[kk], y = yk[kk], A = Ak[kk];
          if (fact) {
            int piv = -1;
            double evc = 1.0, evs = 0.0;
#pragma unroll 4   // the LDS reads of four members in flight before the first fma; the order of operations is unchanged
            for (int ml = mb; ml < me; ++ml) {
              const int2 li = mli[ml];
              if (li.y != piv) {
                const double tau = msv[ml] * y;
                sincospi(2.0 * (tau - rint(tau)), &evs, &evc);
                piv = li.y;
              }
              const double2 E = eu[(kk * FB_NU + li.x) * FB_SB + lane];
              const double2 X = xs[ml * FB_KT + kk];
              const double pr = fma(E.x, evc, -(E.y * evs)), pi = fma(E.x, evs, E.y * evc);
              acc_re = fma(X.x, pr, acc_re);
              acc_re = fma(X.y, pi, acc_re);
              if constexpr (PARTS == 2) {
                acc_im = fma(X.y, pr, acc_im);
                acc_im = fma(-X.x, pi, acc_im);
              }
            }
          } else {
            for (int ml = mb; ml < me; ++ml) {
              const double tu = msu[ml] * x, tv = msv[ml] * y;
              double sn, cs;
              sincospi(2.0 * ((tu - rint(tu)) + (tv - rint(tv))), &sn, &cs);
              const double2 X = xs[ml * FB_KT + kk];
              const double pr = A * cs, pi = A * sn;
              acc_re = fma(X.x, pr, acc_re);
              acc_re = fma(X.y, pi, acc_re);
              if constexpr (PARTS == 2) {
                acc_im = fma(X.y, pr, acc_im);
                acc_im = fma(-X.x, pi, acc_im);
              }
            }
          }
        }
      }
      Kt += len;
    }
  }
  // ---- the four partial sums in wave order, the division, the stores
  __syncthreads();
  double* red = reinterpret_cast<double*>(xs);
  red[(wave * 4 + 0) * FB_SB + lane] = acc_re;
  red[(wave * 4 + 1) * FB_SB + lane] = acc_im;
  red[(wave * 4 + 2) * FB_SB + lane] = D;
  red[(wave * 4 + 3) * FB_SB + lane] = D2;
  __syncthreads();
  if (wave != 0 || !valid) return;
  double tot[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double t = red[q * FB_SB + lane];
#pragma unroll
    for (int w = 1; w < FB_W; ++w) t += red[(w * 4 + q) * FB_SB + lane];
    tot[q] = t;
  }
  const bool ok = tot[2] != 0.0;
  const size_t fp = (size_t)f * a.ngroup + p;
  dm_stg(a.beam, (fp * PARTS + 0) * a.nsrc + s, ok ? tot[0] / tot[2] : 0.0);
  if constexpr (PARTS == 2) dm_stg(a.beam, (fp * PARTS + 1) * a.nsrc + s, ok ? tot[1] / tot[2] : 0.0);
  if (a.norm) dm_stg(a.norm, fp * a.nsrc + s, ok ? tot[2] : 0.0);
  if (a.norm2) dm_stg(a.norm2, fp * a.nsrc + s, ok ? tot[3] : 0.0);
}

}  // namespace

extern "C" int dm_formedbeam_block(void) { return FB_SB; }
extern "C" int dm_formedbeam_max_nu(void) { return FB_NU; }

extern "C" int dm_formed_beam(dm_ctx* ctx, int nf, int nrow, int nt, int ngroup, const int* group_off_host,
                              const int* members_host, const int* iu_host, const int* iv_host, int nu,
                              const double* uvals_dev, int nv, const double* vvals_dev, const double* taper_dev,
                              const double* scale_dev, const double* env_host, int nsrc, const int* k0_host,
                              const int* half_host, const double* turn_dev, const double* sinth_dev, const double* yc0_dev,
                              const double* yc1_dev, int parts, const void* vis_dev, const double* w_dev, double* beam_dev,
                              double* norm_dev, double* norm2_dev) {
  static const char* who = "dm_formed_beam";
  if (!ctx) return DM_EARG;
  if (nf < 0 || nrow < 0 || nt < 0 || ngroup < 0 || nsrc < 0 || nu < 0 || nv < 0) return dm_refuse(ctx, who, "negative size");
  if (parts != 1 && parts != 2) return dm_refuse(ctx, who, "parts is 1 (real part) or 2 (real and imaginary part)");
  if (nf == 0 || nt == 0 || ngroup == 0 || nsrc == 0) return DM_OK;
  if (!group_off_host || !scale_dev || !env_host || !k0_host || !half_host || !turn_dev || !sinth_dev || !yc0_dev || !yc1_dev ||
      !beam_dev)
    return dm_refuse(ctx, who, "null group_off, scale, env, k0, half, turn, sinth, yc0, yc1 or beam with work to do");
  for (int f = 0; f < nf; ++f)
    if (!(env_host[f] >= 0.0) || !std::isfinite(env_host[f]))
      return dm_refuse(ctx, who, "env of frequency " + std::to_string(f) + " is negative or not finite");
  for (int s = 0; s < nsrc; ++s) {
    if (half_host[s] < -1 || 2 * (int64_t)half_host[s] + 1 > nt)
      return dm_refuse(ctx, who, "half of source " + std::to_string(s) + " is below -1 or 2 half + 1 > nt");
    if (k0_host[s] < 0 || k0_host[s] >= nt) return dm_refuse(ctx, who, "k0 of source " + std::to_string(s) + " is outside [0, nt)");
  }
  if (group_off_host[0] < 0) return dm_refuse(ctx, who, "group_off[0] < 0");
  for (int g = 0; g < ngroup; ++g)
    if (group_off_host[g + 1] < group_off_host[g]) return dm_refuse(ctx, who, "group_off decreases at group " + std::to_string(g));
  const int nmem = group_off_host[ngroup];
  if (nmem > 0 && (!members_host || !iu_host || !iv_host || !uvals_dev || !vvals_dev || !vis_dev))
    return dm_refuse(ctx, who, "null members, iu, iv, uvals, vvals or vis with members listed");
  for (int m = group_off_host[0]; m < nmem; ++m) {
    if (members_host[m] < 0 || members_host[m] >= nrow)
      return dm_refuse(ctx, who, "member " + std::to_string(m) + " is outside [0, nrow)");
    if (iu_host[m] < 0 || iu_host[m] >= nu || iv_host[m] < 0 || iv_host[m] >= nv)
      return dm_refuse(ctx, who, "iu or iv of member " + std::to_string(m) + " is outside its table");
  }
  const uint64_t nvis = (uint64_t)nf * nrow * nt, nout = (uint64_t)nf * ngroup * nsrc;
  {
    const dm_span in[10] = {{vis_dev, nmem > 0 ? 16 * nvis : 0, "vis"},
                            {w_dev, w_dev ? 8 * nvis : 0, "w"},
                            {uvals_dev, 8 * (uint64_t)nu, "uvals"},
                            {vvals_dev, 8 * (uint64_t)nv, "vvals"},
                            {taper_dev, taper_dev ? 8 * (uint64_t)nmem : 0, "taper"},
                            {scale_dev, 8 * (uint64_t)nf, "scale"},
                            {turn_dev, 8 * (uint64_t)nsrc, "turn"},
                            {sinth_dev, 8 * (uint64_t)nsrc, "sinth"},
                            {yc0_dev, 8 * (uint64_t)nsrc, "yc0"},
                            {yc1_dev, 8 * (uint64_t)nsrc, "yc1"}};
    const dm_span out[3] = {{beam_dev, 8 * nout * parts, "beam"},
                            {norm_dev, norm_dev ? 8 * nout : 0, "norm"},
                            {norm2_dev, norm2_dev ? 8 * nout : 0, "norm2"}};
    const std::string shared = dm_spans_shared(in, 10, out, 3);
    if (!shared.empty()) return dm_refuse(ctx, who, shared);
  }
  fb_args a;
  a.nsb = (nsrc + FB_SB - 1) / FB_SB;
  const uint64_t nblocks = (uint64_t)nf * ngroup * a.nsb;
  if (nblocks >= (1ull << 31)) return dm_refuse(ctx, who, "too many workgroups for one launch");
  // the sources in the order of k0 (stable), dropped ones last: neighbours in a block share their windows
  std::vector<int> perm(nsrc);
  std::iota(perm.begin(), perm.end(), 0);
  std::stable_sort(perm.begin(), perm.end(), [&](int i, int j) {
    const int ki = half_host[i] < 0 ? nt : k0_host[i], kj = half_host[j] < 0 ? nt : k0_host[j];
    return ki < kj;
  });
  // every group's own list of distinct u, in the order of the table, and every member's place in it
  std::vector<int> gu_off(ngroup + 1, 0), gu, lu(std::max(nmem, 0), 0);
  {
    std::vector<int> where(nu, -1);
    for (int g = 0; g < ngroup; ++g) {
      std::vector<int> mine;
      for (int m = group_off_host[g]; m < group_off_host[g + 1]; ++m) mine.push_back(iu_host[m]);
      std::sort(mine.begin(), mine.end());
      mine.erase(std::unique(mine.begin(), mine.end()), mine.end());
      for (size_t j = 0; j < mine.size(); ++j) where[mine[j]] = (int)j;
      for (int m = group_off_host[g]; m < group_off_host[g + 1]; ++m) lu[m] = where[iu_host[m]];
      gu.insert(gu.end(), mine.begin(), mine.end());
      gu_off[g + 1] = (int)gu.size();
    }
  }
  DM_HIP(ctx, hipSetDevice(ctx->device));
  dm_ws_scope ws_scope__(ctx);
  const int* none = group_off_host;
  a.group_off = dm_ws_upload(ctx, std::vector<int>(group_off_host, group_off_host + ngroup + 1));
  a.members = dm_ws_upload(ctx, std::vector<int>(nmem > 0 ? members_host : none, nmem > 0 ? members_host + nmem : none));
  a.iu = dm_ws_upload(ctx, std::vector<int>(nmem > 0 ? iu_host : none, nmem > 0 ? iu_host + nmem : none));
  a.iv = dm_ws_upload(ctx, std::vector<int>(nmem > 0 ? iv_host : none, nmem > 0 ? iv_host + nmem : none));
  a.lu = dm_ws_upload(ctx, lu);
  a.gu_off = dm_ws_upload(ctx, gu_off);
  a.gu = dm_ws_upload(ctx, gu);
  a.perm = dm_ws_upload(ctx, perm);
  a.k0 = dm_ws_upload(ctx, std::vector<int>(k0_host, k0_host + nsrc));
  a.half = dm_ws_upload(ctx, std::vector<int>(half_host, half_host + nsrc));
  a.env = dm_ws_upload(ctx, std::vector<double>(env_host, env_host + nf));
  if (!a.group_off || !a.members || !a.iu || !a.iv || !a.lu || !a.gu_off || !a.gu || !a.perm || !a.k0 || !a.half || !a.env)
    return DM_ENOMEM;
  a.vis = static_cast<const cplx*>(vis_dev);
  a.w = w_dev;
  a.taper = taper_dev;
  a.uvals = uvals_dev;
  a.vvals = vvals_dev;
  a.scale = scale_dev;
  a.turn = turn_dev;
  a.sinth = sinth_dev;
  a.yc0 = yc0_dev;
  a.yc1 = yc1_dev;
  a.beam = beam_dev;
  a.norm = norm_dev;
  a.norm2 = norm2_dev;
  a.nf = nf; a.nrow = nrow; a.nt = nt; a.ngroup = ngroup; a.nsrc = nsrc;
  double terms = 0.0;
  for (int s = 0; s < nsrc; ++s) terms += half_host[s] < 0 ? 0.0 : 2.0 * half_host[s] + 1.0;
  const double flops = (8.0 + 4.0 * parts) * (double)nf * std::max(nmem, 0) * terms;
  const dim3 grid((unsigned)nblocks), block(FB_THREADS);
  {
    dm_prof_scope ps(ctx, DM_PROF_UTIL, flops);
    if (parts == 1)
      hipLaunchKernelGGL(formed_beam_kernel<1>, grid, block, 0, ctx->stream, a);
    else
      hipLaunchKernelGGL(formed_beam_kernel<2>, grid, block, 0, ctx->stream, a);
  }
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}
