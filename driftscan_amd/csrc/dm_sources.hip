// dm_sources.hip — exact a_lm of a catalogue of point sources: an analysis over an irregular set of colatitudes.
//   a^T_lm(f) = sum_s I_s(f) lambda_lm(z_s) e^{-i m phi_s}            (a^V alike)
//   a^E_lm(f) = sum_s e^{-i m phi_s} (W_lm Q_s(f) + i X_lm U_s(f)),    a^B_lm(f) = sum_s e^{-i m phi_s} (W_lm U_s(f) - i X_lm Q_s(f))
// the conjugate of what the ring analysis of dm_btgen.hip sums (c_lm = sum w f Y_lm): the same term list
// (bt_stokes_terms) with the sign of the imaginary factors turned.
//
// Stages per (pass of m-blocks, chunk of sources): the tables lambda, W, X at the sources' colatitudes
// (src_legendre_kernel: legendre_column of dm_sht.h, the arithmetic of the ring tables), the phased fluxes
// F_s(f) e^{-i m phi_s} (src_phase_kernel), then per m-block the grouped products complex x real on the matrix cores.
//
// What fixes the bits: sources go in chunks of SRC_CHUNK in catalogue order, each chunk added onto the sum of those
// before it; one grouped launch holds the products of one chunk, one pass of terms and one block of SRC_MBLK m-values
// aligned to multiples of SRC_MBLK, whatever the memory budget — `max_bytes` only sets how many such blocks have their
// tables alive at once.  Inside a product every output is one accumulator walked through the sources of the chunk in order.
#include "dm_sht.h"
#include "dm_kernels.h"
#include "../../include/driftmi.h"

#include <algorithm>
#include <string>
#include <vector>

namespace {

constexpr int SRC_CHUNK = 1024;   // sources per product (its inner dimension)
constexpr int SRC_MBLK = 8;       // m-values per grouped launch
constexpr int SRC_PT = 64;        // sources per workgroup of the phase kernel

// tab[loff[m - m0] + (l - m) * nsc + s] = lambda_lm(z_s), l = m .. lmax, for the m of [m0, m0 + gridDim.y) and the nsc
// sources at z, sth; Wt, Xt alike (nullptr: unpolarised).  One thread per (source, m).  At a pole (sin theta = 0) W and X
// divide by zero and multiply fluxes the entry point has checked to be zero: zeros are stored.
__global__ __launch_bounds__(64) void src_legendre_kernel(const double* __restrict__ z, const double* __restrict__ sth, int nsc,
                                                          int lmax, int m0, const size_t* __restrict__ loff,
                                                          double* __restrict__ lam, double* __restrict__ Wt,
                                                          double* __restrict__ Xt) {
  const int s = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = m0 + blockIdx.y;
  if (s >= nsc || m > lmax) return;
  const size_t o = loff[blockIdx.y] + s;
  const double st = sth[s];
  const bool spin2 = Wt && st > 0.0;
  legendre_column(z[s], st, lmax, m, 1.0, (size_t)nsc, lam + o, spin2 ? Wt + o : nullptr, spin2 ? Xt + o : nullptr);
  if (Wt && !spin2)
    for (int l = m; l <= lmax; ++l) {
      Wt[o + (size_t)(l - m) * nsc] = 0.0;
      Xt[o + (size_t)(l - m) * nsc] = 0.0;
    }
}

// A[((mi * npol + p) * nsc + s) * nf + f] = flux[(f * npol + p) * nsrc + s0 + s] * e^{-i m phi_s}, m = m0 + mi = m0 + blockIdx.y:
// sincos of the double product m * phi, no recurrence in m.  A workgroup takes SRC_PT sources.
__global__ __launch_bounds__(256) void src_phase_kernel(const double* __restrict__ phi, const double* __restrict__ flux, int nsrc,
                                                        int s0, int nsc, int nf, int npol, int m0, cplx* __restrict__ A) {
  __shared__ double cs[SRC_PT], sn[SRC_PT];
  const int t0 = blockIdx.x * SRC_PT;
  const int nt = min(SRC_PT, nsc - t0);
  const int m = m0 + blockIdx.y;
  if ((int)threadIdx.x < nt) {
    double s, c;
    sincos((double)m * phi[s0 + t0 + threadIdx.x], &s, &c);
    cs[threadIdx.x] = c;
    sn[threadIdx.x] = -s;
  }
  __syncthreads();
  for (int p = 0; p < npol; ++p) {
    cplx* Ap = A + (((size_t)blockIdx.y * npol + p) * nsc + t0) * nf;
    for (int e = threadIdx.x; e < nt * nf; e += 256) {
      const int sl = e / nf, f = e - sl * nf;
      const double v = dm_ldg(flux, ((size_t)f * npol + p) * nsrc + s0 + t0 + sl);
      dm_stg(Ap, (size_t)e, make_double2(v * cs[sl], v * sn[sl]));
    }
  }
}

// bytes of tables and phased fluxes alive for the m of [ma, mb] with nsc sources in the chunk
size_t src_block_bytes(int ma, int mb, int lmax, int nsc, int nf, int npol) {
  size_t rows = 0;
  for (int m = ma; m <= mb; ++m) rows += (size_t)(lmax + 1 - m);
  return rows * nsc * sizeof(double) * (npol == 4 ? 3 : 1) + (size_t)(mb - ma + 1) * npol * nsc * nf * sizeof(cplx);
}

}  // namespace

extern "C" int dm_source_alm(dm_ctx* ctx, int nsrc, const double* z_dev, const double* sth_dev, const double* phi_dev, int nf,
                             int npol, const double* flux_dev, int lmax, int m_lo, int m_hi, void* alm_dev, size_t max_bytes) {
  if (!ctx) return DM_EARG;
  if (npol != 1 && npol != 4) {
    ctx->err = "dm_source_alm: npol = " + std::to_string(npol) + ", 1 (I) or 4 (I, Q, U, V) expected";
    return DM_EARG;
  }
  DM_ARG(ctx, nsrc >= 0 && nf >= 0 && lmax >= 0 && lmax < 65535 && m_lo >= 0 && m_hi >= m_lo && alm_dev);
  if (m_hi > lmax) {
    ctx->err = "dm_source_alm: m_hi = " + std::to_string(m_hi) + " above lmax = " + std::to_string(lmax);
    return DM_EARG;
  }
  const int L = lmax + 1, nm = m_hi - m_lo + 1;
  const bool pol = npol == 4;
  DM_ARG(ctx, (size_t)npol * L * nm <= (size_t)INT32_MAX && (size_t)nf * SRC_CHUNK <= (size_t)INT32_MAX);
  if (nf == 0) return DM_OK;
  DM_ARG(ctx, nsrc == 0 || (z_dev && sth_dev && phi_dev && flux_dev));
  if (pol && nsrc > 0) {
    // Q and U have no meaning at a pole, and W and X divide by sin^2 theta
    std::vector<double> sth(nsrc);
    DM_TRY(dm_download(ctx, sth.data(), sth_dev, sizeof(double) * nsrc));
    std::vector<int> poles;
    for (int s = 0; s < nsrc; ++s)
      if (!(sth[s] > 0.0)) poles.push_back(s);
    if (!poles.empty()) {
      std::vector<double> fl((size_t)nf * npol * nsrc);
      DM_TRY(dm_download(ctx, fl.data(), flux_dev, sizeof(double) * fl.size()));
      for (int s : poles)
        for (int f = 0; f < nf; ++f)
          if (fl[((size_t)f * npol + 1) * nsrc + s] != 0.0 || fl[((size_t)f * npol + 2) * nsrc + s] != 0.0) {
            ctx->err = "dm_source_alm: source " + std::to_string(s) + " lies at a pole (sin theta = 0) and is polarised: Q and U are undefined there";
            return DM_EARG;
          }
    }
  }
  cplx* alm = reinterpret_cast<cplx*>(alm_dev);
  DM_TRY(dm_fill_zero(ctx, alm, sizeof(cplx) * (size_t)nf * npol * L * nm));   // l < m, and everything without sources
  if (nsrc == 0) return DM_OK;
  dm_ws_scope ws_scope__(ctx);

  const int chmax = std::min(nsrc, SRC_CHUNK);
  for (int ma = m_lo; ma <= m_hi;) {
    // a pass: whole m-blocks [k SRC_MBLK, (k + 1) SRC_MBLK) while their tables fit max_bytes, one at least
    int mb = std::min(m_hi, (ma / SRC_MBLK + 1) * SRC_MBLK - 1);
    size_t bytes = src_block_bytes(ma, mb, lmax, chmax, nf, npol);
    while (mb < m_hi) {
      const int nb = std::min(m_hi, mb + SRC_MBLK);
      const size_t more = src_block_bytes(mb + 1, nb, lmax, chmax, nf, npol);
      if (bytes + more > max_bytes) break;
      bytes += more;
      mb = nb;
    }
    const int cnt = mb - ma + 1;
    for (int s0 = 0; s0 < nsrc; s0 += SRC_CHUNK) {
      const int nsc = std::min(SRC_CHUNK, nsrc - s0);
      dm_ws_scope pass_scope__(ctx);   // (re-use is ordered by the stream)
      std::vector<size_t> loff(cnt);
      size_t ltot = 0;
      for (int m = ma; m <= mb; ++m) { loff[m - ma] = ltot; ltot += (size_t)(L - m) * nsc; }
      size_t* d_loff = dm_ws_upload(ctx, loff);
      bt_tables tab;
      cplx* A = dm_ws_alloc_t<cplx>(ctx, (size_t)cnt * npol * nsc * nf);
      if (!bt_tables_alloc(ctx, pol, ltot, tab) || !d_loff || !A) return DM_ENOMEM;
      DM_PLAUNCH(ctx, DM_PROF_BT_OTHER, src_legendre_kernel, dim3((unsigned)((nsc + 63) / 64), (unsigned)cnt), dim3(64), 0, ctx->stream,
                 z_dev + s0, sth_dev + s0, nsc, lmax, ma, d_loff, tab.T, tab.W, tab.X);
      DM_PLAUNCH(ctx, DM_PROF_UTIL, src_phase_kernel, dim3((unsigned)((nsc + SRC_PT - 1) / SRC_PT), (unsigned)cnt), dim3(256), 0,
                 ctx->stream, phi_dev, flux_dev, nsrc, s0, nsc, nf, npol, ma, A);
      DM_HIP(ctx, hipGetLastError());
      for (int ba = ma; ba <= mb;) {
        const int bb = std::min(mb, (ba / SRC_MBLK + 1) * SRC_MBLK - 1);
        for (int pass = 0; pass < (pol ? 2 : 1); ++pass) {
          std::vector<dm_gemm_desc> g;
          for (int m = ba; m <= bb; ++m)
            bt_stokes_terms(pol, pass, tab, s0 == 0 ? 0.0 : 1.0,
                            [&](int pin, const double* t, int pout, double are, double aim, double beta) {
              dm_gemm_desc d = dm_gemm_make(A + ((size_t)(m - ma) * npol + pin) * nsc * nf, 1, nf, false, t + loff[m - ma], 1, nsc,
                                            false, alm + ((size_t)pout * L + m) * nm + (m - m_lo), npol * L * nm, nf, L - m, nsc,
                                            are, beta, nullptr, DM_GEMM_B_REAL);
              d.csc = nm;
              d.alpha_im = aim == 0.0 ? 0.0 : -aim;   // a_lm = sum f conj(Y_lm): the conjugate of the ring analysis
              g.push_back(d);
            });
          DM_TRY(dm_gemm_grouped_launch(ctx, g));
        }
        ba = bb + 1;
      }
    }
    ma = mb + 1;
  }
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}
