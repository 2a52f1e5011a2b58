// dm_sht.h — pieces of the spherical-harmonic transforms shared by the analysis (dm_btgen.hip) and the synthesis
// (dm_synth.hip): HEALPix ring geometry on the device, the Legendre and twiddle tables, the LDS ring FFT.
#pragma once

#include "dm_common.h"

#include <cstring>
#include <vector>

namespace {

constexpr double kPi = 3.14159265358979323846;

struct ring_geo {
  const double* cth;   // cos(theta) per ring
  const double* sth;   // sin(theta) per ring
  const double* phi0;  // phi of first pixel
  const int* nphi;     // pixels in ring
  const int* start;    // first pixel index
  int nring;
  int npix;
};

// In-place transform of P maps of length N = 2^logn >= 8 held in LDS in bit-reversed order (padded layout: element a
// at a + (a >> sh), Np per map):  X_p[k] = sum_j x_p[j] exp(+2 pi i j k / N).  TW[ph(k)] = exp(+2 pi i k / N), k < N / 2.
// All TPB threads of the block call it after the barrier that follows the load; it ends with a barrier.  These are the passes
// of bt_fused_fft_kernel (dm_btgen.hip), which keeps them inline: its code generation is what its timings were taken with.
template <int P, int TPB>
__device__ __forceinline__ void sht_lds_fft(cplx* X, const cplx* TW, int N, int logn, int sh, int Np, int tid) {
  auto ph = [&](int a2) { return a2 + (a2 >> sh); };
  // ---- stages 1..3: eight consecutive values per unit, in registers
  for (int U = tid; U < P * N / 8; U += TPB) {
    const int p = U / (N / 8), u = U - p * (N / 8);
    cplx* x = X + (size_t)p * Np + ph(u * 8);   // eight values never straddle a padding slot (2^sh >= 32)
    cplx e[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) e[i] = x[i];
#pragma unroll
    for (int i = 0; i < 8; i += 2) { const cplx t = e[i + 1]; e[i + 1] = csub(e[i], t); e[i] = cadd(e[i], t); }
#pragma unroll
    for (int i = 0; i < 8; i += 4) {
      cplx t = e[i + 2]; e[i + 2] = csub(e[i], t); e[i] = cadd(e[i], t);
      t = make_double2(-e[i + 3].y, e[i + 3].x);   // times exp(2 pi i / 4) = +i
      e[i + 3] = csub(e[i + 1], t); e[i + 1] = cadd(e[i + 1], t);
    }
    {
      const double h = 0.70710678118654752440;
      cplx t = e[4]; e[4] = csub(e[0], t); e[0] = cadd(e[0], t);
      t = make_double2(h * (e[5].x - e[5].y), h * (e[5].x + e[5].y));        // times exp(i pi / 4)
      e[5] = csub(e[1], t); e[1] = cadd(e[1], t);
      t = make_double2(-e[6].y, e[6].x);                                       // times i
      e[6] = csub(e[2], t); e[2] = cadd(e[2], t);
      t = make_double2(-h * (e[7].x + e[7].y), h * (e[7].x - e[7].y));       // times exp(3 i pi / 4)
      e[7] = csub(e[3], t); e[3] = cadd(e[3], t);
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = e[i];
  }
  __syncthreads();
  // ---- the remaining stages two at a time (h = half size of the first of the two), a single one at the end if odd
  int sdone = 3;
  for (; sdone + 2 <= logn; sdone += 2) {
    const int h = 1 << sdone;
    const int s1 = N / (2 * h), s2 = N / (4 * h);
    for (int U = tid; U < P * N / 4; U += TPB) {
      const int p = U / (N / 4), u = U - p * (N / 4);
      const int blk = u / h, pos = u - blk * h;
      cplx* x = X + (size_t)p * Np;
      const int a0 = blk * 4 * h + pos;
      const int i0 = ph(a0), i1 = ph(a0 + h), i2 = ph(a0 + 2 * h), i3 = ph(a0 + 3 * h);
      cplx e0 = x[i0], e1 = x[i1], e2 = x[i2], e3 = x[i3];
      const cplx w1 = TW[ph(pos * s1)], w2 = TW[ph(pos * s2)], w3 = TW[ph((pos + h) * s2)];
      cplx t = cmul(w1, e1); e1 = csub(e0, t); e0 = cadd(e0, t);
      t = cmul(w1, e3); e3 = csub(e2, t); e2 = cadd(e2, t);
      t = cmul(w2, e2); e2 = csub(e0, t); e0 = cadd(e0, t);
      t = cmul(w3, e3); e3 = csub(e1, t); e1 = cadd(e1, t);
      x[i0] = e0; x[i1] = e1; x[i2] = e2; x[i3] = e3;
    }
    __syncthreads();
  }
  if (sdone < logn) {
    const int h = N / 2;
    for (int U = tid; U < P * N / 2; U += TPB) {
      const int p = U / h, u = U - p * h;
      cplx* x = X + (size_t)p * Np;
      const int i0 = ph(u), i1 = ph(u + h);
      const cplx t = cmul(TW[ph(u)], x[i1]);
      const cplx e0 = x[i0];
      x[i0] = cadd(e0, t);
      x[i1] = csub(e0, t);
    }
    __syncthreads();
  }
}

// tw[pix][mm] laid out per ring as (2*mmax+1) x nphi row-major: tw[off_r + mm*nphi + j] = exp(i (mm - mmax) phi_j)
__global__ void bt_twiddle_kernel(ring_geo g, int m_lo, int cnt, const size_t* __restrict__ toff, cplx* __restrict__ tw) {
  // rows [0, cnt): m = +m_lo .. +(m_lo + cnt - 1);  rows [cnt, 2 cnt): the same with a minus sign
  const int r = blockIdx.y;
  const int nphi = g.nphi[r];
  const int nm = 2 * cnt;
  const size_t tot = (size_t)nm * nphi;
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
    const int mm = (int)(idx / nphi), j = (int)(idx % nphi);
    const int m = mm < cnt ? m_lo + mm : -(m_lo + mm - cnt);
    // reduce the argument exactly: m*j mod nphi keeps the phase in [0, 2 pi)
    const long long mj = ((long long)m * j) % nphi;
    const double ph = (double)m * g.phi0[r] + 2.0 * kPi * (double)mj / (double)nphi;
    double s, c;
    sincos(ph, &s, &c);
    tw[toff[r] + idx] = make_double2(c, s);
  }
}

// Seeds of the Legendre recurrence that underflow (m ln(1 / sin theta) > 708).  Returns |lambda_mm| / 2^ex in
// (2^-512, 1] with ex a multiple of 512, at most -1024: the square root of
//   lambda_mm^2 = (2m + 1) / (4 pi) prod_{k <= m} sin^2 theta (2k - 1) / (2k),
// a product carried with its own exponent.  Its relative error grows like sqrt(m) ulp; exp(m ln sin theta) would lose
// |m ln sin theta| ulp here.  sin theta = 0 gives 0.  Shared by bt_legendre_kernel and bt_table_peak (dm_btgen.hip).
constexpr double kDblMin = 2.2250738585072014e-308;
constexpr double kTwoP512 = 1.3407807929942597e154;    // 2^512
constexpr double kTwoM512 = 7.458340731200207e-155;    // 2^-512
constexpr double kTwoM256 = 8.636168555094445e-78;     // 2^-256
__host__ __device__ inline double legendre_scaled_seed(int m, double s2, int* ex) {
  double p = (2.0 * m + 1.0) / (4.0 * kPi);
  int e2 = 0;
  for (int k = 1; k <= m; ++k) {
    p *= s2 * ((2.0 * k - 1.0) / (2.0 * k));
    if (p < kTwoM512) { p *= kTwoP512; e2 -= 512; }
  }
  double v = sqrt(p);
  int e = e2 / 2;   // a multiple of 256
  if (e % 512) { v *= kTwoM256; e += 256; }
  *ex = e;
  return v;
}

// One column of the Legendre tables: out[(l - m) * stride] = w * lambda_lm(z), l = m .. lmax, and the same for W and X at
// wo, xo (nullptr: scalar table only); st = sin(theta) > 0 wherever W and X are asked for.  The arithmetic of every
// table of the package: the ring tables (bt_legendre_kernel) and the tables at source positions (dm_sources.hip).
__device__ __forceinline__ void legendre_column(double z, double st, int lmax, int m, double w, size_t stride,
                                                double* __restrict__ out, double* __restrict__ wo, double* __restrict__ xo) {
  const double s2 = st * st;
  double logpre = 0.5 * (log(2.0 * m + 1.0) - log(4.0 * kPi));
  for (int k = 1; k <= m; ++k) logpre += 0.5 * log((2.0 * k - 1.0) / (2.0 * k));
  double lmm = (m > 0) ? exp(logpre + (double)m * log(st)) : exp(logpre);
  // A seed below the smallest normal double (m ln(1 / sin theta) > 708) while the functions come back to order one at
  // higher l: the pair is carried as (value / 2^ex), ex a multiple of 512 stepped up until it is 0.  ex = 0 from the
  // start for every normal seed: the arithmetic and the bits of those columns are the plain recurrence's.
  int ex = 0;
  if (m > 0 && lmm < kDblMin) lmm = legendre_scaled_seed(m, s2, &ex);
  if (m & 1) lmm = -lmm;
  double pm2 = 0.0, pm1 = lmm;  // lambda_{l-2}, lambda_{l-1} as l advances
  out[0] = w * ldexp(lmm, ex);
  if (wo) {
    // l = m term (needs lambda_{m-1,m} = 0)
    if (m >= 2) {
      const double l = m;
      const double nl = 2.0 * sqrt(1.0 / ((l - 1.0) * l * (l + 1.0) * (l + 2.0)));
      const double lm0 = ldexp(lmm, ex);
      wo[0] = -w * nl * (-((l - l * l) / s2 + 0.5 * l * (l - 1.0)) * lm0);
      xo[0] = w * nl * (l / s2) * ((l - 1.0) * z * lm0);
    } else {
      wo[0] = 0.0;
      xo[0] = 0.0;
    }
  }
  for (int l = m + 1; l <= lmax; ++l) {
    double cur;
    if (l == m + 1) {
      cur = sqrt(2.0 * m + 3.0) * z * pm1;
    } else {
      const double a = sqrt((4.0 * l * l - 1.0) / ((double)l * l - (double)m * m));
      const double b = sqrt(((l - 1.0) * (l - 1.0) - (double)m * m) / (4.0 * (l - 1.0) * (l - 1.0) - 1.0));
      cur = a * (z * pm1 - b * pm2);
    }
    if (ex < 0 && fabs(cur) > kTwoP512) { cur *= kTwoM512; pm1 *= kTwoM512; ex += 512; }
    out[(size_t)(l - m) * stride] = w * ldexp(cur, ex);
    if (wo) {
      double wv = 0.0, xv = 0.0;
      if (l >= 2) {
        const double dl = l, dm = m;
        const double nl = 2.0 * sqrt(1.0 / ((dl - 1.0) * dl * (dl + 1.0) * (dl + 2.0)));
        const double c = sqrt((2.0 * dl + 1.0) / (2.0 * dl - 1.0) * (dl * dl - dm * dm));
        wv = -nl * (-((dl - dm * dm) / s2 + 0.5 * dl * (dl - 1.0)) * cur + c * z / s2 * pm1);
        xv = nl * (dm / s2) * ((dl - 1.0) * z * cur - c * pm1);
      }
      wo[(size_t)(l - m) * stride] = w * ldexp(wv, ex);
      xo[(size_t)(l - m) * stride] = w * ldexp(xv, ex);
    }
    pm2 = pm1;
    pm1 = cur;
  }
}

// Legendre tables: lam[loff[m] + (l-m)*nring + r] = w * lambda_lm(theta_r), same for W and X (polarised)
__global__ void bt_legendre_kernel(ring_geo g, int lmax, int m_lo, int mmax, double w, const size_t* __restrict__ loff_,
                                   double* __restrict__ lam, double* __restrict__ Wt, double* __restrict__ Xt) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const int m = m_lo + blockIdx.y;
  const size_t* loff = loff_ - m_lo;  // tables are stored for m_lo .. mmax
  if (r >= g.nring || m > mmax || m > lmax) return;
  legendre_column(g.cth[r], g.sth[r], lmax, m, w, (size_t)g.nring, lam + loff[m] + r, Wt ? Wt + loff[m] + r : nullptr,
                  Wt ? Xt + loff[m] + r : nullptr);
}

struct geo_host {
  ring_geo g;
  std::vector<double> cth, sth, phi0;
  std::vector<int> nphi, start;
};

int upload_geo(dm_ctx* ctx, int nside, const double* cth, const double* sth, geo_host& gh) {
  const int nring = 4 * nside - 1;
  gh.cth.assign(cth, cth + nring);
  gh.sth.assign(sth, sth + nring);
  gh.phi0.resize(nring);
  gh.nphi.resize(nring);
  gh.start.resize(nring);
  int acc = 0;
  for (int r = 0; r < nring; ++r) {
    const int i = r + 1;
    int np_;
    double p0;
    if (i < nside) { np_ = 4 * i; p0 = kPi / (4.0 * i); }
    else if (i <= 3 * nside) { np_ = 4 * nside; p0 = (((i + nside) & 1) == 0) ? kPi / (4.0 * nside) : 0.0; }
    else { const int j = 4 * nside - i; np_ = 4 * j; p0 = kPi / (4.0 * j); }
    gh.nphi[r] = np_;
    gh.phi0[r] = p0;
    gh.start[r] = acc;
    acc += np_;
  }
  gh.g.nring = nring;
  gh.g.npix = acc;
  // one staged copy for the five arrays (every descriptor upload is a copy kernel of its own in the stream)
  std::vector<double> blob(4 * (size_t)nring);
  std::memcpy(blob.data(), gh.cth.data(), sizeof(double) * nring);
  std::memcpy(blob.data() + nring, gh.sth.data(), sizeof(double) * nring);
  std::memcpy(blob.data() + 2 * (size_t)nring, gh.phi0.data(), sizeof(double) * nring);
  int* ib = reinterpret_cast<int*>(blob.data() + 3 * (size_t)nring);
  std::memcpy(ib, gh.nphi.data(), sizeof(int) * nring);
  std::memcpy(ib + nring, gh.start.data(), sizeof(int) * nring);
  double* d = dm_ws_upload(ctx, blob);
  if (!d) return DM_ENOMEM;
  gh.g.cth = d;
  gh.g.sth = d + nring;
  gh.g.phi0 = d + 2 * (size_t)nring;
  gh.g.nphi = reinterpret_cast<const int*>(d + 3 * (size_t)nring);
  gh.g.start = gh.g.nphi + nring;
  return DM_OK;
}

// ---- which Stokes term takes which table ----------------------------------------------------------------------------
// add(input Stokes, table, output Stokes, alpha_re, alpha_im, beta) for the terms of one pass.  Terms whose outputs
// accumulate (E and B each take two products) go in separate passes = separate launches, so that no two tiles of one
// launch touch the same C entries.  Analysis: T = lam . I, V = lam . V, E = W . Q - i X . U, B = W . U + i X . Q; the
// synthesis (Q = W E - i X B, U = W B + i X E) and the Gram products (E' = K_P E - i K_X B, B' = K_P B + i K_X E) apply
// the same Hermitian block.
struct bt_tables {
  double *T = nullptr, *W = nullptr, *X = nullptr;   // the scalar table and the spin-2 pair (polarised only)
  double* operator[](int i) const { return i == 0 ? T : i == 1 ? W : X; }
};
// n doubles per table out of the workspace
bool bt_tables_alloc(dm_ctx* ctx, bool polarised, size_t n, bt_tables& t) {
  t.T = dm_ws_alloc_t<double>(ctx, n);
  if (polarised) { t.W = dm_ws_alloc_t<double>(ctx, n); t.X = dm_ws_alloc_t<double>(ctx, n); }
  return t.T && (!polarised || (t.W && t.X));
}
template <class Add>
void bt_stokes_terms(bool polarised, int pass, const bt_tables& t, double beta0, Add&& add) {
  if (pass == 0) {
    add(0, t.T, 0, 1.0, 0.0, beta0);
    if (!polarised) return;
    add(3, t.T, 3, 1.0, 0.0, beta0);
    add(1, t.W, 1, 1.0, 0.0, beta0);
    add(2, t.W, 2, 1.0, 0.0, beta0);
  } else {
    add(2, t.X, 1, 0.0, -1.0, 1.0);
    add(1, t.X, 2, 0.0, 1.0, 1.0);
  }
}

}  // namespace
