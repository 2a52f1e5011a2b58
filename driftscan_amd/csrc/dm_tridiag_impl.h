// dm_tridiag_impl.h — panel route of the batched Hermitian eigensolver: the one-stage panel reduction, the two-stage
// reduction (dm_sbr_impl.h, 32-wide build only), and the driver that chains them with the divide & conquer and the
// back-transformation.  Compiled once per panel width (DM_TNB) inside the namespace DM_TRD_NS by dm_tridiag.hip, after
// the kernels and stages that do not depend on the width.  No include guard on purpose.
namespace DM_TRD_NS {

namespace {

constexpr int TNB = DM_TNB;  // reflectors per panel (her2k runs at K = 2 TNB)

struct trd_mat {
  cplx* A; int lda; int n;
  cplx* Vt;      // n x n: row k = Householder vector k (zero for index <= k, 1 at k+1)
  cplx* Vp;      // TNB x n panel of V (row j = vector of panel column j)
  cplx* Wp;      // TNB x n panel of W, stored right behind Vp ...
  cplx* Vp2;     // ... and a second copy of V behind W: [V; W] and [W; V] are both contiguous (her2k at K = 2 TNB)
  cplx* x;       // n: unnormalised Householder column of the current step
  cplx* p;       // n: row part of A v
  cplx* Pc;      // (n / SYG + 1) x n: mirrored (column) parts of A v, one row per SYG-row group
  double* Sp;    // n / SYG + 1: partial sums of v^H A v
  double* Np;    // n / WXR + 1: partial sums of |x|^2
  cplx* ab;      // 2*TNB scratch: panel dot products W^H v, V^H v
  double* d;     // n
  double* e;     // n
  cplx* tau;     // n
};

// ---- T1: one column of the reduction = two launches, both spread over (row tiles x matrices) ----
//
// Only the UPPER triangle of the trailing matrix is kept up to date (her2k writes tiles on or
// above the block diagonal) and the matrix-vector product reads each stored element once:
//
//   trd_symv(k)  every wave derives the Householder scalars (beta, tau, 1/(alpha-beta)) of column k
//                from the partial norms left by trd_wx and forms v on the fly from the unnormalised
//                column x.  A wave owns SYR = 4 consecutive rows r and streams them in 64-column
//                chunks c >= r: the row part  sum_c A[r][c] v[c]  is accumulated per row, the
//                mirrored part  conj(A[r][c]) v[r]  per column, and written as one partial row
//                Pc[group][c] (no atomics: the consumer adds the partial rows in a fixed order).
//                It also writes v, e[k], tau[k], the panel dot products a = W^H v, b = V^H v and the
//                partial sums of v^H A v (which give p^H v without another pass over p).
//   trd_wx(k)    finishes w_k = tau (A v - V a - W b) - (tau/2)(p^H v) v  for its 64 rows and, in
//                the same pass over the panel rows V[:, i], W[:, i], forms the next column
//                x_{k+1} = conj(A[k+1][i]) - V conj(W[k+1]) - W conj(V[k+1])  and its partial norms.
//
// HBM traffic per column: (n-k)^2/2 matrix elements + one pass over the panel (the zlatrd scheme
// reads the full square and the panel twice).
#ifndef DM_SYR
#define DM_SYR 4
#endif
#ifndef DM_SYC
#define DM_SYC 2
#endif
constexpr int SYR = DM_SYR;     // rows per wave in trd_symv
#ifndef DM_SYW
#define DM_SYW 4
#endif
constexpr int SYW = DM_SYW;     // waves per workgroup in trd_symv
constexpr int SYG = SYW * SYR;  // rows per workgroup = rows behind one partial row of Pc
constexpr int SYC = DM_SYC;        // 64-column chunks per loop iteration of trd_symv
constexpr int WXR = 64;    // rows per workgroup in trd_wx

struct trd_refl { cplx tau, scal; double beta; };

// Householder scalars of column k from this lane's share of the partial norms and alpha = x[k+1]
__device__ __forceinline__ trd_refl trd_reflector_from(double npart_lane, cplx alpha) {
  const double xnorm2 = dm_wave_sum(npart_lane);
  trd_refl R;
  if ((xnorm2 == 0.0 && alpha.y == 0.0) || alpha.x * alpha.x + alpha.y * alpha.y + xnorm2 < DM_REFL_TINY) {
    R.tau = make_double2(0.0, 0.0);
    R.beta = alpha.x;
    R.scal = make_double2(0.0, 0.0);
  } else {
    R.beta = -copysign(sqrt(alpha.x * alpha.x + alpha.y * alpha.y + xnorm2), alpha.x);
    R.tau = make_double2((R.beta - alpha.x) / R.beta, -alpha.y / R.beta);
    const double dr = alpha.x - R.beta, di = alpha.y;  // 1 / (alpha - beta)
    const double den = dr * dr + di * di;
    R.scal = make_double2(dr / den, -di / den);
  }
  return R;
}

// the partial norms are fetched one per lane and folded with shuffles: a serial scalar loop
// over up to n/64 partials would put that many dependent load latencies in front of every wave
__device__ __forceinline__ double trd_npart_lane(const trd_mat& M, int k) {
  const int np = (M.n - k + WXR - 1) / WXR;
  double s = 0.0;
  for (int t = threadIdx.x & 63; t < np; t += 64) s += dm_ldg(M.Np, t);
  return s;
}

__device__ __forceinline__ trd_refl trd_reflector(const trd_mat& M, int k) {
  const double npart = trd_npart_lane(M, k);
  const cplx alpha = dm_ldg(M.x, k + 1);
  return trd_reflector_from(npart, alpha);
}

// v[c] for c > k (v[k+1] = 1, the rest is the scaled column)
__device__ __forceinline__ cplx trd_v_at(const trd_mat& M, const trd_refl& R, int k, int c) {
  const cplx t = cmul(dm_ldg(M.x, c), R.scal);
  return c == k + 1 ? make_double2(1.0, 0.0) : t;
}

__global__ __launch_bounds__(64 * SYW) void trd_symv_kernel(const trd_mat* __restrict__ ms, int k, int j) {
  const trd_mat M = ms[blockIdx.y];
  const int n = M.n;
  if (k >= n - 1) return;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // scalar: row bases stay in SGPRs
  // the panel dot products take SLV vectors per wave: v is formed once per element and reused
  constexpr int SLV = 4;
  const int nslot = (2 * j + SLV - 1) / SLV;
  const int nslotblk = (nslot + SYW - 1) / SYW;
  if ((int)blockIdx.x >= nslotblk && k + 1 + SYG * ((int)blockIdx.x - nslotblk) >= n) return;  // no rows left
  if ((int)blockIdx.x < nslotblk && (int)blockIdx.x * SYW + wave >= nslot) return;
  if ((int)blockIdx.x < nslotblk) {
    const trd_refl R = trd_reflector(M, k);
    // a[q] = W_q^H v, b[q] = V_q^H v (needed by trd_wx); vector index q < j: W_q, else V_{q-j}
    const int q0 = (blockIdx.x * SYW + wave) * SLV;
    const cplx* xs[SLV];
#pragma unroll
    for (int u = 0; u < SLV; ++u) {
      const int q = min(q0 + u, 2 * j - 1);
      xs[u] = (q < j ? M.Wp + (size_t)q * n : M.Vp + (size_t)(q - j) * n);
    }
    double sr[SLV], si[SLV];
#pragma unroll
    for (int u = 0; u < SLV; ++u) sr[u] = si[u] = 0.0;
    for (int i = k + 1 + lane; i < n; i += 64) {
      const cplx vv = trd_v_at(M, R, k, i);
#pragma unroll
      for (int u = 0; u < SLV; ++u) {
        const cplx xx = dm_ldg(xs[u], i);  // conj(x) * v
        sr[u] += xx.x * vv.x + xx.y * vv.y;
        si[u] += xx.x * vv.y - xx.y * vv.x;
      }
    }
#pragma unroll
    for (int u = 0; u < SLV; ++u) {
      const double tr = dm_wave_sum(sr[u]), ti = dm_wave_sum(si[u]);
      if (lane == 0 && q0 + u < 2 * j) M.ab[q0 + u] = make_double2(tr, ti);
    }
    return;
  }
  // ---- a workgroup owns SYG = 4 SYR consecutive rows; its four waves walk the same 64-column
  // chunks (starting at the group's first row) so that the mirrored column sums of the whole
  // group can be folded through LDS into ONE partial row Pc[g][:]
  const int g = blockIdx.x - nslotblk;
  const int R0 = k + 1 + SYG * g;
  if (R0 >= n) return;
  __shared__ cplx colbuf[2][SYC][SYW][64];
  __shared__ double sbuf[SYW];
  const int rstart = R0 + SYR * wave;
  const int dl = SYR * wave;  // lane of this wave's first diagonal element in chunk 0
  const cplx* __restrict__ A = M.A;
  const size_t lda = M.lda;
  cplx* __restrict__ pc = M.Pc + (size_t)g * n;
  const cplx zero = make_double2(0.0, 0.0);

  // Loads always hit a valid address (indices clamped) and are masked afterwards, so the row
  // loads of a chunk are issued back to back instead of one branch each.
  int c = R0 + lane;
  bool valid = c < n;
  int cc = min(c, n - 1);
  // Every load of the prologue is issued before anything waits: the partial norms, alpha, the
  // column values under this chunk and the SYR matrix rows are independent of each other, only
  // their USE needs the Householder scalars — one exposed memory latency instead of three.
  const double npart = trd_npart_lane(M, k);
  const cplx alpha = dm_ldg(M.x, k + 1);
  const cplx xraw0 = dm_ldg(M.x, cc);
  cplx araw[SYR];
#pragma unroll
  for (int rr = 0; rr < SYR; ++rr) araw[rr] = dm_ldg(A, (size_t)min(rstart + rr, n - 1) * lda + cc);
  const trd_refl R = trd_reflector_from(npart, alpha);
  const cplx vc0t = (cc == k + 1) ? make_double2(1.0, 0.0) : cmul(xraw0, R.scal);
  const cplx vc0 = valid ? vc0t : zero;
  if (wave == 0) {
    if (lane < SYG && valid) {
      M.Vp[(size_t)j * n + c] = vc0;
      M.Vp2[(size_t)j * n + c] = vc0;
      M.Vt[(size_t)k * n + c] = vc0;
    }
    if (g == 0 && lane == 0) {
      M.e[k] = R.beta;
      M.tau[k] = R.tau;
    }
  }
  cplx vr[SYR];
#pragma unroll
  for (int rr = 0; rr < SYR; ++rr) vr[rr] = make_double2(__shfl(vc0.x, dl + rr, 64), __shfl(vc0.y, dl + rr, 64));
  double acc[2 * SYR];
#pragma unroll
  for (int q = 0; q < 2 * SYR; ++q) acc[q] = 0.0;
  double adiag = 0.0;
  int t = 0;
  {
    cplx a[SYR];
#pragma unroll
    for (int rr = 0; rr < SYR; ++rr) {
      const int r = rstart + rr;
      a[rr] = (valid && r < n && c >= r) ? araw[rr] : zero;
    }
    cplx col = zero;
#pragma unroll
    for (int rr = 0; rr < SYR; ++rr) {
      if (lane == dl + rr) adiag = a[rr].x;
      acc[2 * rr] += a[rr].x * vc0.x - a[rr].y * vc0.y;
      acc[2 * rr + 1] += a[rr].x * vc0.y + a[rr].y * vc0.x;
      if (lane > dl + rr) {  // strictly above the diagonal: mirrored contribution conj(a) * v[r]
        col.x += a[rr].x * vr[rr].x + a[rr].y * vr[rr].y;
        col.y += a[rr].x * vr[rr].y - a[rr].y * vr[rr].x;
      }
    }
    colbuf[0][0][wave][lane] = col;
    __syncthreads();
    if (wave == 0 && valid) {
      cplx tsum = colbuf[0][0][0][lane];
#pragma unroll
      for (int w = 1; w < SYW; ++w) tsum = cadd(tsum, colbuf[0][0][w][lane]);
      dm_stg(pc, c, tsum);
    }
    t = 1;
  }
  // main loop: SYC chunks (64 SYC columns) per iteration -> SYC * SYR row loads in flight per lane;
  // HBM latency under load is ~5 us, so the bytes in flight per CU set the streaming rate
#pragma unroll 1
  for (int c0 = R0 + 64; c0 < n; c0 += 64 * SYC, ++t) {
    cplx a[SYC][SYR], vcu[SYC];
    bool vld[SYC];
#pragma unroll
    for (int u = 0; u < SYC; ++u) {
      const int cu = c0 + 64 * u + lane;
      vld[u] = cu < n;
      const int ccu = min(cu, n - 1);
      const cplx vct = trd_v_at(M, R, k, ccu);
      vcu[u] = vld[u] ? vct : zero;
#pragma unroll
      for (int rr = 0; rr < SYR; ++rr) {
        const int r = rstart + rr;
        const cplx v = dm_ldg(A, (size_t)min(r, n - 1) * lda + ccu);
        a[u][rr] = (vld[u] && r < n) ? v : zero;
      }
    }
    const int pb = t & 1;  // double buffer: the reader of iteration t-1 may still be summing
#pragma unroll
    for (int u = 0; u < SYC; ++u) {
      cplx col = zero;
#pragma unroll
      for (int rr = 0; rr < SYR; ++rr) {
        acc[2 * rr] += a[u][rr].x * vcu[u].x - a[u][rr].y * vcu[u].y;
        acc[2 * rr + 1] += a[u][rr].x * vcu[u].y + a[u][rr].y * vcu[u].x;
        col.x += a[u][rr].x * vr[rr].x + a[u][rr].y * vr[rr].y;
        col.y += a[u][rr].x * vr[rr].y - a[u][rr].y * vr[rr].x;
      }
      colbuf[pb][u][wave][lane] = col;
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SYC; ++u)
      if (wave == ((t * SYC + u) & (SYW - 1)) && vld[u]) {
        cplx tsum = colbuf[pb][u][0][lane];
#pragma unroll
        for (int w = 1; w < SYW; ++w) tsum = cadd(tsum, colbuf[pb][u][w][lane]);
        dm_stg(pc, c0 + 64 * u + lane, tsum);
      }
  }
  // Transposing butterfly: the 2 SYR per-lane partial sums are folded so that lane L ends up with
  // the wave total of entry L / PER (2 SYR + log2(PER) shuffles instead of 2 SYR full reductions).
  constexpr int PER = 64 / (2 * SYR);
#pragma unroll
  for (int o = 32, cnt = 2 * SYR; cnt > 1; o >>= 1, cnt >>= 1) {
    const bool lo = (lane & o) == 0;
    const int h = cnt >> 1;
#pragma unroll
    for (int q = 0; q < h; ++q) {
      const double send = lo ? acc[q + h] : acc[q];
      const double keep = lo ? acc[q] : acc[q + h];
      acc[q] = keep + __shfl_xor(send, o, 64);
    }
  }
  double tot = acc[0];
#pragma unroll
  for (int o = PER / 2; o > 0; o >>= 1) tot += __shfl_xor(tot, o, 64);
  const double tim = __shfl_down(tot, PER, 64);  // lane 2 PER rr: tot = re, tim = im of row rr
  const int rr = lane / (2 * PER);
  const double vrx = __shfl(vc0.x, dl + rr, 64), vry = __shfl(vc0.y, dl + rr, 64), ad = __shfl(adiag, dl + rr, 64);
  double s = 0.0;
  if (lane % (2 * PER) == 0 && rstart + rr < n) {
    M.p[rstart + rr] = make_double2(tot, tim);
    s = 2.0 * (vrx * tot + vry * tim) - ad * (vrx * vrx + vry * vry);  // v^H A v, upper storage
  }
  s = dm_wave_sum(s);
  if (lane == 0) sbuf[wave] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double tsum = 0.0;
#pragma unroll
    for (int w = 0; w < SYW; ++w) tsum += sbuf[w];
    M.Sp[g] = tsum;
  }
}

__global__ __launch_bounds__(256) void trd_wx_kernel(const trd_mat* __restrict__ ms, int k, int j, int do_w, int do_x) {
  const trd_mat M = ms[blockIdx.y];
  const int n = M.n;
  const bool w_on = do_w && k < n - 1;
  const int kx = do_w ? k + 1 : k;  // column whose x is formed; also the first row handled
  const bool x_on = do_x && kx < n;
  if (!w_on && !x_on) return;
  if (kx + (int)blockIdx.x * WXR >= n) return;
  // 64 rows per workgroup, four waves per row block: wave q takes the panel vectors and the
  // partial rows of A v with index = q (mod 4); wave 0 folds the four partial results and finishes.
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int i = kx + blockIdx.x * WXR + lane;
  const int npan = do_w ? j : 0;  // finished panel vectors
  __shared__ cplx sa[TNB], sb[TNB], swk[TNB], svk[TNB];
  __shared__ cplx qbuf[3][WXR], xbuf[3][WXR];
  // wave 0 finishes the rows: everything it will need from global memory that does not depend on
  // the other waves is requested now, so that its tail pays no further memory latency
  cplx e_tau = make_double2(0.0, 0.0), e_vv = make_double2(0.0, 0.0), e_a = make_double2(0.0, 0.0),
       e_pkx = make_double2(0.0, 0.0);
  double e_s = 0.0;
  if (wave == 0) {
    if (w_on) {
      e_tau = dm_ldg(M.tau, k);
      const int ng = (n - k - 1 + SYG - 1) / SYG;
      for (int t = lane; t < ng; t += 64) e_s += dm_ldg(M.Sp, t);
      if (i < n) e_vv = dm_ldg(M.Vp, (size_t)j * n + i);
      if (x_on) e_pkx = dm_ldg(M.p, kx);
    }
    if (x_on && i < n) e_a = dm_ldg(M.A, (size_t)kx * M.lda + i);
  }
  if (tid < npan) {
    sa[tid] = M.ab[tid];
    sb[tid] = M.ab[j + tid];
    if (x_on) {
      swk[tid] = M.Wp[(size_t)tid * n + kx];
      svk[tid] = M.Vp[(size_t)tid * n + kx];
    }
  }
  __syncthreads();
  cplx q = make_double2(0.0, 0.0), xacc = make_double2(0.0, 0.0);
  if (i < n) {
    if (w_on) {
      if (wave == 0) q = M.p[i];
      const int gi = (i - k - 1) / SYG;
      const cplx* __restrict__ pc = M.Pc + i;
#pragma unroll 4
      for (int g = wave; g <= gi; g += 4) q = cadd(q, dm_ldg(pc, (size_t)g * n));
    }
    const cplx* __restrict__ vp = M.Vp + i;
    const cplx* __restrict__ wp = M.Wp + i;
#pragma unroll 4
    for (int jj = wave; jj < npan; jj += 4) {
      const cplx vji = dm_ldg(vp, (size_t)jj * n), wji = dm_ldg(wp, (size_t)jj * n);
      q = csub(q, cadd(cmul(vji, sa[jj]), cmul(wji, sb[jj])));
      if (x_on) xacc = csub(xacc, cadd(cmulc(vji, swk[jj]), cmulc(wji, svk[jj])));
    }
  }
  if (wave > 0) {
    qbuf[wave - 1][lane] = q;
    xbuf[wave - 1][lane] = xacc;
  }
  __syncthreads();
  if (wave > 0) return;
  q = cadd(cadd(q, qbuf[0][lane]), cadd(qbuf[1][lane], qbuf[2][lane]));
  xacc = cadd(cadd(xacc, xbuf[0][lane]), cadd(xbuf[1][lane], xbuf[2][lane]));
  cplx tau = make_double2(0.0, 0.0), wk1 = make_double2(0.0, 0.0);
  double coef = 0.0;
  if (w_on) {
    tau = e_tau;
    double s = e_s, ab = 0.0, cr = 0.0, ci = 0.0;
    for (int t = lane; t < npan; t += 64) {
      ab += sa[t].x * sb[t].x + sa[t].y * sb[t].y;  // Re(conj(a) b)
      if (x_on) {
        const cplx u = cadd(cmul(svk[t], sa[t]), cmul(swk[t], sb[t]));
        cr += u.x;
        ci += u.y;
      }
    }
    s = dm_wave_sum(s);
    ab = dm_wave_sum(ab);
    cr = dm_wave_sum(cr);
    ci = dm_wave_sum(ci);
    // p^H v = conj(tau) (v^H A v - a^H b - b^H a)  (real);  coef = (tau/2) p^H v
    coef = 0.5 * (tau.x * tau.x + tau.y * tau.y) * (s - 2.0 * ab);
    if (x_on) {  // w_k[k+1]: the mirrored part of p vanishes on the first trailing row
      const cplx q1 = csub(e_pkx, make_double2(cr, ci));
      wk1 = cmul(tau, q1);
      wk1.x -= coef;
    }
  }
  double part = 0.0;
  if (i < n) {
    cplx wv = make_double2(0.0, 0.0), vv = make_double2(0.0, 0.0);
    if (w_on) {
      vv = e_vv;
      wv = cmul(tau, q);
      wv.x -= coef * vv.x;
      wv.y -= coef * vv.y;
      M.Wp[(size_t)j * n + i] = wv;
    }
    if (x_on) {
      const cplx a = e_a;
      cplx xx = make_double2(a.x + xacc.x, -a.y + xacc.y);
      if (w_on) xx = csub(xx, cadd(cmulc(vv, wk1), wv));  // panel vector j: V[j][kx] = 1
      M.x[i] = xx;
      if (i == kx) M.d[kx] = xx.x;
      if (i > kx + 1) part = cabs2(xx);
    }
  }
  if (x_on) {
    part = dm_wave_sum(part);
    if (lane == 0) M.Np[blockIdx.x] = part;
  }
}

// ---- T4 helper: T factor of a block of reflectors from its Gram matrix (zlarft, forward/columnwise) ----
struct tf_mat {
  cplx* G; const cplx* tau; cplx* T; int kb; int ldt;  // G: TNB x TNB row-major; T: leading dimension ldt
  const cplx* part; int nslice;                         // nslice > 0: G = sum of nslice (kb x kb) slices at `part` (stored to G)
};
// The Gram matrix goes to LDS first (summed over the split-K slices if there are any) and the recurrence runs from LDS with
// eight threads per row of T sharing each dot product: 32 dependent steps of a few operations each (one thread per row
// walking along it, waiting for a global load per element, took 50 us per call).
__global__ __launch_bounds__(256) void larft_kernel(const tf_mat* __restrict__ ts) {
  const tf_mat F = ts[blockIdx.x];
  extern __shared__ __align__(16) unsigned char larft_smem[];
  cplx (*T)[TNB + 1] = reinterpret_cast<cplx (*)[TNB + 1]>(larft_smem);
  cplx (*Gl)[TNB + 1] = reinterpret_cast<cplx (*)[TNB + 1]>(larft_smem + sizeof(cplx) * TNB * (TNB + 1));
  const int tid = threadIdx.x, nth = blockDim.x;
  for (int idx = tid; idx < TNB * TNB; idx += nth) {
    const int r = idx / TNB, c = idx % TNB;
    T[r][c] = make_double2(0.0, 0.0);
    cplx g = make_double2(0.0, 0.0);
    if (r < F.kb && c < F.kb) {
      if (F.nslice > 0) {
        const size_t ss = (size_t)F.kb * F.kb, o = (size_t)r * F.kb + c;
        int sl = 0;
        for (; sl + 4 <= F.nslice; sl += 4) {   // four slices in flight (the sum keeps its order)
          const cplx v0 = F.part[sl * ss + o], v1 = F.part[(sl + 1) * ss + o], v2 = F.part[(sl + 2) * ss + o], v3 = F.part[(sl + 3) * ss + o];
          g = cadd(cadd(cadd(cadd(g, v0), v1), v2), v3);
        }
        for (; sl < F.nslice; ++sl) g = cadd(g, F.part[sl * ss + o]);
        F.G[r * TNB + c] = g;
      } else {
        g = F.G[r * TNB + c];
      }
    }
    Gl[r][c] = g;
  }
  __syncthreads();
  constexpr int TPR = 256 / TNB >= 8 ? 8 : 4;   // threads per row of T (8 for the 32-wide panels, 4 for the 64-wide ones)
  const int row = tid / TPR, part = tid % TPR;
  for (int j = 0; j < F.kb; ++j) {
    const cplx tj = F.tau[j];
    // T[0:j, j] = -tau_j * T[0:j, 0:j] * G[0:j, j]   (T upper triangular: columns c >= row)
    cplx acc = make_double2(0.0, 0.0);
    if (row < j)
      for (int c = row + part; c < j; c += TPR) acc = cadd(acc, cmul(T[row][c], Gl[c][j]));
#pragma unroll
    for (int o = 1; o < TPR; o <<= 1) {
      acc.x += __shfl_xor(acc.x, o, 64);
      acc.y += __shfl_xor(acc.y, o, 64);
    }
    if (part == 0 && row < j) T[row][j] = cmul(make_double2(-tj.x, -tj.y), acc);
    if (tid == 0) T[j][j] = tj;
    __syncthreads();
  }
  for (int idx = tid; idx < TNB * TNB; idx += nth) F.T[(size_t)(idx / TNB) * F.ldt + idx % TNB] = T[idx / TNB][idx % TNB];
}

constexpr int NBB = 128;  // back-transformation in compact-WY blocks of NBB reflectors (merged from the TNB-wide panels)

// dynamic LDS of larft_kernel: the T factor and the Gram matrix
constexpr size_t LARFT_LDS = 2 * sizeof(cplx) * TNB * (TNB + 1);
int larft_allow_lds(dm_ctx* ctx) {
  static bool attr = false;
  if (!attr) {
    DM_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(larft_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    (int)LARFT_LDS));
    attr = true;
  }
  return DM_OK;
}

// ---- storage of the panel route.  Problem p owns the slice at its offset of every array: b.off (n x n), b.offn (n),
// offpc / offsp / offnp (partial sums of trd_symv / trd_wx), offtb (T factors), offg (Gram scratch), and offyp / offvd /
// offt2 (two-stage reduction, sb_alloc).  Vt: row k = Householder vector k; PP: per problem the panels V, W, V (trd_mat);
// Tbig: NBB x NBB T factor per block; Gs / Gt: Gram / T_left * Gram scratch; Ut: T V^H (layout of Vt); W1: U^H X.
struct trd_ws {
  const trd_batch& b;
  bool two_stage;
  cplx *Vt{}, *PP{}, *pv{}, *xv{}, *Pcv{}, *abv{}, *tau{}, *Tbig{}, *Gs{}, *Gt{}, *Ut{}, *W1{};
  double *Spv{}, *Npv{}, *dd{}, *ee{};
  size_t tottb = 0, tott2 = 0;
  std::vector<size_t> offpc, offsp, offnp, offtb, offg, offyp, offvd, offt2;
  cplx *sbPw{}, *sbXt{}, *sbYp{}, *sbAB{}, *sbVd{}, *sbTau2{}, *sbM1{}, *sbS{}, *sbPart{};
  double* sbNp{};
  unsigned* sbProg{};
  int* sbNext{};
  std::vector<int> sb_jb;
  trd_ws(const trd_batch& b_, bool two_stage_)
      : b(b_), two_stage(two_stage_), offpc(b.np), offsp(b.np), offnp(b.np), offtb(b.np), offg(b.np), offyp(b.np),
        offvd(b.np), offt2(b.np), sb_jb(b.np) {}
};

#if DM_TNB == 32
#include "dm_sbr_impl.h"
#endif

}  // namespace

static int trd_alloc(dm_ctx* ctx, trd_ws& w) {
  const auto& probs = w.b.probs;
  const int np = w.b.np;
  const size_t tot = w.b.tot, totn = w.b.totn;
  w.Vt = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(tot, 1));
  w.PP = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totn * 3 * TNB, 1));
  w.pv = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totn, 1));
  w.xv = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totn, 1));
  size_t totpc = 0, totsp = 0, totnp = 0;
  for (int p = 0; p < np; ++p) {
    const size_t n = probs[p].n;
    w.offpc[p] = totpc; totpc += (n / SYG + 1) * n;
    w.offsp[p] = totsp; totsp += n / SYG + 1;
    w.offnp[p] = totnp; totnp += n / WXR + 1;
  }
  w.Pcv = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totpc, 1));
  w.Spv = dm_ws_alloc_t<double>(ctx, std::max<size_t>(totsp, 1));
  w.Npv = dm_ws_alloc_t<double>(ctx, std::max<size_t>(totnp, 1));
  w.abv = dm_ws_alloc_t<cplx>(ctx, (size_t)np * 2 * TNB);
  w.dd = dm_ws_alloc_t<double>(ctx, std::max<size_t>(totn, 1));
  w.ee = dm_ws_alloc_t<double>(ctx, std::max<size_t>(totn, 1));
  w.tau = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totn, 1));
  for (int p = 0; p < np; ++p) {
    w.offtb[p] = w.tottb;
    w.tottb += (size_t)((probs[p].n + NBB - 1) / NBB) * NBB * NBB;
  }
  w.Tbig = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(w.tottb, 1));
  size_t totg = 0;
  for (int p = 0; p < np; ++p) {
    w.offg[p] = totg;
    totg += (size_t)(probs[p].n / TNB + 1) * TNB * TNB + (size_t)NBB * NBB;  // enough for every merge level
  }
  w.Gs = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totg, 1));
  w.Gt = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totg, 1));
  w.Ut = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(tot, 1));
  w.W1 = dm_ws_alloc_t<cplx>(ctx, std::max<size_t>(totn * NBB, 1));
  if (!w.Vt || !w.PP || !w.pv || !w.xv || !w.Pcv || !w.Spv || !w.Npv || !w.abv || !w.dd || !w.ee || !w.tau || !w.Tbig ||
      !w.Gs || !w.Gt || !w.Ut || !w.W1)
    return DM_ENOMEM;
  DM_TRY(dm_fill_zero(ctx, w.PP, sizeof(cplx) * totn * 3 * TNB));
  DM_TRY(dm_fill_zero(ctx, w.Vt, sizeof(cplx) * tot));  // trd_symv only writes the non-zero part of each vector
  DM_TRY(dm_fill_zero(ctx, w.tau, sizeof(cplx) * totn));
  return DM_OK;
}

// ---- T1, one stage: per panel of TNB columns two launches per column (trd_symv, trd_wx), then one her2k
static int trd_reduce(dm_ctx* ctx, const trd_ws& w) {
  const auto& probs = w.b.probs;
  const std::vector<int>& order = w.b.order;
  const std::vector<size_t>& offn = w.b.offn;
  const int nc = w.b.np, cmax = w.b.maxn;
  std::vector<trd_mat> tm(nc);
  for (int i = 0; i < nc; ++i) {
    const int p = order[i];
    cplx* pp = w.PP + offn[p] * 3 * TNB;
    const size_t n = probs[p].n;
    tm[i] = trd_mat{probs[p].C, probs[p].ldc, probs[p].n, w.Vt + w.b.off[p], pp, pp + n * TNB, pp + 2 * n * TNB,
                    w.xv + offn[p], w.pv + offn[p], w.Pcv + w.offpc[p], w.Spv + w.offsp[p], w.Npv + w.offnp[p],
                    w.abv + (size_t)p * 2 * TNB, w.dd + offn[p], w.ee + offn[p], w.tau + offn[p]};
  }
  trd_mat* d_tm = dm_ws_upload(ctx, tm);
  if (!d_tm) return DM_ENOMEM;
  for (int k0 = 0; k0 < cmax; k0 += TNB) {
    const int k1 = std::min(k0 + TNB, cmax);
    // first column of the panel: plain row of the (just updated) matrix
    hipLaunchKernelGGL(trd_wx_kernel, dim3((cmax - k0 + WXR - 1) / WXR, nc), dim3(256), 0, ctx->stream, d_tm, k0, 0,
                       0, 1);
    for (int k = k0; k < k1; ++k) {
      const int j = k - k0;
      if (k < cmax - 1) {
        const int ng = (cmax - k - 1 + SYG - 1) / SYG;
        const int nslotblk = ((2 * j + 3) / 4 + SYW - 1) / SYW;  // 4 vectors per wave, SYW waves per workgroup
        // algorithmic HBM bytes of this column: half of every trailing matrix (symv), one pass over
        // the panel rows of V and W (wx)
        // Timed with events on every DM_PROF_TRD_STRIDE-th column only (event records on a chain of
        // ~2400 short launches are not free: all of them cost 7 % of the step); columns are sampled
        // uniformly, so the ratio bytes / time of the sample estimates the average of the kernel.
        // (the sampled position walks through the panel: every column index j of a panel is drawn equally often)
        const bool timed = ctx->prof_on && (k % DM_PROF_TRD_STRIDE) == ((k / DM_PROF_TRD_STRIDE) * 13) % DM_PROF_TRD_STRIDE;
        double by_symv = 0.0, by_wx = 0.0;
        if (timed)
          for (int p : order) {
            const double r = probs[p].n - k - 1;
            if (r > 0) { by_symv += 8.0 * r * r; by_wx += 32.0 * r * j; }
          }
        hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;
        if (timed) { e0 = dm_prof_event(ctx); (void)hipEventRecord(e0, ctx->stream); }
        hipLaunchKernelGGL(trd_symv_kernel, dim3(nslotblk + ng, nc), dim3(64 * SYW), 0, ctx->stream, d_tm, k, j);
        hipEvent_t e1b = nullptr;  // a record owns both of its events: end of symv and start of wx are two events
        if (timed) {
          e1 = dm_prof_event(ctx);
          (void)hipEventRecord(e1, ctx->stream);
          e1b = dm_prof_event(ctx);
          (void)hipEventRecord(e1b, ctx->stream);
        }
        hipLaunchKernelGGL(trd_wx_kernel, dim3((cmax - k - 1 + WXR - 1) / WXR, nc), dim3(256), 0, ctx->stream, d_tm,
                           k, j, 1, k + 1 < k1 ? 1 : 0);
        if (timed) {
          e2 = dm_prof_event(ctx);
          (void)hipEventRecord(e2, ctx->stream);
          // weight = stride: dm_prof_report returns estimates of the totals over ALL columns
          ctx->prof.push_back(dm_ctx::prof_rec{DM_PROF_TRD_SYMV, e0, e1, by_symv, (double)DM_PROF_TRD_STRIDE});
          ctx->prof.push_back(dm_ctx::prof_rec{DM_PROF_TRD_WX, e1b, e2, by_wx, (double)DM_PROF_TRD_STRIDE});
        }
      }
    }
    if (k1 < cmax) {
      // her2k on the upper triangle in one pass: C -= [V W] [W V]^H  (K = 2 TNB; unused panel rows are zero)
      std::vector<dm_gemm_desc> g;
      for (int p : order) {
        const int n = probs[p].n;
        const int rem = n - k1;
        if (rem <= 0) continue;
        const cplx* pp = w.PP + offn[p] * 3 * TNB;
        g.push_back(dm_gemm_make(pp + k1, 1, n, false, pp + (size_t)n * TNB + k1, n, 1, true,
                                 probs[p].C + (size_t)k1 * probs[p].ldc + k1, probs[p].ldc, rem, rem, 2 * TNB, -1.0,
                                 1.0, nullptr, DM_GEMM_UPPER));
      }
      DM_TRY(dm_gemm_grouped_launch(ctx, g));
      // The panel buffers are NOT cleared between panels: every entry a kernel reads has been written inside the
      // current panel — trd_symv / trd_wx read the vectors q < j at rows > k only (v_q and w_q are written for all
      // rows > k0 + q), the her2k above reads rows >= k1 of all TNB vectors of a FULL panel (a matrix that ends
      // inside the panel has n - k1 <= 0 and takes no part).  (170 MB of memset per panel at configs[1].)
    }
  }
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

// ---- T4: X = Q Z into the (now free) storage of C, then W = X^H, for the eigenvectors zsrc[p] / ncolv[p] of trd_select:
// zt_to_x, the reflectors of the bulge chase (two-stage), then the compact-WY blocks of T1, last to first.
static int trd_back_transform(dm_ctx* ctx, const trd_ws& w, const std::vector<const double*>& zsrc,
                              const std::vector<int>& ncolv) {
  const auto& probs = w.b.probs;
  const std::vector<int>& order = w.b.order;
  const std::vector<size_t>& off = w.b.off;
  const int nc = w.b.np, cmax = w.b.maxn;
  const int shift = w.two_stage ? TNB : 1;  // reflector k has its leading 1 at row k + shift
  auto nrefl_of = [&](int n) { return w.two_stage ? std::max(0, n - TNB - 1) : std::max(0, n - 1); };
  std::vector<cvt_mat> cm(nc);
  for (int i = 0; i < nc; ++i)
    cm[i] = cvt_mat{zsrc[order[i]], probs[order[i]].C, probs[order[i]].ldc, probs[order[i]].n, ncolv[order[i]]};
  cvt_mat* d_cm = dm_ws_upload(ctx, cm);
  if (!d_cm) return DM_ENOMEM;
  const int tb = (cmax + 31) / 32;
  DM_PLAUNCH(ctx, DM_PROF_EIG_OTHER, zt_to_x_kernel, dim3(tb, tb, nc), dim3(256), 0, ctx->stream, d_cm);
#if DM_TNB == 32
  if (w.two_stage) DM_TRY(sb_apply_q2(ctx, w, ncolv));
#endif
  // ---- T factors of all blocks up front (they depend on V only), batched over blocks and matrices:
  //   level 0: T of every TNB-wide panel from its Gram matrix (zlarft; S1 of the two-stage reduction left them in Tbig)
  //   merge:   [T_l, -T_l (V_l^H V_r) T_r; 0, T_r] for neighbouring blocks until NBB is reached
  //   U^H = T V^H per block, so that applying a block is two products: W = U^H X, X -= V W
  if (!w.two_stage) {
    DM_TRY(dm_fill_zero(ctx, w.Tbig, sizeof(cplx) * w.tottb));
    std::vector<dm_gemm_desc> g;
    std::vector<tf_mat> tf;
    for (int p : order) {
      const int n = probs[p].n;
      for (int k0 = 0; k0 < n - 1; k0 += TNB) {
        const int kb = std::min(k0 + TNB, n - 1) - k0;
        const int r0 = k0 + 1, nr = n - r0;
        const cplx* Vb = w.Vt + off[p] + (size_t)k0 * n + r0;
        cplx* G = w.Gs + w.offg[p] + (size_t)(k0 / TNB) * TNB * TNB;
        cplx* T = w.Tbig + w.offtb[p] + (size_t)(k0 / NBB) * NBB * NBB + (size_t)(k0 % NBB) * NBB + (k0 % NBB);
        g.push_back(dm_gemm_make(Vb, n, 1, true, Vb, 1, n, false, G, TNB, kb, kb, nr));
        tf.push_back(tf_mat{G, w.tau + w.b.offn[p] + k0, T, kb, NBB, nullptr, 0});
      }
    }
    if (!g.empty()) {
      DM_TRY(dm_gemm_grouped_launch(ctx, g));
      tf_mat* d_tf = dm_ws_upload(ctx, tf);
      if (!d_tf) return DM_ENOMEM;
      DM_TRY(larft_allow_lds(ctx));
      DM_PLAUNCH(ctx, DM_PROF_EIG_OTHER, larft_kernel, dim3((unsigned)tf.size()), dim3(256), LARFT_LDS, ctx->stream, d_tf);
    }
  }
  std::deque<dm_gemm_plan> plans;
  for (int sz = TNB; sz < NBB; sz *= 2) {
    std::vector<dm_gemm_desc> ga, gb, gc;
    for (int p : order) {
      const int n = probs[p].n;
      const int nrefl = nrefl_of(n);
      for (int k0 = 0; k0 + sz < nrefl; k0 += 2 * sz) {  // left block [k0, k0+sz), right block [k0+sz, ...)
        const int kr0 = k0 + sz;
        const int kl = sz, kr = std::min(kr0 + sz, nrefl) - kr0;
        const int r0 = kr0 + shift, nr = n - r0;         // rows where the right block is non-zero
        const cplx* Vl = w.Vt + off[p] + (size_t)k0 * n + r0;
        const cplx* Vr = w.Vt + off[p] + (size_t)kr0 * n + r0;
        cplx* G = w.Gs + w.offg[p] + (size_t)(k0 / (2 * sz)) * sz * sz;
        cplx* H = w.Gt + w.offg[p] + (size_t)(k0 / (2 * sz)) * sz * sz;
        cplx* Tblk = w.Tbig + w.offtb[p] + (size_t)(k0 / NBB) * NBB * NBB;
        const int o = k0 % NBB;
        cplx* Tl = Tblk + (size_t)o * NBB + o;
        cplx* Tr = Tblk + (size_t)(o + sz) * NBB + (o + sz);
        cplx* T12 = Tblk + (size_t)o * NBB + (o + sz);
        ga.push_back(dm_gemm_make(Vl, n, 1, true, Vr, 1, n, false, G, sz, kl, kr, nr));
        gb.push_back(dm_gemm_make(Tl, NBB, 1, false, G, sz, 1, false, H, sz, kl, kr, kl));
        gc.push_back(dm_gemm_make(H, sz, 1, false, Tr, NBB, 1, false, T12, NBB, kl, kr, kr, -1.0, 0.0));
      }
    }
    for (const auto* gv : {&ga, &gb, &gc}) {
      plans.emplace_back();
      DM_TRY(dm_gemm_plan_build(*gv, plans.back()));
    }
  }
  {
    std::vector<dm_gemm_desc> g;
    for (int p : order) {
      const int n = probs[p].n;
      const int nrefl = nrefl_of(n);
      for (int k0 = 0; k0 < nrefl; k0 += NBB) {
        const int kb = std::min(k0 + NBB, nrefl) - k0;
        const int r0 = k0 + shift, nr = n - r0;
        const cplx* T = w.Tbig + w.offtb[p] + (size_t)(k0 / NBB) * NBB * NBB;
        g.push_back(dm_gemm_make(T, NBB, 1, false, w.Vt + off[p] + (size_t)k0 * n + r0, n, 1, true,
                                 w.Ut + off[p] + (size_t)k0 * n + r0, n, kb, nr, kb));
      }
    }
    plans.emplace_back();
    DM_TRY(dm_gemm_plan_build(g, plans.back()));
  }
  // ---- apply the blocks, last to first
  const int nblk = (nrefl_of(cmax) + NBB - 1) / NBB;
  for (int b = nblk - 1; b >= 0; --b) {
    const int k0 = b * NBB;
    std::vector<dm_gemm_desc> g2, g4;
    for (int p : order) {
      const int n = probs[p].n;
      const int kb = std::min(k0 + NBB, nrefl_of(n)) - k0;
      if (kb <= 0) continue;
      // reflectors k >= k0 vanish on rows < k0 + shift: only rows r0.. of X take part
      const int r0 = k0 + shift, nr = n - r0;
      cplx* Xr = probs[p].C + (size_t)r0 * probs[p].ldc;
      cplx* w1 = w.W1 + w.b.offn[p] * NBB;
      const int nx = ncolv[p];  // columns of X = eigenvectors being back-transformed
      if (nx <= 0) continue;
      g2.push_back(dm_gemm_make(w.Ut + off[p] + (size_t)k0 * n + r0, n, 1, false, Xr, probs[p].ldc, 1, false, w1, n, kb,
                                nx, nr));
      g4.push_back(dm_gemm_make(w.Vt + off[p] + (size_t)k0 * n + r0, 1, n, false, w1, n, 1, false, Xr, probs[p].ldc, nr,
                                nx, kb, -1.0, 1.0));
    }
    if (g2.empty()) continue;
    for (const auto* gv : {&g2, &g4}) {
      plans.emplace_back();
      DM_TRY(dm_gemm_plan_build(*gv, plans.back()));
    }
  }
  // the merges of the T factors, U^H = T V^H and the two products per block are a chain of ~25 dependent launches:
  // their descriptors travel in one staged copy, then the launches follow each other without a copy in between
  {
    std::vector<const dm_gemm_plan*> pp;
    for (const auto& pl : plans) pp.push_back(&pl);
    std::vector<const char*> dv;
    DM_TRY(dm_gemm_plans_upload(ctx, pp, dv));
    for (size_t i = 0; i < plans.size(); ++i) DM_TRY(dm_gemm_plan_run(ctx, plans[i], dv[i]));
  }
  {
    std::vector<dm_tdesc> tr;
    for (int p : order) tr.push_back(dm_tdesc{probs[p].C, probs[p].ldc, probs[p].W, probs[p].ldw, probs[p].n, ncolv[p]});
    DM_TRY(dm_conj_transpose_batched(ctx, tr));
  }
  DM_HIP(ctx, hipGetLastError());
  return DM_OK;
}

// ===========================================================================
// panel route: C (destroyed) -> evals (unsorted), W rows = eigenvectors^H, for the batches of n_max > TSM.  The whole
// batch, largest matrices first, goes through the stages on ctx->stream, all matrices in lock-step:
//   T1  the one-stage reduction (trd_reduce) or, when `two_stage` (trd_policy_of), the two-stage one (sb_reduce)
//   T2  the divide & conquer (dc_solve), then the eigenvalues out and the optional selection (trd_select)
//   T4  the back-transformation (trd_back_transform)
// ===========================================================================
int herm_eig_tridiag(dm_ctx* ctx, const trd_batch& b, double* evals, int evals_stride, dm_eig_select* sel,
                     bool two_stage) {
  trd_ws w(b, two_stage);
  DM_TRY(trd_alloc(ctx, w));
#if DM_TNB == 32
  if (two_stage) DM_TRY(sb_reduce(ctx, w));
  else
#endif
    DM_TRY(trd_reduce(ctx, w));
  // Ut is first written by the back-transformation: the D&C borrows it as scratch
  std::vector<const double*> zsrc;
  DM_TRY(dc_solve(ctx, b.probs, w.dd, w.ee, b.offn, b.off, b.tot, b.totn, zsrc, reinterpret_cast<double*>(w.Ut)));
  std::vector<int> ncolv;
  DM_TRY(trd_select(ctx, b, w.dd, evals, evals_stride, sel, zsrc, ncolv));
  DM_TRY(trd_back_transform(ctx, w, zsrc, ncolv));
  DM_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return DM_OK;
}

}  // namespace DM_TRD_NS
