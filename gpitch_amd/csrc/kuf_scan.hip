// kuf_scan.hip — the Kuf-side hyper-parameter contraction of a Matern-3/2 / Matern-5/2 family WITHOUT the Kuf_bar product.
//
// pdgp_bwd.hip forms Kuf_bar = R (A D) + alpha gm^T (2 M^2 N flops per latent GP) for one purpose when the inducing inputs are
// fixed: the two sums  sum_ij Kuf_bar_ij dK_ij/d(variance, lengthscale).  A Matern kernel of half-integer order is
// semiseparable along sorted inputs: with u = c |z_i - x_j| / l (c = sqrt 3, sqrt 5) every derivative is a polynomial in u
// times e^-u, and on either side of z_i   u^p e^-u   is a sum of (function of i) x (function of j).  So with
//     At = [A diag(2 gv) ; gm^T]   (M + 1 rows),     Rt = [R, alpha]   (M x (M + 1)),     Kuf_bar = Rt At,
//     S_p = sum_ij Kuf_bar_ij u_ij^p e^-u_ij:   Matern-3/2  g_var = S0 + S1,            g_l = v S2 / l
//                                               Matern-5/2  g_var = S0 + S1 + S2 / 3,   g_l = v (S2 + S3) / (3 l)
// the sums need the rows of At only through exponentially weighted moment sums over the frames on each side of z_i.
// The ascending frames are cut into chunks of KS_LC; three launches per family:
//   1. kuf_scan_stream_kernel (the one pass over A; bound by LDS issue): per chunk c and row k the moments
//        L[c][k][p] = sum_{j in c} At_kj u^p e^-u,  u = c (e_c - x_j) / l   (e_c: last frame of the chunk)
//        R[c][k][p] = the same with u = c (x_j - s_c) / l                   (s_c: first frame)
//      and, for the thresholds z_i that lie in the chunk (s_c <= z_i < s_{c+1}), the chunk's own entries one by one:
//      Kuf_bar_ij = Rt_i . At[:, j] formed explicitly and contracted with hyper_contract_kernel's per-entry arithmetic
//      (the sqrt(r^2 + 1e-12) of the reference included), so the entries next to the diagonal stay what they are.
//   2. kuf_scan_prefix_kernel: PL[c] = T(c (e_c - e_{c-1}) / l) PL[c-1] + L[c] and the mirror image PR, in place;
//        (T(a) m)^p = e^-a sum_{q <= p} C(p, q) a^(p-q) m^q   moves the reference point by a >= 0 (no cancellation).
//   3. kuf_scan_far_kernel: per threshold i in chunk c_i,  Rt_i . T(..) PL[c_i - 1]  +  Rt_i . T(..) PR[c_i + 1].
// O(M N + M^2) per latent GP instead of O(M^2 N).  Away from the chunk of z_i the reference's sqrt(d^2 / l^2 + 1e-12)
// becomes |d| / l: dK/dl carries r^2 - 1e-12 = rho^2 exactly, K is flat at 0, and e^(-c (r - rho)) deviates by at most
// c 5e-13 / rho against a weight ~ rho^2.  Matern-1/2 (a kink at 0: the entry at d = 0 would be off by 1e-6) and RBF (not
// semiseparable) keep the product.  Every sum has a fixed order and there are no atomics: two runs agree bit for bit.
// The number of moment orders NQ is the only place the kernel type enters the layout  mom[chunk][side][q][M + 1].
#include "pdgp_plan.h"

#define KS_LC 64            // frames per chunk = tile width
#define KS_THR 4            // thresholds of a chunk contracted per pass over its tile rows
#define KS_MAXM 1024        // inducing points (the chunk's threshold list lives in LDS)
static_assert(KS_THR == 4, "one threshold of a pass per wavefront of the 256-thread workgroup");
#define KS_TB 32            // thresholds per workgroup of the far kernel (one partial record each)

int kuf_scan_nq(int ktype) { return ktype == GP_KERN_MATERN32 ? 3 : (ktype == GP_KERN_MATERN52 ? 4 : 0); }
int kuf_scan_chunks(int N) { return (N + KS_LC - 1) / KS_LC; }
size_t kuf_scan_moment_doubles(int N, int M, int ktype) {
  return (size_t)kuf_scan_chunks(N) * 2 * (size_t)kuf_scan_nq(ktype) * ((size_t)M + 1);
}
int kuf_scan_records(int M) { return (M + KS_TB - 1) / KS_TB + 1; }

typedef const double __attribute__((address_space(1))) * ks_gcptr;
typedef double __attribute__((address_space(1))) * ks_gptr;

template <int KT> struct KsType {
  static constexpr int NQ = (KT == GP_KERN_MATERN52) ? 4 : 3;
  static constexpr double CS = (KT == GP_KERN_MATERN52) ? 2.23606797749979 : 1.7320508075688772;
};

// grid (chunks, GPs of the family), 256 threads.  Lane = frame of the chunk wherever frames are walked.
template <int KT>
__global__ void __launch_bounds__(256) kuf_scan_stream_kernel(const KufScanItem* __restrict__ items, const double* __restrict__ x,
                                                              int n, int32_t* __restrict__ status) {
  constexpr int NQ = KsType<KT>::NQ;
  const KufScanItem it = items[blockIdx.y];
  const int M = it.M, KP = M + 1;
  const int c = blockIdx.x, C = gridDim.x;
  const int j0 = c * KS_LC, nj = min(KS_LC, n - j0);
  const ks_gcptr gA = (ks_gcptr)it.A, gx = (ks_gcptr)x, ggv = (ks_gcptr)it.gv, ggm = (ks_gcptr)it.gm, gR = (ks_gcptr)it.R,
                 galpha = (ks_gcptr)it.alpha, gz = (ks_gcptr)it.z, th = (ks_gcptr)it.theta;
  const ks_gptr gmom = (ks_gptr)it.mom, gnear = (ks_gptr)it.near;
  __shared__ double tile[KS_LC][KS_LC + 1];     // 64 rows of At x the chunk's frames
  __shared__ double wts[2 * NQ][KS_LC];         // [side * NQ + q][frame]: u^q e^-u
  __shared__ double Rs[KS_THR][KS_LC];          // Rt rows of the pass's thresholds, the tile's 64 k
  __shared__ double kbs[4][KS_THR][KS_LC];
  __shared__ unsigned short thr[KS_MAXM];       // thresholds of this chunk, ascending index
  __shared__ int wcount[4];
  __shared__ double red[4][2];
  __shared__ double etab[GP_EXP_TAB];
  gp_exp_tab_init(etab);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double var = th[0], ls = th[1];
  const double inv_ls = 1.0 / ls, kap = KsType<KT>::CS * inv_ls;
  const bool live = (lane < nj);
  const double sc = gx[j0], ec = gx[j0 + nj - 1];
  const double xj = live ? gx[j0 + lane] : ec;
  const double gv2 = live ? 2.0 * ggv[j0 + lane] : 0.0;
  // the promise of gp_pdgp_set_frames_ascending, checked on the pairs this workgroup reads anyway.  Plain stores: every lane
  // that sees a descending pair, in every workgroup and GP, writes the two words, and a factorisation on the helper stream
  // may be raising its own code at the same moment.  Whichever store lands last is a true report; the other one is lost.
  if (wave == 0 && live && j0 + lane + 1 < n && gx[j0 + lane + 1] < xj) { status[0] = 3; status[1] = j0 + lane; }
  __syncthreads();
  if (wave == 0) {
    const double uL = kap * (ec - xj), uR = kap * (xj - sc);
    double pL = live ? gp_exp_neg(-uL, etab) : 0.0, pR = live ? gp_exp_neg(-uR, etab) : 0.0;
#pragma unroll
    for (int q = 0; q < NQ; q++) { wts[q][lane] = pL; wts[NQ + q][lane] = pR; pL *= uL; pR *= uR; }
  }
  // thresholds of the chunk: s_c <= z_i < s_{c+1}, the outermost chunks open-ended (kuf_scan_far_kernel finds the same chunk)
  const double snext = (c + 1 < C) ? gx[j0 + KS_LC] : 0.0;
  int nthr = 0;
  for (int i0 = 0; i0 < M; i0 += 256) {
    const int i = i0 + tid;
    bool in = false;
    if (i < M) { const double zi = gz[i]; in = (c == 0 || zi >= sc) && (c + 1 == C || zi < snext); }
    const unsigned long long mask = __ballot(in);
    if (lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int off = nthr;
    for (int w = 0; w < wave; w++) off += wcount[w];
    if (in) thr[off + __popcll(mask & ((1ull << lane) - 1ull))] = (unsigned short)i;
    nthr += (wcount[0] + wcount[1]) + (wcount[2] + wcount[3]);
    __syncthreads();
  }
  const int ntile = (KP + KS_LC - 1) / KS_LC;
  const int npass = nthr > 0 ? (nthr + KS_THR - 1) / KS_THR : 1;
  // 16 rows of a tile per wavefront, requested one tile ahead; row M of At is gm, rows past it are zero.  EVERY pass walks
  // the chunk's whole (M + 1) x 64 slab again (from L2 after the first), in this one workgroup: inducing inputs spread over
  // the frames cost one or two passes per chunk, but all M of them inside one chunk make M / 4 serial passes of
  // ceil((M + 1) / 64) tiles — 128 x 9 at M = 512 — a single-workgroup tail the rest of the grid does not share.
  auto request = [&](int kt, double (&pre)[16]) {
#pragma unroll
    for (int rr = 0; rr < 16; rr++) {
      const int k = kt * KS_LC + wave * 16 + rr;
      double v = 0.0;
      if (live && k < M) v = gA[(int64_t)k * it.lda + j0 + lane];
      else if (live && k == M) v = ggm[j0 + lane];
      pre[rr] = v;
    }
  };
  double acc_v = 0.0, acc_l = 0.0;
  for (int pass = 0; pass < npass; pass++) {
    const int t0 = pass * KS_THR;
    double kb[KS_THR];
#pragma unroll
    for (int t = 0; t < KS_THR; t++) kb[t] = 0.0;
    double pre[16];
    request(0, pre);
    for (int kt = 0; kt < ntile; kt++) {
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        const int k = kt * KS_LC + wave * 16 + rr;
        tile[wave * 16 + rr][lane] = (k < M) ? pre[rr] * gv2 : pre[rr];
      }
      if (nthr > 0) {
        const int k = kt * KS_LC + lane;
        double v = 0.0;
        if (t0 + wave < nthr && k <= M) {
          const int i = thr[t0 + wave];
          v = (k < M) ? gR[(int64_t)i * M + k] : galpha[i];
        }
        Rs[wave][lane] = v;
      }
      __syncthreads();
      if (kt + 1 < ntile) request(kt + 1, pre);
      if (pass == 0) {
        // moments: lane = row of the tile, the 2 NQ (side, order) pairs dealt to the four wavefronts
        const int cA = wave, cB = wave + 4;
        const bool hasB = (cB < 2 * NQ);
        const int cBc = hasB ? cB : cA;
        double m0 = 0.0, m1 = 0.0;
#pragma unroll 8
        for (int j = 0; j < KS_LC; j++) {
          const double a = tile[lane][j];
          m0 = fma(a, wts[cA][j], m0);
          m1 = fma(a, wts[cBc][j], m1);
        }
        const int k = kt * KS_LC + lane;
        if (k <= M) {
          gmom[((int64_t)c * 2 * NQ + cA) * KP + k] = m0;
          if (hasB) gmom[((int64_t)c * 2 * NQ + cB) * KP + k] = m1;
        }
      }
      if (nthr > 0) {
        // Kuf_bar rows of the pass's thresholds over the chunk: lane = frame, 16 of the tile's k per wavefront
#pragma unroll
        for (int rr = 0; rr < 16; rr++) {
          const double a = tile[wave * 16 + rr][lane];
#pragma unroll
          for (int t = 0; t < KS_THR; t++) kb[t] = fma(Rs[t][wave * 16 + rr], a, kb[t]);
        }
      }
      __syncthreads();
    }
    if (nthr > 0) {
#pragma unroll
      for (int t = 0; t < KS_THR; t++) kbs[wave][t][lane] = kb[t];
      __syncthreads();
      if (t0 + wave < nthr && live) {      // wavefront = threshold, lane = frame: hyper_contract_kernel's entry arithmetic
        const double w = (kbs[0][wave][lane] + kbs[1][wave][lane]) + (kbs[2][wave][lane] + kbs[3][wave][lane]);
        const double zi = gz[thr[t0 + wave]];
        const double a = zi / ls, aa = __dmul_rn(a, a), b = xj / ls, bb = __dmul_rn(b, b);
        const double r2 = __dadd_rn(__dadd_rn(-2.0 * __dmul_rn(a, b), aa), bb);
        double r, rinv;
        gp_sqrt_rsqrt_pos(__dadd_rn(r2, 1e-12), r, rinv);
        double phi, dphi;
        if (KT == GP_KERN_MATERN32) {
          const double s3 = 1.7320508075688772, e = gp_exp_neg(-s3 * r, etab);
          phi = (1.0 + s3 * r) * e; dphi = -3.0 * r * e;
        } else {
          const double s5 = 2.23606797749979, e = gp_exp_neg(-s5 * r, etab);
          phi = (1.0 + s5 * r + (5.0 / 3.0) * r * r) * e; dphi = -(5.0 / 3.0) * r * (1.0 + s5 * r) * e;
        }
        acc_v = fma(w, phi, acc_v);
        acc_l = fma(w * var * dphi, -r2 * rinv * inv_ls, acc_l);
      }
      __syncthreads();
    }
  }
  for (int o = 32; o > 0; o >>= 1) { acc_v += __shfl_down(acc_v, o, 64); acc_l += __shfl_down(acc_l, o, 64); }
  if (lane == 0) { red[wave][0] = acc_v; red[wave][1] = acc_l; }
  __syncthreads();
  if (tid < 2) gnear[(int64_t)c * 2 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

// m <- T(a) m: the moments about a reference point a >= 0 further away; E = e^-a
template <int NQ>
__device__ __forceinline__ void ks_shift(double (&m)[NQ], double a, double E) {
  if constexpr (NQ > 3) m[3] = E * fma(a, fma(a, fma(a, m[0], 3.0 * m[1]), 3.0 * m[2]), m[3]);
  m[2] = E * fma(a, fma(a, m[0], 2.0 * m[1]), m[2]);
  m[1] = E * fma(a, m[0], m[1]);
  m[0] = E * m[0];
}

// grid (ceil((M + 1) / 64), 2 sides, GPs), 64 threads: thread = row of At, a chain over the chunks, in place.
// Eight chunks' moments are requested before the chain walks them (the chain itself is a dozen dependent operations a step).
template <int KT>
__global__ void __launch_bounds__(64) kuf_scan_prefix_kernel(const KufScanItem* __restrict__ items, const double* __restrict__ x, int n) {
  constexpr int NQ = KsType<KT>::NQ;
  const KufScanItem it = items[blockIdx.z];
  __shared__ double etab[GP_EXP_TAB];
  gp_exp_tab_init(etab);
  __syncthreads();
  const int KP = it.M + 1, side = blockIdx.y;
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= KP) return;
  const ks_gcptr gx = (ks_gcptr)x, th = (ks_gcptr)it.theta;
  const ks_gptr gmom = (ks_gptr)it.mom;
  const int C = (n + KS_LC - 1) / KS_LC;
  const double kap = KsType<KT>::CS / th[1];
  double P[NQ];
#pragma unroll
  for (int q = 0; q < NQ; q++) P[q] = 0.0;
  for (int b0 = 0; b0 < C; b0 += 8) {
    double v[8][NQ], a[8];
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int cc = b0 + u;
      a[u] = 0.0;
#pragma unroll
      for (int q = 0; q < NQ; q++) v[u][q] = 0.0;
      if (cc < C) {
        const int c = side ? C - 1 - cc : cc;
#pragma unroll
        for (int q = 0; q < NQ; q++) v[u][q] = gmom[((int64_t)c * 2 * NQ + side * NQ + q) * KP + k];
        if (cc > 0) {
          if (side == 0) a[u] = kap * (gx[min((c + 1) * KS_LC, n) - 1] - gx[c * KS_LC - 1]);   // e_c - e_{c-1}
          else a[u] = kap * (gx[(c + 1) * KS_LC] - gx[c * KS_LC]);                              // s_{c+1} - s_c
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const int cc = b0 + u;
      if (cc < C) {
        const int c = side ? C - 1 - cc : cc;
        ks_shift<NQ>(P, a[u], gp_exp_neg(-a[u], etab));
#pragma unroll
        for (int q = 0; q < NQ; q++) {
          P[q] += v[u][q];
          gmom[((int64_t)c * 2 * NQ + side * NQ + q) * KP + k] = P[q];
        }
      }
    }
  }
}

// grid (ceil(M / KS_TB) + 1, GPs), 256 threads.  Workgroup b < last: thresholds [32 b, 32 b + 32), eight per wavefront, lanes over
// the M + 1 entries of Rt_i; one record [d_variance, d_lengthscale].  The last workgroup adds the chunks' near sums into one more.
template <int KT>
__global__ void __launch_bounds__(256) kuf_scan_far_kernel(const KufScanItem* __restrict__ items, const double* __restrict__ x, int n) {
  constexpr int NQ = KsType<KT>::NQ;
  const KufScanItem it = items[blockIdx.y];
  const int M = it.M, KP = M + 1;
  const int C = (n + KS_LC - 1) / KS_LC;
  const ks_gcptr gx = (ks_gcptr)x, gR = (ks_gcptr)it.R, galpha = (ks_gcptr)it.alpha, gz = (ks_gcptr)it.z, th = (ks_gcptr)it.theta,
                 gmom = (ks_gcptr)it.mom, gnear = (ks_gcptr)it.near;
  const ks_gptr gout = (ks_gptr)it.partials;
  __shared__ double etab[GP_EXP_TAB];
  __shared__ double red[256][2];
  gp_exp_tab_init(etab);
  __syncthreads();
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  if (b == (int)gridDim.x - 1) {
    double s0 = 0.0, s1 = 0.0;
    for (int c = tid; c < C; c += 256) { s0 += gnear[(int64_t)c * 2]; s1 += gnear[(int64_t)c * 2 + 1]; }
    red[tid][0] = s0; red[tid][1] = s1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) { red[tid][0] += red[tid + o][0]; red[tid][1] += red[tid + o][1]; }
      __syncthreads();
    }
    if (tid < 2) gout[(int64_t)b * 2 + tid] = red[0][tid];
    return;
  }
  const double var = th[0], inv_ls = 1.0 / th[1], kap = KsType<KT>::CS * inv_ls;
  double gvar = 0.0, glen = 0.0;
  for (int tt = 0; tt < KS_TB / 4; tt++) {
    const int i = b * KS_TB + wave * (KS_TB / 4) + tt;
    if (i >= M) break;                      // (uniform per wavefront)
    const double zi = gz[i];
    int lo = 0, hi = C;                      // c_i = the last chunk with s_c <= z_i, 0 if there is none
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (gx[mid * KS_LC] <= zi) lo = mid; else hi = mid;
    }
    const int ci = lo;
    double S[NQ];
#pragma unroll
    for (int q = 0; q < NQ; q++) S[q] = 0.0;
#pragma unroll
    for (int side = 0; side < 2; side++) {
      const int cs = side ? ci + 1 : ci - 1;
      if (cs < 0 || cs >= C) continue;
      const double a = side ? kap * (gx[cs * KS_LC] - zi) : kap * (zi - gx[ci * KS_LC - 1]);
      double D[NQ];
#pragma unroll
      for (int q = 0; q < NQ; q++) D[q] = 0.0;
      for (int k = lane; k < KP; k += 64) {
        const double rt = (k < M) ? gR[(int64_t)i * M + k] : galpha[i];
#pragma unroll
        for (int q = 0; q < NQ; q++) D[q] = fma(rt, gmom[((int64_t)cs * 2 * NQ + side * NQ + q) * KP + k], D[q]);
      }
#pragma unroll
      for (int q = 0; q < NQ; q++)
        for (int o = 32; o > 0; o >>= 1) D[q] += __shfl_xor(D[q], o, 64);
      ks_shift<NQ>(D, a, gp_exp_neg(-a, etab));
#pragma unroll
      for (int q = 0; q < NQ; q++) S[q] += D[q];
    }
    if constexpr (KT == GP_KERN_MATERN32) { gvar += S[0] + S[1]; glen += var * S[2] * inv_ls; }
    else { gvar += S[0] + S[1] + S[2] * (1.0 / 3.0); glen += var * (S[2] + S[3]) * inv_ls * (1.0 / 3.0); }
  }
  if (lane == 0) { red[wave][0] = gvar; red[wave][1] = glen; }
  __syncthreads();
  if (tid < 2) gout[(int64_t)b * 2 + tid] = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
}

gp_status launch_kuf_scan(gp_handle h, int ktype, const KufScanItem* d_items, int count, int maxM, const double* x, int n) {
  if (count <= 0) return GP_OK;
  if (kuf_scan_nq(ktype) == 0 || maxM < 1 || maxM > KS_MAXM || n < 1)
    return gp_fail(h, GP_ERR_UNSUPPORTED, "kuf_scan: Matern-3/2 or Matern-5/2, 1 <= M <= 1024");
  const dim3 gs(kuf_scan_chunks(n), count), gp((maxM + 1 + 63) / 64, 2, count), gf(kuf_scan_records(maxM), count);
  const bool m32 = (ktype == GP_KERN_MATERN32);
  {   // (a timer scope per launch: the stream kernel is the HBM-bound one, the other two are M-sized)
    GpTimerScope ts(h, GP_TIMER_HYPER);
    if (m32) hipLaunchKernelGGL((kuf_scan_stream_kernel<GP_KERN_MATERN32>), gs, dim3(256), 0, h->stream, d_items, x, n, h->d_status);
    else hipLaunchKernelGGL((kuf_scan_stream_kernel<GP_KERN_MATERN52>), gs, dim3(256), 0, h->stream, d_items, x, n, h->d_status);
  }
  {
    GpTimerScope ts(h, GP_TIMER_HYPER);
    if (m32) hipLaunchKernelGGL((kuf_scan_prefix_kernel<GP_KERN_MATERN32>), gp, dim3(64), 0, h->stream, d_items, x, n);
    else hipLaunchKernelGGL((kuf_scan_prefix_kernel<GP_KERN_MATERN52>), gp, dim3(64), 0, h->stream, d_items, x, n);
  }
  {
    GpTimerScope ts(h, GP_TIMER_HYPER);
    if (m32) hipLaunchKernelGGL((kuf_scan_far_kernel<GP_KERN_MATERN32>), gf, dim3(256), 0, h->stream, d_items, x, n);
    else hipLaunchKernelGGL((kuf_scan_far_kernel<GP_KERN_MATERN52>), gf, dim3(256), 0, h->stream, d_items, x, n);
  }
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}
