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
//      Where afar.hip formed this step's A (Matern-3/2), kuf_scan_far_moments_kernel takes the place of this launch: the same
//      moments and near sums from A's factors, without the pass over A (below).
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

// ---- launch 1 without the pass over A ---------------------------------------------------------------
// Where afar.hip formed this step's A, the forward pass holds it per 256-frame group S in product form,
//     A[:, S] = P_S B_S,    P_S = [T-_W(S), T+_W(S), W[:, near(S)]]  (M x nr),    B_S = [Psi-; Psi+; Kuf[near(S), S]]  (nr x 256),
// with nr = 4 + (kend - kbeg), about 20.  The chunk moments are linear in A, so
//     mom[c][side][q][k] = sum_r P_S[k, r] y[r][c][q],     y[r][c][q] = sum_{j in c} B_S[r, j] (2 gv_j) w_q(j),
// and a threshold's Kuf_bar row over its own chunk is  2 gv_j (rho_i . B_S[:, j]) + alpha_i gm_j  with  rho_i = R_i P_S:
// W enters once, as in A = W Kuf itself.  One workgroup per (group, GP); a wavefront is one chunk of the group, a lane a frame.
//   phase 1  y for KS_YB rows of B_S at a time (16 rows through LDS per step; a lane sums a quarter chunk, the quarters are
//            added as (q0 + q1) + (q2 + q3)); the gm row's moments go straight to row M
//   phase 2  thread = row k of A: 4 chunks x 2 NQ running sums over those rows of B_S.  W is lower triangular: entries above
//            the diagonal count as zero whatever the buffer holds, and a wavefront stops at the first column past its rows
//   phase 3  KS_TW thresholds per workgroup at a time: rho 16 columns at a time (wavefront = quarter of the k range, lane =
//            column x k mod 4), then wavefront = threshold over its chunk's entries with kuf_scan_stream_kernel's per-entry
//            arithmetic.  One record per threshold in LDS, added per chunk in list order by one thread.
// Every sum has a fixed order, no atomics.  Any near-row count and any number of thresholds per chunk: nothing depends on
// what fits on chip (rows past KS_YB continue the running sums through mom itself: same thread, same address).
#define KS_YB 64            // rows of B_S whose sums phase 1 leaves in LDS at a time
#define KS_TW 4             // thresholds a workgroup takes at a time in phase 3: one per wavefront for the entries
#define KS_GC (AFAR_GROUP / KS_LC)
static_assert(KS_GC == 4, "one chunk of the group per wavefront of the 256-thread workgroup");

__global__ void __launch_bounds__(256) kuf_scan_far_moments_kernel(const KufScanItem* __restrict__ items, const double* __restrict__ x,
                                                                   int n, int32_t* __restrict__ status) {
  constexpr int NQ = KsType<GP_KERN_MATERN32>::NQ, NS = 2 * NQ;
  const KufScanItem it = items[blockIdx.y];
  const int M = it.M, KP = M + 1;
  const int S = blockIdx.x, C = n / KS_LC;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = S * KS_GC + wave, j0 = c * KS_LC, j = j0 + lane;
  const ks_gcptr gx = (ks_gcptr)x, gK = (ks_gcptr)it.Kuf, gW = (ks_gcptr)it.W, gT = (ks_gcptr)(it.T + (int64_t)S * M * 8),
                 gPsi = (ks_gcptr)it.Psi, ggv = (ks_gcptr)it.gv, ggm = (ks_gcptr)it.gm, gR = (ks_gcptr)it.R,
                 galpha = (ks_gcptr)it.alpha, gz = (ks_gcptr)it.z, th = (ks_gcptr)it.theta;
  const ks_gptr gmom = (ks_gptr)it.mom, gnear = (ks_gptr)it.near;
  const int64_t ldk = it.lda;
  const int kbeg = min(max(it.rng[2 * S], 0), M), kend = min(max(it.rng[2 * S + 1], kbeg), M);
  const int nr = 4 + (kend - kbeg);                       // rows of B_S; row nr of the walk below is gm
  __shared__ double buf[KS_GC * 16 * (KS_LC + 1)];        // phase 1: [wave][16 rows][frames + 1]; phase 3: [threshold][2]
  __shared__ double wq[KS_GC][NS][KS_LC];                 // [chunk][side * NQ + q][frame]: u^q e^-u
  __shared__ double ys[KS_YB][KS_GC * NS];
  __shared__ unsigned short thr[KS_MAXM];                 // thresholds of the group's chunks, ascending index
  __shared__ unsigned char thc[KS_MAXM];                  // ... and which of the four chunks each lies in
  __shared__ int wcount[4];
  __shared__ double etab[GP_EXP_TAB];
  gp_exp_tab_init(etab);
  double (*vt)[KS_LC + 1] = (double (*)[KS_LC + 1])(buf + wave * 16 * (KS_LC + 1));
  const double var = th[0], ls = th[1];
  const double inv_ls = 1.0 / ls, kap = KsType<GP_KERN_MATERN32>::CS * inv_ls;
  const double sc = gx[j0], ec = gx[j0 + KS_LC - 1], xj = gx[j];
  const double gv2 = 2.0 * ggv[j], gmj = ggm[j];
  // the promise of gp_pdgp_set_frames_ascending, as kuf_scan_stream_kernel checks it: plain stores, the last one is a true report
  if (j + 1 < n && gx[j + 1] < xj) { status[0] = 3; status[1] = j; }
  __syncthreads();
  {
    const double uL = kap * (ec - xj), uR = kap * (xj - sc);
    double pL = gp_exp_neg(-uL, etab), pR = gp_exp_neg(-uR, etab);
#pragma unroll
    for (int q = 0; q < NQ; q++) { wq[wave][q][lane] = pL; wq[wave][NQ + q][lane] = pR; pL *= uL; pR *= uR; }
  }
  // thresholds of the group: s_c <= z_i < s_{c+1} per chunk, the outermost chunks of the batch open-ended
  const int cg = S * KS_GC;
  const double s1 = gx[(cg + 1) * KS_LC], s2 = gx[(cg + 2) * KS_LC], s3 = gx[(cg + 3) * KS_LC];
  const double sg = gx[cg * KS_LC], snext = (cg + KS_GC < C) ? gx[(cg + KS_GC) * KS_LC] : 0.0;
  int nthr = 0;
  for (int i0 = 0; i0 < M; i0 += 256) {
    const int i = i0 + tid;
    bool in = false;
    int wc = 0;
    if (i < M) {
      const double zi = gz[i];
      in = (cg == 0 || zi >= sg) && (cg + KS_GC == C || zi < snext);
      wc = (zi >= s1 ? 1 : 0) + (zi >= s2 ? 1 : 0) + (zi >= s3 ? 1 : 0);
    }
    const unsigned long long mask = __ballot(in);
    if (lane == 0) wcount[wave] = __popcll(mask);
    __syncthreads();
    int off = nthr;
    for (int w = 0; w < wave; w++) off += wcount[w];
    if (in) { const int s = off + __popcll(mask & ((1ull << lane) - 1ull)); thr[s] = (unsigned short)i; thc[s] = (unsigned char)wc; }
    nthr += (wcount[0] + wcount[1]) + (wcount[2] + wcount[3]);
    __syncthreads();
  }
  // phases 1 and 2, KS_YB rows of B_S at a time
  const int nrow = nr + 1;
  for (int rb = 0; rb < nrow; rb += KS_YB) {
    const int rcount = min(KS_YB, nrow - rb);
    for (int r0 = 0; r0 < rcount; r0 += 16) {
#pragma unroll
      for (int rr = 0; rr < 16; rr++) {
        const int r = rb + r0 + rr;
        double v = 0.0;
        if (r < 4) v = gPsi[(int64_t)r * n + j] * gv2;
        else if (r < nr) v = gK[(int64_t)(kbeg + r - 4) * ldk + j] * gv2;
        else if (r == nr) v = gmj;
        vt[rr][lane] = v;
      }
      __syncthreads();
      const int rr = lane & 15, qt = lane >> 4;
      double m[NS];
#pragma unroll
      for (int q = 0; q < NS; q++) m[q] = 0.0;
#pragma unroll
      for (int jj = 0; jj < 16; jj++) {
        const double a = vt[rr][qt * 16 + jj];
#pragma unroll
        for (int q = 0; q < NS; q++) m[q] = fma(a, wq[wave][q][qt * 16 + jj], m[q]);
      }
#pragma unroll
      for (int q = 0; q < NS; q++) { m[q] += __shfl_xor(m[q], 16, 64); m[q] += __shfl_xor(m[q], 32, 64); }
      const int r = rb + r0 + rr;
      if (qt == 0 && r <= nr) {
#pragma unroll
        for (int q = 0; q < NS; q++) {
          if (r == nr) gmom[((int64_t)c * NS + q) * KP + M] = m[q];
          else ys[r0 + rr][wave * NS + q] = m[q];
        }
      }
      __syncthreads();
    }
    const int re = min(rb + KS_YB, nr);
    if (re > rb) {
      for (int k = tid; k < M; k += 256) {
        const int kw = (k | 63);                          // the wavefront's last row
        double acc[KS_GC * NS];
#pragma unroll
        for (int w = 0; w < KS_GC; w++)
#pragma unroll
          for (int q = 0; q < NS; q++)
            acc[w * NS + q] = (rb == 0) ? 0.0 : gmom[((int64_t)(cg + w) * NS + q) * KP + k];
        // (uniform) column kbeg + r - 4 of W is above the diagonal for every row of the wavefront once it passes kw: stop there
        // (the four far columns always count)
        const int rend = min(re, max(4, kw - kbeg + 5));
#pragma unroll 4
        for (int r = rb; r < rend; r++) {
          const int i = kbeg + r - 4;
          double pv = (r < 4) ? gT[(int64_t)k * 8 + r] : gW[(int64_t)k * M + i];
          if (r >= 4 && i > k) pv = 0.0;
#pragma unroll
          for (int q = 0; q < KS_GC * NS; q++) acc[q] = fma(pv, ys[r - rb][q], acc[q]);
        }
#pragma unroll
        for (int w = 0; w < KS_GC; w++)
#pragma unroll
          for (int q = 0; q < NS; q++) gmom[((int64_t)(cg + w) * NS + q) * KP + k] = acc[w * NS + q];
      }
    }
    __syncthreads();
  }
  // phase 3: the near part, KS_TW thresholds at a time.  rho: wavefront = a quarter of the k range, lane = (column of the
  // 16-column block, k mod 4); the sixteen partial sums of a column are added as (q0 + q1) + (q2 + q3) inside a wavefront,
  // then across the wavefronts through LDS.  Entries: wavefront = threshold, lane = frame of its chunk.
  double* tacc = buf;                                                     // [threshold][2]
  double (*rpart)[KS_TW][16] = (double (*)[KS_TW][16])(buf + 2 * KS_MAXM);  // [wavefront][threshold][column]
  static_assert(2 * KS_MAXM + KS_GC * KS_TW * 16 <= KS_GC * 16 * (KS_LC + 1), "phase 3's records fit phase 1's tile");
  const int kspan = M / KS_GC;                            // (M is a multiple of 16: a multiple of 4 rows per wavefront)
  for (int t0 = 0; t0 < nthr; t0 += KS_TW) {
    int ti[KS_TW];
#pragma unroll
    for (int t = 0; t < KS_TW; t++) ti[t] = thr[min(t0 + t, nthr - 1)];   // (a short last batch repeats its last threshold; not recorded)
    const bool mine = (t0 + wave < nthr);
    const int sm = mine ? t0 + wave : t0, im = thr[sm], jm = (cg + thc[sm]) * KS_LC + lane;
    double kb = 0.0;
    for (int rb = 0; rb < nr; rb += 16) {
      const int rr = lane & 15, kq = lane >> 4, r = rb + rr;
      const bool valid = (r < nr), nearc = valid && r >= 4;
      const int col = kbeg + r - 4;
      const ks_gcptr pp = nearc ? gW + col : gT + (valid ? r : 0);
      const int64_t stride = nearc ? M : 8;
      const int kstart = (rb == 0) ? 0 : ((kbeg + rb - 4) & ~3);     // W[k, i] = 0 for k < i: the block's first column
      // the entries' operands of this block, requested ahead of the k walk
      double bv[16];
#pragma unroll
      for (int r2 = 0; r2 < 16; r2++) {
        const int rg = rb + r2;
        bv[r2] = 0.0;
        if (rg < 4) bv[r2] = gPsi[(int64_t)rg * n + jm];
        else if (rg < nr) bv[r2] = gK[(int64_t)(kbeg + rg - 4) * ldk + jm];
      }
      double a[KS_TW];
#pragma unroll
      for (int t = 0; t < KS_TW; t++) a[t] = 0.0;
      const int kend_w = (wave + 1) * kspan;
#pragma unroll 8
      for (int k = max(wave * kspan, kstart) + kq; k < kend_w; k += 4) {
        double pv = pp[(int64_t)k * stride];
        if (!valid || (nearc && col > k)) pv = 0.0;
#pragma unroll
        for (int t = 0; t < KS_TW; t++) a[t] = fma(gR[(int64_t)ti[t] * M + k], pv, a[t]);
      }
#pragma unroll
      for (int t = 0; t < KS_TW; t++) {
        a[t] += __shfl_xor(a[t], 16, 64); a[t] += __shfl_xor(a[t], 32, 64);
        if (kq == 0) rpart[wave][t][rr] = a[t];
      }
      __syncthreads();
      const double rho = (rpart[0][wave][rr] + rpart[1][wave][rr]) + (rpart[2][wave][rr] + rpart[3][wave][rr]);
#pragma unroll
      for (int r2 = 0; r2 < 16; r2++) kb = fma(__shfl(rho, r2, 64), bv[r2], kb);      // (columns past nr: rho = 0, bv = 0)
      __syncthreads();
    }
    if (mine) {                                           // (uniform per wavefront)
      const double w = fma(2.0 * ggv[jm], kb, galpha[im] * ggm[jm]);
      const double zi = gz[im], xt = gx[jm];
      const double a_ = zi / ls, aa = __dmul_rn(a_, a_), b_ = xt / ls, bb = __dmul_rn(b_, b_);
      const double r2 = __dadd_rn(__dadd_rn(-2.0 * __dmul_rn(a_, b_), aa), bb);
      double r, rinv;
      gp_sqrt_rsqrt_pos(__dadd_rn(r2, 1e-12), r, rinv);
      const double q3 = 1.7320508075688772, e = gp_exp_neg(-q3 * r, etab);
      const double phi = (1.0 + q3 * r) * e, dphi = -3.0 * r * e;
      double av = w * phi, al = (w * var * dphi) * (-r2 * rinv * inv_ls);
      for (int o = 32; o > 0; o >>= 1) { av += __shfl_down(av, o, 64); al += __shfl_down(al, o, 64); }
      if (lane == 0) { tacc[2 * (t0 + wave)] = av; tacc[2 * (t0 + wave) + 1] = al; }
    }
  }
  __syncthreads();
  if (tid < 2 * KS_GC) {
    const int w = tid >> 1, comp = tid & 1;
    double s = 0.0;
    for (int t = 0; t < nthr; t++) if (thc[t] == w) s += tacc[2 * t + comp];
    gnear[(int64_t)(cg + w) * 2 + comp] = s;
  }
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

gp_status launch_kuf_scan(gp_handle h, int ktype, const KufScanItem* d_items, int count, int maxM, const double* x, int n, int far) {
  if (count <= 0) return GP_OK;
  if (kuf_scan_nq(ktype) == 0 || maxM < 1 || maxM > KS_MAXM || n < 1)
    return gp_fail(h, GP_ERR_UNSUPPORTED, "kuf_scan: Matern-3/2 or Matern-5/2, 1 <= M <= 1024");
  if (far && (ktype != GP_KERN_MATERN32 || !afar_takes(maxM, n)))
    return gp_fail(h, GP_ERR_UNSUPPORTED, "kuf_scan: the far-field moments need a Matern-3/2 family on the activation far field's shapes");
  const dim3 gs(kuf_scan_chunks(n), count), gp((maxM + 1 + 63) / 64, 2, count), gf(kuf_scan_records(maxM), count);
  const bool m32 = (ktype == GP_KERN_MATERN32);
  {   // (a timer scope per launch: the stream kernel is the HBM-bound one, the other two are M-sized)
    GpTimerScope ts(h, GP_TIMER_HYPER);
    if (far) hipLaunchKernelGGL(kuf_scan_far_moments_kernel, dim3(n / AFAR_GROUP, count), dim3(256), 0, h->stream, d_items, x, n, h->d_status);
    else if (m32) hipLaunchKernelGGL((kuf_scan_stream_kernel<GP_KERN_MATERN32>), gs, dim3(256), 0, h->stream, d_items, x, n, h->d_status);
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
