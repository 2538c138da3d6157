// ssm_smooth.hip — the exact per-source posterior of an SGPRSS window in O(N) by a Kalman filter and a Bryson-Frazier (de Jong)
// backward pass (gfx950, float64 throughout).  Beside gpitch/sgpr_ss.py:73-114 (the N x N exact posterior this computes
// without the N x N matrix) and sample.hip (the state-space form of the Matern-1/2 families it rests on).
//
// Every kernel of the sum must be Matern12, MercerMatern12sm or Matern12sm.  Such a source is
//   f_p(t) = sum_k sqrt(e_k) [a_k(t) cos 2 pi f_k t + b_k(t) sin 2 pi f_k t],   a_k, b_k independent OU(variance v_p, lengthscale l_p)
// (Matern12: one OU process observed through 1), so y_t = sum_p f_p(t) + noise is a linear-Gaussian state-space model with
// state x in R^d, d = sum_p c_p (c_p = 1 or 2 m_p; the sources' blocks in kern_list order, (a_0, b_0, a_1, b_1, ...) inside
// a mixture), diagonal transition, scalar time-varying observation row h_j and a stationary start P_0 = diag(v).
//
// Timeline: `order` lists the steps in ascending time, entry < N the training frame X[entry] (an observed step), entry >= N
// the new frame Xnew[entry - N] (unobserved); out_step[i] is the step of new frame i (a new frame bit-equal to a training
// frame shares its step).  Per step j and coordinate i of source p, D_j = t_j - t_(j-1) >= 0:
//   phi_j[i] = exp(-D_j / l_p),   q_j[i] = v_p (-expm1(-2 D_j / l_p))          (exactly 1 and 0 at D = 0 and at j = 0)
//   h_j[i]   = 1 | sqrt(e_k) cos 2 pi f_k t_j | sqrt(e_k) sin 2 pi f_k t_j      (the feature kernel of cov.hip on t)
// Forward (a = 0, P = diag(v)):  a <- phi a;  P <- phi P phi + diag(q);  keep a^-, P^-;  observed: g = P h, F = h.g + s2,
//   e = y - h.a, a <- a + g e / F, P <- P - g g^T / F; keep g, e, F.   loglik = -1/2 sum_obs (log(2 pi F) + e^2 / F)
// Backward (r = 0, Nm = 0 behind the last step):  r <- phi_(j+1) r;  Nm <- phi_(j+1) Nm phi_(j+1);  observed: k = g / F, u = Nm k,
//   Nm <- Nm - h u^T - u h^T + h h^T (k.u + 1/F),  r <- r - h (k.r) + h e / F;   s = a^- + P^- r;  per source p with
//   w_p = P^- h_p (h_p = h with the other sources' coordinates zeroed):  mean_p = h_p.s,  var_p = h_p.w_p - w_p^T Nm w_p.
//
// Launches per call (all windows of the call in each):
//   1. ssms_times_kernel       t_j and y_j of every step in walk order
//   2. sm_features_kernel      cov.hip's feature tables of the merged times, one launch per spectral-mixture source
//   3. ssms_rows_kernel        h_j as rows [steps][d], phi and q as [steps][P]: no exp, sin or cos is left for the walks
//   4. ssms_forward_kernel     one workgroup of DP = 64 (d <= 64: one wavefront) or 128 (d <= 128: two) threads per window; thread
//                              i holds row i of P in registers (DP doubles), h, phi and g are broadcast through LDS, F and e
//                              are one butterfly (+ one LDS exchange between the two wavefronts).  The history a^-, g, e, F
//                              and P^- (d^2 doubles per step, stored transposed so that a wavefront's stores are contiguous)
//                              goes to the workspace.
//   5. ssms_backward_kernel    the same shape with row i of Nm in registers; P^- comes back once per wanted step (thread i reads
//                              its own row, contiguous across the wavefront), a source's block of columns at a time with
//                              SSMS_BATCH loads in flight.  A source's w_p goes through LDS.
//   6. ssms_loglik_kernel      the sum over the observed steps in a fixed order (the walk carries no log)
//   7. ssms_gather_kernel      mean / var [P][n] through out_step
// Determinism: no atomics, every sum in a fixed order; a window is one workgroup and reads nothing of the others', so its
// result is bit-identical between calls and whatever shares the launch.
//
// The score (ssm_score_run: the gradient of loglik in [noise | theta_0 | ...]).  Timeline = the N training frames,
// launches 1 - 4 and 6 as above with the history on, then
//   8. ssms_score_kernel       the backward walk's shape with every step wanted.  Before step j + 1's (r, Nm) are propagated to
//                              step j:  P+ = P^-_j - g g^T / F,  a+ = a^-_j + g e / F,  phi = phi_(j+1),
//                                gphi[j+1][i] = r_i a+_i + sum_k (r_i r_k - Nm_ik) phi_k P+_ik,    gq[j+1][i] = (r_i^2 - Nm_ii) / 2
//                              then with the propagated pair:  k = g / F, u = Nm k, kr = k.r, ku = k.u, uu = e / F - kr,
//                              Fb = (uu^2 - (1 / F + ku)) / 2:   gs2 += Fb,  gres[j] = -uu (= d loglik / d y_j),
//                                gh[j] = uu a^- + P^- (uu r + u + Fb h) + Fb g
//                              and the backward walk's update.  After step 0: gv0[i] = (r_i^2 - Nm_ii) / 2 (the start diag(v)).
//                              u and the scalars come from the unpropagated row (u_i = phi_i sum_k Nm_ik phi_k k_k), so that
//                              ONE pass over row i of P^-_j feeds both row sums.
//   9. ssms_score_reduce_kernel  one workgroup per (window, parameter): for the coordinates i of source p, D_j = t_j - t_(j-1),
//                                d/d v_p = sum_(j,i) gq[j][i] q_j / v_p + sum_i gv0[i]        (q_j / v_p = 1 - phi^2)
//                                d/d l_p = sum_(j,i) (gphi[j][i] - 2 v_p phi gq[j][i]) phi D_j / l_p^2
//                                d/d e_k = sum_j (gh_c h_c + gh_s h_s) / (2 e_k),   d/d f_k = sum_j 2 pi t_j (gh_s h_c - gh_c h_s)
//                              and d/d noise = gs2; one more workgroup per window scatters gres through `order`.
//
// Joint draws from the same posterior (ssm_sample_run): launches 1 - 4 with the history off (the gain walk), then the
// simulation smoother's ssmp_* kernels, described above them: three elementwise walks of one d-vector per draw, one wavefront per
// (window, draw), and a gather.  No steps * d^2 block in that call's workspace.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"

#define SSMS_MAX_D 128
// columns of P^- the backward walk fetches at a time: 32 with two wavefronts (a mixture of up to 16 partials in one fetch), 4 with
// one (measured: 32.9 - 35.8 ms per N = 2001, d = 60 window against 38.8 ms with 32)
#define SSMS_BATCH (DP == 64 ? 4 : 32)

// one per window: what the kernels of a call read
struct SsmsWin {
  const double* params; const double* X; const double* Y; const double* xnew;
  const int* order; const int* want; const int* ostep;
  double *t, *ys, *feat, *hrow, *phi, *q;          // prologue
  double *am, *g, *ef, *Pm;                        // history: a^- [steps][d], g [steps][d], (e, F) [steps][2], P^- [steps][d][d]
  double *smean, *svar;                            // [P][steps]
  double *mean, *var, *loglik;                     // the caller's
  int steps, hist;                                 // hist: the backward pass will run (n > 0)
};
// the structure of the state, shared by the windows of a call
struct SsmsMeta {
  int d, P, N, n;
  int coff[SSMS_MAX_D + 1];                        // first coordinate of source p; coff[P] = d
  int toff[SSMS_MAX_D];                            // source p's theta within a parameter row
  int crow[SSMS_MAX_D];                            // coordinate i's row among the window's feature rows, -1: h = 1 (Matern12)
  int csrc[SSMS_MAX_D];                            // coordinate i's source
};

// the score's own blocks of a window (beside its SsmsWin)
struct SsmsScoreWin {
  double *gphi, *gq, *gh;                          // [steps][d]; row 0 of gphi and gq is never written nor read
  double *gres, *gs2, *gv0;                        // [steps], one, [d]
  double *grad, *resid;                            // the caller's: [num_params], [N] or null
};
// what entry q of a parameter row is: a source has at most 2 + its components entries, so 1 + 3 * 128 cover a row
#define SSMS_MAX_PARAMS (1 + 3 * SSMS_MAX_D)
enum { SSMS_PAR_NONE = 0, SSMS_PAR_NOISE, SSMS_PAR_VARIANCE, SSMS_PAR_LENGTHSCALE, SSMS_PAR_ENERGY, SSMS_PAR_FREQUENCY };
struct SsmsScoreMeta {
  int nparams;
  int kind[SSMS_MAX_PARAMS];
  int src[SSMS_MAX_PARAMS];                        // the entry's source
  int coord[SSMS_MAX_PARAMS];                      // energy / frequency: the partial's cosine coordinate (its sine: + 1)
};
// columns of P^- the score walk fetches at a time (a measurement variant may set its own: tools/build_variant.sh)
#ifndef SSMS_SCORE_BATCH
#define SSMS_SCORE_BATCH (DP == 64 ? 8 : 16)
#endif

static inline bool ssms_kernel_ok(int type) {
  return type == GP_KERN_MATERN12 || type == GP_KERN_MERCER_MATERN12SM || type == GP_KERN_MATERN12SM;
}

// ---- 1. ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ssms_times_kernel(const SsmsWin* __restrict__ wins, int N) {
  const SsmsWin w = wins[blockIdx.y];
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= w.steps) return;
  const int o = w.order[j];
  w.t[j] = o < N ? w.X[o] : w.xnew[o - N];
  w.ys[j] = o < N ? w.Y[o] : 0.0;
}

// ---- 3. ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) ssms_rows_kernel(const SsmsWin* __restrict__ wins, const SsmsMeta* __restrict__ mt) {
  const SsmsWin w = wins[blockIdx.y];
  const int d = mt->d, np = mt->P;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t j = e / d;
  const int i = (int)(e % d);
  if (j >= (size_t)w.steps) return;
  const int r = mt->crow[i];
  w.hrow[j * d + i] = r < 0 ? 1.0 : w.feat[(size_t)r * w.steps + j];
  if (i < np) {                                    // (P <= d: every source has a coordinate)
    const double* th = w.params + mt->toff[i];
    const double dt = j > 0 ? fmax(w.t[j] - w.t[j - 1], 0.0) : 0.0;
    const double dl = dt / th[1];
    w.phi[j * np + i] = exp(-dl);
    w.q[j * np + i] = th[0] * (-expm1(-2.0 * dl));
  }
}

// the sum of x and of y over a wavefront, the same bits in every lane (a + b = b + a at every level of the butterfly)
__device__ __forceinline__ void ssms_wave_sum2(double& x, double& y) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { x += __shfl_xor(x, o, 64); y += __shfl_xor(y, o, 64); }
}
__device__ __forceinline__ void ssms_wave_sum(double& x) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
}
// sum_k row[k] * b[k] over the DP registers of a row, b broadcast from LDS: four chains, added in a fixed order
template <int DP>
__device__ __forceinline__ double ssms_row_dot(const double (&row)[DP], const double* b) {
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
  for (int k = 0; k < DP; k += 4) {
    a0 = fma(row[k], b[k], a0); a1 = fma(row[k + 1], b[k + 1], a1);
    a2 = fma(row[k + 2], b[k + 2], a2); a3 = fma(row[k + 3], b[k + 3], a3);
  }
  return (a0 + a1) + (a2 + a3);
}

// ---- 4. forward: one workgroup of DP threads per window, thread i = row i of P ------------------------------------------------
// Lanes i >= d and columns k >= d carry zeros throughout (h = phi = q = v = 0 there).  The values of step j + 1 are loaded while
// step j is computed.  Barriers: hb / pb alternate between two buffers, so a step's reads end before the buffer is written
// again two steps later (the barrier of the step between lies in every thread's way); gb and red are written behind the
// step's first barrier and read behind its second.
template <int DP>
__global__ void __launch_bounds__(DP) ssms_forward_kernel(const SsmsWin* __restrict__ wins, const SsmsMeta* __restrict__ mt) {
  constexpr int NW = DP / 64;
  __shared__ double hb[2][DP], pb[2][DP], gb[DP], red[NW][2];
  const SsmsWin w = wins[blockIdx.x];
  const int i = threadIdx.x, d = mt->d, N = mt->N, np = mt->P, steps = w.steps;
  const bool on = i < d;
  const int src = on ? mt->csrc[i] : 0;
  const double s2 = w.params[0];
  const double vi = on ? w.params[mt->toff[src]] : 0.0;
  const size_t dd = (size_t)d * d;
  double P[DP];
#pragma unroll
  for (int k = 0; k < DP; k++) P[k] = (k == i) ? vi : 0.0;
  double a = 0.0;
  double hn = on ? w.hrow[i] : 0.0, pn = on ? w.phi[src] : 0.0, qn = on ? w.q[src] : 0.0, yn = w.ys[0];
  int on_ = w.order[0];
  for (int j = 0; j < steps; j++) {
    const int b = j & 1;
    const double hh = hn, ph = pn, qq = qn, y = yn;
    const int o = on_;
    if (j + 1 < steps) {
      const size_t j1 = (size_t)j + 1;
      hn = on ? w.hrow[j1 * d + i] : 0.0;
      pn = on ? w.phi[j1 * np + src] : 0.0;
      qn = on ? w.q[j1 * np + src] : 0.0;
      yn = w.ys[j1];
      on_ = w.order[j1];
    }
    hb[b][i] = hh; pb[b][i] = ph;
    __syncthreads();
    a *= ph;
#pragma unroll
    for (int k = 0; k < DP; k++) P[k] = fma(ph * pb[b][k], P[k], (k == i) ? qq : 0.0);
    if (w.hist && on) {
      w.am[(size_t)j * d + i] = a;
      double* dst = w.Pm + (size_t)j * dd + i;     // P^- transposed: element (row i, column k) at [k][i]
#pragma unroll
      for (int k = 0; k < DP; k++)
        if (k < d) dst[(size_t)k * d] = P[k];
    }
    if (o < N) {                                   // observed (the same for the whole workgroup)
      const double g = ssms_row_dot<DP>(P, hb[b]);
      double x1 = hh * g, x2 = hh * a;
      ssms_wave_sum2(x1, x2);
      if (NW > 1 && (i & 63) == 0) { red[i >> 6][0] = x1; red[i >> 6][1] = x2; }
      gb[i] = g;
      __syncthreads();
      if (NW > 1) { x1 = red[0][0] + red[NW - 1][0]; x2 = red[0][1] + red[NW - 1][1]; }
      const double F = x1 + s2, e = y - x2, c = 1.0 / F;
      a = fma(g, e * c, a);
#pragma unroll
      for (int k = 0; k < DP; k++) P[k] = fma(-(g * gb[k]), c, P[k]);
      if (on) w.g[(size_t)j * d + i] = g;
      if (i == 0) { w.ef[2 * (size_t)j] = e; w.ef[2 * (size_t)j + 1] = F; }
    }
  }
}

// ---- 5. backward: thread i = row i of Nm -------------------------------------------------------------------------------------
// Barriers as in the forward walk: hb / pb alternate; kb, ub, rb, mb, red and outv are each written once per step behind the
// step's first barrier and read behind a later one of the same step; wb alternates between two buffers along the sources.
template <int DP>
__global__ void __launch_bounds__(DP) ssms_backward_kernel(const SsmsWin* __restrict__ wins, const SsmsMeta* __restrict__ mt) {
  constexpr int NW = DP / 64;
  __shared__ double hb[2][DP], pb[2][DP], kb[DP], ub[DP], rb[DP], mb[DP], wb[2][DP], outv[NW][SSMS_MAX_D], red[NW][2];
  const SsmsWin w = wins[blockIdx.x];
  const int i = threadIdx.x, d = mt->d, N = mt->N, np = mt->P, steps = w.steps;
  const bool on = i < d;
  const int src = on ? mt->csrc[i] : 0;
  const size_t dd = (size_t)d * d;
  double Nm[DP];
#pragma unroll
  for (int k = 0; k < DP; k++) Nm[k] = 0.0;
  double r = 0.0;
  // the values of step j - 1 are loaded while step j is computed; `pn` is phi of the step above (the transition into step j)
  int j = steps - 1;
  double hn = on ? w.hrow[(size_t)j * d + i] : 0.0, pn = 1.0, an = on ? w.am[(size_t)j * d + i] : 0.0;
  int on_ = w.order[j], wn = w.want[j];
  double gn = (on && on_ < N) ? w.g[(size_t)j * d + i] : 0.0;
  double en = on_ < N ? w.ef[2 * (size_t)j] : 0.0, Fn = on_ < N ? w.ef[2 * (size_t)j + 1] : 1.0;
  for (; j >= 0; j--) {
    const int b = j & 1;
    const double hh = hn, ph = pn, am = an, g = gn, e = en, F = Fn;
    const int o = on_, want = wn;
    if (j > 0) {
      const size_t j1 = (size_t)j - 1;
      hn = on ? w.hrow[j1 * d + i] : 0.0;
      pn = on ? w.phi[(size_t)j * np + src] : 0.0;
      an = on ? w.am[j1 * d + i] : 0.0;
      on_ = w.order[j1]; wn = w.want[j1];
      gn = (on && on_ < N) ? w.g[j1 * d + i] : 0.0;
      en = on_ < N ? w.ef[2 * j1] : 0.0; Fn = on_ < N ? w.ef[2 * j1 + 1] : 1.0;
    }
    hb[b][i] = hh; pb[b][i] = ph;
    const double* __restrict__ Pj = w.Pm + (size_t)j * dd + i;
    __syncthreads();
    r *= ph;
#pragma unroll
    for (int k = 0; k < DP; k++) Nm[k] = (ph * pb[b][k]) * Nm[k];
    if (o < N) {
      const double c = 1.0 / F, kk = g * c;
      kb[i] = kk;
      __syncthreads();
      const double u = ssms_row_dot<DP>(Nm, kb);
      double x1 = kk * u, x2 = kk * r;
      ssms_wave_sum2(x1, x2);
      if (NW > 1 && (i & 63) == 0) { red[i >> 6][0] = x1; red[i >> 6][1] = x2; }
      ub[i] = u;
      __syncthreads();
      if (NW > 1) { x1 = red[0][0] + red[NW - 1][0]; x2 = red[0][1] + red[NW - 1][1]; }
      const double cc = x1 + c;
#pragma unroll
      for (int k = 0; k < DP; k++) Nm[k] += fma(hh, fma(hb[b][k], cc, -ub[k]), -(u * hb[b][k]));
      r = fma(hh, e * c - x2, r);
    }
    if (want) {
      rb[i] = r;
      __syncthreads();
      double sacc = 0.0;
      for (int p = 0; p < np; p++) {
        const int k0 = mt->coff[p], k1 = mt->coff[p + 1];
        double wp = 0.0;
        if (on) {                                  // the source's columns of the row, SSMS_BATCH loads in flight at a time
          for (int kb0 = k0; kb0 < k1; kb0 += SSMS_BATCH) {
            double pv[SSMS_BATCH];
#pragma unroll
            for (int c = 0; c < SSMS_BATCH; c++) pv[c] = kb0 + c < k1 ? Pj[(size_t)(kb0 + c) * d] : 0.0;
#pragma unroll
            for (int c = 0; c < SSMS_BATCH; c++) {
              const int k = kb0 + c < k1 ? kb0 + c : k0;       // (a column past the block: its pv is 0, the index stays inside)
              sacc = fma(pv[c], rb[k], sacc);
              wp = fma(pv[c], hb[b][k], wp);
            }
          }
        }
        wb[p & 1][i] = wp;
        __syncthreads();
        const double v = ssms_row_dot<DP>(Nm, wb[p & 1]);
        double vp = wp * (((i >= k0 && i < k1) ? hh : 0.0) - v);
        ssms_wave_sum(vp);
        if ((i & 63) == 0) outv[i >> 6][p] = vp;
      }
      mb[i] = hh * (am + sacc);
      __syncthreads();
      if (i < np) {
        double m = 0.0;
        for (int k = mt->coff[i]; k < mt->coff[i + 1]; k++) m += mb[k];
        w.smean[(size_t)i * steps + j] = m;
        w.svar[(size_t)i * steps + j] = NW > 1 ? outv[0][i] + outv[NW - 1][i] : outv[0][i];
      }
    }
  }
}

// ---- 6. loglik = -1/2 sum over the observed steps of log(2 pi F) + e^2 / F; one workgroup per window -------------------------
__global__ void __launch_bounds__(256) ssms_loglik_kernel(const SsmsWin* __restrict__ wins, int N) {
  __shared__ double red[256];
  const SsmsWin w = wins[blockIdx.x];
  double a = 0.0;
  for (int j = threadIdx.x; j < w.steps; j += 256)
    if (w.order[j] < N) {
      const double e = w.ef[2 * (size_t)j], F = w.ef[2 * (size_t)j + 1];
      a += log(6.283185307179586 * F) + e * e / F;
    }
  red[threadIdx.x] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) w.loglik[0] = -0.5 * red[0];
}

// ---- 7. new frames i0 .. i0 + cnt - 1 of every window through out_step (ostep holds that slice) ------------------------------
__global__ void __launch_bounds__(256) ssms_gather_kernel(const SsmsWin* __restrict__ wins, int np, int n, int i0, int cnt) {
  const SsmsWin w = wins[blockIdx.z];
  const int p = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cnt) return;
  const int s = w.ostep[c];
  w.mean[(size_t)p * n + i0 + c] = w.smean[(size_t)p * w.steps + s];
  w.var[(size_t)p * n + i0 + c] = w.svar[(size_t)p * w.steps + s];
}

// ---- 8. score: thread i = row i of Nm, every step observed -------------------------------------------------------------------
// Barriers as in the backward walk: hb / cb alternate between two buffers; ub, zb and red are written behind the step's first
// barrier and read behind a later one of the same step.  cb[k] = (k_k, phi_k r_k, phi_k, phi_k k_k): what the row sums take of
// column k, one 32-byte record.  Lanes i >= d and columns k >= d carry zeros (h = phi = g = 0 there).  `nmd` is Nm_ii, carried
// beside the row by the row's own operations.
template <int DP>
__global__ void __launch_bounds__(DP) ssms_score_kernel(const SsmsWin* __restrict__ wins, const SsmsScoreWin* __restrict__ swins,
                                                        const SsmsMeta* __restrict__ mt) {
  constexpr int NW = DP / 64;
  constexpr int NB = SSMS_SCORE_BATCH;
  __shared__ double hb[2][DP], cb[2][DP][4], ub[DP], zb[DP], red[NW][2];
  const SsmsWin w = wins[blockIdx.x];
  const SsmsScoreWin s = swins[blockIdx.x];
  const int i = threadIdx.x, d = mt->d, np = mt->P, steps = w.steps;
  const bool on = i < d;
  const int src = on ? mt->csrc[i] : 0;
  const size_t dd = (size_t)d * d;
  double Nm[DP];
#pragma unroll
  for (int k = 0; k < DP; k++) Nm[k] = 0.0;
  double r = 0.0, nmd = 0.0, gs2 = 0.0;
  // the values of step j - 1 are loaded while step j is computed; `pn` is phi of the step above (the transition into step j + 1)
  int j = steps - 1;
  double hn = on ? w.hrow[(size_t)j * d + i] : 0.0, pn = on ? 1.0 : 0.0, an = on ? w.am[(size_t)j * d + i] : 0.0;
  double gn = on ? w.g[(size_t)j * d + i] : 0.0, en = w.ef[2 * (size_t)j], Fn = w.ef[2 * (size_t)j + 1];
  for (; j >= 0; j--) {
    const int b = j & 1;
    const double hh = hn, ph = pn, am = an, g = gn, e = en, F = Fn;
    if (j > 0) {
      const size_t j1 = (size_t)j - 1;
      hn = on ? w.hrow[j1 * d + i] : 0.0;
      pn = on ? w.phi[(size_t)j * np + src] : 0.0;
      an = on ? w.am[j1 * d + i] : 0.0;
      gn = on ? w.g[j1 * d + i] : 0.0;
      en = w.ef[2 * j1]; Fn = w.ef[2 * j1 + 1];
    }
    const double c = 1.0 / F, kk = g * c, pr = ph * r;
    hb[b][i] = hh;
    cb[b][i][0] = kk; cb[b][i][1] = pr; cb[b][i][2] = ph; cb[b][i][3] = ph * kk;
    const double* __restrict__ Pj = w.Pm + (size_t)j * dd + i;
    __syncthreads();
    // u = (phi Nm phi) k from the unpropagated row: four chains, added in a fixed order
    double u;
    {
      double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
      for (int k = 0; k < DP; k += 4) {
        a0 = fma(Nm[k], cb[b][k][3], a0); a1 = fma(Nm[k + 1], cb[b][k + 1][3], a1);
        a2 = fma(Nm[k + 2], cb[b][k + 2][3], a2); a3 = fma(Nm[k + 3], cb[b][k + 3][3], a3);
      }
      u = ph * ((a0 + a1) + (a2 + a3));
    }
    double x1 = kk * u, x2 = kk * pr;              // k.u and k.r of the propagated pair
    ssms_wave_sum2(x1, x2);
    if (NW > 1) {
      if ((i & 63) == 0) { red[i >> 6][0] = x1; red[i >> 6][1] = x2; }
      __syncthreads();
      x1 = red[0][0] + red[NW - 1][0]; x2 = red[0][1] + red[NW - 1][1];
    }
    const double cc = x1 + c, uu = e * c - x2, Fb = 0.5 * (uu * uu - cc);
    ub[i] = u;
    zb[i] = fma(uu, pr, fma(Fb, hh, u));
    __syncthreads();
    // one pass over row i of P^-_j, NB loads in flight: the transition sum (the unpropagated row) and P^- z
    double at = 0.0, az = 0.0;
#pragma unroll
    for (int kb0 = 0; kb0 < DP; kb0 += NB) {
      if (kb0 < d) {                               // (the same for the whole workgroup)
        double pv[NB];
#pragma unroll
        for (int q = 0; q < NB; q++) pv[q] = (on && kb0 + q < d) ? Pj[(size_t)(kb0 + q) * d] : 0.0;
#pragma unroll
        for (int q = 0; q < NB; q++) {
          const int k = kb0 + q;
          const double pp = fma(-g, cb[b][k][0], pv[q]);                          // P+_ik
          const double co = fma(r, cb[b][k][1], -(Nm[k] * cb[b][k][2]));          // (r_i r_k - Nm_ik) phi_k
          at = fma(co, pp, at);
          az = fma(pv[q], zb[k], az);
        }
      }
    }
    if (on) {
      if (j + 1 < steps) {
        s.gphi[((size_t)j + 1) * d + i] = fma(r, fma(g, e * c, am), at);
        s.gq[((size_t)j + 1) * d + i] = 0.5 * (r * r - nmd);
      }
      s.gh[(size_t)j * d + i] = fma(uu, am, az) + Fb * g;
    }
    if (i == 0) s.gres[j] = -uu;
    gs2 += Fb;
    // propagate, then the update of the backward walk
#pragma unroll
    for (int k = 0; k < DP; k++)
      Nm[k] = fma(ph * cb[b][k][2], Nm[k], fma(hh, fma(hb[b][k], cc, -ub[k]), -(u * hb[b][k])));
    nmd = fma(ph * ph, nmd, fma(hh, fma(hh, cc, -u), -(u * hh)));
    r = fma(hh, e * c - x2, pr);
  }
  if (on) s.gv0[i] = 0.5 * (r * r - nmd);
  if (i == 0) s.gs2[0] = gs2;
}

// ---- 9. the chain rule: workgroup (window, q) sums entry q of the window's gradient, thread t the items t, t + 256, ... in
// order, then a tree; workgroup (window, nparams) scatters gres to training-frame order --------------------------------------
__global__ void __launch_bounds__(256) ssms_score_reduce_kernel(const SsmsWin* __restrict__ wins, const SsmsScoreWin* __restrict__ swins,
                                                               const SsmsMeta* __restrict__ mt, const SsmsScoreMeta* __restrict__ sm) {
  __shared__ double red[256];
  const SsmsWin w = wins[blockIdx.x];
  const SsmsScoreWin s = swins[blockIdx.x];
  const int q = blockIdx.y, tid = threadIdx.x, d = mt->d, np = mt->P, steps = w.steps;
  if (q >= sm->nparams) {
    if (s.resid)
      for (int j = tid; j < steps; j += 256) s.resid[w.order[j]] = s.gres[j];
    return;
  }
  const int kind = sm->kind[q], p = sm->src[q];
  double a = 0.0;
  if (kind == SSMS_PAR_NOISE) {
    if (tid == 0) a = s.gs2[0];
  } else if (kind == SSMS_PAR_VARIANCE || kind == SSMS_PAR_LENGTHSCALE) {
    const int k0 = mt->coff[p], cp = mt->coff[p + 1] - k0;
    const double v = w.params[mt->toff[p]], l = w.params[mt->toff[p] + 1];
    const size_t items = (size_t)steps * cp;
    for (size_t it = tid; it < items; it += 256) {
      const size_t j = it / cp;
      const int i = k0 + (int)(it % cp);
      if (j == 0) {
        if (kind == SSMS_PAR_VARIANCE) a += s.gv0[i];
      } else if (kind == SSMS_PAR_VARIANCE) {
        a += s.gq[j * d + i] * (w.q[j * np + p] / v);
      } else {
        const double phi = w.phi[j * np + p], dt = fmax(w.t[j] - w.t[j - 1], 0.0);
        a += (s.gphi[j * d + i] - 2.0 * v * phi * s.gq[j * d + i]) * (phi * dt / (l * l));
      }
    }
  } else if (kind == SSMS_PAR_ENERGY || kind == SSMS_PAR_FREQUENCY) {
    const int c = sm->coord[q];
    for (int j = tid; j < steps; j += 256) {
      const double hc = w.hrow[(size_t)j * d + c], hs = w.hrow[(size_t)j * d + c + 1];
      const double gc = s.gh[(size_t)j * d + c], gs = s.gh[(size_t)j * d + c + 1];
      a += kind == SSMS_PAR_ENERGY ? gc * hc + gs * hs : w.t[j] * (gs * hc - gc * hs);
    }
    a *= kind == SSMS_PAR_ENERGY ? 0.5 / w.params[q] : 6.283185307179586;
  }
  red[tid] = a;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) s.grad[q] = red[0];
}

// ==== host ===================================================================================================================
struct SsmsDesc { size_t wins, meta, feat, bytes; };
static SsmsDesc ssms_desc_layout(size_t count, size_t P) {
  SsmsDesc o;
  GpRegions region;
  o.wins = region(count * sizeof(SsmsWin));
  o.meta = region(sizeof(SsmsMeta));
  o.feat = region(count * P * sizeof(FeatItem));
  o.bytes = region.off;
  return o;
}
// the operator's one carve; every per-window block has the size of the longest timeline (`steps`).  Feature tables: a
// mixture of m partials takes 2 sm_mpad(m) <= c_p + 6 rows, so d + 6 P rows cover a window
struct SsmsBufs { char* desc; int *order, *want, *ostep; double *t, *ys, *feat, *hrow, *phi, *q, *am, *g, *ef, *smean, *svar, *Pm; };
static SsmsBufs ssms_carve(GpArena& ar, size_t d, size_t steps, size_t P, size_t count) {
  SsmsBufs b;
  b.desc = ar.take<char>(ssms_desc_layout(count, P).bytes);
  b.order = ar.take<int>(count * steps);
  b.want = ar.take<int>(count * steps);
  b.ostep = ar.take<int>(count * steps);
  b.t = ar.take<double>(count * steps);
  b.ys = ar.take<double>(count * steps);
  b.feat = ar.take<double>(count * (d + 6 * P) * steps);
  b.hrow = ar.take<double>(count * steps * d);
  b.phi = ar.take<double>(count * steps * P);
  b.q = ar.take<double>(count * steps * P);
  b.am = ar.take<double>(count * steps * d);
  b.g = ar.take<double>(count * steps * d);
  b.ef = ar.take<double>(count * steps * 2);
  b.smean = ar.take<double>(count * steps * P);
  b.svar = ar.take<double>(count * steps * P);
  b.Pm = ar.take<double>(count * steps * d * d);
  return b;
}

size_t ssm_smooth_workspace_bytes(int d, int steps, int P, int count) {
  if (d < 1 || d > SSMS_MAX_D || steps < 1 || P < 1 || P > d || count < 1) return 0;
  return gp_measure([&](GpArena& ar) { ssms_carve(ar, d, steps, P, count); }) + GP_WS_TAIL_OP;
}

// the score's carve: the smoother's, then its own descriptor block and per-step terms
struct SsmsScoreDesc { size_t wins, meta, bytes; };
static SsmsScoreDesc ssms_score_desc_layout(size_t count) {
  SsmsScoreDesc o;
  GpRegions region;
  o.wins = region(count * sizeof(SsmsScoreWin));
  o.meta = region(sizeof(SsmsScoreMeta));
  o.bytes = region.off;
  return o;
}
struct SsmsScoreBufs { char* desc; double *gphi, *gq, *gh, *gres, *gs2, *gv0; };
static SsmsScoreBufs ssms_score_carve(GpArena& ar, size_t d, size_t steps, size_t count) {
  SsmsScoreBufs b;
  b.desc = ar.take<char>(ssms_score_desc_layout(count).bytes);
  b.gphi = ar.take<double>(count * steps * d);
  b.gq = ar.take<double>(count * steps * d);
  b.gh = ar.take<double>(count * steps * d);
  b.gres = ar.take<double>(count * steps);
  b.gs2 = ar.take<double>(count);
  b.gv0 = ar.take<double>(count * d);
  return b;
}

size_t ssm_score_workspace_bytes(int d, int steps, int P, int count) {
  if (d < 1 || d > SSMS_MAX_D || steps < 1 || P < 1 || P > d || count < 1) return 0;
  return gp_measure([&](GpArena& ar) { ssms_carve(ar, d, steps, P, count); ssms_score_carve(ar, d, steps, count); }) + GP_WS_TAIL_OP;
}

// ==== joint draws: the simulation smoother =====================================================================
// A draw of all sources at all new frames from the exact posterior, by Durbin and Koopman's simulation smoother written with the
// disturbance smoother.  Transition, process noise and start covariance are diagonal, so a draw is three elementwise walks of one
// d-vector on top of the gain walk (ssms_forward_kernel with hist = 0: g and F of the observed steps, no a^-, no P^-).  Per draw s
// with standard normals ex[j][i] (step j, coordinate i) and ey[o] (training frame o):
//   1. w = 0;  w <- phi_j w + sq_j ex_j  (sq_0 = sqrt(v), sq_j = sqrt(q_j));  observed: c_j = (y_o - sigma ey_o - h_j.w) / F_j,
//      w <- w + g_j c_j.   (the prior path and the filter mean of its residual obey one transition: only their sum is carried)
//   2. r = 0 behind the last step;  r <- phi_(j+1) r;  observed: r <- r + h_j (c_j - (g_j.r) / F_j);  keep r_j.
//   3. z = 0;  z <- phi_j z + sq_j ex_j + q_j r_j  (q_0 = v);  keep h_j z, of which source p's value at step j is the sum over its
//      coordinates.
// The map is affine in (ex, ey); at zero it is the smoothed mean, and its linear part T has T T^T = the joint posterior covariance.
// Launches behind the prologue and the gain walk (all windows and draws of the call in each):
//   a. ssmp_prep_kernel        sq [steps][P] (row 0: sqrt(v)), 1 / F per step (0 at an unobserved step), sigma: the walks carry no
//                              sqrt, exp or division
//   b. ssmp_obs_kernel         y_o - sigma ey_o per (draw, step), in walk order
//   c. ssmp_walk1_kernel       one wavefront per (window, draw): lane l holds coordinates l and l + 64 (NC = 2, d > 64), no LDS, no
//   d. ssmp_walk2_kernel       barrier; the dot product of an observed step is one butterfly (ssms_wave_sum); the rows of step
//   e. ssmp_walk3_kernel       j + SSMP_PF are loaded while step j is computed (a ring of SSMP_PF register slots)
//   f. ssmp_gather_kernel      out [P][S][n] through out_step: 32 frames' rows of h_j z through LDS, a source's coordinates summed in
//                              ascending order
// Determinism: no atomics, every sum in a fixed order; a (window, draw) is one wavefront that reads nothing of the others', so a
// draw's bits depend neither on S, nor on the windows that share the call.
// steps in flight per walk (a measurement variant may set its own: tools/build_variant.sh)
#ifndef SSMP_PF
#define SSMP_PF 4
#endif
struct SsmpWin {
  const double* eps_x; const double* eps_y;        // [S][ldx], [S][N]
  double* out;                                     // [P][S][n]
  double *sq, *fi, *sg;                            // [steps][P], [steps], one
  double *yd, *c, *R;                              // [S][lds], [S][lds], [S][lds][d]
  size_t ldx, lds;                                 // the call's longest timeline times d, and that timeline
};

__global__ void __launch_bounds__(256) ssmp_prep_kernel(const SsmsWin* __restrict__ wins, const SsmpWin* __restrict__ pwins,
                                                        const SsmsMeta* __restrict__ mt) {
  const SsmsWin w = wins[blockIdx.y];
  const SsmpWin pw = pwins[blockIdx.y];
  const int np = mt->P;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t j = e / np;
  const int p = (int)(e % np);
  if (j >= (size_t)w.steps) return;
  pw.sq[j * np + p] = sqrt(j == 0 ? w.params[mt->toff[p]] : w.q[j * np + p]);
  if (p == 0) pw.fi[j] = w.order[j] < mt->N ? 1.0 / w.ef[2 * j + 1] : 0.0;
  if (e == 0) pw.sg[0] = sqrt(w.params[0]);
}

__global__ void __launch_bounds__(256) ssmp_obs_kernel(const SsmsWin* __restrict__ wins, const SsmpWin* __restrict__ pwins, int N) {
  const SsmsWin w = wins[blockIdx.z];
  const SsmpWin pw = pwins[blockIdx.z];
  const int j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  if (j >= w.steps) return;
  const int o = w.order[j];
  pw.yd[(size_t)s * pw.lds + j] = o < N ? w.ys[j] - pw.sg[0] * pw.eps_y[(size_t)s * N + o] : 0.0;
}

// a lane's coordinates and what does not change along the walk
template <int NC>
struct SsmpLane {
  int i[NC], src[NC];
  bool on[NC];
  __device__ __forceinline__ SsmpLane(const SsmsMeta* mt) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
      i[c] = (int)threadIdx.x + 64 * c;
      on[c] = i[c] < mt->d;
      src[c] = on[c] ? mt->csrc[i[c]] : 0;
    }
  }
};

// ---- c. walk 1 -------------------------------------------------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(64) ssmp_walk1_kernel(const SsmsWin* __restrict__ wins, const SsmpWin* __restrict__ pwins,
                                                        const SsmsMeta* __restrict__ mt) {
  struct Slot { double h[NC], ph[NC], sq[NC], ex[NC], g[NC], yd, fi; };
  const SsmsWin w = wins[blockIdx.y];
  const SsmpWin pw = pwins[blockIdx.y];
  const int s = blockIdx.x, d = mt->d, np = mt->P, steps = w.steps;
  const SsmpLane<NC> ln(mt);
  const double* __restrict__ ex = pw.eps_x + (size_t)s * pw.ldx;
  const double* __restrict__ yd = pw.yd + (size_t)s * pw.lds;
  double* __restrict__ cs = pw.c + (size_t)s * pw.lds;
  auto load = [&](Slot& t, int j) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const size_t e = (size_t)j * d + ln.i[c], q = (size_t)j * np + ln.src[c];
      t.h[c] = ln.on[c] ? w.hrow[e] : 0.0;
      t.ph[c] = ln.on[c] ? w.phi[q] : 0.0;
      t.sq[c] = ln.on[c] ? pw.sq[q] : 0.0;
      t.ex[c] = ln.on[c] ? ex[e] : 0.0;
      t.g[c] = ln.on[c] ? w.g[e] : 0.0;            // (an unobserved step's g was never written and is not used)
    }
    t.yd = yd[j]; t.fi = pw.fi[j];
  };
  Slot ring[SSMP_PF];
#pragma unroll
  for (int k = 0; k < SSMP_PF; k++)
    if (k < steps) load(ring[k], k);
  double wv[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) wv[c] = 0.0;
  for (int j0 = 0; j0 < steps; j0 += SSMP_PF) {
#pragma unroll
    for (int k = 0; k < SSMP_PF; k++) {
      const int j = j0 + k;
      if (j < steps) {                             // (the same for the whole wavefront, as is fi below)
        const Slot t = ring[k];
        if (j + SSMP_PF < steps) load(ring[k], j + SSMP_PF);
#pragma unroll
        for (int c = 0; c < NC; c++) wv[c] = fma(t.ph[c], wv[c], t.sq[c] * t.ex[c]);
        if (t.fi != 0.0) {
          double x = t.h[0] * wv[0];
#pragma unroll
          for (int c = 1; c < NC; c++) x = fma(t.h[c], wv[c], x);
          ssms_wave_sum(x);
          const double cj = (t.yd - x) * t.fi;
#pragma unroll
          for (int c = 0; c < NC; c++) wv[c] = fma(t.g[c], cj, wv[c]);
          if (threadIdx.x == 0) cs[j] = cj;
        }
      }
    }
  }
}

// ---- d. walk 2: slot k holds a step counted from the last ---------------------------------------------------------------------
template <int NC>
__global__ void __launch_bounds__(64) ssmp_walk2_kernel(const SsmsWin* __restrict__ wins, const SsmpWin* __restrict__ pwins,
                                                        const SsmsMeta* __restrict__ mt) {
  struct Slot { double h[NC], ph[NC], g[NC], c, fi; };
  const SsmsWin w = wins[blockIdx.y];
  const SsmpWin pw = pwins[blockIdx.y];
  const int s = blockIdx.x, d = mt->d, np = mt->P, steps = w.steps;
  const SsmpLane<NC> ln(mt);
  const double* __restrict__ cs = pw.c + (size_t)s * pw.lds;
  double* __restrict__ R = pw.R + (size_t)s * pw.lds * d;
  auto load = [&](Slot& t, int j) {                // ph: the transition out of step j, 1 behind the last step
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const size_t e = (size_t)j * d + ln.i[c];
      t.h[c] = ln.on[c] ? w.hrow[e] : 0.0;
      t.ph[c] = (ln.on[c] && j + 1 < steps) ? w.phi[((size_t)j + 1) * np + ln.src[c]] : 1.0;
      t.g[c] = ln.on[c] ? w.g[e] : 0.0;
    }
    t.c = cs[j]; t.fi = pw.fi[j];                  // (an unobserved step's c was never written and is not used)
  };
  Slot ring[SSMP_PF];
#pragma unroll
  for (int k = 0; k < SSMP_PF; k++)
    if (k < steps) load(ring[k], steps - 1 - k);
  double r[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) r[c] = 0.0;
  for (int b0 = 0; b0 < steps; b0 += SSMP_PF) {
#pragma unroll
    for (int k = 0; k < SSMP_PF; k++) {
      const int b = b0 + k, j = steps - 1 - b;
      if (b < steps) {
        const Slot t = ring[k];
        if (b + SSMP_PF < steps) load(ring[k], j - SSMP_PF);
#pragma unroll
        for (int c = 0; c < NC; c++) r[c] *= t.ph[c];
        if (t.fi != 0.0) {
          double x = t.g[0] * r[0];
#pragma unroll
          for (int c = 1; c < NC; c++) x = fma(t.g[c], r[c], x);
          ssms_wave_sum(x);
          const double u = fma(-x, t.fi, t.c);
#pragma unroll
          for (int c = 0; c < NC; c++) r[c] = fma(t.h[c], u, r[c]);
        }
#pragma unroll
        for (int c = 0; c < NC; c++)
          if (ln.on[c]) R[(size_t)j * d + ln.i[c]] = r[c];
      }
    }
  }
}

// ---- e. walk 3: r_j is read SSMP_PF steps ahead of the store of h_j z over it (a lane reads and writes its own entries only) ----
template <int NC>
__global__ void __launch_bounds__(64) ssmp_walk3_kernel(const SsmsWin* __restrict__ wins, const SsmpWin* __restrict__ pwins,
                                                        const SsmsMeta* __restrict__ mt) {
  struct Slot { double h[NC], ph[NC], sq[NC], q[NC], ex[NC], r[NC]; };
  const SsmsWin w = wins[blockIdx.y];
  const SsmpWin pw = pwins[blockIdx.y];
  const int s = blockIdx.x, d = mt->d, np = mt->P, steps = w.steps;
  const SsmpLane<NC> ln(mt);
  const double* __restrict__ ex = pw.eps_x + (size_t)s * pw.ldx;
  double* R = pw.R + (size_t)s * pw.lds * d;
  double v[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) v[c] = ln.on[c] ? w.params[mt->toff[ln.src[c]]] : 0.0;
  auto load = [&](Slot& t, int j) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const size_t e = (size_t)j * d + ln.i[c], q = (size_t)j * np + ln.src[c];
      t.h[c] = ln.on[c] ? w.hrow[e] : 0.0;
      t.ph[c] = ln.on[c] ? w.phi[q] : 0.0;
      t.sq[c] = ln.on[c] ? pw.sq[q] : 0.0;
      t.q[c] = j == 0 ? v[c] : (ln.on[c] ? w.q[q] : 0.0);
      t.ex[c] = ln.on[c] ? ex[e] : 0.0;
      t.r[c] = ln.on[c] ? R[e] : 0.0;
    }
  };
  Slot ring[SSMP_PF];
#pragma unroll
  for (int k = 0; k < SSMP_PF; k++)
    if (k < steps) load(ring[k], k);
  double z[NC];
#pragma unroll
  for (int c = 0; c < NC; c++) z[c] = 0.0;
  for (int j0 = 0; j0 < steps; j0 += SSMP_PF) {
#pragma unroll
    for (int k = 0; k < SSMP_PF; k++) {
      const int j = j0 + k;
      if (j < steps) {
        const Slot t = ring[k];
        if (j + SSMP_PF < steps) load(ring[k], j + SSMP_PF);
#pragma unroll
        for (int c = 0; c < NC; c++) {
          z[c] = fma(t.ph[c], z[c], fma(t.q[c], t.r[c], t.sq[c] * t.ex[c]));
          if (ln.on[c]) R[(size_t)j * d + ln.i[c]] = t.h[c] * z[c];
        }
      }
    }
  }
}

// ---- f. new frames i0 .. i0 + cnt - 1 of every window and draw through out_step (ostep holds that slice) ----------------------
// A workgroup takes SSMP_GF frames of one (window, draw): their rows of h_j z come into LDS with the wavefronts reading along the
// rows (a thread per frame reading its own row would stride by d), then thread (source, frame) adds the source's coordinates
// in ascending order.  The rows lie an odd number of doubles apart, so the frames of one coordinate fall into different banks.
#define SSMP_GF 32
__global__ void __launch_bounds__(256) ssmp_gather_kernel(const SsmsWin* __restrict__ wins, const SsmpWin* __restrict__ pwins,
                                                          const SsmsMeta* __restrict__ mt, int S, int n, int i0, int cnt) {
  __shared__ double tile[SSMP_GF * (SSMS_MAX_D + 1)];
  const SsmsWin w = wins[blockIdx.z];
  const SsmpWin pw = pwins[blockIdx.z];
  const int s = blockIdx.y, f0 = blockIdx.x * SSMP_GF, d = mt->d, np = mt->P, ld = d | 1;
  const int nf = min(SSMP_GF, cnt - f0);
  const double* __restrict__ R = pw.R + (size_t)s * pw.lds * d;
  for (int e = threadIdx.x; e < nf * d; e += 256) {
    const int f = e / d, k = e - f * d;
    tile[f * ld + k] = R[(size_t)w.ostep[f0 + f] * d + k];
  }
  __syncthreads();
  for (int e = threadIdx.x; e < nf * np; e += 256) {
    const int p = e / nf, f = e - p * nf;
    double m = 0.0;
    for (int k = mt->coff[p]; k < mt->coff[p + 1]; k++) m += tile[f * ld + k];
    pw.out[((size_t)p * S + s) * n + i0 + f0 + f] = m;
  }
}

// the sampler's carve: the smoother's prologue and gain blocks (no a^-, no P^-, no per-step posterior), then its own
struct SsmpBufs { SsmsBufs b; char* desc; double *sq, *fi, *sg, *yd, *c, *R; };
static SsmpBufs ssmp_carve(GpArena& ar, size_t d, size_t steps, size_t P, size_t S, size_t count) {
  SsmpBufs o{};
  SsmsBufs& b = o.b;
  b.desc = ar.take<char>(ssms_desc_layout(count, P).bytes);
  b.order = ar.take<int>(count * steps);
  b.want = ar.take<int>(count * steps);
  b.ostep = ar.take<int>(count * steps);
  b.t = ar.take<double>(count * steps);
  b.ys = ar.take<double>(count * steps);
  b.feat = ar.take<double>(count * (d + 6 * P) * steps);
  b.hrow = ar.take<double>(count * steps * d);
  b.phi = ar.take<double>(count * steps * P);
  b.q = ar.take<double>(count * steps * P);
  b.g = ar.take<double>(count * steps * d);
  b.ef = ar.take<double>(count * steps * 2);
  o.desc = ar.take<char>(count * sizeof(SsmpWin));
  o.sq = ar.take<double>(count * steps * P);
  o.fi = ar.take<double>(count * steps);
  o.sg = ar.take<double>(count);
  o.yd = ar.take<double>(count * S * steps);
  o.c = ar.take<double>(count * S * steps);
  o.R = ar.take<double>(count * S * steps * d);
  return o;
}

size_t ssm_sample_workspace_bytes(int d, int steps, int P, int S, int count) {
  if (d < 1 || d > SSMS_MAX_D || steps < 1 || P < 1 || P > d || S < 1 || count < 1) return 0;
  return gp_measure([&](GpArena& ar) { ssmp_carve(ar, d, steps, P, S, count); }) + GP_WS_TAIL_OP;
}

// Every check, then the launches.  Windows w < count: params + w * param_stride, X / Y + w * N, Xnew + w * n, order_host
// + w * (N + n) (the first steps_host[w] entries), out_step_host + w * n, mean / var + w * P * n, loglik + w.
// (`score`: the call is ssm_score_run's; n = 0, the history is kept and launches 8 and 9 follow the forward walk)
// (`smp`: the call is ssm_sample_run's; n >= 1, the sampler's carve, no history, and ssmp_launch follows the forward walk; mean,
// var and loglik are null)
struct SsmsScoreOut { double* grad; double* resid; };
struct SsmsSampleIn { int S; const double* eps_x; const double* eps_y; double* out; };
static gp_status ssmp_launch(gp_handle h, const SsmsSampleIn& smp, const SsmpBufs& pb, const SsmsWin* d_wins,
                             const SsmsMeta* d_meta, int d, int P, int N, int n, int steps, int count, const int32_t* out_step_host);
static gp_status ssms_run(gp_handle h, const int* ktype, const int* km, const int64_t* off_theta, int P, int64_t param_stride,
                          const double* params, const double* X, const double* Y, int N, const double* Xnew, int n, int count,
                          const int32_t* order_host, const int32_t* out_step_host, const int32_t* steps_host, double* mean,
                          double* var, double* loglik, void* ws, size_t ws_bytes, const SsmsScoreOut* score,
                          const SsmsSampleIn* smp = nullptr) {
  if (!params || !X || !Y || !order_host || !steps_host || (!loglik && !smp) || !ws || N < 1 || n < 0 || count < 1 || P < 1)
    return gp_fail(h, GP_ERR_BAD_ARG, "state-space smoother: bad argument (N >= 1, n >= 0, no null pointers)");
  if (n > 0 && (!Xnew || !out_step_host || ((!mean || !var) && !smp)))
    return gp_fail(h, GP_ERR_BAD_ARG, "state-space smoother: Xnew, out_step, mean and var may be null only with n = 0");
  if (smp && (n < 1 || smp->S < 1 || !smp->eps_x || !smp->eps_y || !smp->out))
    return gp_fail(h, GP_ERR_BAD_ARG, "state-space sampler: bad argument (n >= 1, S >= 1, no null pointers)");
  int d = 0;
  for (int i = 0; i < P; i++) {
    if (!ssms_kernel_ok(ktype[i]))
      return gp_fail(h, GP_ERR_UNSUPPORTED,
                     "state-space smoother: every kernel of the sum must have a Matern-1/2 envelope (MercerMatern12sm, Matern12sm, "
                     "Matern12)");
    if (ktype[i] != GP_KERN_MATERN12 && (km[i] < 1 || km[i] > 32))
      return gp_fail(h, GP_ERR_UNSUPPORTED, "state-space smoother: num_partials must be in [1, 32]");
    d += ktype[i] == GP_KERN_MATERN12 ? 1 : 2 * km[i];
    if (d > SSMS_MAX_D)
      return gp_fail(h, GP_ERR_UNSUPPORTED, "state-space smoother: the state dimension d = sum of the sources' components must be in [1, 128]");
  }
  if ((int64_t)N + n > INT32_MAX / 2) return gp_fail(h, GP_ERR_UNSUPPORTED, "state-space smoother: N + n too large");
  if ((int64_t)count * P > 65535 || count > 65535)
    return gp_fail(h, GP_ERR_UNSUPPORTED, "state-space smoother: at most 65535 (window, source) pairs per call");
  int steps = 0;
  for (int w = 0; w < count; w++) {
    if (steps_host[w] < N || steps_host[w] > N + n)
      return gp_fail(h, GP_ERR_BAD_ARG, "state-space smoother: steps must be in [N, N + n]");
    steps = std::max(steps, (int)steps_host[w]);
  }
  if (score) {
    if (param_stride < 1 || param_stride > SSMS_MAX_PARAMS)
      return gp_fail(h, GP_ERR_UNSUPPORTED, "state-space score: the parameter row is longer than 1 + 3 * 128 entries");
    for (int p = 0; p < P; p++)
      if (off_theta[p] < 1 || off_theta[p] + 2 + (ktype[p] == GP_KERN_MATERN12 ? 0 : 2 * km[p]) > param_stride)
        return gp_fail(h, GP_ERR_BAD_ARG, "state-space score: a source's parameters lie outside the parameter row");
    if ((((uintptr_t)ws) & 255) || ws_bytes < ssm_score_workspace_bytes(d, steps, P, count))
      return gp_fail(h, GP_ERR_BAD_ARG, "state-space score: workspace too small for steps * d^2 doubles of history per window "
                                        "(gp_ssm_score_workspace_bytes) or not 256-byte aligned");
  } else if (smp) {
    if ((((uintptr_t)ws) & 255) || ws_bytes < ssm_sample_workspace_bytes(d, steps, P, smp->S, count))
      return gp_fail(h, GP_ERR_BAD_ARG, "state-space sampler: workspace too small for S * steps * d doubles per window "
                                        "(gp_ssm_sample_workspace_bytes) or not 256-byte aligned");
  } else if ((((uintptr_t)ws) & 255) || ws_bytes < ssm_smooth_workspace_bytes(d, steps, P, count))
    return gp_fail(h, GP_ERR_BAD_ARG, "state-space smoother: workspace too small for steps * d^2 doubles of history per window "
                                      "(gp_ssm_smooth_workspace_bytes) or not 256-byte aligned");
  // `order` and `out_step` become device addresses
  std::vector<int> want((size_t)count * steps, 0);
  {
    std::vector<char> seen;
    for (int w = 0; w < count; w++) {
      const int32_t* o = order_host + (size_t)w * (N + n);
      const int sw = steps_host[w];
      seen.assign((size_t)N + n, 0);
      int train = 0;
      for (int j = 0; j < sw; j++) {
        if (o[j] < 0 || o[j] >= N + n || seen[o[j]])
          return gp_fail(h, GP_ERR_BAD_ARG, "state-space smoother: order is not a permutation (every training frame once, no "
                                            "frame twice, entries in [0, N + n))");
        seen[o[j]] = 1;
        train += o[j] < N;
      }
      if (train != N)
        return gp_fail(h, GP_ERR_BAD_ARG, "state-space smoother: order is not a permutation (every training frame once, no frame "
                                          "twice, entries in [0, N + n))");
      for (int i = 0; i < n; i++) {
        const int s = out_step_host[(size_t)w * n + i];
        if (s < 0 || s >= sw) return gp_fail(h, GP_ERR_BAD_ARG, "state-space smoother: out_step out of range [0, steps)");
        want[(size_t)w * steps + s] = 1;
      }
    }
  }
  GpArena ar(ws, ws_bytes);
  SsmpBufs pb{};
  if (smp) pb = ssmp_carve(ar, d, steps, P, smp->S, count);
  const SsmsBufs b = smp ? pb.b : ssms_carve(ar, d, steps, P, count);
  SsmsScoreBufs sb{};
  if (score) sb = ssms_score_carve(ar, d, steps, count);
  if (!ar.ok) return gp_fail(h, GP_ERR_BAD_ARG, "state-space smoother: workspace too small");
  const SsmsDesc lay = ssms_desc_layout(count, P);
  std::vector<char> hd(lay.bytes, 0);
  SsmsWin* wins = (SsmsWin*)(hd.data() + lay.wins);
  SsmsMeta* mt = (SsmsMeta*)(hd.data() + lay.meta);
  FeatItem* feats = (FeatItem*)(hd.data() + lay.feat);
  mt->d = d; mt->P = P; mt->N = N; mt->n = n;
  std::vector<int> foff(P), mpad(P);
  {
    int c = 0, row = 0;
    for (int p = 0; p < P; p++) {
      mt->coff[p] = c; mt->toff[p] = (int)off_theta[p];
      const bool sm = ktype[p] != GP_KERN_MATERN12;
      mpad[p] = sm ? sm_mpad(km[p]) : 0;
      foff[p] = row;
      const int cp = sm ? 2 * km[p] : 1;
      for (int q = 0; q < cp; q++) {
        mt->csrc[c + q] = p;
        mt->crow[c + q] = sm ? row + ((q & 1) ? mpad[p] + (q >> 1) : (q >> 1)) : -1;    // (a_0, b_0, a_1, b_1, ...)
      }
      c += cp; row += 2 * mpad[p];
    }
    mt->coff[P] = c;
  }
  const size_t frows = (size_t)d + 6 * (size_t)P;
  std::vector<int> order_dev((size_t)count * steps, 0);
  for (int w = 0; w < count; w++) {
    SsmsWin& sw = wins[w];
    const size_t s0 = (size_t)w * steps;
    sw.params = params + (size_t)w * param_stride; sw.X = X + (size_t)w * N; sw.Y = Y + (size_t)w * N;
    sw.xnew = n > 0 ? Xnew + (size_t)w * n : nullptr;
    sw.order = b.order + s0; sw.want = b.want + s0; sw.ostep = b.ostep + s0;
    sw.t = b.t + s0; sw.ys = b.ys + s0; sw.feat = b.feat + s0 * frows; sw.hrow = b.hrow + s0 * d;
    sw.phi = b.phi + s0 * P; sw.q = b.q + s0 * P; sw.g = b.g + s0 * d; sw.ef = b.ef + s0 * 2;
    if (!smp) {                                    // (the sampler's carve has no history and no per-step posterior)
      sw.am = b.am + s0 * d; sw.Pm = b.Pm + s0 * d * d; sw.smean = b.smean + s0 * P; sw.svar = b.svar + s0 * P;
      sw.mean = n > 0 ? mean + (size_t)w * P * n : nullptr; sw.var = n > 0 ? var + (size_t)w * P * n : nullptr;
      sw.loglik = loglik + w;
    }
    sw.steps = steps_host[w]; sw.hist = !smp && (n > 0 || score);
    memcpy(order_dev.data() + s0, order_host + (size_t)w * (N + n), (size_t)sw.steps * sizeof(int));
    for (int p = 0; p < P; p++)
      feats[(size_t)p * count + w] = FeatItem{DevKern{ktype[p], km[p], sw.params + off_theta[p]}, sw.t,
                                              sw.feat + (size_t)foff[p] * sw.steps, sw.steps, 0};
  }
  GP_HIP_CHECK(h, hipMemcpyAsync(b.desc, hd.data(), lay.bytes, hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(b.order, order_dev.data(), order_dev.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(b.want, want.data(), want.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  std::vector<char> hs;                                   // the score's descriptor block
  const SsmsScoreDesc slay = ssms_score_desc_layout(count);
  if (score) {
    hs.assign(slay.bytes, 0);
    SsmsScoreWin* swins = (SsmsScoreWin*)(hs.data() + slay.wins);
    SsmsScoreMeta* sm = (SsmsScoreMeta*)(hs.data() + slay.meta);
    sm->nparams = (int)param_stride;
    sm->kind[0] = SSMS_PAR_NOISE;
    for (int p = 0; p < P; p++) {
      const int o = (int)off_theta[p], mp = ktype[p] == GP_KERN_MATERN12 ? 0 : km[p];
      for (int e = 0; e < 2 + 2 * mp; e++) {
        sm->kind[o + e] = e == 0 ? SSMS_PAR_VARIANCE : e == 1 ? SSMS_PAR_LENGTHSCALE : e < 2 + mp ? SSMS_PAR_ENERGY : SSMS_PAR_FREQUENCY;
        sm->src[o + e] = p;
        sm->coord[o + e] = e < 2 ? 0 : mt->coff[p] + 2 * ((e - 2) % mp);
      }
    }
    for (int w = 0; w < count; w++) {
      SsmsScoreWin& s = swins[w];
      const size_t s0 = (size_t)w * steps;
      s.gphi = sb.gphi + s0 * d; s.gq = sb.gq + s0 * d; s.gh = sb.gh + s0 * d; s.gres = sb.gres + s0;
      s.gs2 = sb.gs2 + w; s.gv0 = sb.gv0 + (size_t)w * d;
      s.grad = score->grad + (size_t)w * param_stride;
      s.resid = score->resid ? score->resid + (size_t)w * N : nullptr;
    }
    GP_HIP_CHECK(h, hipMemcpyAsync(sb.desc, hs.data(), slay.bytes, hipMemcpyHostToDevice, h->stream));
  }
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));       // the three are host vectors
  const SsmsWin* d_wins = (const SsmsWin*)(b.desc + lay.wins);
  const SsmsMeta* d_meta = (const SsmsMeta*)(b.desc + lay.meta);
  const FeatItem* d_feat = (const FeatItem*)(b.desc + lay.feat);
  hipLaunchKernelGGL(ssms_times_kernel, dim3((steps + 255) / 256, count), dim3(256), 0, h->stream, d_wins, N);
  GP_HIP_CHECK(h, hipGetLastError());
  for (int p = 0; p < P; p++)
    if (mpad[p]) GP_CHECK(launch_sm_features_items(h, d_feat + (size_t)p * count, count, steps, mpad[p], nullptr, 0));
  hipLaunchKernelGGL(ssms_rows_kernel, dim3((unsigned)(((size_t)steps * d + 255) / 256), count), dim3(256), 0, h->stream, d_wins,
                     d_meta);
  GP_HIP_CHECK(h, hipGetLastError());
  const bool narrow = d <= 64 && !gp_switches().ssm_wide;
  if (narrow) hipLaunchKernelGGL(ssms_forward_kernel<64>, dim3(count), dim3(64), 0, h->stream, d_wins, d_meta);
  else hipLaunchKernelGGL(ssms_forward_kernel<128>, dim3(count), dim3(128), 0, h->stream, d_wins, d_meta);
  GP_HIP_CHECK(h, hipGetLastError());
  if (smp) return ssmp_launch(h, *smp, pb, d_wins, d_meta, d, P, N, n, steps, count, out_step_host);
  hipLaunchKernelGGL(ssms_loglik_kernel, dim3(count), dim3(256), 0, h->stream, d_wins, N);
  GP_HIP_CHECK(h, hipGetLastError());
  if (n > 0) {
    if (narrow) hipLaunchKernelGGL(ssms_backward_kernel<64>, dim3(count), dim3(64), 0, h->stream, d_wins, d_meta);
    else hipLaunchKernelGGL(ssms_backward_kernel<128>, dim3(count), dim3(128), 0, h->stream, d_wins, d_meta);
    GP_HIP_CHECK(h, hipGetLastError());
    // out_step goes through a staging area of `steps` entries per window: new frames may outnumber the steps (repeated frames)
    std::vector<int> stage((size_t)count * steps);
    for (int i0 = 0; i0 < n; i0 += steps) {
      const int cnt = std::min(steps, n - i0);
      for (int w = 0; w < count; w++)
        memcpy(stage.data() + (size_t)w * steps, out_step_host + (size_t)w * n + i0, (size_t)cnt * sizeof(int));
      GP_HIP_CHECK(h, hipMemcpyAsync(b.ostep, stage.data(), stage.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
      GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
      hipLaunchKernelGGL(ssms_gather_kernel, dim3((cnt + 255) / 256, P, count), dim3(256), 0, h->stream, d_wins, P, n, i0, cnt);
      GP_HIP_CHECK(h, hipGetLastError());
    }
  }
  if (score) {
    const SsmsScoreWin* d_swins = (const SsmsScoreWin*)(sb.desc + slay.wins);
    const SsmsScoreMeta* d_smeta = (const SsmsScoreMeta*)(sb.desc + slay.meta);
    if (narrow) hipLaunchKernelGGL(ssms_score_kernel<64>, dim3(count), dim3(64), 0, h->stream, d_wins, d_swins, d_meta);
    else hipLaunchKernelGGL(ssms_score_kernel<128>, dim3(count), dim3(128), 0, h->stream, d_wins, d_swins, d_meta);
    GP_HIP_CHECK(h, hipGetLastError());
    hipLaunchKernelGGL(ssms_score_reduce_kernel, dim3(count, (unsigned)param_stride + 1), dim3(256), 0, h->stream, d_wins, d_swins,
                       d_meta, d_smeta);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return GP_OK;
}

gp_status ssm_smooth_run(gp_handle h, const int* ktype, const int* km, const int64_t* off_theta, int P, int64_t param_stride,
                         const double* params, const double* X, const double* Y, int N, const double* Xnew, int n, int count,
                         const int32_t* order_host, const int32_t* out_step_host, const int32_t* steps_host, double* mean,
                         double* var, double* loglik, void* ws, size_t ws_bytes) {
  return ssms_run(h, ktype, km, off_theta, P, param_stride, params, X, Y, N, Xnew, n, count, order_host, out_step_host, steps_host,
                  mean, var, loglik, ws, ws_bytes, nullptr);
}

// loglik [count], grad [count][param_stride] and, if not null, resid_grad [count][N] = d loglik / d Y of windows w < count, whose
// timelines are their N training frames: order_host + w * N, a permutation of 0 .. N - 1 in ascending time
gp_status ssm_score_run(gp_handle h, const int* ktype, const int* km, const int64_t* off_theta, int P, int64_t param_stride,
                        const double* params, const double* X, const double* Y, int N, int count, const int32_t* order_host,
                        double* loglik, double* grad, double* resid_grad, void* ws, size_t ws_bytes) {
  if (!grad || N < 1 || count < 1)
    return gp_fail(h, GP_ERR_BAD_ARG, "state-space score: bad argument (N >= 1, no null pointers but resid_grad)");
  const std::vector<int32_t> steps((size_t)count, N);
  const SsmsScoreOut out{grad, resid_grad};
  return ssms_run(h, ktype, km, off_theta, P, param_stride, params, X, Y, N, nullptr, 0, count, order_host, nullptr, steps.data(),
                  nullptr, nullptr, loglik, ws, ws_bytes, &out);
}

// The sampler's launches behind the gain walk (ssms_run with `smp`: every check has passed, the prologue and the forward walk are
// enqueued).
static gp_status ssmp_launch(gp_handle h, const SsmsSampleIn& smp, const SsmpBufs& pb, const SsmsWin* d_wins,
                             const SsmsMeta* d_meta, int d, int P, int N, int n, int steps, int count, const int32_t* out_step_host) {
  const size_t S = (size_t)smp.S;
  std::vector<SsmpWin> pw((size_t)count);
  for (int w = 0; w < count; w++) {
    SsmpWin& x = pw[w];
    const size_t s0 = (size_t)w * steps;
    x.eps_x = smp.eps_x + (size_t)w * S * steps * d; x.eps_y = smp.eps_y + (size_t)w * S * N;
    x.out = smp.out + (size_t)w * P * S * n;
    x.sq = pb.sq + s0 * P; x.fi = pb.fi + s0; x.sg = pb.sg + w;
    x.yd = pb.yd + s0 * S; x.c = pb.c + s0 * S; x.R = pb.R + s0 * S * d;
    x.ldx = (size_t)steps * d; x.lds = (size_t)steps;
  }
  GP_HIP_CHECK(h, hipMemcpyAsync(pb.desc, pw.data(), pw.size() * sizeof(SsmpWin), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));       // a host vector
  const SsmpWin* d_pw = (const SsmpWin*)pb.desc;
  hipLaunchKernelGGL(ssmp_prep_kernel, dim3((unsigned)(((size_t)steps * P + 255) / 256), count), dim3(256), 0, h->stream, d_wins, d_pw,
                     d_meta);
  GP_HIP_CHECK(h, hipGetLastError());
  hipLaunchKernelGGL(ssmp_obs_kernel, dim3((steps + 255) / 256, smp.S, count), dim3(256), 0, h->stream, d_wins, d_pw, N);
  GP_HIP_CHECK(h, hipGetLastError());
  const dim3 grid(smp.S, count), wave(64);
  if (d <= 64) {
    hipLaunchKernelGGL(ssmp_walk1_kernel<1>, grid, wave, 0, h->stream, d_wins, d_pw, d_meta);
    hipLaunchKernelGGL(ssmp_walk2_kernel<1>, grid, wave, 0, h->stream, d_wins, d_pw, d_meta);
    hipLaunchKernelGGL(ssmp_walk3_kernel<1>, grid, wave, 0, h->stream, d_wins, d_pw, d_meta);
  } else {
    hipLaunchKernelGGL(ssmp_walk1_kernel<2>, grid, wave, 0, h->stream, d_wins, d_pw, d_meta);
    hipLaunchKernelGGL(ssmp_walk2_kernel<2>, grid, wave, 0, h->stream, d_wins, d_pw, d_meta);
    hipLaunchKernelGGL(ssmp_walk3_kernel<2>, grid, wave, 0, h->stream, d_wins, d_pw, d_meta);
  }
  GP_HIP_CHECK(h, hipGetLastError());
  // out_step through the staging area of `steps` entries per window, as the smoother's gather
  std::vector<int> stage((size_t)count * steps);
  for (int i0 = 0; i0 < n; i0 += steps) {
    const int cnt = std::min(steps, n - i0);
    for (int w = 0; w < count; w++)
      memcpy(stage.data() + (size_t)w * steps, out_step_host + (size_t)w * n + i0, (size_t)cnt * sizeof(int));
    GP_HIP_CHECK(h, hipMemcpyAsync(pb.b.ostep, stage.data(), stage.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
    GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    hipLaunchKernelGGL(ssmp_gather_kernel, dim3((cnt + SSMP_GF - 1) / SSMP_GF, smp.S, count), dim3(256), 0, h->stream, d_wins, d_pw, d_meta, smp.S,
                       n, i0, cnt);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return GP_OK;
}

// S joint draws of every source of windows w < count at their new frames: eps_x + w * S * steps * d laid out [S][steps][d] with
// `steps` the call's longest timeline, eps_y + w * S * N, out + w * P * S * n laid out [P][S][n]; the rest as ssm_smooth_run
gp_status ssm_sample_run(gp_handle h, const int* ktype, const int* km, const int64_t* off_theta, int P, int64_t param_stride,
                         const double* params, const double* X, const double* Y, int N, const double* Xnew, int n, int count,
                         const int32_t* order_host, const int32_t* out_step_host, const int32_t* steps_host, int S,
                         const double* eps_x, const double* eps_y, double* out, void* ws, size_t ws_bytes) {
  if (S > 65535) return gp_fail(h, GP_ERR_UNSUPPORTED, "state-space sampler: at most 65535 draws per call");
  const SsmsSampleIn smp{S, eps_x, eps_y, out};
  return ssms_run(h, ktype, km, off_theta, P, param_stride, params, X, Y, N, Xnew, n, count, order_host, out_step_host, steps_host,
                  nullptr, nullptr, nullptr, ws, ws_bytes, nullptr, &smp);
}

extern "C" size_t gp_ssm_sample_workspace_bytes(int32_t d, int32_t steps, int32_t P, int32_t S, int32_t count) {
  return ssm_sample_workspace_bytes(d, steps, P, S, count);
}
extern "C" size_t gp_ssm_smooth_workspace_bytes(int32_t d, int32_t steps, int32_t P, int32_t count) {
  return ssm_smooth_workspace_bytes(d, steps, P, count);
}
extern "C" size_t gp_ssm_score_workspace_bytes(int32_t d, int32_t steps, int32_t P, int32_t count) {
  return ssm_score_workspace_bytes(d, steps, P, count);
}
