// pdgp_batch.hip — many small, independent Pdgp models per launch sequence (gfx950).
//
// Replaces, for a list of models, the loop  for m in models: m.optimize(method=AdamOptimizer(...), maxiter)
//   Pdgp.build_likelihood   gpitch/pdgp.py:113-170 (whitened: gauss_kl without K, conditional with whiten=True)
//   AdamOptimizer steps     demos/scripts/demo-modgp.py:44-45 (TF-1.2 update on GPflow's free state)
// At the demo's size (minibatch 100, about 100 inducing points per GP) one model's step is a few dozen launches of
// 100 x 100 problems, bound by launch overhead.  Here one step of ALL models is four launches whatever their number:
//   pdgpb_fwd_kernel   one workgroup per latent GP: Kuu + jitter I factored and inverted in LDS, Kuf, A = L^-1 Kuf,
//                      S' = Lq Lq^T - I, U = S' A, fmean = A^T q_mu, fvar = Kdiag + A^T S' A (per column), whitened KL
//   pdgpb_lik_kernel   one workgroup per model: Gauss-Hermite expectations, d/dfmean, d/dfvar, d/dnoise, the ELBO
//   pdgpb_bwd_kernel   one workgroup per latent GP: gradients of q_mu, tril(Lq), the hyper-parameters and z
//   pdgpb_adam_kernel  the TF-1.2 Adam update over the concatenated free state, frozen per model after a failed Cholesky
// With a NatGradAdam token (gp_pdgpb_natgrad) two more launches sit between the backward and the Adam kernel:
//   pdgpb_ng_form_kernel, pdgpb_ng_apply_kernel   the natural-gradient step on q(u) of every stepped latent GP (further down)
// With tied parameters (gp_pdgpb_set_ties) one more launch sits right before the Adam kernel:
//   pdgpb_tie_kernel   every tie group's summed gradient into each member's slot; a tied set with a failed model frozen
// and, for  [m.predict_act_n_com(x) for m, x in zip(models, xnews)], the prediction kernels pdgpb_pred_* further down.
// Every reduction is one thread's sequential loop or a fixed tree: two runs give bit-identical results.
#include "common.h"
#include "gh_quad.h"
#include "sps_tile.h"
#include <algorithm>

#define PB_THREADS 256
#define PB_MAX_M 128
#define PB_MAX_B 1024
#define PB_MAX_PARTIALS 32
#define PB_TILE 64
#define PB_KT 16
#define PB_TILE_DOUBLES (2 * PB_TILE * PB_KT)

struct PbGp {
  int model, row, type, m, M, B, need_theta, need_z;
  int64_t off_theta, off_z, off_qmu, off_qsq;
  int64_t ws;          // this GP's scratch (doubles from the plan's scratch base); prediction plans: its G block
  int64_t f_off;       // row offset in the model-major fmean / fvar / gm / gv arrays
  int64_t batch_off;   // offset of the model's frames in the step's index vector
};
struct PbModel {
  int P, B, nlin, g0;
  int64_t off_noise, p0, p1;   // parameter range [p0, p1) (Adam freeze)
  int64_t f_base, batch_off;
  double num_data;
};

// prediction (gp_pdgpb_predict): one record per latent GP and call
struct PbPredGp {
  int64_t x_off;       // the model's first frame in xnew
  int64_t out_off;     // this GP's row in fmean / fvar (model-major: per model 2P rows of n frames)
  int64_t src_off;     // activation rows: the source's row in mean_source (per model P rows of n frames)
  int64_t n;           // frames of the model
  int32_t P, nlin;
};

// natural-gradient step (gp_pdgpb_natgrad): one record per stepped latent GP of the call
struct PbNgGp {
  int32_t g, pad_;     // its index in the plan
  int64_t ws;          // its [C^-1 (M x M) | w (M)] block, doubles from the first block of the step's workspace
};

// tied parameters (gp_pdgpb_set_ties): group j is members[group_start[j] .. group_start[j + 1]), offsets into
// the parameter vector of slots that are ONE parameter; tied set s is set_models[set_start[s] .. set_start[s + 1]), ascending,
// the models that a chain of groups joins (two models or more); frozen: one sticky word per model of the plan
struct PbTies {
  const int32_t* group_start; const int64_t* members;
  const int32_t* set_start; const int32_t* set_models;
  int32_t* frozen;
  int32_t ngroups, nsets;
};

struct gp_pdgpb_plan_s {
  gp_handle h = nullptr;
  bool predict_only = false;     // created with cfg->batch == NULL
  int nm = 0, G = 0, maxM = 0, maxB = 0, maxm = 0, sumB = 0;
  double jitter = 1e-6;
  int64_t nparams = 0, f_len = 0, scratch = 0;
  std::vector<PbGp> gps;
  std::vector<PbModel> models;
  std::vector<int32_t> owner;
  // device (inside the caller's workspace)
  PbGp* d_gps = nullptr; PbModel* d_models = nullptr; int32_t* d_owner = nullptr; int32_t* d_status = nullptr;
  double *d_fm = nullptr, *d_fv = nullptr, *d_gm = nullptr, *d_gv = nullptr, *d_kl = nullptr, *d_grad = nullptr,
         *d_elbo = nullptr, *d_scr = nullptr;
  bool ready = false;
  // gp_pdgpb_natgrad: every latent GP's block offset in the step's workspace (doubles) and their total; the workspace the
  // plan has seen last (its refusal words were zeroed then) and the list of stepped GPs of the call in flight
  std::vector<int64_t> ng_off;
  int64_t ng_blocks = 0;
  const void* ng_ws = nullptr;
  int32_t* d_refused = nullptr;
  std::vector<PbNgGp> ng_list;
  // gp_pdgpb_natgrad_adaptive: the workspace whose counters the plan has cleared, and their place
  const void* nga_ws = nullptr;
  int64_t* d_ng_halv = nullptr; double* d_ng_short = nullptr;
  // gp_pdgpb_set_ties: the uploaded tie groups and tied sets (all in the caller's ties workspace); ngroups == 0: no ties, the
  // step entries launch no pdgpb_tie_kernel and hand pdgpb_adam_kernel a null tie_frozen
  PbTies ties = {};
  // prediction-only plans: G blocks (doubles; PbGp::ws is a GP's offset among them), the per-call records, and the
  // workspace / parameters of the last gp_pdgpb_predict_prepare
  int64_t pred_g = 0;
  std::vector<PbPredGp> pgs;
  std::vector<int64_t> tiles;
  PbPredGp* d_pgs = nullptr; int64_t* d_tiles = nullptr; double* d_G = nullptr;
  const void* pred_ws = nullptr; const double* pred_params = nullptr;
};

// ---------------------------------------------------------------------------------------------------------------
// covariance entries and their derivatives (the reference's kernels; the squared distance keeps GPflow's expansion,
// as cov.hip does: r2 = ((-2 (a b)) + a a) + b b with a = x / l, b = x' / l, each operation rounded)
__device__ __forceinline__ double pb_r2(double xa, double xb, double ls) {
  const double a = xa / ls, b = xb / ls;
  return __dadd_rn(__dadd_rn(-2.0 * __dmul_rn(a, b), __dmul_rn(a, a)), __dmul_rn(b, b));
}

__device__ double pb_kern(int type, int m, const double* __restrict__ th, double xa, double xb) {
  const double v = th[0], ls = th[1];
  if (type == GP_KERN_MATERN32SM) {                    // kernels.py:232-247 (broadcast form)
    const double d = __dadd_rn(__dadd_rn(xa, -xb), 1e-12);
    const double r = fabs(d);
    const double r1 = 1.7320508075688772 * (r / ls);
    double s = 0.0;
    for (int p = 0; p < m; p++) s += th[2 + p] * cos(6.283185307179586 * th[2 + m + p] * r);
    return v * ((1.0 + r1) * exp(-r1)) * s;
  }
  const double r2 = pb_r2(xa, xb, ls);
  if (type == GP_KERN_RBF) return v * exp(-0.5 * r2);
  const double r = sqrt(r2 + 1e-12);
  if (type == GP_KERN_MATERN12) return v * exp(-r);
  if (type == GP_KERN_MATERN32) return v * (1.0 + 1.7320508075688772 * r) * exp(-1.7320508075688772 * r);
  if (type == GP_KERN_MATERN52) {
    const double s5 = 2.23606797749979;
    return v * (1.0 + s5 * r + (5.0 / 3.0) * (r * r)) * exp(-s5 * r);
  }
  // MercerMatern12sm (matern12_spectral_mixture.py:102-133): v exp(-r) sum_k e_k cos(2 pi f_k (x - x'))
  const double d = xa - xb;
  double s = 0.0;
  for (int p = 0; p < m; p++) s += th[2 + p] * cos(6.283185307179586 * th[2 + m + p] * d);
  return v * exp(-r) * s;
}

__device__ __forceinline__ double pb_kdiag(int type, int m, const double* __restrict__ th) {
  if (type == GP_KERN_MERCER_MATERN12SM || type == GP_KERN_MATERN32SM) {
    double s = th[2];
    for (int p = 1; p < m; p++) s += th[2 + p];
    return th[0] * s;
  }
  return th[0];
}

// acc[c] += w * dK(xa, xb)/dtheta_c (theta = [v, l, e_0.., f_0..]); returns dK/dxa
__device__ double pb_kern_grad(int type, int m, const double* __restrict__ th, double xa, double xb, double w,
                               double* __restrict__ acc, bool want_theta) {
  const double v = th[0], ls = th[1];
  const double TWO_PI = 6.283185307179586;
  if (type == GP_KERN_MATERN32SM) {
    const double d = __dadd_rn(__dadd_rn(xa, -xb), 1e-12);
    const double r = fabs(d), sg = d >= 0.0 ? 1.0 : -1.0;
    const double r1 = 1.7320508075688772 * (r / ls);
    const double e1 = exp(-r1), E = (1.0 + r1) * e1;
    double s = 0.0, ds = 0.0;
    for (int p = 0; p < m; p++) {
      const double om = TWO_PI * th[2 + m + p];
      double sn, cs;
      sincos(om * r, &sn, &cs);
      s += th[2 + p] * cs;
      ds -= th[2 + p] * om * sn;
      if (want_theta) {
        acc[2 + p] += w * v * E * cs;
        acc[2 + m + p] += w * v * E * th[2 + p] * (-TWO_PI * r * sn);
      }
    }
    if (want_theta) {
      acc[0] += w * E * s;
      acc[1] += w * v * s * r1 * r1 * e1 / ls;
    }
    return sg * v * (s * (-r1 * e1) * (1.7320508075688772 / ls) + E * ds);
  }
  const double a = xa / ls, b = xb / ls;
  const double r2 = pb_r2(xa, xb, ls);
  const double dr2_da = (2.0 * a - 2.0 * b) / ls;      // d r2 / d xa
  const double dr2_dl = -2.0 * r2 / ls;
  if (type == GP_KERN_RBF) {
    const double e = exp(-0.5 * r2), K = v * e;
    if (want_theta) { acc[0] += w * e; acc[1] += w * K * (-0.5) * dr2_dl; }
    return K * (-0.5) * dr2_da;
  }
  const double r = sqrt(r2 + 1e-12);
  const double dr_da = 0.5 * dr2_da / r, dr_dl = 0.5 * dr2_dl / r;
  double prof, dprof;                                  // K = v prof(r) [* S]
  if (type == GP_KERN_MATERN32) {
    const double s3 = 1.7320508075688772, e = exp(-s3 * r);
    prof = (1.0 + s3 * r) * e; dprof = -3.0 * r * e;
  } else if (type == GP_KERN_MATERN52) {
    const double s5 = 2.23606797749979, e = exp(-s5 * r);
    prof = (1.0 + s5 * r + (5.0 / 3.0) * (r * r)) * e; dprof = -(5.0 / 3.0) * r * (1.0 + s5 * r) * e;
  } else {                                             // Matern12 and the Mercer envelope
    prof = exp(-r); dprof = -prof;
  }
  if (type != GP_KERN_MERCER_MATERN12SM) {
    if (want_theta) { acc[0] += w * prof; acc[1] += w * v * dprof * dr_dl; }
    return v * dprof * dr_da;
  }
  const double d = xa - xb;
  double s = 0.0, ds = 0.0;
  for (int p = 0; p < m; p++) {
    const double om = TWO_PI * th[2 + m + p];
    double sn, cs;
    sincos(om * d, &sn, &cs);
    s += th[2 + p] * cs;
    ds -= th[2 + p] * om * sn;
    if (want_theta) {
      acc[2 + p] += w * v * prof * cs;
      acc[2 + m + p] += w * v * prof * th[2 + p] * (-TWO_PI * d * sn);
    }
  }
  if (want_theta) { acc[0] += w * prof * s; acc[1] += w * v * dprof * dr_dl * s; }
  return v * (dprof * dr_da * s + prof * ds);
}

// ---------------------------------------------------------------------------------------------------------------
// C (M x N, row stride ldc) = alpha op(A) op(B) + beta C with op(A)(i, k) = A[i ars + k acs], op(B)(k, j) = B[k brs + j bcs].
// 64 x 64 output tiles, 16-deep k slices through LDS, 4 x 4 outputs per thread, k in ascending order (deterministic).
struct PbMat { const double* p; int64_t rs, cs; };
__device__ void pb_gemm(int M, int N, int K, PbMat A, PbMat B, double* C, int64_t ldc, double alpha, double beta,
                        double* __restrict__ sm) {
  double* As = sm;
  double* Bs = sm + PB_TILE * PB_KT;
  const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
  for (int i0 = 0; i0 < M; i0 += PB_TILE)
    for (int j0 = 0; j0 < N; j0 += PB_TILE) {
      double acc[4][4];
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) acc[r][c] = 0.0;
      for (int k0 = 0; k0 < K; k0 += PB_KT) {
        for (int e = tid; e < PB_TILE * PB_KT; e += PB_THREADS) {
          const int kk = e / PB_TILE, ii = e % PB_TILE;
          const int gi = i0 + ii, gj = j0 + ii, gk = k0 + kk;
          As[e] = (gi < M && gk < K) ? A.p[gi * A.rs + gk * A.cs] : 0.0;
          Bs[e] = (gj < N && gk < K) ? B.p[gk * B.rs + gj * B.cs] : 0.0;
        }
        __syncthreads();
#pragma unroll 4
        for (int kk = 0; kk < PB_KT; kk++) {
          double a[4], b[4];
#pragma unroll
          for (int r = 0; r < 4; r++) a[r] = As[kk * PB_TILE + ty * 4 + r];
#pragma unroll
          for (int c = 0; c < 4; c++) b[c] = Bs[kk * PB_TILE + tx * 4 + c];
#pragma unroll
          for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[r][c] = fma(a[r], b[c], acc[r][c]);
        }
        __syncthreads();
      }
#pragma unroll
      for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
          const int gi = i0 + ty * 4 + r, gj = j0 + tx * 4 + c;
          if (gi < M && gj < N) {
            double* o = C + (int64_t)gi * ldc + gj;
            *o = beta != 0.0 ? alpha * acc[r][c] + beta * *o : alpha * acc[r][c];
          }
        }
    }
  __syncthreads();
}

// scratch of one latent GP (doubles): six M x M and six M x B blocks
__host__ __device__ inline int64_t pb_gp_scratch(int M, int B) { return 6 * (int64_t)M * M + 6 * (int64_t)M * B; }
struct PbScr { double *L, *W, *Lq, *S, *T1, *T2, *K, *A, *U, *Ab, *Kb, *TB; };
__device__ inline PbScr pb_scr(double* base, int M, int B) {
  PbScr s;
  const int64_t mm = (int64_t)M * M, mb = (int64_t)M * B;
  s.L = base; s.W = s.L + mm; s.Lq = s.W + mm; s.S = s.Lq + mm; s.T1 = s.S + mm; s.T2 = s.T1 + mm;
  s.K = s.T2 + mm; s.A = s.K + mb; s.U = s.A + mb; s.Ab = s.U + mb; s.Kb = s.Ab + mb; s.TB = s.Kb + mb;
  return s;
}

// ---------------------------------------------------------------------------------------------------------------
// A symmetric M x M matrix in LDS (Ls, row-major ld = M, written and synchronised by the caller) factored and inverted in
// place by the whole workgroup: on return Ls holds the inverse of its lower Cholesky factor L, zeros above the diagonal; L
// itself is copied to Lcopy (global) when COPY_L.  tmp: M doubles of LDS.  Shared by Kuu + jitter I (pb_factor_invert) and
// the natural-gradient step's reversed B (pdgpb_ng_form_kernel); `word` is the model's word for this kind of failure.
// RAISE = false (the adaptive natural-gradient step, which factors again at half the length): the word is left to the caller.
template <bool COPY_L, bool RAISE = true>
__device__ __forceinline__ void pb_chol_invert(int M, double* Ls, double* tmp, int& bad_pivot, int32_t* __restrict__ word,
                                               int row, double* Lcopy) {
  const int tid = threadIdx.x;
  // right-looking Cholesky in place (lower); a non-positive pivot is recorded and replaced by 1 so that the rest of the
  // pass stays finite (the model is frozen by the Adam kernel and reported to the host)
  for (int k = 0; k < M; k++) {
    if (tid == 0) {
      double d = Ls[k * M + k];
      if (!(d > 0.0)) { if (bad_pivot < 0) bad_pivot = k; d = 1.0; }
      Ls[k * M + k] = sqrt(d);
    }
    __syncthreads();
    const double dk = Ls[k * M + k];
    for (int i = k + 1 + tid; i < M; i += PB_THREADS) Ls[i * M + k] /= dk;
    __syncthreads();
    const int n = M - k - 1;
    for (int e = tid; e < n * n; e += PB_THREADS) {
      const int i = k + 1 + e / n, j = k + 1 + e % n;
      if (j <= i) Ls[i * M + j] = fma(-Ls[i * M + k], Ls[j * M + k], Ls[i * M + j]);
    }
    __syncthreads();
  }
  for (int e = tid; e < M * M; e += PB_THREADS) {
    const int i = e / M, j = e % M;
    if (j > i) Ls[e] = 0.0;
  }
  __syncthreads();
  // status word of the model: 0, or INT_MAX - (128 row + pivot); the maximum keeps the failure with the smallest
  // (row, pivot) whatever order the model's workgroups finish in
  if (RAISE && tid == 0 && bad_pivot >= 0) atomicMax(word, 0x7fffffff - (PB_MAX_M * row + bad_pivot));
  if (COPY_L)
    for (int e = tid; e < M * M; e += PB_THREADS) Lcopy[e] = Ls[e];
  __syncthreads();
  // W = L^-1 in place (LAPACK trti2, lower, columns from the last): W[j+1:, j] = -W[j+1:, j+1:] L[j+1:, j] / L[j, j]
  for (int j = M - 1; j >= 0; j--) {
    if (tid > j && tid < M) tmp[tid] = Ls[tid * M + j];
    __syncthreads();
    const double ajj = -1.0 / Ls[j * M + j];
    if (tid > j && tid < M) {
      double y = 0.0;
      for (int k = j + 1; k <= tid; k++) y = fma(Ls[tid * M + k], tmp[k], y);
      Ls[tid * M + j] = y * ajj;
    }
    __syncthreads();
    if (tid == 0) Ls[j * M + j] = -ajj;
    __syncthreads();
  }
}

// Kuu + jitter I of one latent GP factored and inverted in LDS by the whole workgroup (pdgpb_fwd_kernel and
// pdgpb_pred_prep_kernel): on return Ls holds W = L^-1.  zs: the z of the GP in LDS.
template <bool COPY_L>
__device__ __forceinline__ void pb_factor_invert(int type, int m, const double* __restrict__ th, const double* zs, int M,
                                                 double jitter, double* Ls, double* tmp, int& bad_pivot,
                                                 int32_t* __restrict__ status, int model, int row, double* Lcopy) {
  const int tid = threadIdx.x;
  // Kuu + jitter I (pdgp.py:126-129 / GPflow conditional), full matrix, row-major ld = M
  for (int e = tid; e < M * M; e += PB_THREADS) {
    const int i = e / M, j = e % M;
    Ls[e] = pb_kern(type, m, th, zs[i], zs[j]) + (i == j ? jitter : 0.0);
  }
  __syncthreads();
  pb_chol_invert<COPY_L>(M, Ls, tmp, bad_pivot, &status[model], row, Lcopy);
}

// ---------------------------------------------------------------------------------------------------------------
// forward: one workgroup per latent GP.  LDS: [maxM^2 factor | maxB frames | maxM z | maxM tmp | gemm tiles]
__global__ void __launch_bounds__(PB_THREADS) pdgpb_fwd_kernel(const PbGp* __restrict__ gps, const double* __restrict__ params,
                                                               const double* __restrict__ xall, const int32_t* __restrict__ idx,
                                                               double* __restrict__ scr_base, double* __restrict__ fmean,
                                                               double* __restrict__ fvar, double* __restrict__ kl,
                                                               int32_t* __restrict__ status, double jitter, int maxM, int maxB) {
  extern __shared__ double pb_sm[];
  const PbGp g = gps[blockIdx.x];
  const int M = g.M, B = g.B, tid = threadIdx.x;
  double* Ls = pb_sm;
  double* xs = Ls + (int64_t)maxM * maxM;
  double* zs = xs + maxB;
  double* tmp = zs + maxM;
  double* tiles = tmp + maxM;
  __shared__ int bad_pivot;
  const double* th = params + g.off_theta;
  const double* z = params + g.off_z;
  const double* qmu = params + g.off_qmu;
  const double* qsq = params + g.off_qsq;
  PbScr s = pb_scr(scr_base + g.ws, M, B);
  for (int n = tid; n < B; n += PB_THREADS) xs[n] = xall[idx[g.batch_off + n]];
  for (int i = tid; i < M; i += PB_THREADS) zs[i] = z[i];
  if (tid == 0) bad_pivot = -1;
  __syncthreads();
  pb_factor_invert<true>(g.type, g.m, th, zs, M, jitter, Ls, tmp, bad_pivot, status, g.model, g.row, s.L);
  for (int e = tid; e < M * M; e += PB_THREADS) s.W[e] = Ls[e];
  // tril(q_sqrt) (band_part in GPflow's conditional / gauss_kl)
  for (int e = tid; e < M * M; e += PB_THREADS) {
    const int i = e / M, j = e % M;
    s.Lq[e] = j <= i ? qsq[e] : 0.0;
  }
  // Kuf (M x B)
  for (int e = tid; e < M * B; e += PB_THREADS) {
    const int i = e / B, n = e % B;
    s.K[e] = pb_kern(g.type, g.m, th, zs[i], xs[n]);
  }
  __syncthreads();
  // A = W Kuf; S' = Lq Lq^T - I; U = S' A
  pb_gemm(M, B, M, PbMat{s.W, M, 1}, PbMat{s.K, B, 1}, s.A, B, 1.0, 0.0, tiles);
  pb_gemm(M, M, M, PbMat{s.Lq, M, 1}, PbMat{s.Lq, 1, M}, s.S, M, 1.0, 0.0, tiles);
  for (int i = tid; i < M; i += PB_THREADS) s.S[(int64_t)i * M + i] -= 1.0;
  __syncthreads();
  pb_gemm(M, B, M, PbMat{s.S, M, 1}, PbMat{s.A, B, 1}, s.U, B, 1.0, 0.0, tiles);
  // fmean = A^T q_mu, fvar = Kdiag + sum_i A U (GPflow: Kdiag - sum A^2 + sum (Lq^T A)^2)
  const double kd = pb_kdiag(g.type, g.m, th);
  for (int n = tid; n < B; n += PB_THREADS) {
    double fm = 0.0, q = 0.0;
    for (int i = 0; i < M; i++) {
      const double a = s.A[(int64_t)i * B + n];
      fm = fma(a, qmu[i], fm);
      q = fma(a, s.U[(int64_t)i * B + n], q);
    }
    fmean[g.f_off + n] = fm;
    fvar[g.f_off + n] = kd + q;
  }
  // whitened KL (GPflow gauss_kl, K = None): 0.5 (|q_mu|^2 - M - sum log Lq_ii^2 + |tril Lq|^2); one thread, fixed order
  if (tid == 0) {
    double a = 0.0, ld = 0.0, tr = 0.0;
    for (int i = 0; i < M; i++) {
      a = fma(qmu[i], qmu[i], a);
      const double dq = qsq[(int64_t)i * M + i];
      ld += log(dq * dq);
      for (int j = 0; j <= i; j++) { const double l = qsq[(int64_t)i * M + j]; tr = fma(l, l, tr); }
    }
    kl[blockIdx.x] = 0.5 * (a - (double)M - ld + tr);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// likelihood: one workgroup per model (likelihoods.py:422-447 and :47-68, scaled by N / B: pdgp.py:166-170)
__global__ void __launch_bounds__(PB_THREADS) pdgpb_lik_kernel(const PbModel* __restrict__ models, const double* __restrict__ params,
                                                               const double* __restrict__ yall, const int32_t* __restrict__ idx,
                                                               const double* __restrict__ fmean, const double* __restrict__ fvar,
                                                               const double* __restrict__ kl, double* __restrict__ gm,
                                                               double* __restrict__ gv, double* __restrict__ grad,
                                                               double* __restrict__ elbo) {
  const PbModel md = models[blockIdx.x];
  const int P = md.P, B = md.B, tid = threadIdx.x;
  const double s2 = params[md.off_noise];
  const double scale = md.num_data / (double)B;
  const double* Fm = fmean + md.f_base;
  const double* Fv = fvar + md.f_base;
  const bool want_grad = grad != nullptr;
  double ve = 0.0, dnoise = 0.0;
  for (int n = tid; n < B; n += PB_THREADS) {
    const double Y = yall[idx[md.batch_off + n]];
    double A = 0.0, Bs = 0.0, Cpair = 0.0;
    for (int i = 0; i < P; i++) {
      const Quad q = gh_quad(md.nlin, Fm[(int64_t)i * B + n], Fv[(int64_t)i * B + n], false);
      const double mf = Fm[(int64_t)(i + P) * B + n], vf = Fv[(int64_t)(i + P) * B + n];
      const double a = q.E1 * mf;
      Cpair = fma(a, A, Cpair);
      A += a;
      Bs = fma(q.E2, vf + mf * mf, Bs);
    }
    const double resid = Y * Y - 2.0 * Y * A + Bs + 2.0 * Cpair;
    const double LOG2PI = 1.8378770664093453;
    ve += scale * (-0.5 * ((1.0 / s2) * resid + LOG2PI + log(s2)));
    if (!want_grad) continue;
    dnoise += scale * (0.5 * resid / (s2 * s2) - 0.5 / s2);
    const double qf = -0.5 * scale / s2;
    for (int i = 0; i < P; i++) {
      const double mg = Fm[(int64_t)i * B + n], vg = Fv[(int64_t)i * B + n];
      const double mf = Fm[(int64_t)(i + P) * B + n], vf = Fv[(int64_t)(i + P) * B + n];
      const Quad q = gh_quad(md.nlin, mg, vg, true);
      const double a = q.E1 * mf;
      const double da = qf * (-2.0 * Y + 2.0 * (A - a));
      const double dE1 = da * mf, dE2 = qf * (vf + mf * mf);
      const double sd = sqrt(2.0 * vg);
      const double inv_sd = sd > 0.0 ? 1.0 / sd : 0.0;
      gm[md.f_base + (int64_t)i * B + n] = dE1 * q.dE1m + dE2 * q.dE2m;
      gv[md.f_base + (int64_t)i * B + n] = (dE1 * q.dE1s + dE2 * q.dE2s) * inv_sd;
      gm[md.f_base + (int64_t)(i + P) * B + n] = da * q.E1 + qf * q.E2 * 2.0 * mf;
      gv[md.f_base + (int64_t)(i + P) * B + n] = qf * q.E2;
    }
  }
  __shared__ double red[2][PB_THREADS];
  red[0][tid] = ve; red[1][tid] = dnoise;
  __syncthreads();
  for (int o = PB_THREADS / 2; o > 0; o >>= 1) {
    if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
    __syncthreads();
  }
  if (tid == 0) {
    double k = 0.0;
    for (int g = 0; g < 2 * P; g++) k += kl[md.g0 + g];
    elbo[blockIdx.x] = red[0][0] - k;
    if (want_grad) grad[md.off_noise] = red[1][0];
  }
}

// ---------------------------------------------------------------------------------------------------------------
// backward: one workgroup per latent GP (the whitened path of bwd.hip, restated per GP).  With Abar = dELBO/dA:
//   Abar = q_mu gm^T + 2 U diag(gv);  d q_mu = A gm - q_mu;  d Lq = tril(2 (A diag(gv) A^T) Lq) - Lq + diag(1 / Lq_ii)
//   Kbar = W^T Abar (d/dKuf);  Lbar = -tril(Kbar A^T);  Kuu_bar = sym(W^T Phi(L^T Lbar) W)  (Cholesky backward)
//   d theta = <Kuu_bar, dKuu> + <Kbar, dKuf> + sum_n gv_n dKdiag;  d z_i = 2 sum_{j != i} Kuu_bar_ij dK(z_i, z_j)/dz_i
//             + sum_n Kbar_in dK(z_i, x_n)/dz_i
__global__ void __launch_bounds__(PB_THREADS) pdgpb_bwd_kernel(const PbGp* __restrict__ gps, const double* __restrict__ params,
                                                               const double* __restrict__ xall, const int32_t* __restrict__ idx,
                                                               double* __restrict__ scr_base, const double* __restrict__ gm_all,
                                                               const double* __restrict__ gv_all, double* __restrict__ grad,
                                                               int maxM, int maxB, int maxth) {
  extern __shared__ double pb_sm[];
  const PbGp g = gps[blockIdx.x];
  const int M = g.M, B = g.B, tid = threadIdx.x, NT = GP_THETA_LEN(g.m);
  double* xs = pb_sm;
  double* zs = xs + maxB;
  double* tiles = zs + maxM;
  double* thacc = tiles + PB_TILE_DOUBLES;      // [maxM][maxth]
  const double* th = params + g.off_theta;
  const double* z = params + g.off_z;
  const double* qmu = params + g.off_qmu;
  const double* gm = gm_all + g.f_off;
  const double* gv = gv_all + g.f_off;
  PbScr s = pb_scr(scr_base + g.ws, M, B);
  for (int n = tid; n < B; n += PB_THREADS) xs[n] = xall[idx[g.batch_off + n]];
  for (int i = tid; i < M; i += PB_THREADS) zs[i] = z[i];
  // Abar and A diag(gv)
  for (int e = tid; e < M * B; e += PB_THREADS) {
    const int i = e / B, n = e % B;
    s.Ab[e] = fma(qmu[i], gm[n], 2.0 * s.U[e] * gv[n]);
    s.TB[e] = s.A[e] * gv[n];
  }
  // d q_mu (the KL's -q_mu included)
  for (int i = tid; i < M; i += PB_THREADS) {
    double a = 0.0;
    for (int n = 0; n < B; n++) a = fma(s.A[(int64_t)i * B + n], gm[n], a);
    grad[g.off_qmu + i] = a - qmu[i];
  }
  __syncthreads();
  // H = A diag(gv) A^T -> T1; T2 = H Lq; d Lq = tril(2 T2) - Lq + diag(1 / Lq_ii)
  pb_gemm(M, M, B, PbMat{s.TB, B, 1}, PbMat{s.A, 1, B}, s.T1, M, 1.0, 0.0, tiles);
  pb_gemm(M, M, M, PbMat{s.T1, M, 1}, PbMat{s.Lq, M, 1}, s.T2, M, 2.0, 0.0, tiles);
  for (int e = tid; e < M * M; e += PB_THREADS) {
    const int i = e / M, j = e % M;
    double d = 0.0;
    if (j <= i) {
      d = s.T2[e] - s.Lq[e];
      if (i == j) d += 1.0 / s.Lq[e];
    }
    grad[g.off_qsq + e] = d;
  }
  __syncthreads();
  if (!g.need_theta && !g.need_z) {      // every hyper-parameter and z fixed: their slots read 0
    for (int c = tid; c < NT; c += PB_THREADS) grad[g.off_theta + c] = 0.0;
    for (int i = tid; i < M; i += PB_THREADS) grad[g.off_z + i] = 0.0;
    return;
  }
  // Kbar = W^T Abar; T1 = Lbar = -tril(Kbar A^T); T2 = Phi(L^T Lbar) (lower, halved diagonal); T1 = T2 W; S-block
  // reuse: X = W^T T1 -> T2, Kuu_bar = sym(X)
  pb_gemm(M, B, M, PbMat{s.W, 1, M}, PbMat{s.Ab, B, 1}, s.Kb, B, 1.0, 0.0, tiles);
  pb_gemm(M, M, B, PbMat{s.Kb, B, 1}, PbMat{s.A, 1, B}, s.T1, M, -1.0, 0.0, tiles);
  for (int e = tid; e < M * M; e += PB_THREADS) {
    const int i = e / M, j = e % M;
    if (j > i) s.T1[e] = 0.0;
  }
  __syncthreads();
  pb_gemm(M, M, M, PbMat{s.L, 1, M}, PbMat{s.T1, M, 1}, s.T2, M, 1.0, 0.0, tiles);
  for (int e = tid; e < M * M; e += PB_THREADS) {
    const int i = e / M, j = e % M;
    if (j > i) s.T2[e] = 0.0;
    else if (j == i) s.T2[e] *= 0.5;
  }
  __syncthreads();
  pb_gemm(M, M, M, PbMat{s.T2, M, 1}, PbMat{s.W, M, 1}, s.T1, M, 1.0, 0.0, tiles);
  pb_gemm(M, M, M, PbMat{s.W, 1, M}, PbMat{s.T1, M, 1}, s.T2, M, 1.0, 0.0, tiles);
  // contraction: thread i < M takes row i of Kuu and Kuf; theta partial sums per row in LDS, summed over rows in order
  const bool want_theta = g.need_theta != 0;
  if (tid < M) {
    const int i = tid;
    double* acc = thacc + (int64_t)i * maxth;
    for (int c = 0; c < NT; c++) acc[c] = 0.0;
    double dz = 0.0;
    const double zi = zs[i];
    for (int j = 0; j < M; j++) {
      const double w = 0.5 * (s.T2[(int64_t)i * M + j] + s.T2[(int64_t)j * M + i]);
      const double dk = pb_kern_grad(g.type, g.m, th, zi, zs[j], w, acc, want_theta);
      if (j != i) dz = fma(2.0 * w, dk, dz);
    }
    for (int n = 0; n < B; n++) {
      const double w = s.Kb[(int64_t)i * B + n];
      dz = fma(w, pb_kern_grad(g.type, g.m, th, zi, xs[n], w, acc, want_theta), dz);
    }
    grad[g.off_z + i] = dz;
  }
  __syncthreads();
  if (tid < NT) {
    double a = 0.0;
    for (int i = 0; i < M; i++) a += thacc[(int64_t)i * maxth + tid];
    // Kdiag: d/dv of v (stationary) or v sum e (spectral mixtures), d/de_k = v
    double sgv = 0.0;
    for (int n = 0; n < B; n++) sgv += gv[n];
    const bool energy = (g.type == GP_KERN_MERCER_MATERN12SM || g.type == GP_KERN_MATERN32SM);
    if (tid == 0) {
      double e = 1.0;
      if (energy) { e = th[2]; for (int p = 1; p < g.m; p++) e += th[2 + p]; }
      a = fma(sgv, e, a);
    } else if (energy && tid >= 2 && tid < 2 + g.m) {
      a = fma(sgv, th[0], a);
    }
    grad[g.off_theta + tid] = a;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// TF-1.2 Adam on the concatenated free state (opt.hip adam_kernel, per-model step size and freeze)
__device__ __forceinline__ double pb_softplus_pos(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))) + 1e-6; }

__global__ void __launch_bounds__(256) pdgpb_adam_kernel(double* __restrict__ fs, double* __restrict__ params,
                                                         const double* __restrict__ grad, const uint8_t* __restrict__ tc,
                                                         double* __restrict__ m, double* __restrict__ v,
                                                         const int32_t* __restrict__ owner, const int32_t* __restrict__ status,
                                                         const int32_t* __restrict__ refused,
                                                         const int32_t* __restrict__ tie_frozen,
                                                         const double* __restrict__ lr_t, int64_t n, double b1, double b2,
                                                         double eps, GpLogisticTable T) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const uint8_t t = tc[i];
    const int k = owner[i];
    // frozen: a failed Kuu, or (gp_pdgpb_natgrad; null on the Adam-only path) a refused natural-gradient step, or
    // (gp_pdgpb_set_ties; null without ties) a failed model of the same tied set
    if (t == 2 || status[k] != 0 || (refused && refused[k] != 0) || (tie_frozen && tie_frozen[k] != 0)) continue;
    double x = fs[i];
    double g = -grad[i];
    if (t == 1) g *= 1.0 / (1.0 + exp(-x));
    else if (t >= 3) { const double s = 1.0 / (1.0 + exp(-x)); g *= (T.b[t - 3] - T.a[t - 3]) * s * (1.0 - s); }
    const double mi = b1 * m[i] + (1.0 - b1) * g;
    const double vi = b2 * v[i] + (1.0 - b2) * g * g;
    m[i] = mi; v[i] = vi;
    x -= lr_t[k] * mi / (sqrt(vi) + eps);
    fs[i] = x;
    params[i] = (t == 1) ? pb_softplus_pos(x)
                         : (t >= 3 ? T.a[t - 3] + (T.b[t - 3] - T.a[t - 3]) / (1.0 + exp(-x)) : x);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// tied parameters (gp_pdgpb_set_ties): one launch between the backward pass (and the natural-gradient kernels)
// and pdgpb_adam_kernel.  One thread per tie group, PB_TIE_GROUPS groups per workgroup; behind the groups one thread per tied
// set.  A group's thread walks its member list twice, in the listed order: it sums d ELBO / d parameter over the members
// (sequentially: no atomics, the same bits in every run) and writes the sum into every member's slot of `grad`.  Every slot
// belongs to one group at most (gp_pdgpb_set_ties checks it), so no two threads touch the same slot.  The members hold the
// same free state, moments, transform code and step length: pdgpb_adam_kernel's unchanged arithmetic then moves them alike.
// A set's thread reads its models' Kuu status and refusal words; when one is raised, every model of the set whose sticky
// `frozen` word is still 0 gets 1 + the lowest failed model's index, which freezes it in the Adam launch behind this one —
// the failed model's gradient has been summed into the groups above, and is never applied.
#define PB_TIE_GROUPS 256
__global__ void __launch_bounds__(PB_TIE_GROUPS) pdgpb_tie_kernel(PbTies t, double* __restrict__ grad,
                                                                  const int32_t* __restrict__ status,
                                                                  const int32_t* __restrict__ refused) {
  const int i = blockIdx.x * PB_TIE_GROUPS + threadIdx.x;
  if (i < t.ngroups) {
    const int32_t a = t.group_start[i], b = t.group_start[i + 1];
    double s = 0.0;
    for (int32_t j = a; j < b; j++) s += grad[t.members[j]];
    for (int32_t j = a; j < b; j++) grad[t.members[j]] = s;
  } else if (i < t.ngroups + t.nsets) {
    const int32_t a = t.set_start[i - t.ngroups], b = t.set_start[i - t.ngroups + 1];
    int32_t failed = -1;
    for (int32_t j = a; j < b && failed < 0; j++) {       // set_models ascends: the first raised word is the lowest model's
      const int32_t k = t.set_models[j];
      if (status[k] != 0 || (refused && refused[k] != 0)) failed = k;
    }
    if (failed >= 0)
      for (int32_t j = a; j < b; j++) {
        const int32_t k = t.set_models[j];
        if (t.frozen[k] == 0) t.frozen[k] = 1 + failed;
      }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// natural-gradient step on q(u) of many models (gp_pdgpb_natgrad; the map of natgrad.hip's header): per stepped
// latent GP, with Lq = tril(q_sqrt), g = d ELBO / d q_mu, G_L = tril(d ELBO / d q_sqrt),
//   Phi = tril(Lq^T G_L),  B = I - gamma (Phi + Phi^T - diag Phi),  J B J = C C^T,  Lq' = Lq U^-T (U^-T = J C^-T J),
//   q_mu' = q_mu + gamma Lq' (Lq'^T g).
// Two launches between pdgpb_bwd_kernel and pdgpb_adam_kernel whatever the number of models, over the uploaded list of
// stepped GPs:
//   pdgpb_ng_form_kernel   one workgroup per stepped GP: the reversed B formed in LDS on v_mfma_f64_16x16x4_f64 from params /
//                          grad in place, w = Lq^T g, then B factored and inverted where it lies (pb_chol_invert); C^-1 and w
//                          go to the step's workspace.  A non-positive pivot raises the model's refusal word (not the Kuu word)
//   pdgpb_ng_apply_kernel  one workgroup per (stepped GP, block of 32 rows): nothing when the model's Kuu word or refusal word is
//                          set (every B of the model was factored by the launch before: none of a refused model's GPs moves);
//                          else Lq' = Lq U^-T on the MFMA in place, q_mu', both to params and free_state, their gradient blocks
//                          zeroed so that Adam behind it leaves them alone.
// Lq is never inverted.  Every sum is one thread's ordered loop, the MFMA's fixed k order or a fixed butterfly.
typedef double pb_d4 __attribute__((ext_vector_type(4)));
#define PB_NG_TILE 32

// LDS: [maxM^2 reversed B -> C -> C^-1 | maxM tmp].  Phi_ij = sum_{k >= max(i, j)} Lq_ki G_kj over 16 x 16 sub-tiles (ti, tj <=
// ti) of the lower triangle, dealt to the four wavefronts in turn; the k loop starts at the sub-tile's first row, and the masks
// k >= i, k >= j are the two tril()s: the stored strict upper triangle of q_sqrt may hold anything.
// ADAPT (gp_pdgpb_natgrad_adaptive): the length is the GP's own, ad.gamma[g], and a recorded non-positive pivot
// with halvings left forms B again at half the length (there is no room for a second copy at M = 128; Phi is recomputed from
// params / grad, which this kernel does not write).  The branch is uniform over the workgroup.  The accepted length and j go to
// ad.len / ad.j; the refusal word is raised only when the last length fails.
struct PbNgAdapt {
  const double* gamma;   // per latent GP of the plan: gamma_r
  double* len;           // the length its B was accepted at (the last tried, if none was)
  int32_t* j;            // its halvings of this iteration
  int64_t* halv;         // the call's counters: sum of j over the iterations of steps taken,
  double* shortest;      //   and the smallest length taken
  int halvings;
};
struct PbNgNone {};
template <bool ADAPT, typename AD>
__device__ __forceinline__ void pb_ng_form_body(const PbGp* __restrict__ gps, const PbNgGp* __restrict__ list,
                                                const double* __restrict__ params, const double* __restrict__ grad,
                                                double gamma, double* __restrict__ blocks, int32_t* __restrict__ refused,
                                                int maxM, const AD& ad) {
  extern __shared__ double pb_sm[];
  __shared__ int bad_pivot;
  const PbNgGp e = list[blockIdx.x];
  const PbGp g = gps[e.g];
  const int M = g.M, tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double* Bs = pb_sm;
  double* tmp = Bs + (int64_t)maxM * maxM;
  const double* __restrict__ Lq = params + g.off_qsq;
  const double* __restrict__ GL = grad + g.off_qsq;
  double* __restrict__ Cinv = blocks + e.ws;
  if (tid == 0) bad_pivot = -1;
  const int kq = lane >> 4, lc = lane & 15, T = (M + 15) >> 4;
  double gamma0 = gamma;
  if constexpr (ADAPT) gamma0 = ad.gamma[e.g];
  for (int jh = 0;; jh++) {
    if constexpr (ADAPT) gamma = scalbn(gamma0, -jh);       // an exact scaling; jh = 0 is gamma_r itself
    int s = 0;
    for (int ti = 0; ti < T; ti++)
      for (int tj = 0; tj <= ti; tj++, s++) {
        if ((s & 3) != wave) continue;                         // wave-uniform
        const int i0 = 16 * ti, j0 = 16 * tj;
        const int ia = i0 + lc, jb = j0 + lc;
        pb_d4 acc = {0.0, 0.0, 0.0, 0.0};
        for (int kk = i0; kk < M; kk += 4) {
          const int k = kk + kq;
          const bool kin = k < M;
          const double av = (kin && ia < M && k >= ia) ? Lq[(int64_t)k * M + ia] : 0.0;    // A(i, k) = Lq(k, i)
          const double bv = (kin && jb < M && k >= jb) ? GL[(int64_t)k * M + jb] : 0.0;    // B(k, j) = G_L(k, j)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int i = i0 + kq + 4 * q, j = j0 + lc;
          if (i < M && j <= i) {
            const double v = (i == j ? 1.0 : 0.0) - gamma * acc[q];
            const int ri = M - 1 - i, rj = M - 1 - j;          // rj >= ri: (rj, ri) is in the lower triangle of the reversed matrix
            Bs[rj * M + ri] = v;
            Bs[ri * M + rj] = v;
          }
        }
      }
    // w_i = sum_{k >= i} Lq_ki g_k: thread i, k ascending
    if (jh == 0 && tid < M) {
      const double* __restrict__ gq = grad + g.off_qmu;
      double a = 0.0;
      for (int k = tid; k < M; k++) a = fma(Lq[(int64_t)k * M + tid], gq[k], a);
      Cinv[(int64_t)M * M + tid] = a;
    }
    __syncthreads();
    // the pivot replaced by 1 keeps every loop's trip count and the pass finite whatever the gradient held (a model whose Kuu
    // failed in this evaluation hands over garbage; its Kuu word, raised by the forward launch, is what the host reports)
    pb_chol_invert<false, !ADAPT>(M, Bs, tmp, bad_pivot, &refused[g.model], g.row, nullptr);
    if constexpr (!ADAPT) break;
    else {
      const int bp = bad_pivot;                                // (pb_chol_invert ends behind a barrier)
      __syncthreads();
      if (bp < 0 || jh == ad.halvings) {
        if (tid == 0) {
          if (bp >= 0) atomicMax(&refused[g.model], 0x7fffffff - (PB_MAX_M * g.row + bp));
          ad.len[e.g] = gamma;
          ad.j[e.g] = jh;
        }
        break;
      }
      if (tid == 0) bad_pivot = -1;
      __syncthreads();
    }
  }
  for (int i = tid; i < M * M; i += PB_THREADS) Cinv[i] = Bs[i];
}
__global__ void __launch_bounds__(PB_THREADS) pdgpb_ng_form_kernel(const PbGp* __restrict__ gps, const PbNgGp* __restrict__ list,
                                                                   const double* __restrict__ params, const double* __restrict__ grad,
                                                                   double gamma, double* __restrict__ blocks,
                                                                   int32_t* __restrict__ refused, int maxM) {
  pb_ng_form_body<false>(gps, list, params, grad, gamma, blocks, refused, maxM, PbNgNone{});
}
__global__ void __launch_bounds__(PB_THREADS) pdgpb_ng_form_adaptive_kernel(const PbGp* __restrict__ gps,
                                                                            const PbNgGp* __restrict__ list,
                                                                            const double* __restrict__ params,
                                                                            const double* __restrict__ grad, const PbNgAdapt ad,
                                                                            double* __restrict__ blocks,
                                                                            int32_t* __restrict__ refused, int maxM) {
  pb_ng_form_body<true>(gps, list, params, grad, 0.0, blocks, refused, maxM, ad);
}

// Lq' = Lq V, V = U^-T (V_kj = Cinv(M-1-j, M-1-k), lower);  q_mu' = q_mu + gamma Lq' t, t = V^T w.  Row i of Lq' needs row i of
// Lq and nothing else of it, so the update runs in place: column tiles ascend, tile tj reads Lq(i, k) for k >= 32 tj only and
// overwrites columns [32 tj, 32 tj + 32) after a barrier, so no wavefront reads what another has replaced.
// LDS: [t (maxM, padded to even) | 32 x 33 row shares]
template <bool ADAPT, typename AD>
__device__ __forceinline__ void pb_ng_apply_body(const PbGp* __restrict__ gps, const PbNgGp* __restrict__ list,
                                                 double* __restrict__ params, double* __restrict__ fs, double* __restrict__ grad,
                                                 double gamma, const double* __restrict__ blocks,
                                                 const int32_t* __restrict__ status, const int32_t* __restrict__ refused,
                                                 const AD& ad) {
  extern __shared__ double pb_sm[];
  const PbNgGp e = list[blockIdx.x];
  const PbGp g = gps[e.g];
  const int M = g.M, ti = blockIdx.y, row0 = ti * PB_NG_TILE;
  if (row0 >= M || status[g.model] != 0 || refused[g.model] != 0) return;       // (uniform over the workgroup)
  if constexpr (ADAPT) {
    // the length this GP's B was accepted at; the call's counters, once per GP and step taken
    gamma = ad.len[e.g];
    if (ti == 0 && threadIdx.x == 0) {
      ad.halv[e.g] += ad.j[e.g];
      ad.shortest[e.g] = fmin(ad.shortest[e.g], gamma);
    }
  }
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int iend = min(M, row0 + PB_NG_TILE);
  double* __restrict__ Lq = params + g.off_qsq;
  const double* __restrict__ Cinv = blocks + e.ws;
  const double* __restrict__ w = Cinv + (int64_t)M * M;
  double* tv = pb_sm;                                    // t_j, j < iend
  double (*red)[PB_NG_TILE + 1] = reinterpret_cast<double (*)[PB_NG_TILE + 1]>(pb_sm + ((M + 1) & ~1));

  // t_j = sum_{k >= j} V_kj w_k = sum_{c = 0}^{M-1-j} Cinv(M-1-j, c) w_{M-1-c}: a wavefront per j, lanes over c, one butterfly
  for (int j = wave; j < iend; j += PB_THREADS / 64) {
    const int R = M - 1 - j;
    const double* __restrict__ row = Cinv + (int64_t)R * M;
    double s = 0.0;
    for (int c = lane; c <= R; c += 64) s = fma(row[c], w[M - 1 - c], s);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) tv[j] = s;
  }
  __syncthreads();

  const int kq = lane >> 4, lc = lane & 15;
  const int rh = wave >> 1, ch = wave & 1;
  const int i0 = row0 + rh * 16;
  const int ia = i0 + lc;
  double rs[4] = {0.0, 0.0, 0.0, 0.0};                   // this lane's share of (Lq' t) for rows i0 + kq + 4 q
  for (int tj = 0; tj <= ti; tj++) {
    const int j0 = tj * PB_NG_TILE + ch * 16;
    const bool live = (j0 <= i0) && (i0 < M);            // wave-uniform
    pb_d4 acc = {0.0, 0.0, 0.0, 0.0};
    if (live) {
      const int jb = j0 + lc;
      const int kend = min(M, i0 + 16);
      const double* __restrict__ crow = Cinv + (int64_t)(M - 1 - min(jb, M - 1)) * M;
      for (int kk = j0; kk < kend; kk += 4) {
        const int k = kk + kq;
        const bool kin = k < M;
        const double av = (kin && ia < M && k <= ia) ? Lq[(int64_t)ia * M + k] : 0.0;   // A(i, k) = Lq(i, k)
        const double bv = (kin && jb < M && k >= jb) ? crow[M - 1 - k] : 0.0;           // B(k, j) = V(k, j)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
      }
    }
    __syncthreads();                                     // every wavefront has read this tile's operands
    if (live) {
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int i = i0 + kq + 4 * q, j = j0 + lc;
        if (i < M && j <= i) {
          Lq[(int64_t)i * M + j] = acc[q];
          fs[g.off_qsq + (int64_t)i * M + j] = acc[q];
          rs[q] = fma(acc[q], tv[j], rs[q]);
        }
      }
    }
  }
  // (Lq' t)_i: the 32 column shares of a row, added in column order
#pragma unroll
  for (int q = 0; q < 4; q++) red[rh * 16 + kq + 4 * q][ch * 16 + lc] = rs[q];
  __syncthreads();
  if (tid < PB_NG_TILE) {
    const int i = row0 + tid;
    if (i < M) {
      double sum = red[tid][0];
      for (int c = 1; c < PB_NG_TILE; c++) sum += red[tid][c];
      const double v = params[g.off_qmu + i] + gamma * sum;
      params[g.off_qmu + i] = v;
      fs[g.off_qmu + i] = v;
      grad[g.off_qmu + i] = 0.0;
    }
  }
  // this step has used the gradient of these rows: what the Adam kernel sees of them is zero
  double* __restrict__ GLrows = grad + g.off_qsq + (int64_t)row0 * M;
  const int cnt = (iend - row0) * M;
  for (int idx = tid; idx < cnt; idx += PB_THREADS) GLrows[idx] = 0.0;
}
__global__ void __launch_bounds__(PB_THREADS) pdgpb_ng_apply_kernel(const PbGp* __restrict__ gps, const PbNgGp* __restrict__ list,
                                                                    double* __restrict__ params, double* __restrict__ fs,
                                                                    double* __restrict__ grad, double gamma,
                                                                    const double* __restrict__ blocks,
                                                                    const int32_t* __restrict__ status,
                                                                    const int32_t* __restrict__ refused) {
  pb_ng_apply_body<false>(gps, list, params, fs, grad, gamma, blocks, status, refused, PbNgNone{});
}
__global__ void __launch_bounds__(PB_THREADS) pdgpb_ng_apply_adaptive_kernel(const PbGp* __restrict__ gps,
                                                                             const PbNgGp* __restrict__ list,
                                                                             double* __restrict__ params, double* __restrict__ fs,
                                                                             double* __restrict__ grad, const PbNgAdapt ad,
                                                                             const double* __restrict__ blocks,
                                                                             const int32_t* __restrict__ status,
                                                                             const int32_t* __restrict__ refused) {
  pb_ng_apply_body<true>(gps, list, params, fs, grad, 0.0, blocks, status, refused, ad);
}

// ---------------------------------------------------------------------------------------------------------------
// prediction: Pdgp.predict_act_n_com (pdgp.py:190-208; GPflow conditional, whiten=True, full_cov=False) of every model at
// its own inputs.  Two launches and the source means:
//   pdgpb_pred_prep_kernel    one workgroup per latent GP: Kuu + jitter I factored and inverted in LDS (pb_factor_invert),
//                             then G = [W ; tril(Lq)^T W] (W = L^-1) to the workspace: 2 Mp x Mp stored transposed,
//                             Mp = M rounded up to 16, zero rows and columns beyond M
//   pdgpb_pred_kernel         one workgroup per (latent GP, tile of PB_PT frames), GP-major: the Kuf tile in LDS,
//                             [A ; Lq^T A] = G Kuf_tile on v_mfma_f64_16x16x4_f64, per frame fmean = A^T q_mu and
//                             fvar = Kdiag - sum A^2 + sum (Lq^T A)^2 (GPflow's expression: A's entries are bounded by
//                             sqrt(Kdiag), so nothing of size |W|^2 ~ 1 / jitter is formed or cancelled)
//   pdgpb_pred_source_kernel  mean_source = nlin(fmean_act) * fmean_com (lik.hip mean_source_kernel, per model)
// Every sum is one lane's sequential loop or a fixed butterfly: two calls give bit-identical results, and a model's results
// do not depend on the other models of the call nor on how its frames are split between calls.
#define PB_PT 64      // frames per (latent GP, frame tile) entry: four column groups of 16
#define PB_PRED_THREADS 512

typedef double pb_d2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline int pb_pad16(int M) { return (M + 15) & ~15; }
__host__ __device__ inline int64_t pb_pred_g_doubles(int M) { return 2 * (int64_t)pb_pad16(M) * pb_pad16(M); }

__global__ void __launch_bounds__(PB_THREADS) pdgpb_pred_prep_kernel(const PbGp* __restrict__ gps, const double* __restrict__ params,
                                                                     double* __restrict__ g_all, int32_t* __restrict__ status,
                                                                     double jitter, int maxM) {
  extern __shared__ double pb_sm[];
  const PbGp g = gps[blockIdx.x];
  const int M = g.M, Mp = pb_pad16(M), tid = threadIdx.x;
  double* Ls = pb_sm;
  double* zs = Ls + (int64_t)maxM * maxM;
  double* tmp = zs + maxM;
  __shared__ int bad_pivot;
  const double* th = params + g.off_theta;
  const double* z = params + g.off_z;
  const double* qsq = params + g.off_qsq;
  for (int i = tid; i < M; i += PB_THREADS) zs[i] = z[i];
  if (tid == 0) bad_pivot = -1;
  __syncthreads();
  pb_factor_invert<false>(g.type, g.m, th, zs, M, jitter, Ls, tmp, bad_pivot, status, g.model, g.row, nullptr);
  // G[r][k]: r < M: W[r][k];  r = Mp + i, i < M: (tril(Lq)^T W)[i][k] = sum_{j >= max(i, k)} Lq[j][i] W[j][k] in ascending j
  // (the strict upper triangle of q_sqrt is masked away, matrix_band_part in GPflow's conditional).  Stored transposed,
  // GT[k][r] (ld 2 Mp): the 16 rows of an MFMA fragment are 128 contiguous bytes
  double* Gt = g_all + g.ws;
  for (int e = tid; e < 2 * Mp * Mp; e += PB_THREADS) {
    const int k = e / (2 * Mp), r = e % (2 * Mp);
    double v = 0.0;
    if (k < M) {
      if (r < M) {
        v = Ls[r * M + k];
      } else if (r >= Mp && r - Mp < M) {
        const int i = r - Mp;
        for (int j = max(i, k); j < M; j++) v = fma(qsq[(int64_t)j * M + i], Ls[j * M + k], v);
      }
    }
    Gt[e] = v;
  }
}

// the entry's products and per-frame sums.  Wavefront w owns the 16 frames 16 (w & 3) .. + 15 of the tile and one half of
// G's row tiles: h = w >> 2 = 0 the NB tiles of W (A = W Kuf: fm = A^T q_mu, sa = sum A^2), h = 1 those of tril(Lq)^T W
// (sb = sum (Lq^T A)^2).  v_mfma_f64_16x16x4_f64 operands as gemm_wave.hip: A lane (kq, lc) = G[row lc][k0 + kq], B lane
// (kq, lc) = Kuf[k0 + kq][frame lc]; C/D: acc[a][r] = (G Kuf)[h Mp + 16 a + 4 r + kq][16 (w & 3) + lc].  G^T (L2-resident,
// shared by the GP's tiles) is read straight from memory, four 128-byte rows per load; four wavefronts per SIMD hide its
// latency.
template <int NB>
__device__ __forceinline__ void pb_pred_products(const double* __restrict__ Gt, const double* Ks, const double* qs, int w,
                                                 int lane, double& fm, double& sq) {
  constexpr int Mp = 16 * NB;
  const int lc = lane & 15, kq = lane >> 4, h = w >> 2;
  pb_d4 acc[NB];
#pragma unroll
  for (int a = 0; a < NB; a++) acc[a] = pb_d4{0.0, 0.0, 0.0, 0.0};
  const double* ga = Gt + (int64_t)kq * 2 * Mp + h * Mp + lc;
  const double* kb = Ks + kq * PB_PT + 16 * (w & 3) + lc;
#pragma unroll 2
  for (int k0 = 0; k0 < Mp; k0 += 4) {
    double af[NB];
#pragma unroll
    for (int a = 0; a < NB; a++) af[a] = ga[(int64_t)k0 * 2 * Mp + 16 * a];
    const double bf = kb[k0 * PB_PT];
#pragma unroll
    for (int a = 0; a < NB; a++) acc[a] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[a], bf, acc[a], 0, 0, 0);
  }
  fm = 0.0; sq = 0.0;
#pragma unroll
  for (int a = 0; a < NB; a++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const double v = acc[a][r];
      if (h == 0) fm = fma(v, qs[16 * a + 4 * r + kq], fm);
      sq = fma(v, v, sq);
    }
}

// the latent GP of entry b: the last g with tile_start[g] <= b (tile_start ascending, G + 1 entries)
__device__ __forceinline__ int pb_entry_gp(const int64_t* __restrict__ tile_start, int G, int64_t b) {
  return gp_entry_owner(tile_start, G, b);
}

// LDS: [maxMp x PB_PT Kuf tile | PB_PT frames | maxMp z | maxMp q_mu]; eight wavefronts, two workgroups per CU
__global__ void __launch_bounds__(PB_PRED_THREADS) __attribute__((amdgpu_waves_per_eu(4))) pdgpb_pred_kernel(const PbGp* __restrict__ gps, const PbPredGp* __restrict__ pgs,
                                                                        const int64_t* __restrict__ tile_start, int G,
                                                                        const double* __restrict__ params, const double* __restrict__ g_all,
                                                                        const double* __restrict__ xnew, double* __restrict__ fmean,
                                                                        double* __restrict__ fvar, int maxMp) {
  extern __shared__ double pb_sm[];
  __shared__ double sb_tile[PB_PT];
  const int64_t b = blockIdx.x;
  const int gi = pb_entry_gp(tile_start, G, b);
  const PbGp g = gps[gi];
  const PbPredGp pg = pgs[gi];
  const int M = g.M, Mp = pb_pad16(M), tid = threadIdx.x;
  const int64_t t0 = (b - tile_start[gi]) * PB_PT;
  const int nv = (int)min((int64_t)PB_PT, pg.n - t0);        // frames of this tile (ragged tail: masked)
  double* Ks = pb_sm;
  double* xs = Ks + (int64_t)maxMp * PB_PT;
  double* zs = xs + PB_PT;
  double* qs = zs + maxMp;
  const double* th = params + g.off_theta;
  const double* z = params + g.off_z;
  const double* qmu = params + g.off_qmu;
  for (int c = tid; c < PB_PT; c += PB_PRED_THREADS) xs[c] = c < nv ? xnew[pg.x_off + t0 + c] : 0.0;
  for (int i = tid; i < Mp; i += PB_PRED_THREADS) {
    zs[i] = i < M ? z[i] : 0.0;
    qs[i] = i < M ? qmu[i] : 0.0;
  }
  __syncthreads();
  // Kuf tile (Mp x PB_PT, row-major): zero rows beyond M and columns beyond the model's frames
  for (int e = tid; e < Mp * PB_PT; e += PB_PRED_THREADS) {
    const int i = e / PB_PT, c = e % PB_PT;
    Ks[e] = (i < M && c < nv) ? pb_kern(g.type, g.m, th, zs[i], xs[c]) : 0.0;
  }
  __syncthreads();
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
  const double* Gt = g_all + g.ws;
  double fm = 0.0, sq = 0.0;
  switch (Mp >> 4) {
    case 1: pb_pred_products<1>(Gt, Ks, qs, w, lane, fm, sq); break;
    case 2: pb_pred_products<2>(Gt, Ks, qs, w, lane, fm, sq); break;
    case 3: pb_pred_products<3>(Gt, Ks, qs, w, lane, fm, sq); break;
    case 4: pb_pred_products<4>(Gt, Ks, qs, w, lane, fm, sq); break;
    case 5: pb_pred_products<5>(Gt, Ks, qs, w, lane, fm, sq); break;
    case 6: pb_pred_products<6>(Gt, Ks, qs, w, lane, fm, sq); break;
    case 7: pb_pred_products<7>(Gt, Ks, qs, w, lane, fm, sq); break;
    default: pb_pred_products<8>(Gt, Ks, qs, w, lane, fm, sq); break;
  }
  // the four lanes of a frame (kq = 0..3) combined by a fixed butterfly: (kq 0 + 1) + (kq 2 + 3) in every lane
  fm += __shfl_xor(fm, 16); fm += __shfl_xor(fm, 32);
  sq += __shfl_xor(sq, 16); sq += __shfl_xor(sq, 32);
  const int c = 16 * (w & 3) + (lane & 15);
  if (w >= 4 && lane < 16) sb_tile[c] = sq;
  __syncthreads();
  if (w < 4 && lane < 16 && c < nv) {
    fmean[pg.out_off + t0 + c] = fm;
    fvar[pg.out_off + t0 + c] = (pb_kdiag(g.type, g.m, th) - sq) + sb_tile[c];
  }
}

// mean_source over the same entries: the activation rows' entries form nlin(g_i) f_i for their frames, the others return
__global__ void __launch_bounds__(PB_PT) pdgpb_pred_source_kernel(const PbGp* __restrict__ gps, const PbPredGp* __restrict__ pgs,
                                                                  const int64_t* __restrict__ tile_start, int G,
                                                                  const double* __restrict__ fmean, double* __restrict__ src) {
  const int64_t b = blockIdx.x;
  const int gi = pb_entry_gp(tile_start, G, b);
  const PbPredGp pg = pgs[gi];
  if (gps[gi].row >= pg.P) return;
  const int64_t n = (b - tile_start[gi]) * PB_PT + threadIdx.x;
  if (n >= pg.n) return;
  double s, ds;
  nlin_eval(pg.nlin, fmean[pg.out_off + n], s, ds);
  src[pg.src_off + n] = s * fmean[pg.out_off + (int64_t)pg.P * pg.n + n];
}

// the moments of gp_mpd_predict_moments over the same entries, from the fmean / fvar pdgpb_pred_kernel left in the workspace:
// the entries of a model's row 0 take the model's frame tile (every source of its PB_PT frames), the others return.  Sixteen
// lanes per frame as lik.hip's mpd_moments_kernel (mpd_moments_frame, gh_quad.h): PB_MOM_FRAMES frames per pass, PB_PT /
// PB_MOM_FRAMES passes.  LDS: [PB_MOM_FRAMES][4][maxP].  A frame's results come from its own model's rows only.
#define PB_MOM_THREADS 256
#define PB_MOM_FRAMES (PB_MOM_THREADS / MOM_LANES)
__global__ void __launch_bounds__(PB_MOM_THREADS) pdgpb_pred_moments_kernel(const PbGp* __restrict__ gps, const PbPredGp* __restrict__ pgs,
                                                                            const int64_t* __restrict__ tile_start, int G,
                                                                            const double* __restrict__ params,
                                                                            const double* __restrict__ fmean, const double* __restrict__ fvar,
                                                                            const double* __restrict__ ynew, double* __restrict__ smean,
                                                                            double* __restrict__ svar, double* __restrict__ ymean,
                                                                            double* __restrict__ yvar, double* __restrict__ logp, int maxP) {
  extern __shared__ double pb_sm[];
  const int64_t b = blockIdx.x;
  const int gi = pb_entry_gp(tile_start, G, b);
  const PbGp g = gps[gi];
  if (g.row != 0) return;
  const PbPredGp pg = pgs[gi];
  const int P = pg.P, fl = threadIdx.x / MOM_LANES, l = threadIdx.x % MOM_LANES;
  const int64_t t0 = (b - tile_start[gi]) * PB_PT;
  const double* noise = params + (g.off_theta - 1);      // the model's noise variance sits right before its first GP
  const double* Fm = fmean + pg.out_off;                 // row 0 of the model: its 2P rows of pg.n frames follow
  const double* Fv = fvar + pg.out_off;
  double* sm = pb_sm + (size_t)fl * 4 * maxP;
  for (int c0 = 0; c0 < PB_PT; c0 += PB_MOM_FRAMES) {
    const int64_t n = t0 + c0 + fl;
    const bool live = n < pg.n;
    const int64_t f = pg.x_off + n;                      // the frame's slot in xnew / ynew / ymean / yvar / logp
    mpd_moments_frame(Fm, Fv, pg.n, n, live, l, P, pg.nlin, noise, true, ynew ? ynew + f : nullptr,
                      smean ? smean + pg.src_off : nullptr, svar ? svar + pg.src_off : nullptr, pg.n, n,
                      ymean ? ymean + f : nullptr, yvar ? yvar + f : nullptr, logp ? logp + f : nullptr, sm);
    __syncthreads();                                     // lane 0 has read the frame's LDS before the next pass writes it
  }
}

// ---------------------------------------------------------------------------------------------------------------
// joint posterior draws of many models (gp_pdgpb_sample): the state-space core of sample.hip over every latent GP of every
// model with frames (a process each, with its own frame count), and between its prior walk and its update the inducing
// side of all of them in ONE launch, from the G^T blocks pdgpb_pred_prep_kernel left:
//   u0 = prior(z) + sqrt(jitter) eps_u[0];  rhs = q_mu + tril(q_sqrt) eps_u[1] - W u0;  beta = W^T rhs      (whitened)
// One record per sampled latent GP, in process order.
struct PbSmpGp {
  const double* Gt;                       // the GP's prepared block: W[i][k] = Gt[k 2 Mp + i]
  const double* eps_u;                    // [S][2][M]
  const double* q_mu; const double* q_sqrt;
  const double* pz;                       // prior(z): [M][S]
  double* beta;                           // [M][S]
  const double* lat_g; const double* lat_f;   // activation rows: the draws of g_i and of f_i, [S][n] each
  double* src;                            // activation rows when sources are wanted: nlin(g_i) f_i, [S][n]; else null
  int64_t n;
  int M, nlin;
};
#define PB_SMP_DRAWS 16                   // draws per workgroup of the inducing kernel
__host__ __device__ inline int64_t pb_smp_tri(int M) { return (int64_t)M * (M + 1) / 2; }
static size_t pb_smp_lds(int maxM) { return (size_t)(pb_smp_tri(maxM) + 2 * (int64_t)maxM * PB_SMP_DRAWS) * sizeof(double); }

// One workgroup per (latent GP, block of PB_SMP_DRAWS draws).  LDS: the lower triangle of W packed by rows (W[i][k] at
// i (i + 1) / 2 + k: 66 KiB at M = 128, and rows i .. i + 3, which a wavefront reads together, start i + 1, i + 2, .. doubles
// apart, on different banks) | u0 [M][16] | eps_u[1], then rhs [M][16].  A thread owns draw tid % 16 and the rows
// tid / 16 + 16 p: the 16 lanes of a row read one W entry (a broadcast) and 16 consecutive doubles of u0 / rhs.  Every sum is one
// thread's loop in ascending index, so a draw depends on its own eps alone: not on S, not on its block, not on the launch.
__global__ void __launch_bounds__(PB_THREADS) pdgpb_sample_inducing_kernel(const PbSmpGp* __restrict__ recs, int S, double sqrt_jitter,
                                                                           int maxM) {
  extern __shared__ double pb_sm[];
  const PbSmpGp g = recs[blockIdx.x];
  const int M = g.M, Mp = pb_pad16(M), tid = threadIdx.x;
  constexpr int DB = PB_SMP_DRAWS;
  double* Wl = pb_sm;
  double* u0 = Wl + pb_smp_tri(maxM);
  double* rh = u0 + (int64_t)maxM * DB;
  const int s0 = blockIdx.y * DB;
  for (int e = tid; e < M * Mp; e += PB_THREADS) {
    const int k = e / Mp, i = e % Mp;
    if (i < M && i >= k) Wl[pb_smp_tri(i) + k] = g.Gt[(int64_t)k * 2 * Mp + i];
  }
  for (int e = tid; e < M * DB; e += PB_THREADS) {
    const int i = e / DB, s = s0 + e % DB;
    double u = 0.0, e1 = 0.0;
    if (s < S) {
      const double* __restrict__ eu = g.eps_u + (int64_t)s * 2 * M;
      u = g.pz[(int64_t)i * S + s] + sqrt_jitter * eu[i];
      e1 = eu[M + i];
    }
    u0[e] = u;
    rh[e] = e1;
  }
  __syncthreads();
  const int sl = tid % DB, row = tid / DB;
  double tv[PB_MAX_M / (PB_THREADS / DB)];
#pragma unroll
  for (int p = 0; p < PB_MAX_M / (PB_THREADS / DB); p++) {
    const int i = row + (PB_THREADS / DB) * p;
    tv[p] = 0.0;
    if (i < M) {
      const double* __restrict__ lq = g.q_sqrt + (int64_t)i * M;   // row i of q_sqrt: the columns j <= i are tril(q_sqrt)'s
      const double* wr = Wl + pb_smp_tri(i);
      double r = g.q_mu[i], a = 0.0;
      for (int j = 0; j <= i; j++) r = fma(lq[j], rh[j * DB + sl], r);
      for (int k = 0; k <= i; k++) a = fma(wr[k], u0[k * DB + sl], a);
      tv[p] = r - a;
    }
  }
  __syncthreads();                                                 // eps_u[1] has been read: rhs takes its place
#pragma unroll
  for (int p = 0; p < PB_MAX_M / (PB_THREADS / DB); p++) {
    const int i = row + (PB_THREADS / DB) * p;
    if (i < M) rh[i * DB + sl] = tv[p];
  }
  __syncthreads();
  const int s = s0 + sl;
  for (int k = row; k < M; k += PB_THREADS / DB) {
    double a = 0.0;
    for (int i = k; i < M; i++) a = fma(Wl[pb_smp_tri(i) + k], rh[i * DB + sl], a);
    if (s < S) g.beta[(int64_t)k * S + s] = a;
  }
}

// src = nlin_k(g) f over the update's (process, frame tile) entries: the activation rows' entries take their frames of every
// draw (grid y strides the draws), the others return.  One thread per frame of the update's tile: the entries are laid out by
// ssm_fill_tiles at the plan's largest M, and every M the batch takes has the 64-frame tile
#define PB_SMP_TILE 64
static_assert(sps_tile_frames(PB_MAX_M) == PB_SMP_TILE && sps_tile_frames(1) == PB_SMP_TILE,
              "pdgpb_sample_source_kernel walks the update's (process, frame tile) entries with one thread per frame");
__global__ void __launch_bounds__(PB_SMP_TILE) pdgpb_sample_source_kernel(const PbSmpGp* __restrict__ recs, const int64_t* __restrict__ tile_start,
                                                                 int count, int S) {
  const int64_t b = blockIdx.x;
  const int gi = gp_entry_owner(tile_start, count, b);
  const PbSmpGp g = recs[gi];
  if (!g.src) return;
  const int64_t t = (b - tile_start[gi]) * blockDim.x + threadIdx.x;
  if (t >= g.n) return;
  for (int s = blockIdx.y; s < S; s += gridDim.y) {
    const int64_t o = (int64_t)s * g.n + t;
    double sg, ds;
    nlin_eval(g.nlin, g.lat_g[o], sg, ds);
    g.src[o] = sg * g.lat_f[o];
  }
}

// ---------------------------------------------------------------------------------------------------------------
static size_t pb_fwd_lds(const gp_pdgpb_plan_s* p) {
  return ((size_t)p->maxM * p->maxM + p->maxB + 2 * (size_t)p->maxM + PB_TILE_DOUBLES) * sizeof(double);
}
static int pb_maxth(const gp_pdgpb_plan_s* p) { return GP_THETA_LEN(p->maxm); }
static size_t pb_bwd_lds(const gp_pdgpb_plan_s* p) {
  return ((size_t)p->maxB + p->maxM + PB_TILE_DOUBLES + (size_t)p->maxM * pb_maxth(p)) * sizeof(double);
}
static size_t pb_prep_lds(const gp_pdgpb_plan_s* p) { return ((size_t)p->maxM * p->maxM + 2 * (size_t)p->maxM) * sizeof(double); }
static size_t pb_pred_lds(const gp_pdgpb_plan_s* p) {
  const size_t mp = pb_pad16(p->maxM);
  return (mp * PB_PT + PB_PT + 2 * mp) * sizeof(double);
}

static gp_status pb_eval(gp_pdgpb_plan_s* p, const double* params, const double* x, const double* y, const int32_t* idx,
                         double* elbo, double* grad) {
  gp_handle h = p->h;
  hipLaunchKernelGGL(pdgpb_fwd_kernel, dim3(p->G), dim3(PB_THREADS), pb_fwd_lds(p), h->stream, p->d_gps, params, x, idx,
                     p->d_scr, p->d_fm, p->d_fv, p->d_kl, p->d_status, p->jitter, p->maxM, p->maxB);
  GP_HIP_CHECK(h, hipGetLastError());
  hipLaunchKernelGGL(pdgpb_lik_kernel, dim3(p->nm), dim3(PB_THREADS), 0, h->stream, p->d_models, params, y, idx, p->d_fm,
                     p->d_fv, p->d_kl, p->d_gm, p->d_gv, grad, elbo);
  GP_HIP_CHECK(h, hipGetLastError());
  if (!grad) return GP_OK;
  hipLaunchKernelGGL(pdgpb_bwd_kernel, dim3(p->G), dim3(PB_THREADS), pb_bwd_lds(p), h->stream, p->d_gps, params, x, idx,
                     p->d_scr, p->d_gm, p->d_gv, grad, p->maxM, p->maxB, pb_maxth(p));
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}

extern "C" {

gp_status gp_pdgpb_create(gp_handle h, const gp_pdgpb_config* cfg, gp_pdgpb_plan* out) {
  if (!h || !out) return GP_ERR_BAD_ARG;
  *out = nullptr;
  const bool pred = cfg && !cfg->batch;          // a prediction-only plan
  if (!cfg || cfg->num_models < 1 || !cfg->num_sources || !cfg->nlin || (!pred && !cfg->num_data) || !cfg->M ||
      !cfg->kern_type || !cfg->partials)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_create: bad config");
  gp_pdgpb_plan_s* p = new gp_pdgpb_plan_s();
  p->h = h; p->nm = cfg->num_models; p->jitter = cfg->jitter; p->predict_only = pred;
  int64_t off = 0, f = 0, scr = 0, bo = 0;
  int g = 0;
  for (int k = 0; k < p->nm; k++) {
    const int P = cfg->num_sources[k], B = pred ? 0 : cfg->batch[k], nl = cfg->nlin[k];
    if (P < 1 || nl < 0 || nl > 2 || (!pred && (B < 1 || B > PB_MAX_B || !(cfg->num_data[k] >= B)))) {
      delete p;
      return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgpb_create: a model's minibatch is outside 1..1024 frames or its "
                                            "sources / nonlinearity are invalid (train it with gp_pdgp_*)");
    }
    PbModel md{P, B, nl, g, off, off, 0, f, bo, pred ? 0.0 : cfg->num_data[k]};
    if (!pred) p->owner.push_back(k);     // the Adam kernel's parameter -> model map (training only)
    off += 1;
    for (int r = 0; r < 2 * P; r++, g++) {
      const int M = cfg->M[g], t = cfg->kern_type[g], m = cfg->partials[g];
      const bool sm = (t == GP_KERN_MERCER_MATERN12SM || t == GP_KERN_MATERN32SM);
      const bool ok_t = sm || t == GP_KERN_MATERN12 || t == GP_KERN_MATERN32 || t == GP_KERN_MATERN52 || t == GP_KERN_RBF;
      if (M < 1 || M > PB_MAX_M || !ok_t || (sm && (m < 1 || m > PB_MAX_PARTIALS)) || (!sm && m != 0)) {
        delete p;
        return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgpb_create: a latent GP has M > 128 or a kernel type the batch does not "
                                              "take (train it with gp_pdgp_*)");
      }
      PbGp gp;
      gp.model = k; gp.row = r; gp.type = t; gp.m = m; gp.M = M; gp.B = B; gp.need_theta = 1; gp.need_z = 1;
      gp.off_theta = off; off += GP_THETA_LEN(m);
      gp.off_z = off; off += M;
      gp.off_qmu = off; off += M;
      gp.off_qsq = off; off += (int64_t)M * M;
      if (pred) { gp.ws = p->pred_g; p->pred_g += gp_align_up(pb_pred_g_doubles(M), 32); }
      else {
        gp.ws = scr; scr += gp_align_up(pb_gp_scratch(M, B), 32);
        p->ng_off.push_back(p->ng_blocks); p->ng_blocks += gp_align_up((size_t)M * M + M, 32);
      }
      gp.f_off = f + (int64_t)r * B;
      gp.batch_off = bo;
      p->gps.push_back(gp);
      p->maxM = std::max(p->maxM, M);
      p->maxm = std::max(p->maxm, m);
    }
    md.p1 = off;
    if (!pred)
      for (int64_t i = md.p0 + 1; i < off; i++) p->owner.push_back(k);
    f += 2 * (int64_t)P * B;
    bo += B;
    p->maxB = std::max(p->maxB, B);
    p->models.push_back(md);
  }
  p->G = g; p->nparams = off; p->f_len = f; p->scratch = scr; p->sumB = (int)bo;
  if (pred ? pb_prep_lds(p) > 160 * 1024 : (pb_fwd_lds(p) > 160 * 1024 || pb_bwd_lds(p) > 160 * 1024)) {
    delete p;
    return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgpb_create: shapes exceed the workgroup's LDS");
  }
  *out = p;
  return GP_OK;
}

gp_status gp_pdgpb_destroy(gp_pdgpb_plan p) { delete p; return GP_OK; }
int64_t gp_pdgpb_num_params(gp_pdgpb_plan p) { return p ? p->nparams : 0; }

gp_status gp_pdgpb_layout(gp_pdgpb_plan p, int32_t g, int64_t* off_theta, int64_t* off_z, int64_t* off_qmu, int64_t* off_qsqrt) {
  if (!p || g < 0 || g >= p->G || !off_theta || !off_z || !off_qmu || !off_qsqrt) return GP_ERR_BAD_ARG;
  const PbGp& gp = p->gps[g];
  *off_theta = gp.off_theta; *off_z = gp.off_z; *off_qmu = gp.off_qmu; *off_qsqrt = gp.off_qsq;
  return GP_OK;
}

gp_status gp_pdgpb_set_grad_needs(gp_pdgpb_plan p, int32_t g, int32_t need_theta, int32_t need_z) {
  if (!p || g < 0 || g >= p->G) return GP_ERR_BAD_ARG;
  p->gps[g].need_theta = need_theta != 0;
  p->gps[g].need_z = need_z != 0;
  p->ready = false;      // descriptors go up again at the next call
  return GP_OK;
}

// gp_pdgpb_set_workspace's regions of a workspace, in order
struct PbRegions { PbGp* gps; PbModel* models; int32_t* owner; int32_t* status; double *fm, *fv, *gm, *gv, *kl, *grad, *elbo, *scr; };
static PbRegions pb_regions(const gp_pdgpb_plan_s* p, GpArena& ar) {
  PbRegions r;
  r.gps = ar.take<PbGp>(p->gps.size());
  r.models = ar.take<PbModel>(p->models.size());
  r.owner = ar.take<int32_t>(p->nparams);
  r.status = ar.take<int32_t>(p->nm);
  r.fm = ar.take<double>(p->f_len); r.fv = ar.take<double>(p->f_len);
  r.gm = ar.take<double>(p->f_len); r.gv = ar.take<double>(p->f_len);
  r.kl = ar.take<double>(p->G);
  r.grad = ar.take<double>(p->nparams);
  r.elbo = ar.take<double>(p->nm);
  r.scr = ar.take<double>(p->scratch);
  return r;
}

size_t gp_pdgpb_workspace_bytes(gp_pdgpb_plan p) {
  if (!p || p->predict_only) return 0;
  return gp_measure([&](GpArena& ar) { pb_regions(p, ar); }) + GP_WS_TAIL_BATCH;
}

gp_status gp_pdgpb_set_workspace(gp_pdgpb_plan p, void* workspace, size_t bytes) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (p->predict_only) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_set_workspace: a prediction-only plan (its workspace goes to gp_pdgpb_predict_prepare)");
  if (!workspace || bytes < gp_pdgpb_workspace_bytes(p) || (((uintptr_t)workspace) & 255))
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_set_workspace: workspace too small or not 256-byte aligned");
  GpArena ar(workspace, bytes);
  const PbRegions r = pb_regions(p, ar);
  if (!ar.ok) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_set_workspace: arena overflow");
  p->d_gps = r.gps; p->d_models = r.models; p->d_owner = r.owner; p->d_status = r.status;
  p->d_fm = r.fm; p->d_fv = r.fv; p->d_gm = r.gm; p->d_gv = r.gv;
  p->d_kl = r.kl; p->d_grad = r.grad; p->d_elbo = r.elbo; p->d_scr = r.scr;
  GP_HIP_CHECK(h, hipMemcpyAsync(p->d_owner, p->owner.data(), p->owner.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemsetAsync(p->d_status, 0, p->nm * sizeof(int32_t), h->stream));
  GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)pdgpb_fwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pb_fwd_lds(p)));
  GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)pdgpb_bwd_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pb_bwd_lds(p)));
  p->ready = false;
  return GP_OK;
}

static gp_status pb_upload(gp_pdgpb_plan_s* p) {
  if (p->ready) return GP_OK;
  gp_handle h = p->h;
  if (!p->d_gps) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb: no workspace set");
  // synchronous: the host vectors may change (gp_pdgpb_set_grad_needs) while a copy from pageable memory is pending
  GP_HIP_CHECK(h, hipMemcpyAsync(p->d_gps, p->gps.data(), p->gps.size() * sizeof(PbGp), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(p->d_models, p->models.data(), p->models.size() * sizeof(PbModel), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  p->ready = true;
  return GP_OK;
}

// ---- tied parameters -----------------------------------------------------------------------------------
// gp_pdgpb_set_ties' regions of its workspace, in order; a plan of nmodels models has at most nmodels / 2 tied sets
struct PbTieRegions { int32_t* group_start; int64_t* members; int32_t* set_start; int32_t* set_models; int32_t* frozen; };
static PbTieRegions pb_tie_regions(GpArena& ar, size_t ngroups, size_t nmembers, size_t nmodels) {
  PbTieRegions r;
  r.group_start = ar.take<int32_t>(ngroups + 1);
  r.members = ar.take<int64_t>(nmembers);
  r.set_start = ar.take<int32_t>(nmodels / 2 + 1);
  r.set_models = ar.take<int32_t>(nmodels);
  r.frozen = ar.take<int32_t>(nmodels);
  return r;
}

size_t gp_pdgpb_ties_workspace_bytes(int32_t ngroups, int64_t nmembers, int32_t nmodels) {
  if (ngroups <= 0 || nmembers <= 0 || nmodels <= 0) return 0;
  return gp_measure([&](GpArena& ar) { pb_tie_regions(ar, (size_t)ngroups, (size_t)nmembers, (size_t)nmodels); }) + GP_WS_TAIL_BATCH;
}

gp_status gp_pdgpb_set_ties(gp_pdgpb_plan p, int32_t ngroups, const int32_t* group_start, const int64_t* members,
                            void* workspace, size_t bytes) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (p->predict_only || ngroups < 0) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_set_ties: bad argument or a prediction-only plan");
  if (ngroups == 0) {                    // no ties: the step entries launch what they launch without this entry
    p->ties = PbTies{};
    return GP_OK;
  }
  if (!group_start || !members) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_set_ties: null group_start or members");
  if (group_start[0] != 0) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_set_ties: group_start must begin at 0");
  for (int32_t j = 0; j < ngroups; j++)
    if (group_start[j + 1] <= group_start[j])
      return gp_fail(h, GP_ERR_BAD_ARG, ("gp_pdgpb_set_ties: group_start does not ascend at group " + std::to_string(j) +
                                         " (every group lists one member or more)").c_str());
  const int64_t nmem = group_start[ngroups];
  // every member: a slot of the parameter vector, outside every q_mu / q_sqrt block, named once
  std::vector<int64_t> seen(members, members + nmem);
  for (int32_t j = 0; j < ngroups; j++)
    for (int32_t i = group_start[j]; i < group_start[j + 1]; i++) {
      const int64_t o = members[i];
      if (o < 0 || o >= p->nparams)
        return gp_fail(h, GP_ERR_BAD_ARG, ("gp_pdgpb_set_ties: group " + std::to_string(j) + ": offset " + std::to_string(o) +
                                           " is outside the parameter vector (" + std::to_string(p->nparams) + " slots)").c_str());
      // the latent GP whose [theta | z | q_mu | q_sqrt] block holds the slot: the last one that starts at or before it
      auto it = std::upper_bound(p->gps.begin(), p->gps.end(), o, [](int64_t v, const PbGp& g) { return v < g.off_theta; });
      if (it != p->gps.begin() && o >= (it - 1)->off_qmu && o < (it - 1)->off_qsq + (int64_t)(it - 1)->M * (it - 1)->M)
        return gp_fail(h, GP_ERR_BAD_ARG, ("gp_pdgpb_set_ties: group " + std::to_string(j) + ": offset " + std::to_string(o) +
                                           " lies in the q_mu / q_sqrt block of latent GP " + std::to_string((it - 1) - p->gps.begin()) +
                                           " (q(u) is never tied)").c_str());
    }
  std::sort(seen.begin(), seen.end());
  for (int64_t i = 1; i < nmem; i++)
    if (seen[i] == seen[i - 1])
      return gp_fail(h, GP_ERR_BAD_ARG, ("gp_pdgpb_set_ties: offset " + std::to_string(seen[i]) + " is named twice").c_str());
  if (!workspace || bytes < gp_pdgpb_ties_workspace_bytes(ngroups, nmem, p->nm) || (((uintptr_t)workspace) & 255))
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_set_ties: workspace too small (gp_pdgpb_ties_workspace_bytes) or not 256-byte aligned");
  GpArena ar(workspace, bytes);
  const PbTieRegions r = pb_tie_regions(ar, (size_t)ngroups, (size_t)nmem, (size_t)p->nm);
  if (!ar.ok) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_set_ties: arena overflow");
  // the tied sets: connected components of the models under "a group has members in both" (union by the lower index)
  std::vector<int32_t> root(p->nm);
  for (int k = 0; k < p->nm; k++) root[k] = k;
  auto find = [&](int32_t k) { while (root[k] != k) k = root[k] = root[root[k]]; return k; };
  for (int32_t j = 0; j < ngroups; j++) {
    int32_t a = find(p->owner[members[group_start[j]]]);
    for (int32_t i = group_start[j] + 1; i < group_start[j + 1]; i++) {
      const int32_t b = find(p->owner[members[i]]);
      root[std::max(a, b)] = std::min(a, b);
      a = std::min(a, b);
    }
  }
  std::vector<std::vector<int32_t>> comp(p->nm);
  for (int k = 0; k < p->nm; k++) comp[find(k)].push_back(k);       // k ascends: every set's list ascends
  std::vector<int32_t> set_start(1, 0), set_models;
  for (int k = 0; k < p->nm; k++)
    if (comp[k].size() >= 2) {
      set_models.insert(set_models.end(), comp[k].begin(), comp[k].end());
      set_start.push_back((int32_t)set_models.size());
    }
  GP_HIP_CHECK(h, hipMemcpyAsync(r.group_start, group_start, ((size_t)ngroups + 1) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(r.members, members, (size_t)nmem * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(r.set_start, set_start.data(), set_start.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  if (!set_models.empty())
    GP_HIP_CHECK(h, hipMemcpyAsync(r.set_models, set_models.data(), set_models.size() * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemsetAsync(r.frozen, 0, p->nm * sizeof(int32_t), h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));      // pageable host memory: the caller's arrays and the vectors above go away
  p->ties = PbTies{r.group_start, r.members, r.set_start, r.set_models, r.frozen, ngroups, (int32_t)set_start.size() - 1};
  return GP_OK;
}

gp_status gp_pdgpb_ties_frozen(gp_pdgpb_plan p, int32_t* host_words, int32_t clear) {
  if (!p || !host_words) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->ties.frozen) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_ties_frozen: no ties set (gp_pdgpb_set_ties)");
  GP_HIP_CHECK(h, hipMemcpyAsync(host_words, p->ties.frozen, p->nm * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  if (clear) GP_HIP_CHECK(h, hipMemsetAsync(p->ties.frozen, 0, p->nm * sizeof(int32_t), h->stream));
  return GP_OK;
}

// the tie launch of one iteration (none without ties); `refused`: the step's refusal words, null on the Adam-only path
static gp_status pb_tie(gp_pdgpb_plan_s* p, const int32_t* refused) {
  if (p->ties.ngroups == 0) return GP_OK;
  gp_handle h = p->h;
  const int n = p->ties.ngroups + p->ties.nsets;
  hipLaunchKernelGGL(pdgpb_tie_kernel, dim3((n + PB_TIE_GROUPS - 1) / PB_TIE_GROUPS), dim3(PB_TIE_GROUPS), 0, h->stream, p->ties,
                     p->d_grad, (const int32_t*)p->d_status, refused);
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}

gp_status gp_pdgpb_objective(gp_pdgpb_plan p, const double* params, const double* x, const double* y, const int32_t* idx,
                             double* elbo_dev, double* grad) {
  if (!p || !params || !x || !y || !idx || !elbo_dev || p->predict_only)
    return p ? gp_fail(p->h, GP_ERR_BAD_ARG, "gp_pdgpb_objective: bad argument or a prediction-only plan") : GP_ERR_BAD_ARG;
  GP_CHECK(pb_upload(p));
  return pb_eval(p, params, x, y, idx, elbo_dev, grad);
}

gp_status gp_pdgpb_adam(gp_pdgpb_plan p, double* free_state, double* params, const uint8_t* tcode, double* m, double* v,
                        const double* x, const double* y, const int32_t* idx, int32_t steps, const double* lr_t,
                        double beta1, double beta2, double eps) {
  if (!p || !free_state || !params || !tcode || !m || !v || !x || !y || !idx || !lr_t || steps < 0 || p->predict_only)
    return p ? gp_fail(p->h, GP_ERR_BAD_ARG, "gp_pdgpb_adam: bad argument or a prediction-only plan") : GP_ERR_BAD_ARG;
  GP_CHECK(pb_upload(p));
  gp_handle h = p->h;
  const int64_t n = p->nparams;
  const int blocks = (int)std::min<int64_t>(2048, std::max<int64_t>(1, (n + 255) / 256));
  for (int s = 0; s < steps; s++) {
    GP_CHECK(pb_eval(p, params, x, y, idx + (int64_t)s * p->sumB, p->d_elbo, p->d_grad));
    GP_CHECK(pb_tie(p, nullptr));
    hipLaunchKernelGGL(pdgpb_adam_kernel, dim3(blocks), dim3(256), 0, h->stream, free_state, params, p->d_grad, tcode, m, v,
                       p->d_owner, p->d_status, (const int32_t*)nullptr, (const int32_t*)p->ties.frozen,
                       lr_t + (int64_t)s * p->nm, n, beta1, beta2, eps, h->logistic);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  return GP_OK;
}

// gp_pdgpb_natgrad's regions of its own workspace, in order
struct PbNgRegions { int32_t* refused; PbNgGp* list; double* blocks; };
static PbNgRegions pb_ng_regions(const gp_pdgpb_plan_s* p, GpArena& ar) {
  PbNgRegions r;
  r.refused = ar.take<int32_t>(p->nm);
  r.list = ar.take<PbNgGp>(p->gps.size());
  r.blocks = ar.take<double>((size_t)p->ng_blocks);
  return r;
}
static size_t pb_ng_form_lds(const gp_pdgpb_plan_s* p) { return ((size_t)p->maxM * p->maxM + p->maxM) * sizeof(double); }
static size_t pb_ng_apply_lds(const gp_pdgpb_plan_s* p) {
  return ((size_t)((p->maxM + 1) & ~1) + (size_t)PB_NG_TILE * (PB_NG_TILE + 1)) * sizeof(double);
}

size_t gp_pdgpb_natgrad_workspace_bytes(gp_pdgpb_plan p) {
  if (!p || p->predict_only) return 0;
  return gp_measure([&](GpArena& ar) { pb_ng_regions(p, ar); }) + GP_WS_TAIL_BATCH;
}

// the adaptive step's workspace: gp_pdgpb_natgrad's regions, then per latent GP of the plan [gamma_r | accepted length | j |
// counters]
struct PbNgaRegions { PbNgRegions r; double* gamma; double* len; int32_t* j; int64_t* halv; double* shortest; };
static PbNgaRegions pb_nga_regions(const gp_pdgpb_plan_s* p, GpArena& ar) {
  PbNgaRegions a;
  a.r = pb_ng_regions(p, ar);
  const size_t G = p->gps.size();
  a.gamma = ar.take<double>(G);
  a.len = ar.take<double>(G);
  a.j = ar.take<int32_t>(G);
  a.halv = ar.take<int64_t>(G);
  a.shortest = ar.take<double>(G);
  return a;
}
#define PB_NG_SHORT_CLEAR_BYTE 0x7f    // a cleared `shortest` counter: every byte 0x7f, a double far above any gamma; read back as +inf

// gp_pdgpb_natgrad (gamma_gp_host null: one length, `gamma`) and gp_pdgpb_natgrad_adaptive
static gp_status pb_natgrad_run(gp_pdgpb_plan p, const char* name, double* free_state, double* params, const uint8_t* tcode,
                                double* m, double* v, const double* x, const double* y, const int32_t* idx, int32_t steps,
                                const double* lr_t, double beta1, double beta2, double eps, double gamma,
                                const double* gamma_gp_host, int32_t halvings, const int32_t* step_gp_host, void* workspace,
                                size_t workspace_bytes) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  const bool adapt = gamma_gp_host != nullptr;
  const std::string nm(name);
  if (!free_state || !params || !tcode || !m || !v || !x || !y || !idx || !lr_t || !workspace || steps < 0 || p->predict_only)
    return gp_fail(h, GP_ERR_BAD_ARG, (nm + ": bad argument or a prediction-only plan").c_str());
  if (adapt) {
    for (int g = 0; g < p->G; g++)
      if (!(gamma_gp_host[g] > 0.0 && gamma_gp_host[g] <= 1.0))
        return gp_fail(h, GP_ERR_BAD_ARG, (nm + ": every gamma must lie in (0, 1]").c_str());
    if (halvings < 0 || halvings > 10) return gp_fail(h, GP_ERR_BAD_ARG, (nm + ": halvings must lie in 0..10").c_str());
  } else if (!(gamma > 0.0 && gamma <= 1.0)) {
    return gp_fail(h, GP_ERR_BAD_ARG, (nm + ": gamma must lie in (0, 1]").c_str());
  }
  if (((uintptr_t)workspace & 255) != 0) return gp_fail(h, GP_ERR_BAD_ARG, (nm + ": workspace not 256-byte aligned").c_str());
  if (workspace_bytes < (adapt ? gp_pdgpb_natgrad_adaptive_workspace_bytes(p) : gp_pdgpb_natgrad_workspace_bytes(p)))
    return gp_fail(h, GP_ERR_WORKSPACE, (nm + ": workspace too small (" + nm + "_workspace_bytes)").c_str());
  GpArena ar(workspace, workspace_bytes);
  PbNgaRegions a = {};
  if (adapt) a = pb_nga_regions(p, ar); else a.r = pb_ng_regions(p, ar);
  const PbNgRegions r = a.r;
  if (!ar.ok) return gp_fail(h, GP_ERR_WORKSPACE, (nm + ": arena overflow").c_str());
  GP_CHECK(pb_upload(p));
  if (workspace != p->ng_ws) {          // a workspace the plan has not seen: no model is refused yet
    GP_HIP_CHECK(h, hipMemsetAsync(r.refused, 0, p->nm * sizeof(int32_t), h->stream));
    p->ng_ws = workspace;
    p->d_refused = r.refused;
  }
  if (adapt && workspace != p->nga_ws) {   // ... and its counters start cleared
    GP_HIP_CHECK(h, hipMemsetAsync(a.halv, 0, p->gps.size() * sizeof(int64_t), h->stream));
    GP_HIP_CHECK(h, hipMemsetAsync(a.shortest, PB_NG_SHORT_CLEAR_BYTE, p->gps.size() * sizeof(double), h->stream));
    p->nga_ws = workspace;
    p->d_ng_halv = a.halv; p->d_ng_short = a.shortest;
  }
  p->ng_list.clear();
  for (int g = 0; g < p->G; g++)
    if (!step_gp_host || step_gp_host[g]) p->ng_list.push_back(PbNgGp{g, 0, p->ng_off[g]});
  const int nstep = (int)p->ng_list.size();
  if (nstep > 0) {
    if (adapt) GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)pdgpb_ng_form_adaptive_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pb_ng_form_lds(p)));
    else GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)pdgpb_ng_form_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pb_ng_form_lds(p)));
    GP_HIP_CHECK(h, hipMemcpyAsync(r.list, p->ng_list.data(), nstep * sizeof(PbNgGp), hipMemcpyHostToDevice, h->stream));
    if (adapt)
      GP_HIP_CHECK(h, hipMemcpyAsync(a.gamma, gamma_gp_host, p->G * sizeof(double), hipMemcpyHostToDevice, h->stream));
    // pageable host memory: the list may be rebuilt by the next call, the caller's lengths may go away
    GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  }
  const PbNgAdapt ad = {a.gamma, a.len, a.j, a.halv, a.shortest, (int)halvings};
  const int64_t n = p->nparams;
  const int blocks = (int)std::min<int64_t>(2048, std::max<int64_t>(1, (n + 255) / 256));
  const int row_blocks = (p->maxM + PB_NG_TILE - 1) / PB_NG_TILE;
  for (int s = 0; s < steps; s++) {
    GP_CHECK(pb_eval(p, params, x, y, idx + (int64_t)s * p->sumB, p->d_elbo, p->d_grad));
    if (nstep > 0 && !adapt) {
      hipLaunchKernelGGL(pdgpb_ng_form_kernel, dim3(nstep), dim3(PB_THREADS), pb_ng_form_lds(p), h->stream, p->d_gps, r.list,
                         (const double*)params, (const double*)p->d_grad, gamma, r.blocks, r.refused, p->maxM);
      GP_HIP_CHECK(h, hipGetLastError());
      hipLaunchKernelGGL(pdgpb_ng_apply_kernel, dim3(nstep, row_blocks), dim3(PB_THREADS), pb_ng_apply_lds(p), h->stream,
                         p->d_gps, r.list, params, free_state, p->d_grad, gamma, (const double*)r.blocks,
                         (const int32_t*)p->d_status, (const int32_t*)r.refused);
      GP_HIP_CHECK(h, hipGetLastError());
    } else if (nstep > 0) {
      hipLaunchKernelGGL(pdgpb_ng_form_adaptive_kernel, dim3(nstep), dim3(PB_THREADS), pb_ng_form_lds(p), h->stream, p->d_gps,
                         r.list, (const double*)params, (const double*)p->d_grad, ad, r.blocks, r.refused, p->maxM);
      GP_HIP_CHECK(h, hipGetLastError());
      hipLaunchKernelGGL(pdgpb_ng_apply_adaptive_kernel, dim3(nstep, row_blocks), dim3(PB_THREADS), pb_ng_apply_lds(p), h->stream,
                         p->d_gps, r.list, params, free_state, p->d_grad, ad, (const double*)r.blocks,
                         (const int32_t*)p->d_status, (const int32_t*)r.refused);
      GP_HIP_CHECK(h, hipGetLastError());
    }
    GP_CHECK(pb_tie(p, r.refused));
    hipLaunchKernelGGL(pdgpb_adam_kernel, dim3(blocks), dim3(256), 0, h->stream, free_state, params, p->d_grad, tcode, m, v,
                       p->d_owner, p->d_status, (const int32_t*)r.refused, (const int32_t*)p->ties.frozen,
                       lr_t + (int64_t)s * p->nm, n, beta1, beta2, eps, h->logistic);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  return GP_OK;
}

gp_status gp_pdgpb_natgrad(gp_pdgpb_plan p, double* free_state, double* params, const uint8_t* tcode, double* m, double* v,
                           const double* x, const double* y, const int32_t* idx, int32_t steps, const double* lr_t,
                           double beta1, double beta2, double eps, double gamma, const int32_t* step_gp_host,
                           void* workspace, size_t workspace_bytes) {
  return pb_natgrad_run(p, "gp_pdgpb_natgrad", free_state, params, tcode, m, v, x, y, idx, steps, lr_t, beta1, beta2, eps, gamma,
                        nullptr, 0, step_gp_host, workspace, workspace_bytes);
}

size_t gp_pdgpb_natgrad_adaptive_workspace_bytes(gp_pdgpb_plan p) {
  if (!p || p->predict_only) return 0;
  return gp_measure([&](GpArena& ar) { pb_nga_regions(p, ar); }) + GP_WS_TAIL_BATCH;
}

gp_status gp_pdgpb_natgrad_adaptive(gp_pdgpb_plan p, double* free_state, double* params, const uint8_t* tcode, double* m,
                                    double* v, const double* x, const double* y, const int32_t* idx, int32_t steps,
                                    const double* lr_t, double beta1, double beta2, double eps, const double* gamma_gp_host,
                                    int32_t halvings, const int32_t* step_gp_host, void* workspace, size_t workspace_bytes) {
  if (p && !gamma_gp_host) return gp_fail(p->h, GP_ERR_BAD_ARG, "gp_pdgpb_natgrad_adaptive: bad argument or a prediction-only plan");
  return pb_natgrad_run(p, "gp_pdgpb_natgrad_adaptive", free_state, params, tcode, m, v, x, y, idx, steps, lr_t, beta1, beta2, eps,
                        0.0, gamma_gp_host, halvings, step_gp_host, workspace, workspace_bytes);
}

gp_status gp_pdgpb_natgrad_counts(gp_pdgpb_plan p, int64_t* halvings_host, double* shortest_host, int32_t clear) {
  if (!p || (!halvings_host != !shortest_host)) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->d_ng_halv) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_natgrad_counts: no gp_pdgpb_natgrad_adaptive call yet");
  const size_t G = p->gps.size();
  if (halvings_host) {
    GP_HIP_CHECK(h, hipMemcpyAsync(halvings_host, p->d_ng_halv, G * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    GP_HIP_CHECK(h, hipMemcpyAsync(shortest_host, p->d_ng_short, G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    for (size_t g = 0; g < G; g++)
      if (!(shortest_host[g] <= 1.0)) shortest_host[g] = HUGE_VAL;   // no step since the reset
  }
  if (clear) {
    GP_HIP_CHECK(h, hipMemsetAsync(p->d_ng_halv, 0, G * sizeof(int64_t), h->stream));
    GP_HIP_CHECK(h, hipMemsetAsync(p->d_ng_short, PB_NG_SHORT_CLEAR_BYTE, G * sizeof(double), h->stream));
  }
  return GP_OK;
}

gp_status gp_pdgpb_natgrad_refused(gp_pdgpb_plan p, int32_t* host_status, int32_t clear) {
  if (!p || !host_status) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->d_refused) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_natgrad_refused: no gp_pdgpb_natgrad call yet");
  GP_HIP_CHECK(h, hipMemcpyAsync(host_status, p->d_refused, p->nm * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < p->nm; k++)
    if (host_status[k] != 0) host_status[k] = 1 + (0x7fffffff - host_status[k]);
  if (clear) GP_HIP_CHECK(h, hipMemsetAsync(p->d_refused, 0, p->nm * sizeof(int32_t), h->stream));
  return GP_OK;
}

gp_status gp_pdgpb_not_pd(gp_pdgpb_plan p, int32_t* host_status, int32_t clear) {
  if (!p || !host_status) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->d_status) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_not_pd: no workspace set (prediction: no gp_pdgpb_predict_prepare yet)");
  GP_HIP_CHECK(h, hipMemcpyAsync(host_status, p->d_status, p->nm * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < p->nm; k++)
    if (host_status[k] != 0) host_status[k] = 1 + (0x7fffffff - host_status[k]);
  if (clear) GP_HIP_CHECK(h, hipMemsetAsync(p->d_status, 0, p->nm * sizeof(int32_t), h->stream));
  return GP_OK;
}

// ---- prediction ----------------------------------------------------------------------------------------------------
// gp_pdgpb_predict_prepare's regions of a workspace, in order (gp_pdgpb_predict_moments keeps fmean / fvar behind them)
struct PbPredRegions { PbGp* gps; int32_t* status; PbPredGp* pgs; int64_t* tiles; double* G; };
static PbPredRegions pb_pred_regions(const gp_pdgpb_plan_s* p, GpArena& ar) {
  PbPredRegions r;
  r.gps = ar.take<PbGp>(p->gps.size());
  r.status = ar.take<int32_t>(p->nm);
  r.pgs = ar.take<PbPredGp>(p->gps.size());
  r.tiles = ar.take<int64_t>(p->gps.size() + 1);
  r.G = ar.take<double>(p->pred_g);
  return r;
}

size_t gp_pdgpb_predict_workspace_bytes(gp_pdgpb_plan p) {
  return (p && p->predict_only) ? gp_measure([&](GpArena& ar) { pb_pred_regions(p, ar); }) + GP_WS_TAIL_BATCH : 0;
}

gp_status gp_pdgpb_predict_prepare(gp_pdgpb_plan p, const double* params, void* workspace, size_t bytes) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->predict_only || !params)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_predict_prepare: bad argument or a training plan (create the plan with cfg->batch == NULL)");
  if (!workspace || bytes < gp_pdgpb_predict_workspace_bytes(p) || (((uintptr_t)workspace) & 255))
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_predict_prepare: workspace too small or not 256-byte aligned");
  GpArena ar(workspace, bytes);
  const PbPredRegions r = pb_pred_regions(p, ar);
  if (!ar.ok) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_predict_prepare: arena overflow");
  p->d_gps = r.gps; p->d_status = r.status; p->d_pgs = r.pgs; p->d_tiles = r.tiles; p->d_G = r.G;
  p->pred_ws = nullptr;
  GP_HIP_CHECK(h, hipMemcpyAsync(p->d_gps, p->gps.data(), p->gps.size() * sizeof(PbGp), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemsetAsync(p->d_status, 0, p->nm * sizeof(int32_t), h->stream));
  GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)pdgpb_pred_prep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pb_prep_lds(p)));
  GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)pdgpb_pred_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pb_pred_lds(p)));
  hipLaunchKernelGGL(pdgpb_pred_prep_kernel, dim3(p->G), dim3(PB_THREADS), pb_prep_lds(p), h->stream, p->d_gps, params, p->d_G,
                     p->d_status, p->jitter, p->maxM);
  GP_HIP_CHECK(h, hipGetLastError());
  // the descriptors were copied from pageable host memory: wait before the host vectors can change
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  p->pred_ws = workspace;
  p->pred_params = params;
  return GP_OK;
}

}  // extern "C"

// what gp_pdgpb_predict and gp_pdgpb_predict_moments (`who`, named in the messages) ask before anything else: a
// predict-only plan, xnew_off starting at 0, and the workspace and parameters gp_pdgpb_predict_prepare was given
static gp_status pb_pred_check(gp_pdgpb_plan_s* p, const char* who, const double* params, const int64_t* xnew_off,
                               const void* workspace, size_t bytes) {
  if (!p) return GP_ERR_BAD_ARG;
  const std::string w(who);
  if (!p->predict_only || !xnew_off)
    return gp_fail(p->h, GP_ERR_BAD_ARG, (w + ": bad argument or a training plan (create the plan with cfg->batch == NULL)").c_str());
  if (!workspace || workspace != p->pred_ws || bytes < gp_pdgpb_predict_workspace_bytes(p) || params != p->pred_params)
    return gp_fail(p->h, GP_ERR_BAD_ARG, (w + ": call gp_pdgpb_predict_prepare first with the same parameters and workspace").c_str());
  if (xnew_off[0] != 0) return gp_fail(p->h, GP_ERR_BAD_ARG, (w + ": xnew_off[0] must be 0").c_str());
  return GP_OK;
}

// the call's records and tile list from xnew_off, on the host and (when there is a tile) on the device; *tiles_out = entries;
// args_ok = 0: the caller's pointers do not allow a call with frames
static gp_status pb_pred_records(gp_pdgpb_plan_s* p, const int64_t* xnew_off, int args_ok, int64_t* tiles_out) {
  gp_handle h = p->h;
  p->pgs.resize(p->G);
  p->tiles.resize(p->G + 1);
  int64_t fbase = 0, sbase = 0, tiles = 0;
  for (int k = 0; k < p->nm; k++) {
    const int64_t n = xnew_off[k + 1] - xnew_off[k];
    if (n < 0) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_predict: xnew_off must not decrease");
    const PbModel& md = p->models[k];
    for (int r = 0; r < 2 * md.P; r++) {
      const int g = md.g0 + r;
      PbPredGp& pg = p->pgs[g];
      pg.x_off = xnew_off[k];
      pg.out_off = fbase + (int64_t)r * n;
      pg.src_off = r < md.P ? sbase + (int64_t)r * n : -1;
      pg.n = n;
      pg.P = md.P;
      pg.nlin = md.nlin;
      p->tiles[g] = tiles;
      tiles += (n + PB_PT - 1) / PB_PT;
    }
    fbase += 2 * (int64_t)md.P * n;
    sbase += (int64_t)md.P * n;
  }
  p->tiles[p->G] = tiles;
  *tiles_out = tiles;
  if (tiles == 0) return GP_OK;
  if (!args_ok) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_predict: bad argument");
  if (tiles > 0x7fffffff) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_predict: more than 2^31 - 1 frame tiles in one call");
  GP_HIP_CHECK(h, hipMemcpyAsync(p->d_pgs, p->pgs.data(), p->pgs.size() * sizeof(PbPredGp), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(p->d_tiles, p->tiles.data(), p->tiles.size() * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  // pageable host vectors again: the next call rewrites them
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
  return GP_OK;
}

extern "C" {

gp_status gp_pdgpb_predict(gp_pdgpb_plan p, const double* params, const double* xnew, const int64_t* xnew_off, double* fmean,
                           double* fvar, double* mean_source, void* workspace, size_t bytes) {
  GP_CHECK(pb_pred_check(p, "gp_pdgpb_predict", params, xnew_off, workspace, bytes));
  gp_handle h = p->h;
  int64_t tiles = 0;
  GP_CHECK(pb_pred_records(p, xnew_off, (xnew && fmean && fvar) ? 1 : 0, &tiles));
  if (tiles == 0) return GP_OK;
  hipLaunchKernelGGL(pdgpb_pred_kernel, dim3((unsigned)tiles), dim3(PB_PRED_THREADS), pb_pred_lds(p), h->stream, p->d_gps, p->d_pgs,
                     p->d_tiles, p->G, params, p->d_G, xnew, fmean, fvar, pb_pad16(p->maxM));
  GP_HIP_CHECK(h, hipGetLastError());
  if (mean_source) {
    hipLaunchKernelGGL(pdgpb_pred_source_kernel, dim3((unsigned)tiles), dim3(PB_PT), 0, h->stream, p->d_gps, p->d_pgs, p->d_tiles,
                       p->G, fmean, mean_source);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  return GP_OK;
}

// gp_pdgpb_predict_moments' carve: gp_pdgpb_predict_prepare's regions, then this call's fmean / fvar (`latent` doubles each)
static std::pair<double*, double*> pb_mom_regions(const gp_pdgpb_plan_s* p, GpArena& ar, int64_t latent) {
  pb_pred_regions(p, ar);
  double* fm = ar.take<double>((size_t)latent);
  return {fm, ar.take<double>((size_t)latent)};
}
size_t gp_pdgpb_predict_moments_workspace_bytes(gp_pdgpb_plan p, int64_t latent_frames) {
  if (!p || !p->predict_only || latent_frames < 0) return 0;
  return gp_measure([&](GpArena& ar) { pb_mom_regions(p, ar, latent_frames); }) + GP_WS_TAIL_BATCH;
}

gp_status gp_pdgpb_predict_moments(gp_pdgpb_plan p, const double* params, const double* xnew, const int64_t* xnew_off,
                                   const double* ynew, double* smean, double* svar, double* ymean, double* yvar, double* logp,
                                   void* workspace, size_t bytes) {
  GP_CHECK(pb_pred_check(p, "gp_pdgpb_predict_moments", params, xnew_off, workspace, bytes));
  gp_handle h = p->h;
  int maxP = 1;
  int64_t latent = 0;      // sum_k 2 P_k n_k; without frames the call is done before any pointer is looked at
  for (int k = 0; k < p->nm; k++) {
    if (xnew_off[k + 1] < xnew_off[k]) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_predict_moments: xnew_off must not decrease");
    latent += 2 * (int64_t)p->models[k].P * (xnew_off[k + 1] - xnew_off[k]);
    maxP = std::max(maxP, p->models[k].P);
  }
  if (latent == 0) return GP_OK;
  if (!xnew || (logp && !ynew)) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_predict_moments: bad argument (logp needs ynew)");
  const size_t lds = (size_t)PB_MOM_FRAMES * 4 * maxP * sizeof(double);
  if (lds > 48 * 1024) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgpb_predict_moments: too many sources for the moments kernel's LDS staging");
  GpArena ar(workspace, bytes);
  const auto [fm, fv] = pb_mom_regions(p, ar, latent);
  if (bytes < gp_pdgpb_predict_moments_workspace_bytes(p, latent) || !ar.ok)
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_predict_moments: the workspace does not hold this call's fmean / fvar (gp_pdgpb_predict_moments_workspace_bytes)");
  int64_t tiles = 0;       // > 0: there are frames
  GP_CHECK(pb_pred_records(p, xnew_off, 1, &tiles));
  hipLaunchKernelGGL(pdgpb_pred_kernel, dim3((unsigned)tiles), dim3(PB_PRED_THREADS), pb_pred_lds(p), h->stream, p->d_gps, p->d_pgs,
                     p->d_tiles, p->G, params, p->d_G, xnew, fm, fv, pb_pad16(p->maxM));
  GP_HIP_CHECK(h, hipGetLastError());
  hipLaunchKernelGGL(pdgpb_pred_moments_kernel, dim3((unsigned)tiles), dim3(PB_MOM_THREADS), lds, h->stream, p->d_gps, p->d_pgs,
                     p->d_tiles, p->G, params, fm, fv, ynew, smean, svar, ymean, yvar, logp, maxP);
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}

}  // extern "C"

// ---- joint posterior draws ------------------------------------------------------------------------------------------
static inline bool pb_smp_kernel_ok(int t) { return t == GP_KERN_MATERN12 || t == GP_KERN_MATERN32 || t == GP_KERN_MERCER_MATERN12SM; }
static inline DevKern pb_smp_kern(const PbGp& g, const double* params) { return DevKern{g.type, g.m, params + g.off_theta}; }
// gp_pdgpb_sample's carve: gp_pdgpb_predict_prepare's regions, then the call's descriptor block, merged orders, feature
// tables of the frames and of z (spectral-mixture GPs), prior(z) and beta.  Only models with frames are sampled.
struct PbSmpBufs { char* desc; int* order; double *fx, *fz, *pz, *beta; size_t nproc; };
static PbSmpBufs pb_smp_carve(const gp_pdgpb_plan_s* p, GpArena& ar, const int64_t* xnew_off, int64_t S) {
  pb_pred_regions(p, ar);
  size_t nproc = 0, norder = 0, fx = 0, fz = 0, ms = 0;
  for (int k = 0; k < p->nm; k++) {
    const int64_t n = xnew_off[k + 1] - xnew_off[k];
    const PbModel& md = p->models[k];
    for (int r = 0; r < 2 * md.P; r++) {
      const PbGp& g = p->gps[md.g0 + r];
      norder += (size_t)(n > 0 ? n : 0) + g.M;               // every model's orders are uploaded, as the caller lays them out
      if (n <= 0) continue;
      const size_t mp = g.type == GP_KERN_MERCER_MATERN12SM ? sm_mpad(g.m) : 0;
      nproc++;
      fx += 2 * mp * (size_t)n;
      fz += 2 * mp * g.M;
      ms += (size_t)g.M * S;
    }
  }
  PbSmpBufs b;
  b.nproc = nproc;
  b.desc = ar.take<char>(ssm_desc_layout(nproc, nproc * sizeof(PbSmpGp), 0).bytes);
  b.order = ar.take<int>(norder);
  b.fx = ar.take<double>(fx);
  b.fz = ar.take<double>(fz);
  b.pz = ar.take<double>(ms);
  b.beta = ar.take<double>(ms);
  return b;
}

extern "C" {

size_t gp_pdgpb_sample_workspace_bytes(gp_pdgpb_plan p, const int64_t* xnew_off, int32_t S) {
  if (!p || !p->predict_only || !xnew_off || S < 1) return 0;
  return gp_measure([&](GpArena& ar) { pb_smp_carve(p, ar, xnew_off, S); }) + GP_WS_TAIL_BATCH;
}

gp_status gp_pdgpb_sample(gp_pdgpb_plan p, const double* params, const double* xnew, const int64_t* xnew_off,
                          const int32_t* order_host, int32_t S, const double* eps_x, const double* eps_z, const double* eps_u,
                          double* latents, double* sources, void* workspace, size_t bytes) {
  GP_CHECK(pb_pred_check(p, "gp_pdgpb_sample", params, xnew_off, workspace, bytes));
  gp_handle h = p->h;
  if (S < 1) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_sample: S >= 1 draws");
  if (S > 65535 * PB_SMP_DRAWS) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgpb_sample: at most 1048560 draws per call");
  int64_t frames = 0;
  for (int k = 0; k < p->nm; k++) {
    const int64_t n = xnew_off[k + 1] - xnew_off[k];
    if (n < 0) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_sample: xnew_off must not decrease");
    if (n + PB_MAX_M > INT32_MAX / 2) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgpb_sample: a model has too many frames");
    frames += n;
  }
  if (!xnew || !order_host || !eps_x || !eps_z || !eps_u || !latents)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgpb_sample: bad argument (no null pointers but sources)");
  for (const PbGp& g : p->gps)
    if (!pb_smp_kernel_ok(g.type))
      return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgpb_sample: every latent GP needs a kernel with an exact state-space prior sampler "
                                            "that the batch takes (Matern12, Matern32, MercerMatern12sm)");
  if (bytes < gp_pdgpb_sample_workspace_bytes(p, xnew_off, S))
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_sample: the workspace does not hold this call's buffers (gp_pdgpb_sample_workspace_bytes)");
  GpArena ar(workspace, bytes);
  const PbSmpBufs b = pb_smp_carve(p, ar, xnew_off, S);
  if (!ar.ok) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgpb_sample: arena overflow");
  if (b.nproc > 32767) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgpb_sample: at most 32767 latent GPs with frames per call");
  std::vector<SsmSpan> spans;                 // every latent GP's n_k + M_r entries back to back, empty models included
  size_t norder = 0;
  for (int k = 0; k < p->nm; k++) {
    const int64_t n = xnew_off[k + 1] - xnew_off[k];
    for (int r = 0; r < 2 * p->models[k].P; r++) {
      const int len = (int)n + p->gps[p->models[k].g0 + r].M;
      spans.push_back(SsmSpan{norder, len});
      norder += len;
    }
  }
  GP_CHECK(ssm_check_orders(h, order_host, spans, "gp_pdgpb_sample: order is not a permutation of a latent GP's n + M points"));
  if (frames == 0) return GP_OK;

  const int count = (int)b.nproc;
  const SsmDesc lay = ssm_desc_layout(b.nproc, b.nproc * sizeof(PbSmpGp), 0);
  std::vector<char> hd(lay.bytes, 0);
  SsmProc* procs = (SsmProc*)(hd.data() + lay.procs);
  PbSmpGp* recs = (PbSmpGp*)(hd.data() + lay.recs);
  FeatItem* feats = (FeatItem*)(hd.data() + lay.feat);
  int nfeat = 0, at = 0, max_mpad = 0, max_n = p->maxM;
  size_t off_x = 0, off_z = 0, off_u = 0, off_o = 0, off_lat = 0, off_src = 0, off_fx = 0, off_fz = 0, off_ms = 0;
  for (int k = 0; k < p->nm; k++) {
    const int64_t n = xnew_off[k + 1] - xnew_off[k];
    const PbModel& md = p->models[k];
    for (int r = 0; r < 2 * md.P; r++) {
      const PbGp& g = p->gps[md.g0 + r];
      const DevKern kern = pb_smp_kern(g, params);
      const int c = ssm_components(g.type, g.m), M = g.M, mp = ssm_mpad(kern);
      if (n > 0) {
        SsmProc& it = procs[at];
        it.k = kern; it.z = params + g.off_z; it.xnew = xnew + xnew_off[k];
        if (mp) {
          double* tx = b.fx + off_fx;
          double* tz = b.fz + off_fz;
          feats[nfeat++] = FeatItem{kern, it.xnew, tx, (int)n, 0};
          feats[nfeat++] = FeatItem{kern, it.z, tz, M, 0};
          it.fx = tx; it.fz = tz;
          off_fx += 2 * (size_t)mp * n; off_fz += 2 * (size_t)mp * M;
        }
        it.order = b.order + off_o;
        it.eps_x = eps_x + off_x; it.eps_z = eps_z + off_z;
        it.beta = b.beta + off_ms;
        it.out = latents + off_lat + (size_t)r * S * n;
        it.pz = b.pz + off_ms;
        it.n = (int)n; it.kz = M; it.mp = mp; it.cs = c; it.ezs = M;
        PbSmpGp& rc = recs[at];
        rc.Gt = p->d_G + g.ws; rc.eps_u = eps_u + off_u;
        rc.q_mu = params + g.off_qmu; rc.q_sqrt = params + g.off_qsq;
        rc.pz = it.pz; rc.beta = b.beta + off_ms;
        rc.n = n; rc.M = M; rc.nlin = md.nlin;
        if (r < md.P) {
          rc.lat_g = it.out;
          rc.lat_f = latents + off_lat + (size_t)(md.P + r) * S * n;
          rc.src = sources ? sources + off_src + (size_t)r * S * n : nullptr;
        }
        off_ms += (size_t)M * S;
        if (mp > max_mpad) max_mpad = mp;
        if (n > max_n) max_n = (int)n;
        at++;
      }
      off_x += (size_t)S * c * n; off_z += (size_t)S * c * M; off_u += (size_t)S * 2 * M; off_o += (size_t)n + M;
    }
    off_lat += 2 * (size_t)md.P * S * n;
    off_src += (size_t)md.P * S * n;
  }
  static const char* const PARTIALS = "gp_pdgpb_sample: num_partials must be in [1, 32]";
  const int64_t entries = ssm_fill_tiles(lay, hd, count, p->maxM);
  GP_CHECK(ssm_upload(h, lay, hd, b.desc, nfeat, order_host, b.order, norder, max_n));
  // (process, draw) pairs packed densely into wavefronts were measured and lost to this grid: DESIGN 3h
  GP_CHECK(ssm_launch_prior(h, (const SsmProc*)(b.desc + lay.procs), count, S, max_mpad, PARTIALS));
  const PbSmpGp* d_recs = (const PbSmpGp*)(b.desc + lay.recs);
  GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)pdgpb_sample_inducing_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                      (int)pb_smp_lds(p->maxM)));
  hipLaunchKernelGGL(pdgpb_sample_inducing_kernel, dim3(count, (S + PB_SMP_DRAWS - 1) / PB_SMP_DRAWS), dim3(PB_THREADS),
                     pb_smp_lds(p->maxM), h->stream, d_recs, S, sqrt(p->jitter), p->maxM);
  GP_HIP_CHECK(h, hipGetLastError());
  GP_CHECK(ssm_launch_update(h, lay, b.desc, count, entries, p->maxM, S, max_mpad, PARTIALS));
  if (sources) {
    hipLaunchKernelGGL(pdgpb_sample_source_kernel, dim3((unsigned)entries, std::min(S, 64)), dim3(PB_SMP_TILE), 0, h->stream, d_recs,
                       (const int64_t*)(b.desc + lay.tiles), count, S);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  return GP_OK;
}

}  // extern "C"
