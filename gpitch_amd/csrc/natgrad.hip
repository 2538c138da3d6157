// natgrad.hip — one natural-gradient step on the variational posteriors q(u_r) = N(q_mu_r, Lq_r Lq_r^T) of a Pdgp plan
// (gp_pdgp_natgrad_step), from the gradient blocks gp_pdgp_elbo has written.  Per latent GP r, with
// Lq = tril(q_sqrt), g = d ELBO / d q_mu, G_L = tril(d ELBO / d q_sqrt) and step length gamma:
//
//   Phi = tril(Lq^T G_L),  P = (Phi + Phi^T - diag(Phi)) / 2  ( = Lq^T (d ELBO / d S) Lq ),  B = I - 2 gamma P
//   B = U U^T with U upper triangular: the index-reversed matrix J B J = C C^T is factored, U = J C J, U^-T = J (C^-1)^T J
//   Lq' = Lq U^-T   (lower triangular; S' = Lq' Lq'^T has S'^-1 = S^-1 - 2 gamma d ELBO / d S)
//   q_mu' = q_mu + gamma Lq' (Lq'^T g)
//
// Three launches, all float64, no atomics, every sum in a fixed order:
//   1. ng_form_kernel    the reversed B of every GP over a ragged list of (GP, 32 x 32 tile of the lower triangle) entries: the
//                        triangular product Lq^T G_L on the float64 MFMA, read in place from the parameter and gradient
//                        vectors; also w = Lq^T g, the chol launch's pointer arrays, and the report word (below)
//   2. chol.hip          launch_cholesky_inverse_batched on the batch of reversed Bs: C in place, C^-1 beside it
//   3. ng_apply_kernel   over (GP, block of 32 rows) entries: Lq' = Lq U^-T on the MFMA, q_mu', the writes to params and
//                        free_state, the zeroing of the gradient blocks.  It looks at the handle's status word first and
//                        writes nothing once that is set, so a B that is not positive definite — for any GP — leaves every
//                        GP's state as it was (and gp_adam_step, behind it, freezes as it does for a failed Kuu).
// Lq is never inverted; the only factorisation is of B = I + O(gamma).
//
// gp_pdgp_natgrad_step_adaptive: a length gamma_r per latent GP, and GP r steps at gamma_r 2^-j for the smallest j
// in 0..halvings whose B factors with every pivot positive.  Rounds j = 0..halvings of three launches each, no host
// synchronisation: ng_form_adaptive_kernel (B at gamma_r 2^-j of the GPs still pending), the factorisation with a per-matrix
// outcome (size 0 for the others: an accepted factor and inverse stay), ng_settle_kernel (what the outcomes decided); then
// ng_apply_adaptive_kernel at each GP's accepted length, which refuses the whole step itself when some GP found none.  The form
// and apply kernels are the bodies below instantiated a second time: at j = 0 the arithmetic is the plain step's.
#include "pdgp_plan.h"

typedef double ng_d4 __attribute__((ext_vector_type(4)));

#define NG_TILE 32
#define NG_THREADS 256
#define NG_MAX_GPS 64       // latent GPs per form / apply launch: their records travel as kernel arguments (no descriptor upload,
                            // so a training loop's step needs neither a host buffer that outlives the call nor a synchronisation)
#define NG_MAX_M 4096       // the apply kernel keeps t = U^-1 Lq^T g (M doubles) in LDS
#define NG_REPORT_WORDS 64  // the workspace's first 256 bytes: int32 {refused, latent GP, pivot, status word was clean at the form launch}

struct NgGp {
  int M, g;                   // inducing points; the GP's index in the plan
  int start_form, start_apply;   // first entry of this GP in the launch's two work lists
  int64_t off_qmu, off_qsqrt; // into params / free_state / grad
  int64_t ws_off;             // doubles from the workspace base to this GP's [reversed B -> C | C^-1 | w]
};
struct NgArgs {
  NgGp gp[NG_MAX_GPS];
  int count, slot0;           // GPs of this launch; the first one's slot in the factorisation batch
  int total_form, total_apply;
  int first;                  // the call's first launch: it keeps the report word
  int pad_;
  int64_t o_ptrA, o_ptrW, o_Ms, o_lds, o_gidx;   // bytes from the workspace base to the factorisation's descriptor arrays
};

// the adaptive step (gp_pdgp_natgrad_step_adaptive): per-GP lengths and the round's place in the workspace.  Round j forms B at
// gamma_r 2^-j for the GPs still pending; acc[slot] is a GP's accepted j (-1: pending), out[slot] the factorisation's outcome
// of the round, ctl = {GPs pending for the next round, some GP exhausted, its slot, its pivot}.
struct NgAdapt {
  double gamma[NG_MAX_GPS];   // gamma_r of the launch's GPs
  int round, halvings;
  int64_t o_acc, o_out, o_ctl, o_halv, o_short;   // bytes from the workspace base
  int32_t* status_w;          // the handle's status word, writable: the apply launch raises it for an exhausted GP
};
struct NgNone {};
#define NG_CTL_WORDS 64

static __host__ __device__ inline int64_t ng_mm(int M) { return (((int64_t)M * M + 31) / 32) * 32; }   // doubles of an M x M block, 256-byte padded

// the owner of entry e: the last GP whose first entry is <= e (wave-uniform: scalar loads from the argument segment)
template <bool FORM>
__device__ __forceinline__ int ng_owner(const NgArgs& a, int e) {
  int lo = 0, hi = a.count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if ((FORM ? a.gp[mid].start_form : a.gp[mid].start_apply) <= e) lo = mid; else hi = mid;
  }
  return lo;
}

// ---- 1. reversed B = J (I - gamma (Phi + Phi^T - diag Phi)) J, Phi = tril(Lq^T G_L);  w = Lq^T g ---------------------------
// One workgroup per 32 x 32 tile (ti, tj <= ti) of a GP's lower triangle, one 16 x 16 sub-tile per wavefront.
// Phi_ij = sum_{k >= max(i, j)} Lq_ki G_kj: the k loop starts at the sub-tile's first row.  The masks k >= i, k >= j apply the
// two tril()s: the stored strict upper triangle of q_sqrt is free to hold anything.
template <bool ADAPT, typename AD>
__device__ __forceinline__ void ng_form_body(const NgArgs& a, const double* __restrict__ params,
                                             const double* __restrict__ grad, double gamma, char* __restrict__ ws,
                                             const int32_t* __restrict__ status, const AD& ad) {
  __shared__ double part[8][NG_TILE];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int e = blockIdx.x;
  if constexpr (ADAPT) {
    // a later round with nothing pending: one word read
    if (ad.round > 0 && ((const int32_t*)(ws + ad.o_ctl))[0] == 0) return;
  }
  bool round0 = true;                // (the adaptive step's later rounds keep what round 0 laid out)
  if constexpr (ADAPT) round0 = ad.round == 0;
  if (e == 0 && round0) {
    // the factorisation's descriptor arrays, and the report word: a status word that is already raised (a failed Kuu of this
    // evaluation, a refusal not yet collected) is not this step's doing
    if (tid < a.count) {
      const NgGp r = a.gp[tid];
      double* blk = (double*)ws + r.ws_off;
      ((double**)(ws + a.o_ptrA))[a.slot0 + tid] = blk;
      ((double**)(ws + a.o_ptrW))[a.slot0 + tid] = blk + ng_mm(r.M);
      ((int*)(ws + a.o_Ms))[a.slot0 + tid] = r.M;
      ((int*)(ws + a.o_lds))[a.slot0 + tid] = r.M;
      ((int*)(ws + a.o_gidx))[a.slot0 + tid] = r.g;
      if constexpr (ADAPT) {
        ((int32_t*)(ws + ad.o_acc))[a.slot0 + tid] = -1;
        ((int32_t*)(ws + ad.o_out))[a.slot0 + tid] = 0;
      }
    }
    if (a.first && tid == 0) {
      int32_t* rep = (int32_t*)ws;
      if (status[0] == 0) { rep[0] = 0; rep[1] = 0; rep[2] = 0; rep[3] = 1; }
      else rep[3] = 0;
      if constexpr (ADAPT) {
        int32_t* ctl = (int32_t*)(ws + ad.o_ctl);
        ctl[0] = 0; ctl[1] = 0; ctl[2] = 0; ctl[3] = 0;
      }
    }
  }
  const int o = ng_owner<true>(a, e);
  const NgGp r = a.gp[o];
  const int M = r.M;
  if constexpr (ADAPT) {
    // only the GPs still pending are formed again: an accepted factor and inverse stay as they are
    if (ad.round > 0 && ((const int32_t*)(ws + ad.o_acc))[a.slot0 + o] >= 0) return;
    gamma = scalbn(ad.gamma[o], -ad.round);     // an exact scaling; round 0 is gamma_r itself
  }
  const int t = e - r.start_form;
  int ti = (int)((__fsqrt_rn(8.0f * (float)t + 1.0f) - 1.0f) * 0.5f);
  while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
  while (ti * (ti + 1) / 2 > t) ti--;
  const int tj = t - ti * (ti + 1) / 2;
  const double* __restrict__ Lq = params + r.off_qsqrt;
  const double* __restrict__ GL = grad + r.off_qsqrt;
  double* __restrict__ Brev = (double*)ws + r.ws_off;

  const int kq = lane >> 4, lc = lane & 15;
  const int i0 = ti * NG_TILE + (wave >> 1) * 16, j0 = tj * NG_TILE + (wave & 1) * 16;
  if (j0 <= i0 && i0 < M) {          // (a sub-tile strictly above the diagonal, or past the last row: nothing to do)
    const int ia = i0 + lc, jb = j0 + lc;
    ng_d4 acc = {0.0, 0.0, 0.0, 0.0};
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
        const int ri = M - 1 - i, rj = M - 1 - j;            // rj >= ri: (rj, ri) is in the lower triangle of the reversed matrix
        Brev[(int64_t)rj * M + ri] = v;
        Brev[(int64_t)ri * M + rj] = v;
      }
    }
  }
  if (tj == 0 && round0) {           // (w does not depend on the length)
    // w_i = sum_{k >= i} Lq_ki g_k for the 32 rows of this tile row: 8 partial sums per row, added in order
    const double* __restrict__ g = grad + r.off_qmu;
    double* __restrict__ w = Brev + 2 * ng_mm(M);
    const int c = tid & 31, kg = tid >> 5;
    const int i = ti * NG_TILE + c;
    double s = 0.0;
    if (i < M)
      for (int k = ti * NG_TILE + kg; k < M; k += 8)
        if (k >= i) s = fma(Lq[(int64_t)k * M + i], g[k], s);
    part[kg][c] = s;
    __syncthreads();
    if (tid < NG_TILE && i < M) {
      double sum = part[0][c];
#pragma unroll
      for (int q = 1; q < 8; q++) sum += part[q][c];
      w[i] = sum;
    }
  }
}
__global__ void __launch_bounds__(NG_THREADS) ng_form_kernel(const NgArgs a, const double* __restrict__ params,
                                                             const double* __restrict__ grad, double gamma, char* __restrict__ ws,
                                                             const int32_t* __restrict__ status) {
  ng_form_body<false>(a, params, grad, gamma, ws, status, NgNone{});
}
__global__ void __launch_bounds__(NG_THREADS) ng_form_adaptive_kernel(const NgArgs a, const NgAdapt ad,
                                                                      const double* __restrict__ params,
                                                                      const double* __restrict__ grad, char* __restrict__ ws,
                                                                      const int32_t* __restrict__ status) {
  ng_form_body<true>(a, params, grad, 0.0, ws, status, ad);
}

// ---- 2b. (adaptive step) what round `round`'s factorisation decided: a pending GP whose B factored is accepted at this length
// and leaves the batch (size 0); one that did not stays for the next round, or, after the last, is the step's refusal.
// One workgroup; the exhausted GP reported is the one with the smallest slot.
__global__ void __launch_bounds__(256) ng_settle_kernel(char* __restrict__ ws, int64_t o_acc, int64_t o_out, int64_t o_ctl,
                                                        int64_t o_Ms, int nslots, int round, int halvings) {
  __shared__ int pend, failslot;
  int32_t* acc = (int32_t*)(ws + o_acc);
  const int32_t* out = (const int32_t*)(ws + o_out);
  int32_t* ctl = (int32_t*)(ws + o_ctl);
  int* Ms = (int*)(ws + o_Ms);
  const int tid = threadIdx.x;
  const bool idle = round > 0 && ctl[0] == 0;
  if (tid == 0) { pend = 0; failslot = 0x7fffffff; }
  __syncthreads();
  if (idle) return;
  for (int s = tid; s < nslots; s += 256) {
    if (acc[s] >= 0) continue;
    // (a size of 0 takes the slot out of the later rounds' factorisation launches; the descriptors hold for this step only:
    // the next step's round-0 form launch writes every slot's size again)
    if (out[s] == 0) { acc[s] = round; Ms[s] = 0; }
    else if (round < halvings) atomicAdd(&pend, 1);
    else { Ms[s] = 0; atomicMin(&failslot, s); }
  }
  __syncthreads();
  if (tid == 0) {
    ctl[0] = pend;
    if (failslot != 0x7fffffff) { ctl[1] = 1; ctl[2] = failslot; ctl[3] = out[failslot] - 1; }
  }
}

// ---- 3. Lq' = Lq V, V = U^-T (V_kj = Cinv(M-1-j, M-1-k), lower);  q_mu' = q_mu + gamma Lq' t, t = V^T w -----------------------
// One workgroup per block of 32 rows of a GP: row i of Lq' needs row i of Lq and nothing else of it, so the update runs in
// place.  Column tiles ascend; tile tj reads Lq(i, k) for k >= 32 tj only and overwrites columns [32 tj, 32 tj + 32) after a
// barrier, so no wavefront reads what another has replaced.
template <bool ADAPT, typename AD>
__device__ __forceinline__ void ng_apply_body(const NgArgs& a, double* __restrict__ params, double* __restrict__ fs,
                                              double* __restrict__ grad, double gamma, char* __restrict__ ws,
                                              const int32_t* __restrict__ status, const AD& ad) {
  extern __shared__ __attribute__((aligned(16))) double ng_smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if constexpr (ADAPT) {
    // some GP found no acceptable length within its halvings: the step of every GP is refused, and this launch raises the
    // handle's status word itself ({1, pivot, slot}, chol_diag.h) and fills the report words; nothing is written
    const int32_t* ctl = (const int32_t*)(ws + ad.o_ctl);
    if (ctl[1] != 0) {
      if (a.first && blockIdx.x == 0 && tid == 0) {
        int32_t* rep = (int32_t*)ws;
        if (atomicCAS(&ad.status_w[0], 0, 1) == 0) {
          ad.status_w[1] = ctl[3]; ad.status_w[2] = ctl[2];
          if (rep[3] == 1 && rep[0] == 0) { rep[0] = 1; rep[1] = ((const int*)(ws + a.o_gidx))[ctl[2]]; rep[2] = ctl[3]; }
        }
      }
      return;
    }
    if (status[0] != 0) return;         // (the evaluation itself had failed)
  } else
  if (status[0] != 0) {
    // refused: some B was not positive definite (or the evaluation itself had failed).  Say which, when it was this step's
    if (a.first && blockIdx.x == 0 && tid == 0) {
      int32_t* rep = (int32_t*)ws;
      if (rep[3] == 1 && rep[0] == 0 && status[0] == 1) {
        rep[0] = 1; rep[1] = ((const int*)(ws + a.o_gidx))[status[2]]; rep[2] = status[1];
      }
    }
    return;
  }
  const int e = blockIdx.x;
  const int o = ng_owner<false>(a, e);
  const NgGp r = a.gp[o];
  const int M = r.M;
  const int ti = e - r.start_apply;
  if constexpr (ADAPT) {
    // the length this GP's B was accepted at; the call's counters, once per GP
    const int j = ((const int32_t*)(ws + ad.o_acc))[a.slot0 + o];
    gamma = scalbn(ad.gamma[o], -j);
    if (ti == 0 && tid == 0) {
      int64_t* hv = (int64_t*)(ws + ad.o_halv);
      double* sg = (double*)(ws + ad.o_short);
      hv[r.g] += j;
      sg[r.g] = fmin(sg[r.g], gamma);
    }
  }
  const int row0 = ti * NG_TILE;
  const int iend = min(M, row0 + NG_TILE);
  double* __restrict__ Lq = params + r.off_qsqrt;
  const double* __restrict__ Cinv = (const double*)ws + r.ws_off + ng_mm(M);
  const double* __restrict__ w = (const double*)ws + r.ws_off + 2 * ng_mm(M);
  double* tv = ng_smem;                                  // t_j, j < iend
  double (*red)[NG_TILE + 1] = reinterpret_cast<double (*)[NG_TILE + 1]>(ng_smem + ((M + 1) & ~1));

  // t_j = sum_{k >= j} V_kj w_k = sum_{c = 0}^{M-1-j} Cinv(M-1-j, c) w_{M-1-c}: a wavefront per j, lanes over c, one butterfly
  for (int j = wave; j < iend; j += NG_THREADS / 64) {
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
    const int j0 = tj * NG_TILE + ch * 16;
    const bool live = (j0 <= i0) && (i0 < M);            // wave-uniform
    ng_d4 acc = {0.0, 0.0, 0.0, 0.0};
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
          fs[r.off_qsqrt + (int64_t)i * M + j] = acc[q];
          rs[q] = fma(acc[q], tv[j], rs[q]);
        }
      }
    }
  }
  // (Lq' t)_i: the 32 column shares of a row, added in column order
#pragma unroll
  for (int q = 0; q < 4; q++) red[rh * 16 + kq + 4 * q][ch * 16 + lc] = rs[q];
  __syncthreads();
  if (tid < NG_TILE) {
    const int i = row0 + tid;
    if (i < M) {
      double sum = red[tid][0];
      for (int c = 1; c < NG_TILE; c++) sum += red[tid][c];
      const double v = params[r.off_qmu + i] + gamma * sum;
      params[r.off_qmu + i] = v;
      fs[r.off_qmu + i] = v;
      grad[r.off_qmu + i] = 0.0;
    }
  }
  // this step has used the gradient of these rows: what gp_adam_step sees of them is zero
  double* __restrict__ GLrows = grad + r.off_qsqrt + (int64_t)row0 * M;
  const int64_t cnt = (int64_t)(iend - row0) * M;
  for (int64_t idx = tid; idx < cnt; idx += NG_THREADS) GLrows[idx] = 0.0;
}
__global__ void __launch_bounds__(NG_THREADS) ng_apply_kernel(const NgArgs a, double* __restrict__ params, double* __restrict__ fs,
                                                              double* __restrict__ grad, double gamma, char* __restrict__ ws,
                                                              const int32_t* __restrict__ status) {
  ng_apply_body<false>(a, params, fs, grad, gamma, ws, status, NgNone{});
}
__global__ void __launch_bounds__(NG_THREADS) ng_apply_adaptive_kernel(const NgArgs a, const NgAdapt ad, double* __restrict__ params,
                                                                       double* __restrict__ fs, double* __restrict__ grad,
                                                                       char* __restrict__ ws, const int32_t* __restrict__ status) {
  ng_apply_body<true>(a, params, fs, grad, 0.0, ws, status, ad);
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// the workspace's one carve: [report | factorisation descriptors | per GP: reversed B -> C, C^-1, w]; off[g] in doubles
struct NgBufs { size_t o_ptrA, o_ptrW, o_Ms, o_lds, o_gidx; std::vector<int64_t> off; };
static NgBufs ng_carve(GpArena& ar, const std::vector<PdgpGP>& gps) {
  NgBufs b;
  const size_t G = gps.size();
  auto at = [&](void* p) { return ar.base ? (size_t)((char*)p - ar.base) : (size_t)0; };
  (void)ar.take<int32_t>(NG_REPORT_WORDS);
  b.o_ptrA = at(ar.take<double*>(G));
  b.o_ptrW = at(ar.take<double*>(G));
  b.o_Ms = at(ar.take<int>(G));
  b.o_lds = at(ar.take<int>(G));
  b.o_gidx = at(ar.take<int>(G));
  b.off.resize(G);
  for (size_t g = 0; g < G; g++) {
    const int M = gps[g].M;
    double* blk = ar.take<double>((size_t)(2 * ng_mm(M)) + (size_t)M);
    b.off[g] = ar.base ? (int64_t)(blk - (double*)ar.base) : 0;
  }
  return b;
}

// the launches' argument records, NG_MAX_GPS latent GPs each
static std::vector<NgArgs> ng_chunks(gp_pdgp_plan p, const NgBufs& b, const std::vector<int>& act) {
  std::vector<NgArgs> chunks;
  for (size_t s = 0; s < act.size(); s += NG_MAX_GPS) {
    NgArgs a = {};
    a.count = (int)std::min(act.size() - s, (size_t)NG_MAX_GPS);
    a.slot0 = (int)s;
    a.first = (s == 0);
    a.o_ptrA = (int64_t)b.o_ptrA; a.o_ptrW = (int64_t)b.o_ptrW; a.o_Ms = (int64_t)b.o_Ms; a.o_lds = (int64_t)b.o_lds;
    a.o_gidx = (int64_t)b.o_gidx;
    int nf = 0, na = 0;
    for (int c = 0; c < a.count; c++) {
      const int g = act[s + c];
      const PdgpGP& gp = p->gps[g];
      const int T = (gp.M + NG_TILE - 1) / NG_TILE;
      a.gp[c] = NgGp{gp.M, g, nf, na, gp.off_qmu, gp.off_qsqrt, b.off[g]};
      nf += T * (T + 1) / 2;
      na += T;
    }
    a.total_form = nf; a.total_apply = na;
    chunks.push_back(a);
  }
  return chunks;
}

// the adaptive step's carve: the plain step's, then [accepted j per slot | outcome per slot | control words | counters per GP]
struct NgAdaptBufs { NgBufs b; size_t o_acc, o_out, o_ctl, o_halv, o_short; };
static NgAdaptBufs ng_carve_adaptive(GpArena& ar, const std::vector<PdgpGP>& gps) {
  NgAdaptBufs a;
  a.b = ng_carve(ar, gps);
  const size_t G = gps.size();
  auto at = [&](void* p) { return ar.base ? (size_t)((char*)p - ar.base) : (size_t)0; };
  a.o_acc = at(ar.take<int32_t>(G));
  a.o_out = at(ar.take<int32_t>(G));
  a.o_ctl = at(ar.take<int32_t>(NG_CTL_WORDS));
  a.o_halv = at(ar.take<int64_t>(G));
  a.o_short = at(ar.take<double>(G));
  return a;
}
#define NG_SHORT_CLEAR_BYTE 0x7f    // a cleared `shortest` counter: every byte 0x7f, a double far above any gamma; read back as +inf

extern "C" {

size_t gp_pdgp_natgrad_workspace_bytes(gp_pdgp_plan p) {
  if (!p) return 0;
  return gp_measure([&](GpArena& ar) { ng_carve(ar, p->gps); }) + GP_WS_TAIL_OP;
}

gp_status gp_pdgp_natgrad_step(gp_pdgp_plan p, double* params, double* free_state, double* grad, double gamma,
                               const int32_t* step_gp_host, void* workspace, size_t workspace_bytes) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!params || !free_state || !grad || !workspace) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step: null pointer");
  if (!(gamma > 0.0 && gamma <= 1.0)) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step: gamma must lie in (0, 1]");
  if (p->subset) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step: a GP-sharded plan holds only some latent GPs");
  if (((uintptr_t)workspace & 255) != 0) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step: workspace not 256-byte aligned");
  int maxM = 0;
  std::vector<int> act;
  for (int g = 0; g < p->G; g++) {
    if (step_gp_host && !step_gp_host[g]) continue;
    if (p->gps[g].M > NG_MAX_M) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgp_natgrad_step: at most 4096 inducing inputs per latent GP");
    act.push_back(g);
    maxM = std::max(maxM, p->gps[g].M);
  }
  GpArena ar(workspace, workspace_bytes);
  const NgBufs b = ng_carve(ar, p->gps);
  if (!ar.ok) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgp_natgrad_step: workspace too small (gp_pdgp_natgrad_workspace_bytes)");
  if (act.empty()) return GP_OK;
  char* ws = (char*)workspace;
  const int32_t* status = (const int32_t*)h->d_status;

  const std::vector<NgArgs> chunks = ng_chunks(p, b, act);
  {
    GpTimerScope ts(h, GP_TIMER_SMALL_GEMM);
    for (const NgArgs& a : chunks) {
      hipLaunchKernelGGL(ng_form_kernel, dim3(a.total_form), dim3(NG_THREADS), 0, h->stream, a, (const double*)params,
                         (const double*)grad, gamma, ws, status);
      GP_HIP_CHECK(h, hipGetLastError());
    }
  }
  // every B is factored before any state is written: one refusal refuses the step of every GP
  GP_CHECK(launch_cholesky_inverse_batched(h, (double* const*)(ws + b.o_ptrA), (double* const*)(ws + b.o_ptrW),
                                           (const int*)(ws + b.o_Ms), (const int*)(ws + b.o_lds), (int)act.size(), maxM));
  {
    GpTimerScope ts(h, GP_TIMER_SMALL_GEMM);
    const size_t lds = ((size_t)((maxM + 1) & ~1) + (size_t)NG_TILE * (NG_TILE + 1)) * sizeof(double);
    for (const NgArgs& a : chunks) {
      hipLaunchKernelGGL(ng_apply_kernel, dim3(a.total_apply), dim3(NG_THREADS), lds, h->stream, a, params, free_state, grad,
                         gamma, ws, status);
      GP_HIP_CHECK(h, hipGetLastError());
    }
  }
  return GP_OK;
}

size_t gp_pdgp_natgrad_adaptive_workspace_bytes(gp_pdgp_plan p) {
  if (!p) return 0;
  return gp_measure([&](GpArena& ar) { ng_carve_adaptive(ar, p->gps); }) + GP_WS_TAIL_OP;
}

gp_status gp_pdgp_natgrad_step_adaptive(gp_pdgp_plan p, double* params, double* free_state, double* grad,
                                        const double* gamma_gp_host, int32_t halvings, const int32_t* step_gp_host,
                                        void* workspace, size_t workspace_bytes) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!params || !free_state || !grad || !workspace || !gamma_gp_host)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step_adaptive: null pointer");
  for (int g = 0; g < p->G; g++)
    if (!(gamma_gp_host[g] > 0.0 && gamma_gp_host[g] <= 1.0))
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step_adaptive: every gamma must lie in (0, 1]");
  if (halvings < 0 || halvings > 10) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step_adaptive: halvings must lie in 0..10");
  if (p->subset) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step_adaptive: a GP-sharded plan holds only some latent GPs");
  if (((uintptr_t)workspace & 255) != 0)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_step_adaptive: workspace not 256-byte aligned");
  int maxM = 0;
  std::vector<int> act;
  for (int g = 0; g < p->G; g++) {
    if (step_gp_host && !step_gp_host[g]) continue;
    if (p->gps[g].M > NG_MAX_M)
      return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_pdgp_natgrad_step_adaptive: at most 4096 inducing inputs per latent GP");
    act.push_back(g);
    maxM = std::max(maxM, p->gps[g].M);
  }
  GpArena ar(workspace, workspace_bytes);
  const NgAdaptBufs ab = ng_carve_adaptive(ar, p->gps);
  if (!ar.ok)
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgp_natgrad_step_adaptive: workspace too small (gp_pdgp_natgrad_adaptive_workspace_bytes)");
  if (act.empty()) return GP_OK;
  const NgBufs& b = ab.b;
  char* ws = (char*)workspace;
  const int32_t* status = (const int32_t*)h->d_status;
  const std::vector<NgArgs> chunks = ng_chunks(p, b, act);
  std::vector<NgAdapt> ads(chunks.size());
  for (size_t c = 0; c < chunks.size(); c++) {
    NgAdapt& ad = ads[c];
    ad = NgAdapt{};
    for (int k = 0; k < chunks[c].count; k++) ad.gamma[k] = gamma_gp_host[chunks[c].gp[k].g];
    ad.halvings = halvings;
    ad.o_acc = (int64_t)ab.o_acc; ad.o_out = (int64_t)ab.o_out; ad.o_ctl = (int64_t)ab.o_ctl;
    ad.o_halv = (int64_t)ab.o_halv; ad.o_short = (int64_t)ab.o_short;
    ad.status_w = h->d_status;
  }
  // rounds j = 0..halvings: B at gamma_r 2^-j for the GPs still pending, their factorisation with a per-matrix outcome, and
  // what it decided.  Every length is decided before any state is written; nothing here waits for the device
  for (int j = 0; j <= halvings; j++) {
    {
      GpTimerScope ts(h, GP_TIMER_SMALL_GEMM);
      for (size_t c = 0; c < chunks.size(); c++) {
        ads[c].round = j;
        hipLaunchKernelGGL(ng_form_adaptive_kernel, dim3(chunks[c].total_form), dim3(NG_THREADS), 0, h->stream, chunks[c], ads[c],
                           (const double*)params, (const double*)grad, ws, status);
        GP_HIP_CHECK(h, hipGetLastError());
      }
    }
    GP_CHECK(launch_cholesky_inverse_batched_outcome(h, (double* const*)(ws + b.o_ptrA), (double* const*)(ws + b.o_ptrW),
                                                     (const int*)(ws + b.o_Ms), (const int*)(ws + b.o_lds), (int)act.size(), maxM,
                                                     (int32_t*)(ws + ab.o_out)));
    {
      GpTimerScope ts(h, GP_TIMER_SMALL_GEMM);
      hipLaunchKernelGGL(ng_settle_kernel, dim3(1), dim3(256), 0, h->stream, ws, (int64_t)ab.o_acc, (int64_t)ab.o_out,
                         (int64_t)ab.o_ctl, (int64_t)b.o_Ms, (int)act.size(), j, (int)halvings);
      GP_HIP_CHECK(h, hipGetLastError());
    }
  }
  {
    GpTimerScope ts(h, GP_TIMER_SMALL_GEMM);
    const size_t lds = ((size_t)((maxM + 1) & ~1) + (size_t)NG_TILE * (NG_TILE + 1)) * sizeof(double);
    for (size_t c = 0; c < chunks.size(); c++) {
      hipLaunchKernelGGL(ng_apply_adaptive_kernel, dim3(chunks[c].total_apply), dim3(NG_THREADS), lds, h->stream, chunks[c], ads[c],
                         params, free_state, grad, ws, status);
      GP_HIP_CHECK(h, hipGetLastError());
    }
  }
  return GP_OK;
}

gp_status gp_pdgp_natgrad_counts(gp_pdgp_plan p, const void* workspace, int64_t* halvings_host, double* shortest_host,
                                 int32_t clear) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!workspace || ((uintptr_t)workspace & 255) != 0) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_counts: workspace null or not 256-byte aligned");
  GpArena ar((void*)workspace, SIZE_MAX);
  const NgAdaptBufs ab = ng_carve_adaptive(ar, p->gps);
  char* ws = (char*)workspace;
  const size_t G = (size_t)p->G;
  if (halvings_host && shortest_host) {
    GP_HIP_CHECK(h, hipMemcpyAsync(halvings_host, ws + ab.o_halv, G * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    GP_HIP_CHECK(h, hipMemcpyAsync(shortest_host, ws + ab.o_short, G * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));
    for (size_t g = 0; g < G; g++)
      if (!(shortest_host[g] <= 1.0)) shortest_host[g] = HUGE_VAL;   // no step since the reset
  } else if (halvings_host || shortest_host) {
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_natgrad_counts: both host arrays or neither");
  }
  if (clear) {
    GP_HIP_CHECK(h, hipMemsetAsync(ws + ab.o_halv, 0, G * sizeof(int64_t), h->stream));
    GP_HIP_CHECK(h, hipMemsetAsync(ws + ab.o_short, NG_SHORT_CLEAR_BYTE, G * sizeof(double), h->stream));
  }
  return GP_OK;
}

}  // extern "C"
