// sample_pdgp.hip — joint posterior draws of every latent GP and every source nlin(g_i) f_i of a Pdgp model under its
// variational posterior q, by Matheron's rule (gfx950, float64 throughout).  No n x n matrix is formed and nothing M x n
// reaches HBM: O((n + M) c + M n) per latent GP and draw.
//
// State: W_r = chol(Kuu_r + jitter I)^-1 of every latent GP r, as the plan's prediction leaves it (CondTask::W), and the
// variational parameters q_mu_r, q_sqrt_r.  The latent GPs are independent under q, each has its own inducing inputs z_r
// (M_r of them) and its own merge of t = (xnew | z_r), walked in the caller's stable ascending `order`.  Per GP and draw:
//   1. prior path (pdgp_sample_prior_kernel: one thread per (draw, GP), D_j = t_(j) - t_(j-1) >= 0)
//        Matern12 / MercerMatern12sm / Matern12sm: the Ornstein-Uhlenbeck recursion and cos / sin mixing of sample_sparse.hip
//          (1 and 2 m normals per point);
//        Matern32: the two-state recursion on (f, f'), lambda = sqrt(3) / l, a = lambda D, x = 2 a, 2 normals per point:
//          start       f = sqrt(v) e0, f' = lambda sqrt(v) e1
//          transition  (f, f') <- exp(-a) [[1 + a, D], [-lambda^2 D, 1 - a]] (f, f') + chol(Q) (e0, e1)
//          Q = Pinf - Phi Pinf Phi^T, Pinf = diag(v, lambda^2 v), written without cancellation through
//            g(x) = 1 - exp(-x)(1 + x + x^2 / 2) = exp(-x) sum_{k >= 3} x^k / k!      (the series below x = 1: g is O(x^3)
//                                                                                       and audio-rate steps have x ~ 1e-4)
//            Q11 = v g,   Q12 = v lambda exp(-x) x^2 / 2,   Q22 = v lambda^2 (g + 2 x exp(-x))
//          At D = 0 the transition is the identity and Q = 0 exactly: a frame on an inducing input repeats its value.
//   2. inducing side (pdgp_sample_u0_kernel, two batched small GEMMs over the GPs)
//        u0 = prior(z_r) + sqrt(jitter) eps_u[0]     (Kuu carries the jitter, so the draw of u does too)
//        whitened:    beta = W^T (q_mu + tril(q_sqrt) eps_u[1] - W u0)
//        unwhitened:  beta = W^T W (q_mu + tril(q_sqrt) eps_u[1] - u0)
//   3. update  draw_r(x*) = prior_r(x*) + K_r(x*, z_r) beta   (pdgp_sample_update_kernel: the K(Z, tile) build of the sparse
//        predictor in LDS (sps_tile.h), then the float64 MFMA, as sgpr_sample_update_kernel)
//   4. sources  src_i = nlin(draw_i) * draw_{P + i}           (pdgp_sample_source_kernel)
// eps layout: the GPs' blocks back to back, GP r's being eps_x [S][c_r][n], eps_z [S][c_r][M_r], eps_u [S][2][M_r], in the
// caller's own point order.  Determinism: no atomics; every sum has a fixed order; draw s depends on nothing but its own eps
// (a thread owns a draw in steps 1 and 2, a GEMM / MFMA column in steps 2 and 3).
#include <cstring>
#include <vector>

#include "common.h"
#include "cov_entry.h"
#include "gh_quad.h"
#include "sps_tile.h"

typedef double psm_d4 __attribute__((ext_vector_type(4)));

// one per latent GP, engine order
struct PsmItem {
  DevKern k;
  const double* z;
  const double* fz; const double* fx;     // sqrt(e) cos / sin tables of z ([2 mp][M]) and of xnew ([2 mp][n]); SM kernels only
  const int* order;                       // this GP's merged order, n + M entries (validated on the host)
  const double* eps_x; const double* eps_z; const double* eps_u;   // this GP's blocks
  const double* q_mu; const double* q_sqrt;
  const double* beta;                     // [M][S]
  double* out;                            // [S][n]: row block r of `latents`
  double* pz; double* u0; double* rhs;    // [M][S] each
  int M, c, mp, pad_;                     // c: normals per point; mp: sm_mpad(m) of an SM kernel, else 0
};

static inline bool psm_kernel_ok(int type) {
  return type == GP_KERN_MATERN12 || type == GP_KERN_MATERN32 || type == GP_KERN_MERCER_MATERN12SM || type == GP_KERN_MATERN12SM;
}
static inline bool psm_kernel_sm(int type) { return type == GP_KERN_MERCER_MATERN12SM || type == GP_KERN_MATERN12SM; }
static inline int psm_components(int type, int m) { return type == GP_KERN_MATERN12 ? 1 : (type == GP_KERN_MATERN32 ? 2 : 2 * m); }

// g(x) = 1 - exp(-x)(1 + x + x^2 / 2) for x >= 0, e2 = exp(-x).  Below x = 1: exp(-x) x^3 / 6 (1 + x/4 (1 + x/5 (... (1 + x/20))))
// (the tail beyond k = 20 is below 3e-18 of the sum); from 1 on the closed form loses at most four bits.
__device__ __forceinline__ double psm_m32_g(double x, double e2) {
  if (x >= 1.0) return 1.0 - e2 * (1.0 + x + 0.5 * x * x);
  double r = 1.0;
#pragma unroll
  for (int k = 20; k >= 4; k--) r = fma(x * (1.0 / (double)k), r, 1.0);
  return e2 * (x * x * x) * (1.0 / 6.0) * r;
}

// ---- 1. prior paths: one thread per (draw, GP), the states in registers -------------------------------------------------
template <int MPAD>
__global__ void __launch_bounds__(64) pdgp_sample_prior_kernel(const PsmItem* __restrict__ items, const double* __restrict__ xnew,
                                                               int n, int S) {
  const PsmItem it = items[blockIdx.y];
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const int m = it.k.m, M = it.M, c = it.c;
  const int type = it.k.type;
  const bool sm = type == GP_KERN_MERCER_MATERN12SM || type == GP_KERN_MATERN12SM;
  const bool m32 = type == GP_KERN_MATERN32;
  const double var = it.k.theta[0], ls = it.k.theta[1];
  const double sv = sqrt(var);
  const double lam = 1.7320508075688772 / ls;
  const double* __restrict__ ex = it.eps_x + (size_t)s * c * n;
  const double* __restrict__ ez = it.eps_z + (size_t)s * c * M;
  double a[MPAD], b[MPAD];                // OU states of the partials; Matern32: a[0] = f, b[0] = f'
#pragma unroll
  for (int q = 0; q < MPAD; q++) { a[q] = 0.0; b[q] = 0.0; }
  double tprev = 0.0;
  const int tot = n + M;
  for (int j = 0; j < tot; j++) {
    const int idx = it.order[j];
    const bool isz = idx >= n;
    const int i = isz ? idx - n : idx;
    const double t = isz ? it.z[i] : xnew[i];
    const double dt = (j > 0) ? fmax(t - tprev, 0.0) : 0.0;
    tprev = t;
    const double* __restrict__ e = isz ? ez + i : ex + i;
    const size_t es = isz ? (size_t)M : (size_t)n;        // stride between the normals of one point
    double acc;
    if (m32) {
      const double e0 = e[0], e1 = e[es];
      if (j == 0) {                                       // the stationary law: Pinf = diag(v, lambda^2 v)
        a[0] = sv * e0;
        b[0] = lam * sv * e1;
      } else {
        const double al = lam * dt, x = 2.0 * al;
        const double ea = exp(-al), e2 = ea * ea;
        const double g = psm_m32_g(x, e2);
        const double q11 = var * g;
        const double q12 = var * lam * e2 * (0.5 * x * x);
        const double q22 = var * lam * lam * (g + 2.0 * x * e2);
        const double l11 = sqrt(fmax(q11, 0.0));
        const double l21 = l11 > 0.0 ? q12 / l11 : 0.0;
        const double l22 = sqrt(fmax(q22 - l21 * l21, 0.0));
        const double f0 = a[0], f1 = b[0];
        a[0] = ea * ((1.0 + al) * f0 + dt * f1) + l11 * e0;
        b[0] = ea * ((1.0 - al) * f1 - lam * lam * dt * f0) + (l21 * e0 + l22 * e1);
      }
      acc = a[0];
    } else {
      double phi = 0.0, sc = sv;                          // the first point: a draw from the stationary law
      if (j > 0) {
        const double d = dt / ls;
        phi = exp(-d);
        sc = sqrt(var * (-expm1(-2.0 * d)));
      }
      if (!sm) {
        a[0] = fma(phi, a[0], sc * e[0]);
        acc = a[0];
      } else {
        const double* __restrict__ f = isz ? it.fz : it.fx;
        const size_t fn = isz ? (size_t)M : (size_t)n, so = (size_t)it.mp * fn;
        acc = 0.0;
#pragma unroll
        for (int q = 0; q < MPAD; q++)
          if (q < m) {
            a[q] = fma(phi, a[q], sc * e[(size_t)(2 * q) * es]);
            b[q] = fma(phi, b[q], sc * e[(size_t)(2 * q + 1) * es]);
            acc = fma(a[q], f[(size_t)q * fn + i], acc);
            acc = fma(b[q], f[so + (size_t)q * fn + i], acc);
          }
      }
    }
    if (isz) it.pz[(size_t)i * S + s] = acc;
    else it.out[(size_t)s * n + i] = acc;
  }
}

// ---- 2. u0 = prior(z) + sqrt(jitter) eps_u[0];  rhs = q_mu + tril(q_sqrt) eps_u[1]  (unwhitened: rhs - u0); grid (blocks, GP) --
__global__ void __launch_bounds__(256) pdgp_sample_u0_kernel(const PsmItem* __restrict__ items, int S, double sqrt_jitter,
                                                             int whiten) {
  const PsmItem it = items[blockIdx.y];
  const int M = it.M;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = e / S;
  const int s = (int)(e % S);
  if (i >= (size_t)M) return;
  const double* __restrict__ eu = it.eps_u + (size_t)s * 2 * M;
  const double u = it.pz[i * S + s] + sqrt_jitter * eu[i];
  const double* __restrict__ lq = it.q_sqrt + i * M;      // row i of q_sqrt: the columns j <= i are tril(q_sqrt)'s
  double r = it.q_mu[i];
  for (size_t j = 0; j <= i; j++) r = fma(lq[j], eu[M + j], r);
  it.u0[i * S + s] = u;
  it.rhs[i * S + s] = whiten ? r : r - u;
}

// ---- 3. out[s][frame] += sum_i K_r(z_i, x*_frame) beta[i][s]: one workgroup per (frame tile, GP) ---------------------------
// The product of sgpr_sample_update_kernel: beta^T (S x M) times the tile (M x frames), A[i = draw][k] = beta[k][draw] from
// HBM / L2, B[k][j = frame] = the tile in LDS, D[draw = kq + 4 r][frame = lc].  T and the tile's stride come from the largest
// M of the launch; a GP with fewer inducing inputs fills the first M_r rows (rounded up to 16) of each frame's column.
template <int MPAD>
__global__ void __launch_bounds__(256) pdgp_sample_update_kernel(const PsmItem* __restrict__ items, const double* __restrict__ xnew,
                                                                 int n, int S_draws, int T, int S) {
  extern __shared__ double psm_lds[];
  const SpsLds lds = sps_lds_carve<MPAD>(psm_lds);
  const PsmItem it = items[blockIdx.y];
  const int tid = threadIdx.x;
  const int kz = it.M, Mp = (kz + 15) & ~15;
  const int j0 = blockIdx.x * T;
  sps_build_tile<MPAD>(lds, it.k, it.z, it.fz, kz, xnew, n, j0, T, S);

  const int lane = tid & 63, wave = tid >> 6, lc = lane & 15, kq = lane >> 4;
  const double* col = lds.buf + (size_t)(16 * wave + lc) * S;      // this lane's frame: B[k][j = lc] = col[k]
  const double* __restrict__ beta = it.beta;
  const int frame = j0 + 16 * wave + lc;
  for (int d0 = 0; d0 < S_draws; d0 += 16) {
    const int da = d0 + lc;                                        // A[i = lc][k = kq]: draw d0 + lc
    const bool da_on = da < S_draws;
    psm_d4 acc = psm_d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < Mp; k0 += 4) {
      const int k = k0 + kq;
      const double af = (da_on && k < kz) ? beta[(size_t)k * S_draws + da] : 0.0;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af, col[k], acc, 0, 0, 0);
    }
    if (frame < n) {
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int dr = d0 + kq + 4 * r;                            // element r: draw kq + 4 r of this 16-draw block
        if (dr < S_draws) {
          double* o = it.out + (size_t)dr * n + frame;
          *o = *o + acc[r];
        }
      }
    }
  }
}

// ---- 4. src[i][s][t] = nlin(g_i[s][t]) f_i[s][t]; lat = [g_0..g_{P-1}, f_0..f_{P-1}], each [S][n] ----------------------------
__global__ void __launch_bounds__(256) pdgp_sample_source_kernel(const double* __restrict__ lat, double* __restrict__ src,
                                                                 size_t count, int nlin) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= count) return;
  double sg, ds;
  nlin_eval(nlin, lat[e], sg, ds);
  src[e] = sg * lat[count + e];
}

// ---- host ---------------------------------------------------------------------------------------------------------------
struct PsmDescLayout { size_t items, feat, probs, bytes; };
static PsmDescLayout psm_desc_layout(size_t G) {
  PsmDescLayout o;
  GpRegions region;
  o.items = region(G * sizeof(PsmItem));
  o.feat = region(2 * G * sizeof(FeatItem));
  o.probs = region(2 * G * sizeof(GemmProblem));
  o.bytes = region.off;
  return o;
}
// the operator's one carve.  Every per-GP block has the largest GP's size (maxM rows).  Feature tables: an SM kernel of m
// partials takes 2 sm_mpad(m) <= c_r + 6 rows, so C + 6 G rows cover all GPs
struct PsmBufs { char* desc; int* order; double *fx, *fz, *pz, *u0, *rhs, *t1; };
static PsmBufs psm_carve(GpArena& ar, size_t G, size_t maxM, size_t C, size_t n, size_t S) {
  PsmBufs b;
  b.desc = ar.take<char>(psm_desc_layout(G).bytes);
  b.order = ar.take<int>(G * (n + maxM));
  b.fx = ar.take<double>((C + 6 * G) * n);
  b.fz = ar.take<double>((C + 6 * G) * maxM);
  b.pz = ar.take<double>(G * maxM * S);
  b.u0 = ar.take<double>(G * maxM * S);
  b.rhs = ar.take<double>(G * maxM * S);
  b.t1 = ar.take<double>(G * maxM * S);                  // beta
  return b;
}

size_t pdgp_sample_workspace_bytes(int G, int maxM, int C, int n, int S) {
  if (G < 1 || maxM < 1 || C < 1 || n < 1 || S < 1) return 0;
  return gp_measure([&](GpArena& ar) { psm_carve(ar, G, maxM, C, n, S); }) + GP_WS_TAIL_OP;
}

static void psm_totals(const PsmGP* gps, int G, int* maxM, int* C, int* max_mpad) {
  *maxM = 0; *C = 0; *max_mpad = 0;
  for (int r = 0; r < G; r++) {
    if (gps[r].M > *maxM) *maxM = gps[r].M;
    *C += psm_components(gps[r].k.type, gps[r].k.m);
    const int mp = psm_kernel_sm(gps[r].k.type) ? sm_mpad(gps[r].k.m) : 0;
    if (mp > *max_mpad) *max_mpad = mp;
  }
}

gp_status pdgp_sample_check(gp_handle h, const PsmGP* gps, int G, int n, int S, const int32_t* order_host, const void* ws,
                            size_t ws_bytes) {
  if (!gps || !order_host || !ws || G < 2 || (G & 1) || n < 1 || S < 1)
    return gp_fail(h, GP_ERR_BAD_ARG, "Pdgp sampling: bad argument (n >= 1, S >= 1, no null pointers)");
  if (G > 32767) return gp_fail(h, GP_ERR_UNSUPPORTED, "Pdgp sampling: at most 32767 latent GPs per call");
  for (int r = 0; r < G; r++) {
    if (!psm_kernel_ok(gps[r].k.type))
      return gp_fail(h, GP_ERR_UNSUPPORTED,
                     "Pdgp sampling: every latent GP needs a kernel with an exact state-space prior sampler (Matern12, Matern32, "
                     "MercerMatern12sm, Matern12sm)");
    if (psm_kernel_sm(gps[r].k.type) && (gps[r].k.m < 1 || gps[r].k.m > 32))
      return gp_fail(h, GP_ERR_UNSUPPORTED, "Pdgp sampling: num_partials must be in [1, 32]");
    if (gps[r].M < 1) return gp_fail(h, GP_ERR_BAD_ARG, "Pdgp sampling: bad inducing-point count");
    if (gps[r].M > SPS_MAX_M) return gp_fail(h, GP_ERR_UNSUPPORTED, "Pdgp sampling: M <= 1024 inducing points per latent GP");
  }
  int maxM, C, max_mpad;
  psm_totals(gps, G, &maxM, &C, &max_mpad);
  if ((int64_t)n + maxM > INT32_MAX / 2) return gp_fail(h, GP_ERR_UNSUPPORTED, "Pdgp sampling: n too large");
  if ((((uintptr_t)ws) & 255) || ws_bytes < pdgp_sample_workspace_bytes(G, maxM, C, n, S))
    return gp_fail(h, GP_ERR_BAD_ARG, "Pdgp sampling: workspace too small (gp_pdgp_sample_workspace_bytes) or not 256-byte aligned");
  // `order` becomes device addresses: every GP's n + M_r entries must be a permutation of 0..n+M_r-1
  std::vector<char> seen;
  const int32_t* o = order_host;
  for (int r = 0; r < G; r++) {
    const int tot = n + gps[r].M;
    seen.assign(tot, 0);
    for (int j = 0; j < tot; j++) {
      if (o[j] < 0 || o[j] >= tot || seen[o[j]])
        return gp_fail(h, GP_ERR_BAD_ARG, "Pdgp sampling: order is not a permutation of a latent GP's n + M points");
      seen[o[j]] = 1;
    }
    o += tot;
  }
  return GP_OK;
}

template <int MPAD>
static gp_status psm_launch(gp_handle h, const PsmItem* d_items, int G, int maxM, const double* xnew, int n, int S, int which) {
  if (which == 0) {
    hipLaunchKernelGGL((pdgp_sample_prior_kernel<MPAD>), dim3((S + 63) / 64, G), dim3(64), 0, h->stream, d_items, xnew, n, S);
  } else {
    const int T = sps_tile_frames(maxM), Sd = sps_stride(maxM);
    const size_t lds = sps_lds_bytes(maxM, MPAD);
    GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)pdgp_sample_update_kernel<MPAD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds));
    hipLaunchKernelGGL((pdgp_sample_update_kernel<MPAD>), dim3((n + T - 1) / T, G), dim3(4 * T), lds, h->stream, d_items, xnew, n,
                       S, T, Sd);
  }
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}
static gp_status psm_dispatch(gp_handle h, const PsmItem* d_items, int G, int maxM, const double* xnew, int n, int S, int max_mpad,
                              int which) {
  switch (max_mpad <= 4 ? 4 : max_mpad) {
    case 4: return psm_launch<4>(h, d_items, G, maxM, xnew, n, S, which);
    case 8: return psm_launch<8>(h, d_items, G, maxM, xnew, n, S, which);
    case 12: return psm_launch<12>(h, d_items, G, maxM, xnew, n, S, which);
    case 16: return psm_launch<16>(h, d_items, G, maxM, xnew, n, S, which);
    case 20: return psm_launch<20>(h, d_items, G, maxM, xnew, n, S, which);
    case 24: return psm_launch<24>(h, d_items, G, maxM, xnew, n, S, which);
    case 28: return psm_launch<28>(h, d_items, G, maxM, xnew, n, S, which);
    case 32: return psm_launch<32>(h, d_items, G, maxM, xnew, n, S, which);
    default: return gp_fail(h, GP_ERR_UNSUPPORTED, "Pdgp sampling: num_partials must be in [1, 32]");
  }
}

// The arguments have passed pdgp_sample_check and the factorisation of every Kuu is enqueued on h->stream (or done).
gp_status pdgp_sample_run(gp_handle h, const PsmGP* gps, int P, bool whiten, int nlin, double jitter, const double* xnew, int n,
                          int S, const int32_t* order_host, const double* eps_x, const double* eps_z, const double* eps_u,
                          double* latents, double* sources, void* ws, size_t ws_bytes) {
  const int G = 2 * P;
  int maxM, C, max_mpad;
  psm_totals(gps, G, &maxM, &C, &max_mpad);
  GpArena ar(ws, ws_bytes);
  const PsmBufs b = psm_carve(ar, G, maxM, C, n, S);
  if (!ar.ok) return gp_fail(h, GP_ERR_BAD_ARG, "Pdgp sampling: workspace too small");
  const PsmDescLayout lay = psm_desc_layout(G);
  std::vector<char> hd(lay.bytes, 0);
  PsmItem* items = (PsmItem*)(hd.data() + lay.items);
  FeatItem* feats = (FeatItem*)(hd.data() + lay.feat);
  GemmProblem* probs = (GemmProblem*)(hd.data() + lay.probs);
  size_t off_x = 0, off_z = 0, off_u = 0, off_o = 0, frow = 0;
  for (int r = 0; r < G; r++) {
    const PsmGP& g = gps[r];
    const int c = psm_components(g.k.type, g.k.m), M = g.M;
    const int mp = psm_kernel_sm(g.k.type) ? sm_mpad(g.k.m) : 0;
    double* pz = b.pz + (size_t)r * maxM * S;
    double* u0 = b.u0 + (size_t)r * maxM * S;
    double* rhs = b.rhs + (size_t)r * maxM * S;
    double* t1 = b.t1 + (size_t)r * maxM * S;
    PsmItem& it = items[r];
    it.k = g.k; it.z = g.z;
    it.fx = mp ? b.fx + frow * n : nullptr;
    it.fz = mp ? b.fz + frow * maxM : nullptr;
    it.order = b.order + off_o;
    it.eps_x = eps_x + off_x; it.eps_z = eps_z + off_z; it.eps_u = eps_u + off_u;
    it.q_mu = g.q_mu; it.q_sqrt = g.q_sqrt;
    it.beta = t1;
    it.out = latents + (size_t)r * S * n;
    it.pz = pz; it.u0 = u0; it.rhs = rhs;
    it.M = M; it.c = c; it.mp = mp;
    off_x += (size_t)S * c * n; off_z += (size_t)S * c * M; off_u += (size_t)S * 2 * M; off_o += (size_t)n + M;
    frow += 2 * (size_t)mp;
    // [M][S] row-major.  whitened: rhs <- rhs - W u0, beta = W^T rhs;  unwhitened (rhs holds q - u0): u0 <- W rhs, beta = W^T u0
    GemmProblem p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = S; p.K = M; p.lda = M; p.ldb = S; p.ldc = S; p.A = g.W;
    p.B = whiten ? u0 : rhs; p.C = whiten ? rhs : u0; probs[r] = p;
    p.B = whiten ? rhs : u0; p.C = t1; probs[(size_t)G + r] = p;
  }
  // feature items grouped by table padding: one launch of the shared feature kernel per distinct sm_mpad
  int nfeat = 0, feat_first[9] = {0}, feat_count[9] = {0};
  for (int q = 1; q <= 8; q++) {
    feat_first[q] = nfeat;
    for (int r = 0; r < G; r++)
      if (items[r].mp == 4 * q) {
        feats[nfeat++] = FeatItem{gps[r].k, xnew, (double*)items[r].fx, n, 0};
        feats[nfeat++] = FeatItem{gps[r].k, gps[r].z, (double*)items[r].fz, gps[r].M, 0};
      }
    feat_count[q] = nfeat - feat_first[q];
  }
  GP_HIP_CHECK(h, hipMemcpyAsync(b.desc, hd.data(), lay.bytes, hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(b.order, order_host, off_o * sizeof(int), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));       // hd is a stack object
  const PsmItem* d_items = (const PsmItem*)(b.desc + lay.items);
  const FeatItem* d_feats = (const FeatItem*)(b.desc + lay.feat);
  const GemmProblem* d_probs = (const GemmProblem*)(b.desc + lay.probs);
  for (int q = 1; q <= 8; q++)
    GP_CHECK(launch_sm_features_items(h, d_feats + feat_first[q], feat_count[q], n > maxM ? n : maxM, 4 * q, nullptr, 0));
  GP_CHECK(psm_dispatch(h, d_items, G, maxM, xnew, n, S, max_mpad, 0));
  hipLaunchKernelGGL(pdgp_sample_u0_kernel, dim3((unsigned)(((size_t)maxM * S + 255) / 256), G), dim3(256), 0, h->stream, d_items, S,
                     sqrt(jitter), whiten ? 1 : 0);
  GP_HIP_CHECK(h, hipGetLastError());
  { GemmFlags f; f.triA = TRI_LOWER;
    if (whiten) { f.alpha = -1.0; f.beta = 1.0; }
    GP_CHECK(launch_gemm_batched(h, d_probs, G, maxM, S, f)); }
  { GemmFlags f; f.transA = 1; f.triA = TRI_UPPER;
    GP_CHECK(launch_gemm_batched(h, d_probs + G, G, maxM, S, f)); }
  {
    GpTimerScope ts(h, GP_TIMER_COND_A);
    GP_CHECK(psm_dispatch(h, d_items, G, maxM, xnew, n, S, max_mpad, 1));
  }
  if (sources) {
    const size_t count = (size_t)P * S * n;
    hipLaunchKernelGGL(pdgp_sample_source_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, latents, sources,
                       count, nlin);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  return GP_OK;
}
