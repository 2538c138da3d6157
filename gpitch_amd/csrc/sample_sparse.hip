// sample_sparse.hip — joint posterior draws of every source of an SGPRSS window under the optimal q(u) of the collapsed
// bound, by Matheron's rule (gfx950, float64 throughout).  No n x n matrix is formed: O((n + M) m + M n) per source and draw.
//
// State: W = L^-1, WB = LB^-1 and c of the plan's forward pass (sgpr_ss.py:43-53), as predict_sparse.hip reads them.  Every
// supported source kernel has a Matern-1/2 envelope, so its prior is a sum of Ornstein-Uhlenbeck processes and has an exact
// first-order sampler along sorted time:
//   MercerMatern12sm / Matern12sm:  f_p(t) = sum_k sqrt(e_k) [a_k(t) cos 2 pi f_k t + b_k(t) sin 2 pi f_k t],
//                                   a_k, b_k independent OU(variance v_p, lengthscale l_p)       (2 m_p components)
//   Matern12:                       f_p = one OU process                                         (1 component)
// Per window and draw s, with t = (Xnew | Z) walked in the caller's stable ascending `order`:
//   1. prior path    s_(1) = sqrt(v) eps_(1);  s_(j) = exp(-D_j / l) s_(j-1) + sqrt(v (-expm1(-2 D_j / l))) eps_(j),
//                    D_j = t_(j) - t_(j-1) >= 0 (the expm1 form is exact at D = 0: a frame on an inducing input repeats it);
//                    prior_p(x*) goes to the output, prior_p(Z) to the workspace          (sgpr_sample_prior_kernel)
//   2. inducing side u0 = sum_p prior_p(Z) + sqrt(jitter) eps_u[0]   (Kuu carries the jitter, so the draw of u does too)
//                    beta = W^T (WB^T (c + eps_u[1]) - W u0)          (sgpr_sample_u0_kernel, three batched small GEMMs)
//   3. update        sample_p(x*) = prior_p(x*) + K_p(x*, Z) beta     (sgpr_sample_update_kernel: the K_p(Z, tile) build of
//                    the sparse predictor in LDS (sps_tile.h), then the float64 MFMA; no M x n array reaches HBM)
// The map is affine in eps; with eps = 0 it is predict_sparse.hip's mean, and its linear part T has T T^T = the joint
// posterior covariance of (f_1*, ..., f_P*) under q(u).
// eps layout per window (caller's point order, so it does not depend on the merge): eps_x [S][C][n], eps_z [S][C][M],
// eps_u [S][2][M], C = sum_p components_p with the sources' blocks in kern_list order.  A ragged slot with k < M inducing
// points is its own k-point problem: rows >= k of eps_z, eps_u, Z, W and WB are never read.
// Determinism: no atomics; every sum has a fixed order; draw s depends on nothing but its own eps (a thread owns a draw in
// step 1, a GEMM / MFMA column in steps 2 and 3), so it is bit-identical whatever S and whatever else shares the launch.
#include <cstring>
#include <vector>

#include "common.h"
#include "cov_entry.h"
#include "sps_tile.h"

typedef double smp_d4 __attribute__((ext_vector_type(4)));

// one per (source, window), kernel-major [P][nwin] as SrcSparseItem
struct SmpItem {
  DevKern k;
  const double* z; const double* xnew;
  const double* fz; const double* fx;     // sqrt(e) cos / sin tables of z ([2 mpz][kz]) and of xnew ([2 mpx][n]); SM kernels only
  const int* order;                       // the window's merged order, n + kz entries (validated on the host)
  const double* eps_x; const double* eps_z; const double* eps_u; const double* c;   // the window's blocks
  const double* beta;                     // [kz][S]
  double* out;                            // [S][n] of this (window, source)
  double* pz;                             // prior_p(Z): [kz][S]
  double* u0; double* rhs;                // [kz][S] each (the window's)
  int kz, coff, mpz, mpx;                 // coff: first component of this source among the window's C
};

static inline int smp_components(int type, int m) { return type == GP_KERN_MATERN12 ? 1 : 2 * m; }
static inline bool smp_kernel_ok(int type) {
  return type == GP_KERN_MATERN12 || type == GP_KERN_MERCER_MATERN12SM || type == GP_KERN_MATERN12SM;
}

// ---- 1. prior paths: one thread per (draw, source, window), the 2 m states in registers --------------------------------
template <int MPAD>
__global__ void __launch_bounds__(64) sgpr_sample_prior_kernel(const SmpItem* __restrict__ items, int nwin, int n, int M, int C,
                                                               int S) {
  const SmpItem it = items[(size_t)blockIdx.y * nwin + blockIdx.z];
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const int m = it.k.m, kz = it.kz;
  const bool sm = it.k.type != GP_KERN_MATERN12;
  const double var = it.k.theta[0], ls = it.k.theta[1];
  const double sv = sqrt(var);
  const double* __restrict__ ex = it.eps_x + ((size_t)s * C + it.coff) * n;
  const double* __restrict__ ez = it.eps_z + ((size_t)s * C + it.coff) * M;
  double a[MPAD], b[MPAD];
#pragma unroll
  for (int q = 0; q < MPAD; q++) { a[q] = 0.0; b[q] = 0.0; }
  double tprev = 0.0;
  const int tot = n + kz;
  for (int j = 0; j < tot; j++) {
    const int idx = it.order[j];
    const bool isz = idx >= n;
    const int i = isz ? idx - n : idx;
    const double t = isz ? it.z[i] : it.xnew[i];
    double phi = 0.0, sc = sv;                            // the first point: a draw from the stationary law
    if (j > 0) {
      const double d = (t - tprev) / ls;
      phi = exp(-d);
      sc = sqrt(var * (-expm1(-2.0 * d)));
    }
    tprev = t;
    const double* __restrict__ e = isz ? ez + i : ex + i;
    const size_t es = isz ? (size_t)M : (size_t)n;        // stride between the components of one point
    double acc;
    if (!sm) {
      a[0] = fma(phi, a[0], sc * e[0]);
      acc = a[0];
    } else {
      const double* __restrict__ f = isz ? it.fz : it.fx;
      const size_t fn = isz ? (size_t)kz : (size_t)n, so = (size_t)(isz ? it.mpz : it.mpx) * fn;
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
    if (isz) it.pz[(size_t)i * S + s] = acc;
    else it.out[(size_t)s * n + i] = acc;
  }
}

// ---- 2. u0 = sum_p prior_p(Z) + sqrt(jitter) eps_u[0] (sources in kern_list order), rhs = c + eps_u[1]; grid (blocks, window) ----
__global__ void __launch_bounds__(256) sgpr_sample_u0_kernel(const SmpItem* __restrict__ items, int nwin, int P, int M, int S,
                                                             double sqrt_jitter) {
  const int w = blockIdx.y;
  const SmpItem it = items[w];
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int i = e / S, s = e % S;
  if (i >= it.kz) return;
  double u = items[w].pz[(size_t)i * S + s];
  for (int p = 1; p < P; p++) u += items[(size_t)p * nwin + w].pz[(size_t)i * S + s];
  const double* __restrict__ eu = it.eps_u + (size_t)s * 2 * M;
  it.u0[(size_t)i * S + s] = u + sqrt_jitter * eu[i];
  it.rhs[(size_t)i * S + s] = it.c[i] + eu[M + i];
}

// ---- 3. out[s][frame] += sum_i K_p(z_i, x*_frame) beta[i][s]: one workgroup per (frame tile, source, window) -----------------
// After the tile build a wavefront owns 16 frames.  The product is taken as beta^T (S x M) times the tile (M x frames) so
// that the 16 lanes of a result row hold 16 consecutive frames of one draw: A[i = draw][k] = beta[k][draw] from HBM / L2,
// B[k][j = frame] = the tile in LDS (the sparse predictor's own read pattern), D[draw = kq + 4 r][frame = lc].  S is padded
// to 16 here only: pad columns of beta are not read and pad draws not written.
template <int MPAD>
__global__ void __launch_bounds__(256) sgpr_sample_update_kernel(const SmpItem* __restrict__ items, int nwin, int n, int S_draws,
                                                                 int T, int S) {
  extern __shared__ double smp_lds[];
  const SpsLds lds = sps_lds_carve<MPAD>(smp_lds);
  const SmpItem it = items[(size_t)blockIdx.y * nwin + blockIdx.z];
  const int tid = threadIdx.x;
  const int kz = it.kz, Mp = (kz + 15) & ~15;
  const int j0 = blockIdx.x * T;
  sps_build_tile<MPAD>(lds, it.k, it.z, it.fz, kz, it.xnew, n, j0, T, S);

  const int lane = tid & 63, wave = tid >> 6, lc = lane & 15, kq = lane >> 4;
  const double* col = lds.buf + (size_t)(16 * wave + lc) * S;      // this lane's frame: B[k][j = lc] = col[k]
  const double* __restrict__ beta = it.beta;
  const int frame = j0 + 16 * wave + lc;
  for (int d0 = 0; d0 < S_draws; d0 += 16) {
    const int da = d0 + lc;                                        // A[i = lc][k = kq]: draw d0 + lc
    const bool da_on = da < S_draws;
    smp_d4 acc = smp_d4{0.0, 0.0, 0.0, 0.0};
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

// ---- host ---------------------------------------------------------------------------------------------------------------
struct SmpDescLayout { size_t items, feat, probs, bytes; };
static SmpDescLayout smp_desc_layout(size_t count, size_t P) {
  SmpDescLayout o;
  GpRegions region;
  o.items = region(count * P * sizeof(SmpItem));
  o.feat = region(2 * count * P * sizeof(FeatItem));
  o.probs = region(3 * count * sizeof(GemmProblem));
  o.bytes = region.off;
  return o;
}
// the operator's one carve.  Feature tables: source p takes 2 sm_mpad(m_p) <= components_p + 6 rows, so (C + 6 P) rows per window
struct SmpBufs { char* desc; int* order; double *fx, *fzb, *pz, *u0, *rhs, *t1; };
static SmpBufs smp_carve(GpArena& ar, size_t M, size_t P, size_t C, size_t n, size_t S, size_t count) {
  SmpBufs b;
  b.desc = ar.take<char>(smp_desc_layout(count, P).bytes);
  b.order = ar.take<int>(count * (n + M));
  b.fx = ar.take<double>(count * (C + 6 * P) * n);       // features of Xnew, once per (window, source)
  b.fzb = ar.take<double>(count * (C + 6 * P) * M);      // features of Z for the kernels whose table the plan does not keep
  b.pz = ar.take<double>(count * P * M * S);
  b.u0 = ar.take<double>(count * M * S);                 // u0, then beta
  b.rhs = ar.take<double>(count * M * S);
  b.t1 = ar.take<double>(count * M * S);
  return b;
}

size_t sgpr_sample_workspace_bytes(int M, int P, int C, int n, int S, int count) {
  if (M < 1 || P < 1 || C < 1 || n < 1 || S < 1 || count < 1) return 0;
  return gp_measure([&](GpArena& ar) { smp_carve(ar, M, P, C, n, S, count); }) + GP_WS_TAIL_OP;
}

gp_status sgpr_sample_check(gp_handle h, const int* ktype, const int* km, int P, int M, const int* kw, int count, int n, int S,
                            const int32_t* order_host, const void* ws, size_t ws_bytes, int* C_out) {
  if (!ktype || !km || !order_host || !ws || P < 1 || count < 1 || n < 1 || S < 1 || M < 1)
    return gp_fail(h, GP_ERR_BAD_ARG, "sparse source sampling: bad argument (n >= 1, S >= 1, no null pointers)");
  if (M > SPS_MAX_M) return gp_fail(h, GP_ERR_UNSUPPORTED, "sparse source sampling: M <= 1024 inducing points");
  if ((int64_t)P * count * 2 > 65535)         // (window, source) pairs index a launch grid, twice over for the feature tables
    return gp_fail(h, GP_ERR_UNSUPPORTED, "sparse source sampling: at most 32767 (window, source) pairs per call");
  int C = 0;
  for (int i = 0; i < P; i++) {
    if (!smp_kernel_ok(ktype[i]))
      return gp_fail(h, GP_ERR_UNSUPPORTED,
                     "sparse source sampling: every kernel of the sum must have a Matern-1/2 envelope (MercerMatern12sm, "
                     "Matern12sm, Matern12)");
    if (ktype[i] != GP_KERN_MATERN12 && (km[i] < 1 || km[i] > 32))
      return gp_fail(h, GP_ERR_UNSUPPORTED, "sparse source sampling: num_partials must be in [1, 32]");
    C += smp_components(ktype[i], km[i]);
  }
  if ((int64_t)n + M > INT32_MAX / 2) return gp_fail(h, GP_ERR_UNSUPPORTED, "sparse source sampling: n too large");
  if ((((uintptr_t)ws) & 255) || ws_bytes < sgpr_sample_workspace_bytes(M, P, C, n, S, count))
    return gp_fail(h, GP_ERR_BAD_ARG, "sparse source sampling: workspace too small (gp_sgpr_sample_source_workspace_bytes) or not "
                                      "256-byte aligned");
  // `order` becomes device addresses: every slot's first n + k entries must be a permutation of 0..n+k-1
  std::vector<char> seen;
  for (int w = 0; w < count; w++) {
    const int k = kw ? kw[w] : M;
    if (k < 1 || k > M) return gp_fail(h, GP_ERR_BAD_ARG, "sparse source sampling: bad inducing-point count");
    const int tot = n + k;
    const int32_t* o = order_host + (size_t)w * (n + M);
    seen.assign(tot, 0);
    for (int j = 0; j < tot; j++) {
      if (o[j] < 0 || o[j] >= tot || seen[o[j]])
        return gp_fail(h, GP_ERR_BAD_ARG, "sparse source sampling: order is not a permutation of the window's n + k points");
      seen[o[j]] = 1;
    }
  }
  if (C_out) *C_out = C;
  return GP_OK;
}

template <int MPAD>
static gp_status smp_launch(gp_handle h, const SmpItem* d_items, int P, int nwin, int M, int n, int C, int S, int which) {
  if (which == 0) {
    hipLaunchKernelGGL((sgpr_sample_prior_kernel<MPAD>), dim3((S + 63) / 64, P, nwin), dim3(64), 0, h->stream, d_items, nwin, n, M,
                       C, S);
  } else {
    const int T = sps_tile_frames(M), Sd = sps_stride(M);
    const size_t lds = sps_lds_bytes(M, MPAD);
    GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)sgpr_sample_update_kernel<MPAD>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds));
    hipLaunchKernelGGL((sgpr_sample_update_kernel<MPAD>), dim3((n + T - 1) / T, P, nwin), dim3(4 * T), lds, h->stream, d_items,
                       nwin, n, S, T, Sd);
  }
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}
static gp_status smp_dispatch(gp_handle h, const SmpItem* d_items, int P, int nwin, int M, int n, int C, int S, int max_mpad,
                              int which) {
  switch (max_mpad <= 4 ? 4 : max_mpad) {
    case 4: return smp_launch<4>(h, d_items, P, nwin, M, n, C, S, which);
    case 8: return smp_launch<8>(h, d_items, P, nwin, M, n, C, S, which);
    case 12: return smp_launch<12>(h, d_items, P, nwin, M, n, C, S, which);
    case 16: return smp_launch<16>(h, d_items, P, nwin, M, n, C, S, which);
    case 20: return smp_launch<20>(h, d_items, P, nwin, M, n, C, S, which);
    case 24: return smp_launch<24>(h, d_items, P, nwin, M, n, C, S, which);
    case 28: return smp_launch<28>(h, d_items, P, nwin, M, n, C, S, which);
    case 32: return smp_launch<32>(h, d_items, P, nwin, M, n, C, S, which);
    default: return gp_fail(h, GP_ERR_UNSUPPORTED, "sparse source sampling: num_partials must be in [1, 32]");
  }
}

// The arguments have passed sgpr_sample_check and the windows' forward state is enqueued on h->stream.
// win: [count]; src: [count][P]; order_host: [count][n + M]; eps_x [count][S][C][n], eps_z [count][S][C][M],
// eps_u [count][S][2][M]; out [count][P][S][n].
gp_status sgpr_sample_run(gp_handle h, const SmpWindow* win, const SmpSource* src, int count, int P, int M, int ldw, int n, int S,
                          double jitter, const int32_t* order_host, const double* eps_x, const double* eps_z, const double* eps_u,
                          double* out, void* ws, size_t ws_bytes) {
  int C = 0, max_mpad = 0;
  std::vector<int> coff(P), mpad(P);
  for (int i = 0; i < P; i++) {
    coff[i] = C;
    C += smp_components(src[i].k.type, src[i].k.m);
    mpad[i] = src[i].k.type == GP_KERN_MATERN12 ? 0 : sm_mpad(src[i].k.m);
    if (mpad[i] > max_mpad) max_mpad = mpad[i];
  }
  GpArena ar(ws, ws_bytes);
  const SmpBufs b = smp_carve(ar, M, P, C, n, S, count);
  if (!ar.ok) return gp_fail(h, GP_ERR_BAD_ARG, "sparse source sampling: workspace too small");
  const SmpDescLayout lay = smp_desc_layout(count, P);
  std::vector<char> hd(lay.bytes, 0);
  SmpItem* items = (SmpItem*)(hd.data() + lay.items);
  FeatItem* feats = (FeatItem*)(hd.data() + lay.feat);
  GemmProblem* probs = (GemmProblem*)(hd.data() + lay.probs);
  // feature items grouped by table padding: one launch of the shared feature kernel per distinct sm_mpad
  int nfeat = 0, feat_first[9] = {0}, feat_count[9] = {0};
  const size_t frows = (size_t)C + 6 * (size_t)P;
  std::vector<const double*> fx((size_t)count * P, nullptr), fz((size_t)count * P, nullptr);
  for (int g = 1; g <= 8; g++) {
    feat_first[g] = nfeat;
    for (int w = 0; w < count; w++) {
      size_t row = 0;
      for (int i = 0; i < P; i++) {
        if (mpad[i] == 4 * g) {
          const SmpSource& sc = src[(size_t)w * P + i];
          double* tx = b.fx + ((size_t)w * frows + row) * n;
          feats[nfeat++] = FeatItem{sc.k, win[w].xnew, tx, n, 0};
          fx[(size_t)w * P + i] = tx;
          if (sc.fz) fz[(size_t)w * P + i] = sc.fz;
          else {
            double* tz = b.fzb + ((size_t)w * frows + row) * M;   // (kz <= M values per row are written)
            feats[nfeat++] = FeatItem{sc.k, win[w].z, tz, win[w].kz, 0};
            fz[(size_t)w * P + i] = tz;
          }
        }
        row += 2 * (size_t)mpad[i];
      }
    }
    feat_count[g] = nfeat - feat_first[g];
  }
  for (int w = 0; w < count; w++) {
    const SmpWindow& sw = win[w];
    double* u0 = b.u0 + (size_t)w * M * S;
    double* rhs = b.rhs + (size_t)w * M * S;
    double* t1 = b.t1 + (size_t)w * M * S;
    for (int i = 0; i < P; i++) {
      SmpItem& it = items[(size_t)i * count + w];
      it.k = src[(size_t)w * P + i].k; it.z = sw.z; it.xnew = sw.xnew;
      it.fz = fz[(size_t)w * P + i]; it.fx = fx[(size_t)w * P + i];
      it.order = b.order + (size_t)w * (n + M);
      it.eps_x = eps_x + (size_t)w * S * C * n; it.eps_z = eps_z + (size_t)w * S * C * M; it.eps_u = eps_u + (size_t)w * S * 2 * M;
      it.c = sw.c; it.beta = u0;
      it.out = out + ((size_t)w * P + i) * S * n;
      it.pz = b.pz + ((size_t)w * P + i) * M * S;
      it.u0 = u0; it.rhs = rhs;
      it.kz = sw.kz; it.coff = coff[i]; it.mpz = mpad[i]; it.mpx = mpad[i];
    }
    // t1 = W u0;  t1 = WB^T rhs - t1;  beta (over u0) = W^T t1     — [kz][S] row-major, the slot's own kz-point problem
    GemmProblem g;
    memset(&g, 0, sizeof(g));
    g.M = sw.kz; g.N = S; g.K = sw.kz; g.lda = ldw; g.ldb = S; g.ldc = S;
    g.A = sw.W; g.B = u0; g.C = t1; probs[0 * (size_t)count + w] = g;
    g.A = sw.WB; g.B = rhs; g.C = t1; probs[1 * (size_t)count + w] = g;
    g.A = sw.W; g.B = t1; g.C = u0; probs[2 * (size_t)count + w] = g;
  }
  GP_HIP_CHECK(h, hipMemcpyAsync(b.desc, hd.data(), lay.bytes, hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(b.order, order_host, (size_t)count * (n + M) * sizeof(int), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));       // hd is a stack object
  const SmpItem* d_items = (const SmpItem*)(b.desc + lay.items);
  const FeatItem* d_feats = (const FeatItem*)(b.desc + lay.feat);
  const GemmProblem* d_probs = (const GemmProblem*)(b.desc + lay.probs);
  for (int g = 1; g <= 8; g++)
    GP_CHECK(launch_sm_features_items(h, d_feats + feat_first[g], feat_count[g], n > M ? n : M, 4 * g, nullptr, 0));
  GP_CHECK(smp_dispatch(h, d_items, P, count, M, n, C, S, max_mpad, 0));
  hipLaunchKernelGGL(sgpr_sample_u0_kernel, dim3((unsigned)(((size_t)M * S + 255) / 256), count), dim3(256), 0, h->stream, d_items, count, P, M,
                     S, sqrt(jitter));
  GP_HIP_CHECK(h, hipGetLastError());
  { GemmFlags f; f.triA = TRI_LOWER;
    GP_CHECK(launch_gemm_batched(h, d_probs, count, M, S, f)); }
  { GemmFlags f; f.transA = 1; f.triA = TRI_UPPER; f.beta = -1.0;
    GP_CHECK(launch_gemm_batched(h, d_probs + count, count, M, S, f)); }
  { GemmFlags f; f.transA = 1; f.triA = TRI_UPPER;
    GP_CHECK(launch_gemm_batched(h, d_probs + 2 * (size_t)count, count, M, S, f)); }
  GpTimerScope ts(h, GP_TIMER_COND_A);
  return smp_dispatch(h, d_items, P, count, M, n, C, S, max_mpad, 1);
}
