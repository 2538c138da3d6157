// sample.hip — joint posterior draws by Matheron's rule (gfx950, float64 throughout) for the two models with a sparse
// variational posterior: every source of an SGPRSS window under the optimal q(u) of the collapsed bound, and every latent GP
// and source nlin(g_i) f_i of a Pdgp model under its q.  No n x n matrix is formed and nothing M x n reaches HBM:
// O((n + M) c + M n) per sampled process and draw, c its normals per point.
//
// A sampled process is one GP with inducing inputs z (kz of them), new frames x* (n) and a kernel with an exact state-space
// prior sampler; t = (x* | z) is walked in the caller's stable ascending `order`.  Per process and draw s (the core):
//   1. prior path (ssm_prior_kernel: one thread per (draw, process), D_j = t_(j) - t_(j-1) >= 0)
//        Matern12:                      one Ornstein-Uhlenbeck process                                  (1 normal per point)
//          s_(1) = sqrt(v) eps_(1);  s_(j) = exp(-D_j / l) s_(j-1) + sqrt(v (-expm1(-2 D_j / l))) eps_(j)
//          (the expm1 form is exact at D = 0: a frame on an inducing input repeats its value)
//        MercerMatern12sm / Matern12sm: f(t) = sum_k sqrt(e_k) [a_k(t) cos 2 pi f_k t + b_k(t) sin 2 pi f_k t],
//          a_k, b_k independent OU(variance v, lengthscale l)                                            (2 m normals)
//        Matern32: the two-state recursion on (f, f'), lambda = sqrt(3) / l, a = lambda D, x = 2 a        (2 normals)
//          start       f = sqrt(v) e0, f' = lambda sqrt(v) e1
//          transition  (f, f') <- exp(-a) [[1 + a, D], [-lambda^2 D, 1 - a]] (f, f') + chol(Q) (e0, e1)
//          Q = Pinf - Phi Pinf Phi^T, Pinf = diag(v, lambda^2 v), written without cancellation through
//            g(x) = 1 - exp(-x)(1 + x + x^2 / 2) = exp(-x) sum_{k >= 3} x^k / k!      (the series below x = 1: g is O(x^3)
//                                                                                       and audio-rate steps have x ~ 1e-4)
//            Q11 = v g,   Q12 = v lambda exp(-x) x^2 / 2,   Q22 = v lambda^2 (g + 2 x exp(-x))
//          At D = 0 the transition is the identity and Q = 0 exactly.
//      prior(x*) goes to the output, prior(z) to the workspace.
//   2. inducing side: the operator's own u0 kernel and batched small GEMMs leave beta [kz][S] (below)
//   3. update   draw(x*) = prior(x*) + K(x*, z) beta   (ssm_update_kernel, one workgroup per (process, frame tile) entry:
//      the K(Z, tile) build of the sparse predictor in LDS (sps_tile.h), then the float64 MFMA)
// The map is affine in eps and its linear part T has T T^T = the joint posterior covariance under q.
//
// SGPRSS (sgpr_sample_*): a process is a (source, window) pair.  State: W = L^-1, WB = LB^-1 and c of the plan's forward
// pass (sgpr_ss.py:43-53), as predict_sparse.hip reads them.  Matern32 is refused: the collapsed bound's kernels all have a
// Matern-1/2 envelope.
//        u0 = sum_p prior_p(Z) + sqrt(jitter) eps_u[0]   (Kuu carries the jitter, so the draw of u does too; sources in
//        kern_list order), beta = W^T (WB^T (c + eps_u[1]) - W u0)       (sgpr_sample_u0_kernel, three batched small GEMMs)
//   With eps = 0 the draw is predict_sparse.hip's mean.  eps layout per window (caller's point order, so it does not depend
//   on the merge): eps_x [S][C][n], eps_z [S][C][M], eps_u [S][2][M], C = sum_p components_p with the sources' blocks in
//   kern_list order.  A ragged slot with k < M inducing points is its own k-point problem: rows >= k of eps_z, eps_u, Z, W
//   and WB are never read.
// Pdgp (pdgp_sample_*): a process is a latent GP r, independent of the others under q, with its own z_r (M_r of them) and
//   its own merge.  State: W_r = chol(Kuu_r + jitter I)^-1 as the plan's prediction leaves it (CondTask::W), q_mu_r, q_sqrt_r.
//        u0 = prior(z_r) + sqrt(jitter) eps_u[0]
//        whitened:    beta = W^T (q_mu + tril(q_sqrt) eps_u[1] - W u0)
//        unwhitened:  beta = W^T W (q_mu + tril(q_sqrt) eps_u[1] - u0)   (pdgp_sample_u0_kernel, two batched small GEMMs)
//   4. sources  src_i = nlin(draw_i) * draw_{P + i}                      (pdgp_sample_source_kernel)
//   eps layout: the GPs' blocks back to back, GP r's being eps_x [S][c_r][n], eps_z [S][c_r][M_r], eps_u [S][2][M_r], in the
//   caller's own point order.
// Many Pdgp models (pdgp_batch.hip, gp_pdgpb_sample): every latent GP of every model with frames is a process of this core with
//   its own frame count (SsmProc::n); the update's grid is the list of (process, frame tile) entries, so ragged models share
//   its launch.  Steps 2 and 4 are that file's own kernels, on the G^T blocks its predict-only plan prepared.
// Determinism: no atomics; every sum has a fixed order; draw s depends on nothing but its own eps (a thread owns a draw in
// step 1 and in Pdgp's u0 kernel, a GEMM / MFMA column in steps 2 and 3), so it is bit-identical whatever S and whatever
// else shares the launch.
#include <algorithm>
#include <cstring>
#include <vector>

#include "common.h"
#include "cov_entry.h"
#include "gh_quad.h"
#include "sps_tile.h"

// ==== core: the state-space sampler of one process =======================================================================
typedef double ssm_d4 __attribute__((ext_vector_type(4)));

// (SsmProc, one per sampled process, is in common.h: pdgp_batch.hip builds the same records)

__host__ __device__ static inline bool ssm_kernel_sm(int type) { return type == GP_KERN_MERCER_MATERN12SM || type == GP_KERN_MATERN12SM; }
int ssm_components(int type, int m) { return type == GP_KERN_MATERN12 ? 1 : (type == GP_KERN_MATERN32 ? 2 : 2 * m); }
int ssm_mpad(DevKern k) { return ssm_kernel_sm(k.type) ? sm_mpad(k.m) : 0; }

// g(x) = 1 - exp(-x)(1 + x + x^2 / 2) for x >= 0, e2 = exp(-x).  Below x = 1: exp(-x) x^3 / 6 (1 + x/4 (1 + x/5 (... (1 + x/20))))
// (the tail beyond k = 20 is below 3e-18 of the sum); from 1 on the closed form loses at most four bits.
__device__ __forceinline__ double psm_m32_g(double x, double e2) {
  if (x >= 1.0) return 1.0 - e2 * (1.0 + x + 0.5 * x * x);
  double r = 1.0;
#pragma unroll
  for (int k = 20; k >= 4; k--) r = fma(x * (1.0 / (double)k), r, 1.0);
  return e2 * (x * x * x) * (1.0 / 6.0) * r;
}

// ---- 1. prior paths: one thread per (draw, process), the states in registers --------------------------------------------
// (fmax clamps a descending step to D = 0; with the ascending `order` both callers document it changes nothing)
// (the walk is compiled once per family, M32 = the two-state step or not: one loop that held both kept the Matern-3/2
// step's registers live across the partials' and cost the Matern-1/2 families a wavefront of occupancy at MPAD 4)
template <int MPAD, bool M32>
__device__ __forceinline__ void ssm_prior_walk(const SsmProc& it, int S, int s) {
  const int m = it.k.m, kz = it.kz, n = it.n;
  const bool sm = ssm_kernel_sm(it.k.type);
  const double var = it.k.theta[0], ls = it.k.theta[1];
  const double sv = sqrt(var);
  const double lam = 1.7320508075688772 / ls;
  const double* __restrict__ ex = it.eps_x + (size_t)s * it.cs * n;
  const double* __restrict__ ez = it.eps_z + (size_t)s * it.cs * it.ezs;
  double a[M32 ? 1 : MPAD], b[M32 ? 1 : MPAD];      // OU states of the partials; Matern32: a[0] = f, b[0] = f'
#pragma unroll
  for (int q = 0; q < (M32 ? 1 : MPAD); q++) { a[q] = 0.0; b[q] = 0.0; }
  double tprev = 0.0;
  const int tot = n + kz;
  for (int j = 0; j < tot; j++) {
    const int idx = it.order[j];
    const bool isz = idx >= n;
    const int i = isz ? idx - n : idx;
    const double t = isz ? it.z[i] : it.xnew[i];
    const double dt = (j > 0) ? fmax(t - tprev, 0.0) : 0.0;
    tprev = t;
    const double* __restrict__ e = isz ? ez + i : ex + i;
    const size_t es = isz ? (size_t)it.ezs : (size_t)n;   // stride between the normals of one point
    double acc;
    if constexpr (M32) {
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
        const size_t fn = isz ? (size_t)kz : (size_t)n, so = (size_t)it.mp * fn;
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
template <int MPAD>
__global__ void __launch_bounds__(64) ssm_prior_kernel(const SsmProc* __restrict__ procs, int S) {
  const SsmProc it = procs[blockIdx.y];
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  if (it.k.type == GP_KERN_MATERN32) ssm_prior_walk<MPAD, true>(it, S, s);
  else ssm_prior_walk<MPAD, false>(it, S, s);
}

// ---- 3. out[s][frame] += sum_i K(z_i, x*_frame) beta[i][s]: one workgroup per (frame tile, process) -------------------------
// After the tile build a wavefront owns 16 frames.  The product is taken as beta^T (S x M) times the tile (M x frames) so
// that the 16 lanes of a result row hold 16 consecutive frames of one draw: A[i = draw][k] = beta[k][draw] from HBM / L2,
// B[k][j = frame] = the tile in LDS (the sparse predictor's own read pattern), D[draw = kq + 4 r][frame = lc].  S is padded
// to 16 here only: pad columns of beta are not read and pad draws not written.  T and the tile's stride come from the largest
// M of the launch; a process with fewer inducing inputs fills the first kz rows (rounded up to 16) of each frame's column.
// The grid is the list of (process, frame tile) entries, process-major: tile_start[p] is process p's first entry (count + 1
// items), so processes with different frame counts share the launch without a rectangle over the longest.
template <int MPAD>
__global__ void __launch_bounds__(256) ssm_update_kernel(const SsmProc* __restrict__ procs, const int64_t* __restrict__ tile_start,
                                                         int count, int S_draws, int T, int S) {
  extern __shared__ double ssm_lds[];
  const SpsLds lds = sps_lds_carve<MPAD>(ssm_lds);
  const int64_t b = blockIdx.x;
  const int pi = gp_entry_owner(tile_start, count, b);
  const SsmProc it = procs[pi];
  const int tid = threadIdx.x;
  const int kz = it.kz, Mp = (kz + 15) & ~15, n = it.n;
  const int j0 = (int)(b - tile_start[pi]) * T;
  sps_build_tile<MPAD>(lds, it.k, it.z, it.fz, kz, it.xnew, n, j0, T, S);

  const int lane = tid & 63, wave = tid >> 6, lc = lane & 15, kq = lane >> 4;
  const double* col = lds.buf + (size_t)(16 * wave + lc) * S;      // this lane's frame: B[k][j = lc] = col[k]
  const double* __restrict__ beta = it.beta;
  const int frame = j0 + 16 * wave + lc;
  for (int d0 = 0; d0 < S_draws; d0 += 16) {
    const int da = d0 + lc;                                        // A[i = lc][k = kq]: draw d0 + lc
    const bool da_on = da < S_draws;
    ssm_d4 acc = ssm_d4{0.0, 0.0, 0.0, 0.0};
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

// ---- core, host side ------------------------------------------------------------------------------------------------------
// d_procs: count <= 32767 processes, none with more than maxM inducing inputs; max_mpad: the largest mp among them
gp_status ssm_launch_prior(gp_handle h, const SsmProc* d_procs, int count, int S, int max_mpad, const char* unsupported) {
  return sps_dispatch_mpad(h, max_mpad, unsupported, [&](auto mpad) -> gp_status {
    hipLaunchKernelGGL((ssm_prior_kernel<decltype(mpad)::value>), dim3((S + 63) / 64, count), dim3(64), 0, h->stream, d_procs, S);
    GP_HIP_CHECK(h, hipGetLastError());
    return GP_OK;
  });
}
int64_t ssm_fill_tiles(const SsmDesc& lay, std::vector<char>& hd, int count, int maxM) {
  const SsmProc* procs = (const SsmProc*)(hd.data() + lay.procs);
  int64_t* tiles = (int64_t*)(hd.data() + lay.tiles);
  const int T = sps_tile_frames(maxM);
  int64_t at = 0;
  for (int r = 0; r < count; r++) {
    tiles[r] = at;
    at += (procs[r].n + T - 1) / T;
  }
  tiles[count] = at;
  return at;
}
gp_status ssm_launch_update(gp_handle h, const SsmDesc& lay, const char* d_desc, int count, int64_t entries, int maxM, int S,
                            int max_mpad, const char* unsupported) {
  if (entries <= 0) return GP_OK;
  if (entries > 0x7fffffff) return gp_fail(h, GP_ERR_UNSUPPORTED, "sampling: more than 2^31 - 1 frame tiles in one call");
  GpTimerScope ts(h, GP_TIMER_COND_A);
  return sps_dispatch_mpad(h, max_mpad, unsupported, [&](auto mpad) -> gp_status {
    const int T = sps_tile_frames(maxM);
    const size_t lds = sps_lds_bytes(maxM, decltype(mpad)::value);
    GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)ssm_update_kernel<decltype(mpad)::value>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)lds));
    hipLaunchKernelGGL((ssm_update_kernel<decltype(mpad)::value>), dim3((unsigned)entries), dim3(4 * T), lds, h->stream,
                       (const SsmProc*)(d_desc + lay.procs), (const int64_t*)(d_desc + lay.tiles), count, S, T, sps_stride(maxM));
    GP_HIP_CHECK(h, hipGetLastError());
    return GP_OK;
  });
}

// `order` becomes device addresses: every span's entries must be a permutation of 0..len-1
gp_status ssm_check_orders(gp_handle h, const int32_t* order_host, const std::vector<SsmSpan>& spans, const char* not_a_permutation) {
  std::vector<char> seen;
  for (const SsmSpan& sp : spans) {
    const int32_t* o = order_host + sp.off;
    seen.assign(sp.len, 0);
    for (int j = 0; j < sp.len; j++) {
      if (o[j] < 0 || o[j] >= sp.len || seen[o[j]]) return gp_fail(h, GP_ERR_BAD_ARG, not_a_permutation);
      seen[o[j]] = 1;
    }
  }
  return GP_OK;
}

// A call's descriptor block (SsmDesc, common.h)
SsmDesc ssm_desc_layout(size_t nproc, size_t rec_bytes, size_t nprob) {
  SsmDesc o;
  GpRegions region;
  o.procs = region(nproc * sizeof(SsmProc));
  o.recs = region(rec_bytes);
  o.feat = region(2 * nproc * sizeof(FeatItem));
  o.probs = region(nprob * sizeof(GemmProblem));
  o.tiles = region((nproc + 1) * sizeof(int64_t));
  o.bytes = region.off;
  return o;
}
// Uploads the block (hd: its host copy, the first nfeat feature items filled in any order) and `order`, then builds the feature
// tables: the items are grouped by table padding, one launch of the shared feature kernel per distinct sm_mpad.
gp_status ssm_upload(gp_handle h, const SsmDesc& lay, std::vector<char>& hd, char* d_desc, int nfeat, const int32_t* order_host,
                            int* d_order, size_t norder, int max_n) {
  FeatItem* feats = (FeatItem*)(hd.data() + lay.feat);
  std::stable_sort(feats, feats + nfeat, [](const FeatItem& a, const FeatItem& b) { return sm_mpad(a.k.m) < sm_mpad(b.k.m); });
  GP_HIP_CHECK(h, hipMemcpyAsync(d_desc, hd.data(), lay.bytes, hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipMemcpyAsync(d_order, order_host, norder * sizeof(int), hipMemcpyHostToDevice, h->stream));
  GP_HIP_CHECK(h, hipStreamSynchronize(h->stream));       // hd is a host vector
  for (int first = 0, end; first < nfeat; first = end) {
    const int mp = sm_mpad(feats[first].k.m);
    for (end = first + 1; end < nfeat && sm_mpad(feats[end].k.m) == mp; end++) {}
    GP_CHECK(launch_sm_features_items(h, (const FeatItem*)(d_desc + lay.feat) + first, end - first, max_n, mp, nullptr, 0));
  }
  return GP_OK;
}

// ==== SGPRSS =================================================================================================================
static inline bool smp_kernel_ok(int type) {
  return type == GP_KERN_MATERN12 || type == GP_KERN_MERCER_MATERN12SM || type == GP_KERN_MATERN12SM;
}
static const char* const SMP_PARTIALS = "sparse source sampling: num_partials must be in [1, 32]";

// one per window: what only the u0 kernel reads
struct SmpU0 { const double* eps_u; const double* c; double* u0; double* rhs; };

// ---- 2. u0 = sum_p prior_p(Z) + sqrt(jitter) eps_u[0] (sources in kern_list order), rhs = c + eps_u[1]; grid (blocks, window);
// procs kernel-major [P][nwin] ----
__global__ void __launch_bounds__(256) sgpr_sample_u0_kernel(const SsmProc* __restrict__ procs, const SmpU0* __restrict__ recs,
                                                             int nwin, int P, int M, int S, double sqrt_jitter) {
  const int w = blockIdx.y;
  const SmpU0 it = recs[w];
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int i = e / S, s = e % S;
  if (i >= procs[w].kz) return;
  double u = procs[w].pz[(size_t)i * S + s];
  for (int p = 1; p < P; p++) u += procs[(size_t)p * nwin + w].pz[(size_t)i * S + s];
  const double* __restrict__ eu = it.eps_u + (size_t)s * 2 * M;
  it.u0[(size_t)i * S + s] = u + sqrt_jitter * eu[i];
  it.rhs[(size_t)i * S + s] = it.c[i] + eu[M + i];
}

// the operator's one carve.  Feature tables: source p takes 2 sm_mpad(m_p) <= components_p + 6 rows, so (C + 6 P) rows per window
struct SmpBufs { char* desc; int* order; double *fx, *fzb, *pz, *u0, *rhs, *t1; };
static SmpBufs smp_carve(GpArena& ar, size_t M, size_t P, size_t C, size_t n, size_t S, size_t count) {
  SmpBufs b;
  b.desc = ar.take<char>(ssm_desc_layout(count * P, count * sizeof(SmpU0), 3 * count).bytes);
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
    if (ktype[i] != GP_KERN_MATERN12 && (km[i] < 1 || km[i] > 32)) return gp_fail(h, GP_ERR_UNSUPPORTED, SMP_PARTIALS);
    C += ssm_components(ktype[i], km[i]);
  }
  if ((int64_t)n + M > INT32_MAX / 2) return gp_fail(h, GP_ERR_UNSUPPORTED, "sparse source sampling: n too large");
  if ((((uintptr_t)ws) & 255) || ws_bytes < sgpr_sample_workspace_bytes(M, P, C, n, S, count))
    return gp_fail(h, GP_ERR_BAD_ARG, "sparse source sampling: workspace too small (gp_sgpr_sample_source_workspace_bytes) or not "
                                      "256-byte aligned");
  std::vector<SsmSpan> spans(count);          // every slot's first n + k entries
  for (int w = 0; w < count; w++) {
    const int k = kw ? kw[w] : M;
    if (k < 1 || k > M) return gp_fail(h, GP_ERR_BAD_ARG, "sparse source sampling: bad inducing-point count");
    spans[w] = SsmSpan{(size_t)w * (n + M), n + k};
  }
  GP_CHECK(ssm_check_orders(h, order_host, spans, "sparse source sampling: order is not a permutation of the window's n + k points"));
  if (C_out) *C_out = C;
  return GP_OK;
}

// The arguments have passed sgpr_sample_check and the windows' forward state is enqueued on h->stream.
// win: [count]; src: [count][P]; order_host: [count][n + M]; eps_x [count][S][C][n], eps_z [count][S][C][M],
// eps_u [count][S][2][M]; out [count][P][S][n].
gp_status sgpr_sample_run(gp_handle h, const SmpWindow* win, const SmpSource* src, int count, int P, int M, int ldw, int n, int S,
                          double jitter, const int32_t* order_host, const double* eps_x, const double* eps_z, const double* eps_u,
                          double* out, void* ws, size_t ws_bytes) {
  int C = 0, max_mpad = 0;
  std::vector<int> coff(P), mpad(P);          // a source's first component among the window's C, and its table padding
  for (int i = 0; i < P; i++) {
    coff[i] = C;
    C += ssm_components(src[i].k.type, src[i].k.m);
    mpad[i] = ssm_mpad(src[i].k);
    if (mpad[i] > max_mpad) max_mpad = mpad[i];
  }
  GpArena ar(ws, ws_bytes);
  const SmpBufs b = smp_carve(ar, M, P, C, n, S, count);
  if (!ar.ok) return gp_fail(h, GP_ERR_BAD_ARG, "sparse source sampling: workspace too small");
  const SsmDesc lay = ssm_desc_layout((size_t)count * P, (size_t)count * sizeof(SmpU0), 3 * (size_t)count);
  std::vector<char> hd(lay.bytes, 0);
  SsmProc* procs = (SsmProc*)(hd.data() + lay.procs);
  SmpU0* recs = (SmpU0*)(hd.data() + lay.recs);
  FeatItem* feats = (FeatItem*)(hd.data() + lay.feat);
  GemmProblem* probs = (GemmProblem*)(hd.data() + lay.probs);
  int nfeat = 0;
  const size_t frows = (size_t)C + 6 * (size_t)P;
  for (int w = 0; w < count; w++) {
    const SmpWindow& sw = win[w];
    double* u0 = b.u0 + (size_t)w * M * S;
    double* rhs = b.rhs + (size_t)w * M * S;
    double* t1 = b.t1 + (size_t)w * M * S;
    recs[w] = SmpU0{eps_u + (size_t)w * S * 2 * M, sw.c, u0, rhs};
    size_t row = 0;
    for (int i = 0; i < P; i++) {
      const SmpSource& sc = src[(size_t)w * P + i];
      SsmProc& it = procs[(size_t)i * count + w];          // kernel-major [P][count], as SrcSparseItem
      it.k = sc.k; it.z = sw.z; it.xnew = sw.xnew;
      if (mpad[i]) {
        double* tx = b.fx + ((size_t)w * frows + row) * n;
        feats[nfeat++] = FeatItem{sc.k, sw.xnew, tx, n, 0};
        it.fx = tx;
        it.fz = sc.fz;
        if (!sc.fz) {
          double* tz = b.fzb + ((size_t)w * frows + row) * M;   // (kz <= M values per row are written)
          feats[nfeat++] = FeatItem{sc.k, sw.z, tz, sw.kz, 0};
          it.fz = tz;
        }
      }
      row += 2 * (size_t)mpad[i];
      it.order = b.order + (size_t)w * (n + M);
      it.eps_x = eps_x + ((size_t)w * S * C + coff[i]) * n;
      it.eps_z = eps_z + ((size_t)w * S * C + coff[i]) * M;
      it.beta = u0;
      it.out = out + ((size_t)w * P + i) * S * n;
      it.pz = b.pz + ((size_t)w * P + i) * M * S;
      it.n = n; it.kz = sw.kz; it.mp = mpad[i]; it.cs = C; it.ezs = M;
    }
    // t1 = W u0;  t1 = WB^T rhs - t1;  beta (over u0) = W^T t1     — [kz][S] row-major, the slot's own kz-point problem
    GemmProblem g;
    memset(&g, 0, sizeof(g));
    g.M = sw.kz; g.N = S; g.K = sw.kz; g.lda = ldw; g.ldb = S; g.ldc = S;
    g.A = sw.W; g.B = u0; g.C = t1; probs[0 * (size_t)count + w] = g;
    g.A = sw.WB; g.B = rhs; g.C = t1; probs[1 * (size_t)count + w] = g;
    g.A = sw.W; g.B = t1; g.C = u0; probs[2 * (size_t)count + w] = g;
  }
  const int64_t entries = ssm_fill_tiles(lay, hd, P * count, M);
  GP_CHECK(ssm_upload(h, lay, hd, b.desc, nfeat, order_host, b.order, (size_t)count * (n + M), n > M ? n : M));
  const SsmProc* d_procs = (const SsmProc*)(b.desc + lay.procs);
  const GemmProblem* d_probs = (const GemmProblem*)(b.desc + lay.probs);
  GP_CHECK(ssm_launch_prior(h, d_procs, P * count, S, max_mpad, SMP_PARTIALS));
  hipLaunchKernelGGL(sgpr_sample_u0_kernel, dim3((unsigned)(((size_t)M * S + 255) / 256), count), dim3(256), 0, h->stream, d_procs,
                     (const SmpU0*)(b.desc + lay.recs), count, P, M, S, sqrt(jitter));
  GP_HIP_CHECK(h, hipGetLastError());
  { GemmFlags f; f.triA = TRI_LOWER;
    GP_CHECK(launch_gemm_batched(h, d_probs, count, M, S, f)); }
  { GemmFlags f; f.transA = 1; f.triA = TRI_UPPER; f.beta = -1.0;
    GP_CHECK(launch_gemm_batched(h, d_probs + count, count, M, S, f)); }
  { GemmFlags f; f.transA = 1; f.triA = TRI_UPPER;
    GP_CHECK(launch_gemm_batched(h, d_probs + 2 * (size_t)count, count, M, S, f)); }
  return ssm_launch_update(h, lay, b.desc, P * count, entries, M, S, max_mpad, SMP_PARTIALS);
}

// ==== Pdgp ===================================================================================================================
static inline bool psm_kernel_ok(int type) { return type == GP_KERN_MATERN32 || smp_kernel_ok(type); }
static const char* const PSM_PARTIALS = "Pdgp sampling: num_partials must be in [1, 32]";

// one per latent GP, engine order: what only the u0 kernel reads
struct PsmU0 { const double* eps_u; const double* q_mu; const double* q_sqrt; double* u0; double* rhs; };

// ---- 2. u0 = prior(z) + sqrt(jitter) eps_u[0];  rhs = q_mu + tril(q_sqrt) eps_u[1]  (unwhitened: rhs - u0); grid (blocks, GP) --
__global__ void __launch_bounds__(256) pdgp_sample_u0_kernel(const SsmProc* __restrict__ procs, const PsmU0* __restrict__ recs, int S,
                                                             double sqrt_jitter, int whiten) {
  const PsmU0 it = recs[blockIdx.y];
  const int M = procs[blockIdx.y].kz;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t i = e / S;
  const int s = (int)(e % S);
  if (i >= (size_t)M) return;
  const double* __restrict__ eu = it.eps_u + (size_t)s * 2 * M;
  const double u = procs[blockIdx.y].pz[i * S + s] + sqrt_jitter * eu[i];
  const double* __restrict__ lq = it.q_sqrt + i * M;      // row i of q_sqrt: the columns j <= i are tril(q_sqrt)'s
  double r = it.q_mu[i];
  for (size_t j = 0; j <= i; j++) r = fma(lq[j], eu[M + j], r);
  it.u0[i * S + s] = u;
  it.rhs[i * S + s] = whiten ? r : r - u;
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

// the operator's one carve.  Every per-GP block has the largest GP's size (maxM rows).  Feature tables: an SM kernel of m
// partials takes 2 sm_mpad(m) <= c_r + 6 rows, so C + 6 G rows cover all GPs
struct PsmBufs { char* desc; int* order; double *fx, *fz, *pz, *u0, *rhs, *t1; };
static PsmBufs psm_carve(GpArena& ar, size_t G, size_t maxM, size_t C, size_t n, size_t S) {
  PsmBufs b;
  b.desc = ar.take<char>(ssm_desc_layout(G, G * sizeof(PsmU0), 2 * G).bytes);
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
    *C += ssm_components(gps[r].k.type, gps[r].k.m);
    if (ssm_mpad(gps[r].k) > *max_mpad) *max_mpad = ssm_mpad(gps[r].k);
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
    if (ssm_kernel_sm(gps[r].k.type) && (gps[r].k.m < 1 || gps[r].k.m > 32)) return gp_fail(h, GP_ERR_UNSUPPORTED, PSM_PARTIALS);
    if (gps[r].M < 1) return gp_fail(h, GP_ERR_BAD_ARG, "Pdgp sampling: bad inducing-point count");
    if (gps[r].M > SPS_MAX_M) return gp_fail(h, GP_ERR_UNSUPPORTED, "Pdgp sampling: M <= 1024 inducing points per latent GP");
  }
  int maxM, C, max_mpad;
  psm_totals(gps, G, &maxM, &C, &max_mpad);
  if ((int64_t)n + maxM > INT32_MAX / 2) return gp_fail(h, GP_ERR_UNSUPPORTED, "Pdgp sampling: n too large");
  if ((((uintptr_t)ws) & 255) || ws_bytes < pdgp_sample_workspace_bytes(G, maxM, C, n, S))
    return gp_fail(h, GP_ERR_BAD_ARG, "Pdgp sampling: workspace too small (gp_pdgp_sample_workspace_bytes) or not 256-byte aligned");
  std::vector<SsmSpan> spans(G);              // the GPs' n + M_r entries back to back
  size_t off = 0;
  for (int r = 0; r < G; r++) {
    spans[r] = SsmSpan{off, n + gps[r].M};
    off += (size_t)n + gps[r].M;
  }
  return ssm_check_orders(h, order_host, spans, "Pdgp sampling: order is not a permutation of a latent GP's n + M points");
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
  const SsmDesc lay = ssm_desc_layout(G, (size_t)G * sizeof(PsmU0), 2 * (size_t)G);
  std::vector<char> hd(lay.bytes, 0);
  SsmProc* procs = (SsmProc*)(hd.data() + lay.procs);
  PsmU0* recs = (PsmU0*)(hd.data() + lay.recs);
  FeatItem* feats = (FeatItem*)(hd.data() + lay.feat);
  GemmProblem* probs = (GemmProblem*)(hd.data() + lay.probs);
  int nfeat = 0;
  size_t off_x = 0, off_z = 0, off_u = 0, off_o = 0, frow = 0;
  for (int r = 0; r < G; r++) {
    const PsmGP& g = gps[r];
    const int c = ssm_components(g.k.type, g.k.m), M = g.M, mp = ssm_mpad(g.k);
    double* u0 = b.u0 + (size_t)r * maxM * S;
    double* rhs = b.rhs + (size_t)r * maxM * S;
    double* t1 = b.t1 + (size_t)r * maxM * S;
    recs[r] = PsmU0{eps_u + off_u, g.q_mu, g.q_sqrt, u0, rhs};
    SsmProc& it = procs[r];
    it.k = g.k; it.z = g.z; it.xnew = xnew;
    if (mp) {
      double* tx = b.fx + frow * n;
      double* tz = b.fz + frow * maxM;
      feats[nfeat++] = FeatItem{g.k, xnew, tx, n, 0};
      feats[nfeat++] = FeatItem{g.k, g.z, tz, M, 0};
      it.fx = tx; it.fz = tz;
    }
    it.order = b.order + off_o;
    it.eps_x = eps_x + off_x; it.eps_z = eps_z + off_z;
    it.beta = t1;
    it.out = latents + (size_t)r * S * n;               // row block r of `latents`
    it.pz = b.pz + (size_t)r * maxM * S;
    it.n = n; it.kz = M; it.mp = mp; it.cs = c; it.ezs = M;
    off_x += (size_t)S * c * n; off_z += (size_t)S * c * M; off_u += (size_t)S * 2 * M; off_o += (size_t)n + M;
    frow += 2 * (size_t)mp;
    // [M][S] row-major.  whitened: rhs <- rhs - W u0, beta = W^T rhs;  unwhitened (rhs holds q - u0): u0 <- W rhs, beta = W^T u0
    GemmProblem p;
    memset(&p, 0, sizeof(p));
    p.M = M; p.N = S; p.K = M; p.lda = M; p.ldb = S; p.ldc = S; p.A = g.W;
    p.B = whiten ? u0 : rhs; p.C = whiten ? rhs : u0; probs[r] = p;
    p.B = whiten ? rhs : u0; p.C = t1; probs[(size_t)G + r] = p;
  }
  const int64_t entries = ssm_fill_tiles(lay, hd, G, maxM);
  GP_CHECK(ssm_upload(h, lay, hd, b.desc, nfeat, order_host, b.order, off_o, n > maxM ? n : maxM));
  const SsmProc* d_procs = (const SsmProc*)(b.desc + lay.procs);
  const GemmProblem* d_probs = (const GemmProblem*)(b.desc + lay.probs);
  GP_CHECK(ssm_launch_prior(h, d_procs, G, S, max_mpad, PSM_PARTIALS));
  hipLaunchKernelGGL(pdgp_sample_u0_kernel, dim3((unsigned)(((size_t)maxM * S + 255) / 256), G), dim3(256), 0, h->stream, d_procs,
                     (const PsmU0*)(b.desc + lay.recs), S, sqrt(jitter), whiten ? 1 : 0);
  GP_HIP_CHECK(h, hipGetLastError());
  { GemmFlags f; f.triA = TRI_LOWER;
    if (whiten) { f.alpha = -1.0; f.beta = 1.0; }
    GP_CHECK(launch_gemm_batched(h, d_probs, G, maxM, S, f)); }
  { GemmFlags f; f.transA = 1; f.triA = TRI_UPPER;
    GP_CHECK(launch_gemm_batched(h, d_probs + G, G, maxM, S, f)); }
  GP_CHECK(ssm_launch_update(h, lay, b.desc, G, entries, maxM, S, max_mpad, PSM_PARTIALS));
  if (sources) {
    const size_t count = (size_t)P * S * n;
    hipLaunchKernelGGL(pdgp_sample_source_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, latents, sources,
                       count, nlin);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  return GP_OK;
}
