/*
 * gpitch_abi.h — C-ABI of libgpitch_hip.so (MI355X / gfx950 only).
 *
 * Drop-in boundary for the gpitch `pdgp` / `sgpr_ss` ELBO path.  The reference
 * (PabloAlvarado/gpitch) has NO FFI boundary of its own: the path is Python objects over a
 * TensorFlow graph.  Each entry point below therefore replaces the TF/GPflow op sequence behind one
 * reference *operator* call; the reference interface it replaces is cited as file:line relative to
 * the reference tree.  The ctypes binding a gpitch maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions
 *  - plain pointers and sizes only; all array arguments are DEVICE pointers to float64 unless the
 *    name ends in `_host`; matrices are row-major with explicit leading dimension where given;
 *  - the caller allocates and owns every buffer (including workspaces); the library owns only the
 *    opaque handle / plan objects;
 *  - every call returns a gp_status; nothing throws across the boundary; calls enqueue work on the
 *    handle's HIP stream and return immediately unless they produce a host scalar;
 *  - a handle is bound to one (process, GPU) and is not thread-safe.
 *  - there is NO CPU fallback: without a gfx950 device every compute entry point fails with
 *    GP_ERR_HIP / GP_ERR_NO_DEVICE.
 */
#ifndef GPITCH_ABI_H
#define GPITCH_ABI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GPITCH_ABI_VERSION 1

typedef int32_t gp_status;
enum {
  GP_OK = 0,
  GP_ERR_BAD_ARG = 1,
  GP_ERR_NOT_PD = 2,     /* Cholesky hit a non-positive pivot (TF InvalidArgumentError in the reference) */
  GP_ERR_HIP = 3,        /* a HIP runtime call failed; gp_last_error() has the text */
  GP_ERR_NO_DEVICE = 4,
  GP_ERR_WORKSPACE = 5,  /* caller-provided workspace too small */
  GP_ERR_UNSUPPORTED = 6
};

/* kernel (covariance function) types — the GPflow operator API `Kern.K(X, X2)`, `Kern.Kdiag(X)` */
enum {
  GP_KERN_MATERN12 = 0,          /* gpflow.kernels.Matern12  (init_models.py:83)                 */
  GP_KERN_MATERN32 = 1,          /* gpflow.kernels.Matern32  (init_kernels.py:12, demo-modgp.py:32) */
  GP_KERN_MATERN52 = 2,          /* gpflow.kernels.Matern52  (init_models.py:188)                */
  GP_KERN_RBF = 3,               /* gpflow.kernels.RBF                                            */
  GP_KERN_MERCER_MATERN12SM = 4, /* gpitch/matern12_spectral_mixture.py:70-133                    */
  GP_KERN_MATERN12SM = 5,        /* gpitch/matern12_spectral_mixture.py:14-67                     */
  GP_KERN_MATERN32SM = 6,        /* gpitch/kernels.py:204-258 (init_models.py:84,96): broadcast form, Matern-3/2
                                  * envelope; theta = [1 (unused, fixed), lengthscales, variance_k.., frequency_k..] */
  GP_KERN_MERCER_MATERN52SM = 7  /* Matern52 * MercerCosMix product (init_models.py:183-198, kernels.py:321-376):
                                  * theta = [v52 * v_cosmix, lengthscales, energy_k.., frequency_k..];
                                  * Kdiag = variance (MercerCosMix.Kdiag fills its variance, no energy sum) */
};

/* nonlinearities of the modulated likelihood — gpitch/methods.py:216-233 */
enum { GP_NLIN_LOGISTIC = 0, GP_NLIN_SOFTPLUS = 1, GP_NLIN_GAUSS = 2 };

/* Kernel descriptor.  `theta` is a DEVICE pointer to the constrained hyper-parameters
 *   [variance, lengthscales, energy_0..energy_{m-1}, frequency_0..frequency_{m-1}]  (m = num_partials,
 *   0 for the plain stationary kernels) — device-resident so an optimiser step never syncs the host. */
typedef struct {
  int32_t type;
  int32_t num_partials;
  const double* theta;
} gp_kernel_desc;

#define GP_THETA_LEN(m) (2 + 2 * (m))

typedef struct gp_handle_s* gp_handle;
typedef struct gp_pdgp_plan_s* gp_pdgp_plan;
typedef struct gp_sgpr_plan_s* gp_sgpr_plan;
typedef struct gp_sgprb_plan_s* gp_sgprb_plan;
typedef struct gp_pdgpb_plan_s* gp_pdgpb_plan;

/* ---- runtime -------------------------------------------------------------------------------- */
/* replaces gpitch.init_settings / the global TF session (gpitch/methods.py:155-180).
 * `stream` is the hipStream_t every call enqueues on; NULL = HIP's default (null) stream. */
gp_status gp_create(int32_t device_id, void* stream, gp_handle* out);
gp_status gp_destroy(gp_handle h);
gp_status gp_sync(gp_handle h);
const char* gp_last_error(gp_handle h);       /* text of the last failure on this handle */
int32_t gp_abi_version(void);
/* host-only query, no device work: would a uniform, aligned strip product of that role (1: A = W Kuf, 2: Lq^T A,
 * 3: Kuf_bar, 5: Kuf_bar with the stationary contraction) over an M x N strip take the wave form (f32 != 0: float32
 * strips)?  Strips of 2^31 bytes or more never do. */
int32_t gp_debug_wave_takes(int32_t role, int32_t M, int32_t N, int32_t f32);
/* For tests; synchronises nothing.  ONE launch of a GEMM host entry on the caller's device buffers, no arithmetic of its
 * own.  `probs` is a HOST array of `batch` records (copied into the library's descriptors with every other field zero and
 * uploaded into `workspace`, a 16-byte aligned DEVICE buffer of at least 160 bytes per problem, on the handle's stream).
 *   kind  0 float64 product C = alpha op(A) op(B) + beta C with the column-sum epilogues, 1 float64 split-K H = X [D] Y^T
 *         with slab reduction (triC lower = symmetric, scale_mode 2 = D given in v1), 2 / 3 the same two on float32 strips
 *   form  0 as the library dispatches, 1 the wave form only, 2 the lean strip form only, 3 the generic kernel (the launch is
 *         passed with uniform_aligned = rows64_ok = 0); a form that does not take the launch: GP_ERR_UNSUPPORTED, nothing runs
 *   nsplit  kinds 1 / 3: K-slices (0 = the library's own choice)
 * Roles 5, 6 and 7 are refused (GP_ERR_UNSUPPORTED).  *partial_rows: rows of the partial-sum arrays o0 / o1 as the engine
 * sizes them, by role and shape (kinds 0 / 2: one per 64-row tile where the wave form takes that role and shape, else one per
 * row block; kinds 1 / 3: K-slices).  An upper bound: a dispatched launch that the wave form declines for its flags (alpha,
 * beta, triC) writes the fewer rows of the form that runs instead. */
typedef struct {
  const void* A; const void* B; void* C;
  const double* v0; const double* v1; const double* v2;
  double* o0; double* o1; double* o2;
  const void* xa; const void* xb;
  int32_t M, N, K, pad_;
  int64_t lda, ldb, ldc;
} gp_debug_gemm_problem;
typedef struct {
  int32_t transA, transB, triA, triB, triC;   /* tri*: 0 none, 1 lower, 2 upper */
  int32_t big_tiles, epilogue, scale_mode, role, tile_m0, tile_mcount, uniform_aligned, a32_ok, rows64_ok;
  double alpha, beta;
} gp_debug_gemm_flags;
gp_status gp_debug_gemm(gp_handle h, const gp_debug_gemm_problem* probs, int32_t batch, int32_t maxM, int32_t maxN,
                        const gp_debug_gemm_flags* flags, int32_t kind, int32_t form, int32_t nsplit, void* workspace,
                        size_t workspace_bytes, int32_t* partial_rows);
/* For tests; synchronises nothing.  ONE launch of a kernel-gradient contraction host entry (or of its finish) on the caller's
 * device buffers, no arithmetic of its own.  `items` / `fins` are HOST arrays of `count` records, uploaded (entries 1, 4) into
 * `workspace`, a 16-byte aligned DEVICE buffer of at least 160 bytes per record, on the handle's stream.
 *   entry 0  the single-record contraction (count = 1)
 *         1  the items form of one kernel family with the flags' with_gz, use_mfma, x2_shared, g32_items, lean_items, gscale_items
 *            (a record with x2 NULL reads the launch's shared x2 / n2_shared)
 *         2  the one-pass contraction for the kernels of a sum: the records share x1, x2, G, alpha, gm; *taken = 0 and
 *            GP_ERR_UNSUPPORTED when the sum kernel declines (nothing is contracted)
 *         3  the single finish (fins[0]; no Kuu side)      4  the items finish, its grid sized by the largest record
 * Contraction sums: partials[record][2 + 2 m] = sum_ij Gw_ij dK_ij/dtheta, Gw = G + alpha gm^T (G symmetrised when `symmetric`,
 * columns scaled by 2 gscale[j] where gscale is given), gz[column block][n1] the same for d/dx1.  G / kvals are float32 strips
 * when g32.  Mercer kernels: feat_from = -1 builds the record's feature tables into `feat` (16-byte aligned, 2 mpad (n1 + n2)
 * + 64 doubles, mpad = m rounded up to 4), k >= 0 uses record k's (k < the record's index; same kernel and inputs).
 * *nparts: the partial records each contraction left (entry 4: the grid's blocks per record).  A launch the selected form does
 * not take: GP_ERR_UNSUPPORTED; records that break what the form reads unasked (matrix-core forms: kvals, alpha and gm in every
 * record; lean_items: 16-byte aligned strips with even strides): GP_ERR_BAD_ARG.  Nothing is launched then. */
typedef struct {
  gp_kernel_desc kern;
  const double* x1; const double* x2;
  const void* G; const double* alpha; const double* gm;
  const void* kvals; const double* gscale;
  double* partials; double* gz; double* feat;
  int64_t ldg, ldk;
  int32_t n1, n2, symmetric, g32, feat_from, pad_;
} gp_debug_hyper_item;
typedef struct {
  gp_kernel_desc kern;
  const double* p_uf; const double* p_uu; const double* gv_sum; double* g_theta;
  const double* gz_uf; const double* gz_uu; double* g_z;
  int32_t np_uf, np_uu, cb_uf, cb_uu, n1, pad_;
} gp_debug_hyper_finish;
typedef struct {
  int32_t with_gz, use_mfma, g32_items, lean_items, gscale_items, n2_shared;
  const double* x2_shared;
} gp_debug_hyper_flags;
gp_status gp_debug_hyper_contract(gp_handle h, int32_t entry, const gp_debug_hyper_item* items, const gp_debug_hyper_finish* fins,
                                  int32_t count, const gp_debug_hyper_flags* flags, void* workspace, size_t workspace_bytes,
                                  int32_t* nparts, int32_t* taken);
/* host-only queries, no device work: the partial records a plan reserves for one Kuf-side contraction of an M x N strip (-1 for
 * an empty shape), and whether an items launch (use_mfma, lean_items, float64 strips) of `count` n1 x n2 records takes the
 * lean matrix-core form, the one that applies gscale */
int64_t gp_debug_hyper_records(int32_t N, int32_t M);
int32_t gp_debug_hyper_lean_takes(int32_t type, int32_t m, int32_t n1, int32_t n2, int32_t count);
/* For tests; synchronises nothing.  ONE launch of a covariance-build host entry on the caller's device buffers, no
 * arithmetic of its own.  `items` is a HOST array of `count` records; entry 1 uploads them into `workspace`, a 16-byte
 * aligned DEVICE buffer of at least 192 bytes per record, on the handle's stream (entries 0 and 2 need none).
 *   entry 0  the single-record build (count = 1), the record passed by value; Mercer feature tables are built inside
 *         1  the grouped build of one kernel family: every record has the same type and the same partial count rounded up
 *            to 4 (else GP_ERR_BAD_ARG).  The feature tables of Mercer records are built by the grouped feature launch
 *            (rows, then columns), then ONE grouped build runs with the grid sized by the largest record.  A record with
 *            n2 < 0 reads the launch's shared x2_shared / n2_shared.  engine_strips is the caller's promise of engine
 *            strips (1 float64, 2 float32) and is checked here: every record then has n2 < 0, an even leading dimension
 *            and a 16-byte aligned output, no accumulation and no diagonal, else GP_ERR_BAD_ARG.  The lean matrix-core form,
 *            which only engine_strips admits, reads whole 128-column blocks of the SHARED frames without a column guard;
 *            no caller in the library passes a record with frames of its own (n2 >= 0) beside x2_shared into that form,
 *            and this entry refuses one with GP_ERR_BAD_ARG.  The matrix-core forms write plain strips: a record that
 *            accumulates or adds a diagonal in a launch that takes one of them is GP_ERR_BAD_ARG too.
 *         2  the one-pass build of the sum of `count` kernels that share x1, x2, out, ld, diag_add and f32out (record 0's
 *            are used; accumulate is ignored); when the sum kernel declines: GP_ERR_UNSUPPORTED, *form = -1, nothing is
 *            written.  The feature tables are built first, one launch_sm_features per kernel.
 * x2 NULL with n2 >= 0: K(x1).  out is a float32 matrix (ld in floats) when f32out.  feat (Mercer kernels): 16-byte aligned,
 * 2 mpad (n1 + n2) + 64 doubles, mpad = m rounded up to 4; rows [0, mpad) of each block are the cos features, [mpad, 2 mpad)
 * the sin features, the x1 block first and the x2 block behind it at 2 mpad n1 doubles rounded up to a multiple of 32.
 * *form: 0 the generic kernel, 1 the staged matrix-core form, 2 the lean matrix-core form (entry 2: 0 taken, -1 declined);
 * *row_seg: the row segment of forms 1 and 2 (else 0).  Nothing is launched when a status other than GP_OK comes back from
 * the checks above. */
typedef struct {
  gp_kernel_desc kern;
  const double* x1; const double* x2;
  void* out; double* feat;
  int64_t ld; double diag_add;
  int32_t n1, n2, accumulate, f32out;
} gp_debug_cov_item;
gp_status gp_debug_cov_build(gp_handle h, int32_t entry, const gp_debug_cov_item* items, int32_t count,
                             const double* x2_shared, int32_t n2_shared, int32_t engine_strips,
                             void* workspace, size_t workspace_bytes, int32_t* form, int32_t* row_seg);
/* For tests; synchronises nothing.  ONE launch of a far field's table kernel on the caller's device buffers, no arithmetic of
 * its own and no cols kernel: the caller writes the ranges rng [N / 256][2] (int32) and the reference points ref [N / 256][2]
 * itself, so it can hand over ranges that no model produces.  The record is uploaded into `workspace`, a 16-byte aligned
 * DEVICE buffer of at least 256 bytes, on the handle's stream.
 *   which 0  the activations' tables (afar.hip): X = W and X2 = C, both M x M; theta = (variance, lengthscale);
 *            T [N / 256][M][8]; M a multiple of 16 up to 1024; fz NULL and nf 0
 *         1  the Q route's tables (qfar.hip): X = Q, M x M, X2 NULL; fz the z feature table [nf][M]; T [N / 256][M][2 nf];
 *            M a multiple of 64 up to 1024, nf a multiple of 8 up to 64; every count a multiple of 16
 *   form  0  the one-thread-per-chain kernels (switches.h far_tables = 0), 1 the kernels that stage the tiles in LDS
 * The caller's promise, as the cols kernels keep it: 0 <= rng[2 S] <= rng[2 S + 1] <= M.  N a multiple of 256; X, X2 and
 * fz 16-byte aligned.  Anything else is GP_ERR_BAD_ARG and launches nothing. */
gp_status gp_debug_far_tables(gp_handle h, int32_t which, int32_t form, const double* X, const double* X2, const double* z,
                              const double* theta, const double* fz, int32_t* rng, double* ref, double* T, int32_t M, int32_t N,
                              int32_t nf, void* workspace, size_t workspace_bytes);
/* pivot index reported by the last GP_ERR_NOT_PD (−1 if none) */
int32_t gp_last_not_pd_index(gp_handle h);

/* ---- L2 operators: Kern.K / Kern.Kdiag --------------------------------------------------------
 * replaces MercerMatern12sm.K (matern12_spectral_mixture.py:102-117), Matern12sm.K (:38-56) and GPflow
 * Stationary.K for Matern12/32/52/RBF.  out[i*ld + j] = k(x1[i], x2[j]);  x2 == NULL means K(X) (x2 = x1).
 * `accumulate` != 0 adds into `out` (GPflow `Add` kernel: sgpr_ss.py:42-43). */
gp_status gp_kernel_build(gp_handle h, const gp_kernel_desc* kern, const double* x1, int32_t n1,
                          const double* x2, int32_t n2, double* out, int64_t ld, int32_t accumulate);
/* The same build with a float32 result (ld in floats; inputs and arithmetic float64, one rounding at the store):
 * the Kuf strips of the configurations the reference would run with float_type = float32
 * (gpitch/matern12_spectral_mixture.py:8-11 np_float_type). */
gp_status gp_kernel_build_f32(gp_handle h, const gp_kernel_desc* kern, const double* x1, int32_t n1,
                              const double* x2, int32_t n2, float* out, int64_t ld, int32_t accumulate);
/* Kern.Kdiag(X): exact fill (matern12_spectral_mixture.py:58-62,119-121) */
gp_status gp_kernel_diag(gp_handle h, const gp_kernel_desc* kern, int32_t n, double* out, int32_t accumulate);

/* ---- GPflow conditional pieces ------------------------------------------------------------------
 * Kmm = K(z) + jitter I ; Lm = chol(Kmm) ; Linv = Lm^-1   (GPflow conditional, from pdgp.py:147;
 * sgpr_ss.py:43-44).  L and Linv are M x M row-major (ld = M), strictly-upper part zeroed.
 * Either output may be NULL.  workspace: gp_chol_workspace_bytes(M). */
size_t gp_chol_workspace_bytes(int32_t M);
gp_status gp_kuu_cholesky(gp_handle h, const gp_kernel_desc* kern, const double* z, int32_t M, double jitter,
                          double* L, double* Linv, void* workspace, size_t workspace_bytes);
/* dense lower Cholesky of a caller-supplied SPD matrix (tf.cholesky: sgpr_ss.py:44,51,89), in place */
gp_status gp_cholesky_inplace(gp_handle h, double* A, int32_t M, int64_t ld);

/* gpflow.conditionals.conditional(Xnew, z, kern, f=q_mu, full_cov=False, q_sqrt, whiten)
 * (call sites pdgp.py:147-155,176-178,185-187,199-205).  q_sqrt is the M x M (x1) matrix; its lower
 * triangle is used (matrix_band_part).  fmean, fvar: N values each.  q_sqrt may be NULL.
 * workspace: gp_conditional_workspace_bytes(N, M). */
size_t gp_conditional_workspace_bytes(int32_t N, int32_t M);
gp_status gp_conditional_diag(gp_handle h, const gp_kernel_desc* kern, const double* xnew, int32_t N,
                              const double* z, int32_t M, const double* q_mu, const double* q_sqrt,
                              int32_t whiten, double jitter, double* fmean, double* fvar,
                              void* workspace, size_t workspace_bytes);

/* float32 form of the whitened conditional (the reference's settings.dtypes.float_type = float32, pdgp.py:13):
 * Kuf and A = Lm^-1 Kuf are float32 strips, both strip products run on v_mfma_f32_16x16x4_f32; Kmm, Lm, Lm^-1 and all
 * reductions (sum A^2, A^T q_mu, sum LTA^2) are float64, as are the inputs and outputs.  Same workspace size bound. */
gp_status gp_conditional_diag_f32(gp_handle h, const gp_kernel_desc* kern, const double* xnew, int32_t N,
                                  const double* z, int32_t M, const double* q_mu, const double* q_sqrt,
                                  double jitter, double* fmean, double* fvar,
                                  void* workspace, size_t workspace_bytes);
/* ... with the `whiten` argument of conditional(): in the reference `whiten` and `float_type` are independent settings
 * (gpitch/pdgp.py:13,49,122-129).  whiten = 0 adds A' = Lm^-T A as a third float32 strip product; its rounding is
 * amplified by cond(Kuu) instead of cond(Kuu)^(1/2) (tolerances: tests/test_gpu_f32.py). */
gp_status gp_conditional_diag_f32w(gp_handle h, const gp_kernel_desc* kern, const double* xnew, int32_t N,
                                   const double* z, int32_t M, const double* q_mu, const double* q_sqrt,
                                   int32_t whiten, double jitter, double* fmean, double* fvar,
                                   void* workspace, size_t workspace_bytes);
/* full_cov = True of the same operator (GPflow 0.5 conditionals.conditional; gpitch/pdgp.py never asks for it): fmean (N)
 * and the N x N posterior covariance fcov (row-major, ld N) = K(xnew) - A^T A + (Lq^T A')^T (Lq^T A').
 * workspace: gp_conditional_full_workspace_bytes(N, M). */
size_t gp_conditional_full_workspace_bytes(int32_t N, int32_t M);
gp_status gp_conditional_full(gp_handle h, const gp_kernel_desc* kern, const double* xnew, int32_t N, const double* z,
                              int32_t M, const double* q_mu, const double* q_sqrt, int32_t whiten, double jitter,
                              double* fmean, double* fcov, void* workspace, size_t workspace_bytes);

/* gpflow.kullback_leiblers.gauss_kl(q_mu, q_sqrt, K=None) (pdgp.py:120-121 whitened; :126-129 with
 * K = kern.K(z) + jitter I built internally when kern != NULL).  Result to *out_host (syncs).
 * workspace: gp_gauss_kl_workspace_bytes(M, kern != NULL). */
size_t gp_gauss_kl_workspace_bytes(int32_t M, int32_t with_kernel);
gp_status gp_gauss_kl(gp_handle h, const double* q_mu, const double* q_sqrt, int32_t M,
                      const gp_kernel_desc* kern_or_null, const double* z, double jitter,
                      double* out_host, void* workspace, size_t workspace_bytes);
/* the same with the caller's own prior covariance: gauss_kl(q_mu, q_sqrt, K) for a device matrix K (M x M,
 * row-major, ld = M, symmetric positive definite; not modified).  GP_ERR_NOT_PD when its Cholesky fails. */
gp_status gp_gauss_kl_matrix(gp_handle h, const double* q_mu, const double* q_sqrt, int32_t M, const double* K,
                             double* out_host, void* workspace, size_t workspace_bytes);

/* MpdLik.variational_expectations(Fmu, Fvar, Y) (likelihoods.py:422-447 + hermgauss1d :33-45 +
 * log_lik_exp :47-68).  Fmu/Fvar are N x 2P row-major with columns [g_0..g_{P-1}, f_0..f_{P-1}]
 * (pdgp.py:157-164).  noise_var is a device scalar.  per_frame (N values) may be NULL; the sum over
 * frames is written to *sum_host when non-NULL (syncs).
 * P <= 128: a workgroup of 16 frames stages 3 P doubles per frame in LDS (16 * 3 * P * 8 bytes <= 48 KiB); a larger P
 * returns GP_ERR_UNSUPPORTED before any launch.  The same limit holds for the likelihood inside gp_pdgp_elbo and its
 * sharded forms, there for the sources one plan holds. */
gp_status gp_mpd_varexp(gp_handle h, const double* Fmu, const double* Fvar, const double* y, int32_t N,
                        int32_t P, int32_t nlin, const double* noise_var, double* per_frame, double* sum_host);

/* Posterior moments of the sources, of the mixture and the expected log density, from the moments of the 2P latent GPs
 * (the prediction-side counterpart of gp_mpd_varexp; same 20-point rule, weights and nonlinearities).  With g ~ N(m_g, v_g),
 * f ~ N(m_f, v_f) independent under q, E1 = E[nlin(g)], E2 = E[nlin(g)^2] and V = sum_h w_h (nlin(x_h) - E1)^2:
 *   smean[i][n] = E1 m_f                      posterior mean of source i = nlin(g_i) f_i
 *   svar[i][n]  = V m_f^2 + E2 v_f            its variance (both terms non-negative: svar >= 0 exactly)
 *   ymean[n]    = sum_i smean[i][n]           in source order
 *   yvar[n]     = sum_i svar[i][n] + noise    in source order; noise_var == NULL: the latent mixture, nothing added
 *   logp[n]     = MpdLik.variational_expectations(Fmu, Fvar, y)[n]   (E_q log p(y_n | g, f); not scaled, no KL)
 * Fmu/Fvar are N x 2P row-major as in gp_mpd_varexp; smean/svar are P x N row-major; ymean/yvar/logp hold N values.
 * Every output may be NULL; logp needs y and noise_var.  noise_var is a device scalar.  float64; asynchronous on the
 * handle's stream; every sum is one lane's sequential loop, so two calls give bit-identical results.
 * P <= 96: the staging is 4 P doubles per frame (svar joins the three of gp_mpd_varexp; 16 * 4 * P * 8 bytes <= 48 KiB),
 * so this entry stops 32 sources before gp_mpd_varexp does; a larger P returns GP_ERR_UNSUPPORTED before any launch. */
gp_status gp_mpd_predict_moments(gp_handle h, const double* Fmu, const double* Fvar, const double* y, int32_t N, int32_t P,
                                 int32_t nlin, const double* noise_var, double* smean, double* svar, double* ymean,
                                 double* yvar, double* logp);

/* ---- L3 model: Pdgp (gpitch/pdgp.py:48-208) ---------------------------------------------------
 * Parameter vector layout (float64, constrained space), offsets returned by gp_pdgp_layout:
 *   [ noise_var | for g in (act_0..act_{P-1}, com_0..com_{P-1}):
 *                   theta_g (2+2m_g) | z_g (M_g) | q_mu_g (M_g) | q_sqrt_g (M_g x M_g row-major) ]
 * The same layout is used for the gradient vector, the free-state vector and the Adam moments. */
typedef struct {
  int32_t num_sources;            /* P */
  int32_t whiten;                 /* pdgp.py:49  */
  int32_t nlin;                   /* GP_NLIN_* (pdgp.py:49 nlinfun) */
  int32_t max_batch;              /* largest minibatch N the plan will see */
  const int32_t* M_act;           /* host, P entries (pdgp.py:93) */
  const int32_t* M_com;           /* host, P entries (pdgp.py:94) */
  const int32_t* kern_type_act;   /* host, P entries GP_KERN_* */
  const int32_t* kern_type_com;
  const int32_t* partials_act;    /* host, P entries (0 for plain stationary) */
  const int32_t* partials_com;
  double jitter;                  /* settings.numerics.jitter_level = 1e-6 (pdgp.py:14) */
} gp_pdgp_config;

gp_status gp_pdgp_create(gp_handle h, const gp_pdgp_config* cfg, gp_pdgp_plan* out);
gp_status gp_pdgp_destroy(gp_pdgp_plan p);
int64_t gp_pdgp_num_params(gp_pdgp_plan p);
/* offsets into the parameter vector for GP index g in [0, 2P): g < P activation i=g, else component */
gp_status gp_pdgp_layout(gp_pdgp_plan p, int32_t g, int64_t* off_theta, int64_t* off_z, int64_t* off_qmu,
                         int64_t* off_qsqrt);
/* Arithmetic type of the O(M^2 N) part — the reference's `float_type` setting (pdgp.py:13,
 * matern12_spectral_mixture.py:8-11; BASELINE configs 3 and 5 are quoted at fp32).  bits = 64 (default) or 32:
 * with 32 the M x N strips Kuf, A = Lm^-1 Kuf and Kuf_bar are stored in float32 and the four strip products
 * (A = W Kuf, Lq^T A, R (A D), A D A^T) run on v_mfma_f32_16x16x4_f32; parameters, Kuu, its Cholesky factor and inverse,
 * every reduction over the inducing index or the frames, the likelihood, the KL terms and the gradient vector stay
 * float64, so the ABI's buffers do not change type.  Whitened models only.  Call before gp_pdgp_workspace_bytes /
 * gp_pdgp_set_workspace (the workspace is smaller).  Tolerance held against the float64 oracle: tests/test_gpu_f32.py. */
gp_status gp_pdgp_set_precision(gp_pdgp_plan p, int32_t bits);
/* The same per latent GP: bits[g] in {32, 64} for the plan's `count` latent GPs in engine order ([g_0..g_{P-1}, f_0..f_{P-1}],
 * a subset plan: its own rows in that order).  The reference's float_type is one global setting (pdgp.py:13); this is the
 * finer form the transcription model wants: its activation GPs (Matern-3/2 over a 16-kHz grid, cond(Kuu) ~ 1e9) are where
 * float32 strips cost accuracy (posterior mean 5e-2, lengthscale gradient 2e-1 of their scale), its component GPs are not,
 * so bits = [64 x P, 32 x P] keeps the float64 tolerances on the former and the float32 speed on the latter.  Float64
 * latent GPs must precede float32 ones (GP_ERR_UNSUPPORTED otherwise).  Call before gp_pdgp_workspace_bytes. */
gp_status gp_pdgp_set_gp_precision(gp_pdgp_plan p, const int32_t* bits, int32_t count);
size_t gp_pdgp_workspace_bytes(gp_pdgp_plan p);
gp_status gp_pdgp_set_workspace(gp_pdgp_plan p, void* workspace, size_t bytes);

/* Which gradients the caller will use for latent GP g (0 = skip that work).  GPflow's `.fixed = True`
 * (demo-modgp.py:40-41: m.za.fixed / m.zc.fixed; init_models.py:97-98: kern.fixed) removes a Param from the
 * TF gradient; here it lets the backward pass skip the inducing-input contraction (need_z = 0) or, when the
 * kernel hyper-parameters are fixed as well (need_theta = 0), the whole Kuf_bar / Kuu_bar chain of that GP.
 * Skipped entries of the gradient vector are left at zero.  Default: everything needed. */
gp_status gp_pdgp_set_grad_needs(gp_pdgp_plan p, int32_t g, int32_t need_theta, int32_t need_z);

/* How much of a step may run on the handle's internal helper stream (same results, different schedule):
 *   0  everything on the handle's stream, in order;
 *   1  forward: Kuu builds + Cholesky / inverse next to the Kuf builds; backward: the Kuu-side chain (Cholesky
 *      adjoint and its contraction) underneath the Kuf_bar product;
 *   2  (default) additionally the H = A diag(2 gv) A^T chain next to Kuf_bar — the two largest backward products then
 *      share the device, so each one's own launch takes longer while the step gets shorter.
 * Batches below 4096 frames always run on one stream. */
gp_status gp_pdgp_set_overlap(gp_pdgp_plan p, int32_t level);

/* A promise about every batch handed to gp_pdgp_elbo from now on: ascending != 0 says its frames x are in ascending order
 * (equal neighbours allowed).  A whitened plan then contracts Kuf_bar of a Matern-3/2 / Matern-5/2 family whose inducing
 * inputs are fixed (need_theta, no need_z) by exponentially weighted moment sums along the sorted frames instead of forming
 * the product (kuf_scan.hip; gradients agree to ~1e-11 relative).  The kernel that streams the frames checks neighbouring
 * pairs: a descending pair raises the handle's device status word, and the next gp_check_not_pd / host-scalar call returns
 * GP_ERR_BAD_ARG ("frames not ascending") and clears it.  Default 0: today's path. */
gp_status gp_pdgp_set_frames_ascending(gp_pdgp_plan p, int32_t ascending);

/* Permission for the Q route, from a caller that knows the plan's MercerMatern12sm kernels are what they are
 * in the transcription model: a Matern-1/2 envelope whose lengthscale stays near the inducing spacing, so that Kuu + jitter I
 * is well conditioned.  enable != 0: when ALL MercerMatern12sm latent GPs of a whitened plan have float64 strips, the same M
 * (a multiple of 64) and partial count, fixed inducing inputs (need_theta, no need_z), sit in one run of the batch, and the
 * batch is a multiple of 256 frames, gp_pdgp_elbo and its staged forms evaluate them through Q = W^T (Lq Lq^T - I) W: one
 * dense product G = Q Kuf replaces A = W Kuf, Lq^T A and the Kuf_bar product (5 -> 3 M^2 N products per GP; results agree with
 * the Cholesky route to ~1e-13 of scale).  Q inverts Kuu explicitly, so every evaluation checks ||L||_F^2 ||W||_F^2
 * (>= cond_2(Kuu + jitter I)) per GP on the device: above 4 M^2 the handle's status word is raised and the next
 * gp_check_not_pd / host-scalar call returns GP_ERR_UNSUPPORTED ("qform: ...") and clears it.  Predictions, samples and every
 * other family keep the Cholesky route.  Default 0: today's path; GPITCH_AMD_SWITCHES=qform=0 overrides an enable.
 * enable is a bit mask.  Bit 0 is the permission above.  Bit 1 (with bit 0): the caller vouches that the inducing inputs of every
 * MercerMatern12sm latent GP ascend.  With frames promised ascending as well (gp_pdgp_set_frames_ascending) and M <= 1024 the
 * product then contracts, per group of 256 frames, only the rows of Kuf within a lengthscale of the group, and adds the rows
 * beyond through two tables of rank 2 * partials (padded to a multiple of 4) each: the same G to rounding, bit-identical when
 * every row is near.  GPITCH_AMD_SWITCHES=qform_far=0 overrides bit 1.  Bit 2 (with bits 0 and 1): the backward pass may form
 * Kuf diag(2 gv) Kuf^T and Kuf gm of those GPs from the same near rows and far field instead of the dense split-K product, which
 * then covers the other latent GPs (taken when those are one run of the batch; the same gradient to rounding, ~1e-12 of a
 * block's scale).  GPITCH_AMD_SWITCHES=qform_qbar=0 overrides bit 2. */
gp_status gp_pdgp_set_qform(gp_pdgp_plan p, int32_t enable);
/* 1 when the batch last bound by gp_pdgp_elbo (or its staged forms) took that near-rows-plus-far-field product, else 0 */
int32_t gp_pdgp_far_field(gp_pdgp_plan p);
/* 1 when that batch's backward pass takes the far field too (bit 2 above), else 0 */
int32_t gp_pdgp_far_field_backward(gp_pdgp_plan p);
/* Debug, read-only: what the device made of the far field for latent GP number `i` of the run that took it (0 <= i < run length)
 * at the batch last bound and evaluated.  Waits for the handle's streams, then copies to HOST buffers: rng [2 groups] (kbeg, kend
 * per group of 256 frames) and ref [2 groups] (bmin, bmax); and, when the backward pass took the far field too and the three
 * pointers are given, rng2 [2 groups] (the ranges widened to monotone) and the tile tables s0 / sa [M / 16 each].  gp_index
 * (may be NULL) receives the GP's index in the plan.  Returns the number of groups written; 0 when the batch did not take the
 * far field, i is outside the run, or the run has more than cap_groups groups (nothing is written then).  Launches nothing. */
int32_t gp_debug_pdgp_far_ranges(gp_pdgp_plan p, int32_t i, int32_t cap_groups, int32_t* gp_index, int32_t* rng, double* ref,
                                 int32_t* rng2, int32_t* s0, int32_t* sa);

/* Permission for the activations' far field, from a caller that knows the inducing inputs of every Matern-3/2
 * latent GP of the plan ascend.  enable != 0: when ALL Matern-3/2 latent GPs of a whitened plan have float64 strips, the batch's
 * one M (a multiple of 16, at most 1024), fixed inducing inputs (no need_z), sit in one run of the batch, the frames are promised
 * ascending (gp_pdgp_set_frames_ascending), the batch is a multiple of 256 frames and a strip has 2^20 entries or more,
 * gp_pdgp_elbo and its staged forms form their A = W Kuf and the column sums of (Lq^T A)^2 per group of 256 frames from the rows
 * of Kuf whose inducing inputs lie inside the group's span, and add the rows beyond through two exact M x 2 tables per side
 * (a Matern-3/2 Kuf is semiseparable along sorted inputs): the same A to rounding.  Nothing is inverted that the dense route
 * does not invert.  Predictions, samples and every other family keep the dense products.  Default 0: the dense products;
 * GPITCH_AMD_SWITCHES=act_far=0 overrides an enable. */
gp_status gp_pdgp_set_far_act(gp_pdgp_plan p, int32_t enable);
/* 1 when the batch last bound qualifies for that route, else 0.  It speaks of ELBO evaluations (gp_pdgp_elbo and its staged
 * forms), which take the route when it is 1; a prediction binds the batch too and always runs the dense products. */
int32_t gp_pdgp_far_field_act(gp_pdgp_plan p);
/* Permission for the scan's far-field moments.  enable != 0 (the default): a Matern-3/2 family that contracts its
 * Kuf_bar by the scan (fixed inducing inputs, frames promised ascending) and whose latent GPs are all in the run that takes the
 * activations' far field above forms the scan's chunk moments and near sums from that far field's factors instead of a pass
 * over the stored A: the same sums to rounding.  enable == 0: the pass over A.  GPITCH_AMD_SWITCHES=scan_far=0 overrides an
 * enable.  It lets one handle evaluate both forms. */
gp_status gp_pdgp_set_scan_far(gp_pdgp_plan p, int32_t enable);
/* 1 when the last gradient evaluation's bind chose that form for some family, else 0 (0 after a bind without a gradient). */
int32_t gp_pdgp_scan_far(gp_pdgp_plan p);
/* Permission for H = A diag(2 gv) A^T and u = A gm of the activations from the stored A once and the far field's factors once
 * (DESIGN.md 3.10).  enable != 0 (the default): in a plan of float64 strips throughout, the run that takes the activations' far
 * field above forms, per group of 256 frames, Y = A diag(2 gv) B^T (B: the rows of Kuf near the group and the four rows of Psi)
 * in one pass over the stored A and then H = sum Y P^T (P: W's near columns and the far field's tables) instead of the dense
 * split-K product over all frames: the same H to rounding, symmetric to the bit.  The latent GPs left to the dense product must
 * be one run of the batch, or none; else every GP keeps it.  enable == 0: the dense product.  GPITCH_AMD_SWITCHES=h_far=0 overrides
 * an enable.  Equal frames across a group boundary together with equal inducing inputs across a tile boundary — which
 * gp_pdgp_set_frames_ascending and gp_pdgp_set_far_act promise away — fail the evaluation with GP_ERR_BAD_ARG. */
gp_status gp_pdgp_set_h_far(gp_pdgp_plan p, int32_t enable);
/* 1 when the last gradient evaluation's bind chose that form, else 0 (0 after a bind without a gradient). */
int32_t gp_pdgp_h_far(gp_pdgp_plan p);
/* Debug, read-only: as gp_debug_pdgp_far_ranges for latent GP number `i` of the activation far field's run — rng [2 groups]
 * (kbeg, kend per group of 256 frames), ref [2 groups] (the group's smallest and largest frame time).  Returns the groups written. */
int32_t gp_debug_pdgp_act_ranges(gp_pdgp_plan p, int32_t i, int32_t cap_groups, int32_t* gp_index, int32_t* rng, double* ref);

/* Pdgp.build_likelihood (pdgp.py:133-170) on the batch (x, y) of n frames:
 *   elbo = (num_data / n) * sum_n varexp_n - KL.   elbo_dev points to TWO device doubles: [0] the ELBO, [1] the
 * summed KL term (Pdgp.build_prior_kl, pdgp.py:113-131).  When
 * elbo_host != NULL the ELBO is also copied to the host (syncs).  When grad != NULL also writes d elbo / d params
 * (constrained space, layout above) — what TF reverse-mode provides through Model.optimize. */
gp_status gp_pdgp_elbo(gp_pdgp_plan p, const double* params, const double* x, const double* y, int32_t n,
                       double num_data, double* elbo_dev, double* elbo_host, double* grad);

/* Pitch-sharded evaluation of ONE Pdgp model over several GPUs (one process per GPU).  Each rank builds a plan
 * over its own subset of the P sources (both GPs of a pitch on the same rank; the noise variance params[0] is
 * replicated).  The likelihood (likelihoods.py:47-68) couples sources only through three per-frame sums
 *   A = sum_i E1_i m_f,i ,  B = sum_i E2_i (v_f,i + m_f,i^2) ,  D = sum_i (E1_i m_f,i)^2     (C = A^2 - D),
 * so the exchange step is ONE sum-all-reduce of 3n+1 doubles (the last slot carries the KL terms):
 *   gp_pdgp_elbo_begin  : conditionals of the local GPs; writes the local [A | B | D | sum KL] to exchange[0..3n]
 *   -- caller: ncclAllReduce(exchange, 3n+1, ncclSum) ordered after begin / before end on the handle's stream --
 *   gp_pdgp_elbo_end    : likelihood + noise gradient from the reduced sums (identical on every rank), local
 *                         backward pass; elbo_dev / elbo_host / grad as in gp_pdgp_elbo (the ELBO is the whole
 *                         model's; grad covers this rank's parameters, and grad[0] is the full noise gradient).
 * No collective is needed in the backward pass.  begin and end must be called with the same params, n and grad. */
gp_status gp_pdgp_elbo_begin(gp_pdgp_plan p, const double* params, const double* x, const double* y, int32_t n,
                             double* grad, double* exchange);
gp_status gp_pdgp_elbo_end(gp_pdgp_plan p, const double* params, const double* x, const double* y, int32_t n,
                           double num_data, const double* exchange, double* elbo_dev, double* elbo_host,
                           double* grad);

/* GP-sharded evaluation of ONE Pdgp model over several GPUs (option 2; one process per GPU).  The 2 P
 * conditionals of Pdgp.build_likelihood are independent (pdgp.py:146-155) and the likelihood needs only (fmean, fvar) of
 * every latent GP (likelihoods.py:422-447), so the latent GPs themselves are the sharding unit: 24 GPs at P = 12 are 3
 * per GPU on 8 GPUs (ceiling 8x; the pitch-sharded form above: 6x).
 *   gp_pdgp_create_subset : a plan over `count` of the model's 2 P latent GPs; gp_index[l] (strictly increasing) is the row
 *                           in the model's order [g_0..g_{P-1}, f_0..f_{P-1}] (pdgp.py:157-164).  `cfg` describes the WHOLE
 *                           model.  The parameter vector holds [noise | the listed GPs] (gp_pdgp_layout by local index).
 *   gp_pdgp_cond_begin    : conditionals of the local GPs -> fmean_local, fvar_local ([count][n], caller's buffers: the
 *                           send buffer of the exchange) and the sum of the local KL terms -> kl_local_sum[0].
 *   -- caller: ONE all-gather of 2 n doubles per latent GP (+ the KL scalar) on the handle's stream --
 *   gp_pdgp_cond_end      : likelihood of the whole model from fmean_full / fvar_full ([2 P][n], model order; computed
 *                           identically on every rank, so the replicated noise variance stays in step) with kl_total[0]
 *                           = the KL sum over all ranks; local backward pass.  elbo_dev / elbo_host / grad as in
 *                           gp_pdgp_elbo (grad covers this plan's parameters; grad[0] is the full noise gradient).
 * No collective in the backward pass.  gp_pdgp_predict on such a plan takes mean_source = NULL. */
gp_status gp_pdgp_create_subset(gp_handle h, const gp_pdgp_config* cfg, const int32_t* gp_index, int32_t count,
                                gp_pdgp_plan* out);
gp_status gp_pdgp_cond_begin(gp_pdgp_plan p, const double* params, const double* x, int32_t n, double* grad,
                             double* fmean_local, double* fvar_local, double* kl_local_sum);
gp_status gp_pdgp_cond_end(gp_pdgp_plan p, const double* params, const double* x, const double* y, int32_t n,
                           double num_data, const double* fmean_full, const double* fvar_full, const double* kl_total,
                           double* elbo_dev, double* elbo_host, double* grad);

/* ---- the sharded forms with their exchange step INSIDE the call (the handle owns "workspace, stream,
 * RCCL comm"; section 8e).  The reference has no distributed code: nothing of it is replaced here beyond what
 * gp_pdgp_elbo_begin/_end, gp_pdgp_cond_begin/_end and gp_sgpr_bound_begin/_end replace (pdgp.py:133-170, sgpr_ss.py:29-71);
 * these entry points issue the collective the "-- caller: --" lines above ask for themselves — ncclAllReduce / ncclAllGather
 * of RCCL on the handle's stream, between the two stages — so that one evaluation, and with `adam` one whole optimiser step,
 * is ONE enqueue with no host code in between.  RCCL is bound at run time (the copy already in the process, else
 * /opt/rocm/lib/librccl.so); without it gp_comm_create returns GP_ERR_UNSUPPORTED and nothing else is affected.
 *   gp_comm_unique_id : rank 0 fills 128 bytes (ncclGetUniqueId) and hands them to every rank by any channel
 *                       (torch.distributed broadcast, a file, MPI ...)
 *   gp_comm_create    : every rank, same id: ncclCommInitRank on the handle's device; the communicator's collectives run on
 *                       the handle's stream.  Plans used with a communicator must live on the same handle.
 * gp_adam_args (may be NULL): gp_adam_step's arguments, applied right behind the evaluation (params is updated in place). */
typedef struct gp_comm_s* gp_comm;
typedef struct {
  double* free_state; const uint8_t* tcode; double* m; double* v;
  int64_t nparams; int64_t t; double lr, beta1, beta2, eps;
} gp_adam_args;
gp_status gp_comm_unique_id(uint8_t* id128);
gp_status gp_comm_create(gp_handle h, const uint8_t* id128, int32_t rank, int32_t world, gp_comm* out);
gp_status gp_comm_destroy(gp_comm c);
int32_t gp_comm_world(gp_comm c);
int32_t gp_comm_rank(gp_comm c);
gp_status gp_comm_allreduce_sum(gp_comm c, double* buf, int64_t count);      /* in place, float64, on the handle's stream */
/* pitch-sharded: gp_pdgp_elbo_begin -> all-reduce of exchange[0 .. 3n] -> gp_pdgp_elbo_end [-> gp_adam_step] */
gp_status gp_pdgp_elbo_pitch_sharded(gp_pdgp_plan p, gp_comm c, double* params, const double* x, const double* y, int32_t n,
                                     double num_data, double* exchange, double* elbo_dev, double* elbo_host, double* grad,
                                     const gp_adam_args* adam);
/* GP-sharded: gp_pdgp_cond_begin -> all-gather of one block per rank -> rows assembled in the model's order ->
 * gp_pdgp_cond_end [-> gp_adam_step].  num_gps = 2 P; local_gps = this plan's count; latent GP g lives on rank g mod world
 * as its (g div world)-th row.  With per = ceil(num_gps / world): send holds 2 per n + 8 doubles
 * [fmean rows | fvar rows | KL sum + pad], recv world times that, full 2 num_gps n + 8 ([fmean | fvar | KL total]). */
gp_status gp_pdgp_elbo_gp_sharded(gp_pdgp_plan p, gp_comm c, double* params, const double* x, const double* y, int32_t n,
                                  double num_data, int32_t num_gps, int32_t local_gps, double* send, double* recv, double* full,
                                  double* elbo_dev, double* elbo_host, double* grad, const gp_adam_args* adam);
/* frame-sharded SGPRSS: gp_sgpr_bound_begin -> all-reduce(exchange) -> gp_sgpr_bound_end (the frame-independent terms on
 * rank 0) [-> all-reduce(grad)]: bound and, when grad != NULL, the full gradient on every rank. */
gp_status gp_sgpr_bound_grad_sharded(gp_sgpr_plan p, gp_comm c, const double* params, const double* X, const double* Y, int32_t N,
                                     int64_t N_total, const double* Z, double* exchange, double* bound_dev, double* bound_host,
                                     double* grad);

/* Pdgp.predict_act / predict_com / predict_act_n_com (pdgp.py:172-208): conditionals at xnew for all 2P
 * GPs.  fmean/fvar: 2P x n row-major (row g as in gp_pdgp_layout).  mean_source (P x n, may be NULL)
 * = nlinfun(mean_act_i) * mean_com_i (pdgp.py:207). */
gp_status gp_pdgp_predict(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n,
                          double* fmean, double* fvar, double* mean_source);
/* The same at further inputs WITHOUT rebuilding Kuu and its Cholesky factor / inverse: valid only when params hold
 * the values of the preceding gp_pdgp_predict[_reuse] call on this plan (no ELBO evaluation or parameter update in
 * between).  pdgp.py:17-44 (predict_windowed) re-factorises for every window and for act / com separately. */
gp_status gp_pdgp_predict_reuse(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n,
                                double* fmean, double* fvar, double* mean_source);

/* gp_pdgp_predict / _reuse into the plan's workspace, then the moments of gp_mpd_predict_moments at xnew with the plan's
 * nonlinearity and the noise variance params[0]: the 2P x n conditional moments never leave the device.  smean / svar:
 * P x n row-major; ymean / yvar / logp: n values; every output may be NULL.  ynew (n device values, may be NULL) is needed
 * for logp only.  with_noise = 0 leaves the noise variance out of yvar (the latent mixture sum_i nlin(g_i) f_i).  A subset
 * (GP-sharded) plan holds only some rows: GP_ERR_BAD_ARG.  Synchronises and reports a failed factorisation as
 * gp_pdgp_predict does; _reuse under gp_pdgp_predict_reuse's condition (either pair of entries may have made the
 * factorisation). */
gp_status gp_pdgp_predict_moments(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, const double* ynew,
                                  int32_t with_noise, double* smean, double* svar, double* ymean, double* yvar, double* logp);
gp_status gp_pdgp_predict_moments_reuse(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n,
                                        const double* ynew, int32_t with_noise, double* smean, double* svar, double* ymean,
                                        double* yvar, double* logp);

/* Joint posterior draws of every latent GP and every source nlin(g_i) f_i of the model under q, by Matheron's rule: S draws
 * that are jointly distributed across the n frames of xnew; latent GPs are independent under q.  Per latent GP r (rows as in
 * gp_pdgp_layout, M_r inducing inputs z_r, W_r = chol(Kuu_r + jitter I)^-1 from the plan):
 *   prior path along the merged sorted points (xnew | z_r) by an exact state-space recursion: GP_KERN_MATERN12 (1 normal per
 *   point), GP_KERN_MATERN32 (state (f, f'), 2 normals per point), GP_KERN_MERCER_MATERN12SM / GP_KERN_MATERN12SM (a_k cos +
 *   b_k sin per partial, 2 m normals per point); any other kernel: GP_ERR_UNSUPPORTED.  A point that coincides with its
 *   predecessor repeats its value exactly.
 *   u0 = prior(z_r) + sqrt(jitter) eps_u[0];  beta = W^T (q_mu + tril(q_sqrt) eps_u[1] - W u0)   (whitened plan)
 *                                             beta = W^T W (q_mu + tril(q_sqrt) eps_u[1] - u0)   (unwhitened plan)
 *   draw_r(x*) = prior_r(x*) + K_r(x*, z_r) beta;   source_i = nlin(draw_i) * draw_{P+i}.
 * Arguments:
 *   order_host  HOST array, the 2P merges back to back: GP r's n + M_r entries are a stable ascending argsort of
 *               (xnew | z_r); entry < n is a frame, n + i is z_r[i].  Each is checked to be a permutation before anything is
 *               enqueued (GP_ERR_BAD_ARG otherwise).
 *   eps_x, eps_z, eps_u (device): the GPs' blocks back to back, GP r's being [S][c_r][n], [S][c_r][M_r], [S][2][M_r] with c_r
 *               the normals per point above; blocks are indexed by the caller's own point order.
 *   latents [2P][S][n] (device, required), sources [P][S][n] (device, may be NULL).
 * The map is affine in eps per GP: eps = 0 gives gp_pdgp_predict's fmean and mean_source, the linear part T_r has
 * T_r T_r^T = the full-covariance conditional of GP r.  workspace: gp_pdgp_sample_workspace_bytes(2P, max_r M_r, sum_r c_r,
 * n, S) bytes, 256-byte aligned (a short one: GP_ERR_BAD_ARG); n is bounded by it, not by max_batch; M_r <= 1024.  A subset
 * (GP-sharded) plan: GP_ERR_BAD_ARG.  gp_pdgp_sample factorises Kuu at `params` (without a conditional); _reuse under
 * gp_pdgp_predict_reuse's condition.  Both synchronise and report a failed factorisation as gp_pdgp_predict does.  float64
 * throughout whatever the plan's strip precision.  Deterministic, no atomics: bit-identical between calls, and draw s depends
 * on nothing but its own eps. */
gp_status gp_pdgp_sample(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, const int32_t* order_host,
                         int32_t S, const double* eps_x, const double* eps_z, const double* eps_u, double* latents,
                         double* sources, void* workspace, size_t workspace_bytes);
gp_status gp_pdgp_sample_reuse(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, const int32_t* order_host,
                               int32_t S, const double* eps_x, const double* eps_z, const double* eps_u, double* latents,
                               double* sources, void* workspace, size_t workspace_bytes);
/* handle-free, runs without a device: the one carve of the sampling operator, measured (0 for an empty problem).  G latent
 * GPs of at most maxM inducing inputs, C = sum_r c_r normals per point, n frames, S draws. */
size_t gp_pdgp_sample_workspace_bytes(int32_t G, int32_t maxM, int32_t C, int32_t n, int32_t S);

/* ---- overlap-add of per-window predictions (gpitch/window_overlap.py:19-59: merged_mean / merged_variance) ----------
 * windows: num_windows x ws (row-major, leading dimension ld) device array of per-window means (square = 0) or
 * variances (square = 1: squared Hann weights); ws odd, 50 % overlap (hop (ws-1)/2); out: n = (ws-1)/2 *
 * (num_windows + 1) + 1 frames.  First / last half-windows are kept flat exactly as the reference does. */
gp_status gp_overlap_merge(gp_handle h, const double* windows, int32_t num_windows, int32_t ws, int64_t ld, int32_t n,
                           int32_t square, double* out);

/* ---- optimiser on the free state (GPflow Model.optimize with tf.train.AdamOptimizer;
 *      demo-modgp.py:44-45; transforms: GPflow Log1pe 'positive') -----------------------------------
 * tcode[i]: 0 identity, 1 positive (y = log(1+e^x) + 1e-6), 2 fixed (identity, no update),
 *           3.. gpflow.transforms.Logistic(a, b): y = a + (b-a)/(1+e^-x), with (a, b) registered on the handle
 *           (kernels.py:219-223 Logistic(0,2) / Logistic(0,0.25); init_models.py:189 Logistic(0,0.5)). */
gp_status gp_transform_register_logistic(gp_handle h, double a, double b, uint8_t* code_out);
gp_status gp_transform_forward(gp_handle h, const double* free_state, const uint8_t* tcode, int64_t n,
                               double* params);
gp_status gp_transform_backward(gp_handle h, const double* params, const uint8_t* tcode, int64_t n,
                                double* free_state);
/* One Adam step maximising the ELBO: g_free = -(grad * dparams/dfree); TF-1.2 update rule; then
 * params = transform(free).  t is the 1-based step count. */
/* A failed Cholesky inside an asynchronous evaluation (sync-free training loops) sets a device flag; while it is set
 * gp_adam_step leaves the free state, the parameters and the moments untouched, so a training loop cannot walk on from
 * garbage gradients (the reference's TF session raises at the offending step).  gp_poll_not_pd looks at the flag without
 * blocking (pinned copy + event): *flag = 1 once a failure has been observed; gp_check_not_pd (drains the streams; or any
 * call that returns a host scalar) then gives GP_ERR_NOT_PD with the pivot index and clears the flag. */
gp_status gp_poll_not_pd(gp_handle h, int32_t* flag);
gp_status gp_check_not_pd(gp_handle h);
/* gp_take_not_pd: asynchronous per-evaluation snapshot — behind everything enqueued so far, copies the device status
 * word {flag, pivot index, matrix index (= window slot in a gp_sgprb_* batch), spare} into host_status4 (pinned host
 * memory, read it after an event recorded behind this call) and clears the device word, so a failure is reported by the
 * evaluation that caused it and does not leak into the next user of the handle.  Replaces what the reference gets from
 * TF raising InvalidArgumentError inside the one session.run that failed (transcription.py:283 per window). */
gp_status gp_take_not_pd(gp_handle h, int32_t* host_status4);
gp_status gp_adam_step(gp_handle h, double* free_state, double* params, const double* grad,
                       const uint8_t* tcode, double* m, double* v, int64_t n, int64_t t, double lr,
                       double beta1, double beta2, double eps);

/* One natural-gradient step on the variational posteriors q(u_r) = N(q_mu_r, tril(q_sqrt_r) tril(q_sqrt_r)^T) of a Pdgp plan,
 * from the gradient gp_pdgp_elbo has just written into `grad` (natgrad.hip; the GPflow releases after 0.5 have it as
 * NatGradOptimizer, the reference moves q entry by entry with Adam: demo-modgp.py:44-45).  A natural gradient does not change
 * under a linear change of the Gaussian's variable, so the same map serves whitened and unwhitened plans.  Per latent GP r with
 * Lq = tril(q_sqrt), g = grad's q_mu block, G_L = tril(grad's q_sqrt block):
 *   Phi = tril(Lq^T G_L),  P = (Phi + Phi^T - diag(Phi)) / 2   ( = Lq^T (d ELBO / d S) Lq, symmetric ),   B = I - 2 gamma P
 *   B = U U^T, U upper triangular (the Cholesky factor of the index-reversed matrix: J B J = C C^T, U = J C J)
 *   Lq' = Lq U^-T   (lower triangular; S' = Lq' Lq'^T has S'^-1 = S^-1 - 2 gamma d ELBO / d S)
 *   q_mu' = q_mu + gamma Lq' (Lq'^T g)
 * i.e. theta_1 += gamma (g - 2 G^ q_mu), theta_2 += gamma G^ in the natural parameters (G^ = d ELBO / d S).  Lq is never
 * inverted.  tril(q_sqrt) receives Lq', the strict upper triangle of the stored block is left as it is; the values go to
 * `params` and to `free_state` (both Params have the identity transform), and the q_mu / q_sqrt blocks of `grad` are zeroed,
 * so that a gp_adam_step behind this call on the same gradient moves every other parameter and leaves these alone.
 * step_gp_host (HOST array, one flag per latent GP in gp_pdgp_layout's order, NULL = all): the GPs that take the step.
 * Refusal: every B is factored before anything is written.  If one is not positive definite (the step was too long) the
 * handle's status word is raised exactly as by a failed Kuu factorisation, NO GP's state is written and the gradient stays, and
 * gp_adam_step freezes; gp_poll_not_pd / gp_check_not_pd report GP_ERR_NOT_PD.  The workspace's first four int32 then read
 * {1, latent GP index, pivot, 1}; they read {0, ...} after a step that was taken, and are left alone by a call that finds the
 * status word already raised.  Three launches on the handle's stream, float64 whatever the plan's strip precision, no atomics,
 * every sum in a fixed order (bit-identical between calls); no host synchronisation.  M <= 4096 per latent GP
 * (GP_ERR_UNSUPPORTED); a subset (GP-sharded) plan: GP_ERR_BAD_ARG.
 * workspace: gp_pdgp_natgrad_workspace_bytes(plan) bytes, 256-byte aligned — per latent GP the reversed B (then its factor),
 * the factor's inverse and Lq^T g, sized by the same carve that lays it out. */
size_t gp_pdgp_natgrad_workspace_bytes(gp_pdgp_plan p);
gp_status gp_pdgp_natgrad_step(gp_pdgp_plan p, double* params, double* free_state, double* grad, double gamma,
                               const int32_t* step_gp_host, void* workspace, size_t workspace_bytes);
/* The same step with one length per latent GP and automatic halving.  gamma_gp_host (HOST, one double in
 * (0, 1] per latent GP of the plan in gp_pdgp_layout's order, read for every GP whether stepped or not) gives gamma_r;
 * halvings in 0..10.  GP r takes the map above at gamma_r 2^-j_r, in B and in q_mu', where j_r is the smallest j in
 * 0..halvings for which I - 2 gamma_r 2^-j P_r factors with every pivot positive (the factorisation's own test, nothing
 * stricter).  gamma 2^-j is an exact scaling, and at j = 0 the arithmetic is gp_pdgp_natgrad_step's: with nothing to halve the
 * two entries write the same bits.  Every length is decided before anything is written, the GPs decide independently, and the
 * next call starts from gamma_r again.  Launches: per round j = 0..halvings a form launch per 64 GPs (only GPs still pending
 * are formed; a round with none pending returns after reading one word), one factorisation launch with a per-matrix outcome
 * (size 0 for the GPs already accepted: their factor and inverse stay) and a one-workgroup launch that settles the outcomes;
 * then the apply launch.  No host synchronisation.
 * Refusal: a GP with no acceptable j <= halvings refuses the step of every GP exactly as above — the apply launch raises the
 * handle's status word {1, pivot, slot} itself, nothing is written, gp_adam_step freezes, the first four int32 of the
 * workspace read {1, latent GP index, pivot at the last length tried (gamma_r 2^-halvings), 1}; of several exhausted GPs the
 * first in the plan's order is named.
 * Counters, per latent GP of the plan, kept in the workspace: the sum of j_r over the calls and the smallest length taken.
 * gp_pdgp_natgrad_counts copies them to the host (both arrays, one entry per latent GP; synchronises the stream) and, with
 * clear != 0, resets them afterwards; both host pointers NULL with clear != 0 only resets.  A fresh workspace must be reset
 * once before its first step.  A GP that took no step since the reset reports 0 and +infinity (the caller knows gamma_r).  A
 * refused step counts nothing.
 * Argument errors, alignment, GP_ERR_WORKSPACE, the subset-plan refusal and M <= 4096 as in gp_pdgp_natgrad_step; a gamma
 * outside (0, 1] or halvings outside 0..10: GP_ERR_BAD_ARG.
 * workspace: gp_pdgp_natgrad_adaptive_workspace_bytes(plan) bytes (0 for a null plan), 256-byte aligned: the plain step's
 * carve, then the accepted j and the round's outcome per GP, the control words and the counters. */
size_t gp_pdgp_natgrad_adaptive_workspace_bytes(gp_pdgp_plan p);
gp_status gp_pdgp_natgrad_step_adaptive(gp_pdgp_plan p, double* params, double* free_state, double* grad,
                                        const double* gamma_gp_host, int32_t halvings, const int32_t* step_gp_host,
                                        void* workspace, size_t workspace_bytes);
gp_status gp_pdgp_natgrad_counts(gp_pdgp_plan p, const void* workspace, int64_t* halvings_host, double* shortest_host,
                                 int32_t clear);

/* ---- L3 model: SGPRSS (gpitch/sgpr_ss.py:10-114) ---------------------------------------------- */
typedef struct {
  int32_t num_kernels;          /* P kernels in the GPflow Add (kern.kern_list) */
  int32_t max_N;
  int32_t M;
  const int32_t* kern_type;     /* host, P entries */
  const int32_t* partials;      /* host, P entries */
  double jitter;
  int32_t reg;                  /* sgpr_ss.py:64-68: subtract 1000 * sum |variance_p| */
} gp_sgpr_config;
/* parameter vector: [ noise_var | theta_0 | ... | theta_{P-1} ]  (Z is a DataHolder: sgpr_ss.py:26) */
gp_status gp_sgpr_create(gp_handle h, const gp_sgpr_config* cfg, gp_sgpr_plan* out);
gp_status gp_sgpr_destroy(gp_sgpr_plan p);
int64_t gp_sgpr_num_params(gp_sgpr_plan p);
/* as gp_pdgp_set_precision: float32 strips (Kuf, A = L^-1 Kuf, Kuf_bar) and float32 matrix-core strip products for
 * the collapsed bound, its gradient and predict_f; Kuu, B = A A^T + I (accumulated in float64), both Cholesky factors
 * and the bound's scalars stay float64.  predict_s (exact N x N posterior) is float64 regardless. */
gp_status gp_sgpr_set_precision(gp_sgpr_plan p, int32_t bits);
size_t gp_sgpr_workspace_bytes(gp_sgpr_plan p);
gp_status gp_sgpr_set_workspace(gp_sgpr_plan p, void* workspace, size_t bytes);
/* SGPRSS.build_likelihood (sgpr_ss.py:29-71), D = 1 output column.  bound_host may be NULL. */
gp_status gp_sgpr_bound(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                        const double* Z, double* bound_dev, double* bound_host);
/* The bound and its gradient w.r.t. the parameter vector (what TF autodiff gives L-BFGS-B in SGPRSS.optimize:
 * transcription.py:283, separation.py:298).  grad has gp_sgpr_num_params entries. */
gp_status gp_sgpr_bound_grad(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                             const double* Z, double* bound_dev, double* bound_host, double* grad);
/* d bound / d err_n, err = Y - mean_function(X) (sgpr_ss.py:40), of the evaluation gp_sgpr_bound_grad has JUST run with the same
 * params, Y and N: r = A'^T (dF/du) - err / sigma^2, N doubles on the device.  This is what a GPflow mean function's trainable
 * Params (gpflow.mean_functions.Constant.c, Linear.A / .b; sgpr_ss.py:14,25) are differentiated through — TF autodiff in the
 * reference: d bound / d theta_m = - sum_n r_n d mean(x_n) / d theta_m.  GP_ERR_BAD_ARG when no such evaluation precedes it. */
gp_status gp_sgpr_residual_grad(gp_sgpr_plan p, const double* params, const double* Y, int32_t N, double* r_dev);

/* One window sharded over its FRAMES across several GPUs (one process per GPU; SURVEY 8e: "SGPRSS single large
 * window").  Each rank holds a slice (X, Y) of N frames; Z and params are replicated.  The collapsed bound couples
 * the slices only through H = A'A'^T (M x M), u = A'y (M), sum y^2 and tr(H):
 *   gp_sgpr_bound_begin : local Kuf, A' = L^-1 Kuf, H, u, scalars -> exchange[0 .. gp_sgpr_exchange_doubles())
 *   -- caller: ncclAllReduce(exchange, M*M + M + 2, sum) --
 *   gp_sgpr_bound_end   : Cholesky of B, the bound for N_total frames (identical on every rank) and, when
 *                         grad != NULL, this rank's share of the gradient: the frame-dependent terms of its slice,
 *                         plus the frame-independent ones (noise, Kdiag, Kuu side, L1 penalty) only when
 *                         include_replicated != 0 (pass 1 on exactly one rank)
 *   -- caller: ncclAllReduce(grad, gp_sgpr_num_params, sum) -> the full gradient everywhere. */
int64_t gp_sgpr_exchange_doubles(gp_sgpr_plan p);
gp_status gp_sgpr_bound_begin(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                              const double* Z, double* exchange);
gp_status gp_sgpr_bound_end(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                            int64_t N_total, const double* Z, const double* exchange, double* bound_dev,
                            double* bound_host, double* grad, int32_t include_replicated);

/* gp_sgpr_bound_grad is launch-bound at window sizes (N ~ 2001, ~50 small kernels), and L-BFGS-B calls it dozens
 * of times per window with the same buffers: from the second call with identical pointer arguments the launch
 * sequence is recorded into a hipGraph and replayed.  Needs a handle created on a real stream (the legacy null
 * stream cannot be captured) and timers off; otherwise the launches stay eager.  enable = 0 turns it off.
 * gp_sgpr_eval_counts reports how many evaluations ran eagerly / were captured / were replayed. */
gp_status gp_sgpr_set_graphs(gp_sgpr_plan p, int32_t enable);
gp_status gp_sgpr_eval_counts(gp_sgpr_plan p, int64_t* eager, int64_t* captured, int64_t* replayed);
/* GPflow SGPR.build_predict (predict_f; separation.py:306) at Xnew: mean, var (n values each) */
gp_status gp_sgpr_predict_f(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                            const double* Z, const double* Xnew, int32_t n, double* mean, double* var);
/* SGPRSS.build_predict_source / predict_s (sgpr_ss.py:73-114): exact GP with an N x N Cholesky;
 * mean/var are P x n row-major.  workspace: gp_sgpr_predict_source_workspace_bytes(N, n). */
/* full_cov = True forms (SGPR.build_predict / sgpr_ss.py:95-99; unused by the reference's callers): cov is n x n
 * (predict_f) or [P][n][n] (predict_source), row-major; `var` still receives the diagonal form.  float64 plans. */
gp_status gp_sgpr_predict_f_full(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                                 const double* Z, const double* Xnew, int32_t n, double* mean, double* var, double* cov);
gp_status gp_sgpr_predict_source_full(gp_sgpr_plan p, const double* params, const double* X, const double* Y,
                                      int32_t N, const double* Xnew, int32_t n, double* mean, double* var, double* cov,
                                      void* workspace, size_t workspace_bytes);
size_t gp_sgpr_predict_source_workspace_bytes(int32_t N, int32_t n);
gp_status gp_sgpr_predict_source(gp_sgpr_plan p, const double* params, const double* X, const double* Y,
                                 int32_t N, const double* Xnew, int32_t n, double* mean, double* var,
                                 void* workspace, size_t workspace_bytes);

/* Sparse per-source posterior: source p under the optimal q(u) of the collapsed bound, at O(M^2 n) per source and
 * independent of N.  The sources are independent a priori, so cov(f_p(x*), u) = K_p(x*, Z); with L, LB, c as in
 * sgpr_ss.py:43-53 (the plan's forward state W = L^-1, WB = LB^-1, c):
 *   tmp1_p = W K_p(Z, Xnew),  tmp2_p = WB tmp1_p,  smean_p = tmp2_p^T c,
 *   svar_p = Kdiag_p(Xnew) + sum_m tmp2_p^2 - sum_m tmp1_p^2
 * i.e. GPflow 0.5 SGPR.build_predict with the one kernel K_p in place of the sum: sum_p smean_p is gp_sgpr_predict_f's mean
 * and for one kernel both outputs are gp_sgpr_predict_f's.  It sits beside the exact posterior of sgpr_ss.py:73-114
 * (gp_sgpr_predict_source), which it approximates; unlike sgpr_ss.py:101 the variance starts from the source's OWN Kdiag,
 * not the sum kernel's.  mean, var: P x n row-major.  One fused float64 launch (predict_sparse.hip): no M x n array is
 * written, no workspace beyond the plan's is used and n may exceed the plan's max_N (any n >= 1; N <= max_N as ever).
 * Runs the forward pass at `params` first, synchronises and reports a failed factorisation like gp_sgpr_predict_f.
 * Limits: 1 <= M <= 1024 (GP_ERR_UNSUPPORTED before any launch otherwise).  float32 plans (gp_sgpr_set_precision) are
 * taken: the state comes from the plan's float32 forward pass, this kernel's own arithmetic is float64 regardless.
 * Deterministic: bit-identical between calls, and a frame's result does not depend on the other frames of the call. */
gp_status gp_sgpr_predict_source_sparse(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                                        const double* Z, const double* Xnew, int32_t n, double* mean, double* var);

/* Joint posterior draws of every source under the q(u) of gp_sgpr_predict_source_sparse, by Matheron's rule: S draws that
 * are jointly distributed across the n frames AND across the P sources, in O((n + M) m + M n) per source and draw; no
 * n x n matrix is formed.  Every kernel of the sum must have a Matern-1/2 envelope (GP_KERN_MERCER_MATERN12SM,
 * GP_KERN_MATERN12SM, GP_KERN_MATERN12; anything else: GP_ERR_UNSUPPORTED): such a source is a sum of Ornstein-Uhlenbeck
 * processes, a_k cos + b_k sin per partial (2 m components; Matern12: one), drawn exactly by a first-order recursion along
 * sorted time.  The caller supplies the standard normals and the merge:
 *   order_host  HOST array, n + M entries: a stable ascending argsort of t = (Xnew | Z); entry < n is a frame, n + i is z_i.
 *               Checked on the host to be a permutation of 0..n+M-1 before anything is enqueued (GP_ERR_BAD_ARG otherwise).
 *   eps_x [S][C][n], eps_z [S][C][M], eps_u [S][2][M] (device), C = sum_p components_p, sources in kernel order; blocks are
 *               indexed by the caller's own point order.  The eps of a point that coincides with its predecessor is
 *               multiplied by 0.
 *   out [P][S][n] (device).  The map is affine in eps: with eps = 0 it returns gp_sgpr_predict_source_sparse's mean, and its
 *               linear part T has T T^T = the joint posterior covariance, block (p, r) =
 *               delta_pr K_p(x*, x*) - tmp1_p^T tmp1_r + tmp2_p^T tmp2_r (up to the kernels' own 1e-12 under the root).
 * The mean function is not added.  workspace: gp_sgpr_sample_source_workspace_bytes(M, P, C, n, S, 1) bytes, 256-byte
 * aligned (a short one: GP_ERR_BAD_ARG); n may exceed max_N; M <= 1024 (GP_ERR_UNSUPPORTED).  Runs the forward pass at
 * `params`, synchronises and reports a failed factorisation like gp_sgpr_predict_f.  float64 throughout, float32 plans are
 * taken as by gp_sgpr_predict_source_sparse.  Deterministic, no atomics: bit-identical between calls, and draw s depends on
 * nothing but its own eps. */
gp_status gp_sgpr_sample_source_sparse(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                                       const double* Z, const double* Xnew, int32_t n, const int32_t* order_host, int32_t S,
                                       const double* eps_x, const double* eps_z, const double* eps_u, double* out,
                                       void* workspace, size_t workspace_bytes);
/* handle-free, runs without a device: the one carve of the sampling operator (also the window-batched entry's), measured */
size_t gp_sgpr_sample_source_workspace_bytes(int32_t M, int32_t P, int32_t C, int32_t n, int32_t S, int32_t count);

/* The EXACT per-source posterior p(f_p | y) of sgpr_ss.py:73-114 in O(N d^2) instead of O(N^3), with no N x N array and no
 * inducing points: every kernel of the sum must have a Matern-1/2 envelope (GP_KERN_MATERN12, GP_KERN_MERCER_MATERN12SM,
 * GP_KERN_MATERN12SM; anything else: GP_ERR_UNSUPPORTED), so that y = sum_p f_p + noise is a linear-Gaussian state-space
 * model of dimension d = sum_p c_p (c_p = 1 for Matern12, 2 m for a mixture of m partials; 1 <= d <= 128 and 1 <= m <= 32,
 * GP_ERR_UNSUPPORTED otherwise).  A Kalman filter and a Bryson-Frazier backward pass (ssm_smooth.hip) give the smoothed mean
 * and variance of every source at every new frame and the exact log marginal likelihood log p(y).  "Exact" is for the
 * idealised kernels, r = |x - x'|: the covariance builds carry the reference's 1e-12 under the square root, so
 * gp_sgpr_predict_source differs from this by that first-order effect times 1 / noise variance (DESIGN has the figures).
 *   params       the plan's layout [noise variance | theta_0 | ...] (device); Z is not an argument and nothing of the plan's
 *                state is read or changed: no forward pass of the bound runs
 *   order_host   HOST, `steps` entries: the timeline in stable ascending order of time.  Entry < N is training frame X[entry]
 *                (an observed step), entry >= N is new frame Xnew[entry - N].  The N training frames all appear, once each;
 *                a new frame that is bit-equal to a training frame, or to an earlier new frame, shares that step and does not
 *                appear, so N <= steps <= N + n.  Duplicate training frames are separate steps.
 *   out_step_host HOST, n entries: the step of each new frame, in [0, steps)
 *   mean, var    [P][n] (device).  The variance starts from the source's OWN k_p(x, x), as gp_sgpr_predict_source_sparse does;
 *                sgpr_ss.py:101 starts from the sum kernel's: svar_ref = var_p + (Kdiag_sum - Kdiag_p).  The mean function
 *                is not added (Y is the residual).  Both may be null with n = 0 (Xnew and out_step_host too): then only the
 *                forward walk runs
 *   loglik       one double (device): log p(y), from the forward walk
 *   workspace    gp_ssm_smooth_workspace_bytes(d, steps, P, 1) bytes, 256-byte aligned: the history of the forward walk is
 *                steps * d^2 doubles per window.  A short one is GP_ERR_BAD_ARG.
 * Both host arrays are checked before anything is enqueued (order: every training frame once, no entry twice, entries in
 * [0, N + n); out_step in range): GP_ERR_BAD_ARG otherwise.  float64 throughout whatever the plan's precision.  Synchronises.
 * Deterministic, no atomics: two calls are bit-identical and a window's result does not depend on what shares the launch. */
gp_status gp_sgpr_predict_source_ssm(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                                     const double* Xnew, int32_t n, const int32_t* order_host, const int32_t* out_step_host,
                                     int32_t steps, double* mean, double* var, double* loglik, void* workspace,
                                     size_t workspace_bytes);
/* handle-free, runs without a device: the one carve of the smoother (also the window-batched entry's, with `steps` the longest
 * timeline of the call), measured.  0 for arguments outside 1 <= P <= d <= 128, steps >= 1, count >= 1. */
size_t gp_ssm_smooth_workspace_bytes(int32_t d, int32_t steps, int32_t P, int32_t count);

/* S joint draws of every source at the n new frames from the exact posterior of gp_sgpr_predict_source_ssm: joint across frames
 * and across sources, in O(S (N + n) d) behind one gain walk of O((N + n) d^2), by Durbin and Koopman's simulation smoother in
 * its disturbance form (ssm_smooth.hip).  No d x d array is kept per step: the workspace holds 3 steps d doubles per
 * window and steps (d + 2) per draw, where the smoother's holds steps d^2.  Scope, timeline arguments, host checks and error codes
 * are gp_sgpr_predict_source_ssm's; n >= 1 and 1 <= S <= 65535.
 *   eps_x   [S][steps][d] standard normals (device), STEP-major along the merged timeline: entry [s][j][i] drives coordinate i of
 *           the state at step j (the sources' blocks in kern_list order, (a_0, b_0, a_1, b_1, ...) inside a mixture).  The same
 *           normals with another Xnew are another draw.
 *   eps_y   [S][N] standard normals (device), in the caller's frame order: the observation noise of the simulated data
 *   out     [P][S][n] (device).  The map is affine in (eps_x, eps_y): zeros give the smoothed mean of gp_sgpr_predict_source_ssm
 *           (to rounding), and the linear part T has T T^T = the joint posterior covariance of all sources at all new frames.
 *           The mean function is not added; a repeated new frame repeats its value.
 *   workspace  gp_ssm_sample_workspace_bytes(d, steps, P, S, 1) bytes, 256-byte aligned; a short one is GP_ERR_BAD_ARG
 * Every check precedes the first launch.  float64 whatever the plan's precision.  Synchronises.  No atomics, every sum in a fixed
 * order, one wavefront per (window, draw): a draw's bits depend on nothing but its own normals, whatever S. */
gp_status gp_sgpr_sample_source_ssm(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                                    const double* Xnew, int32_t n, const int32_t* order_host, const int32_t* out_step_host,
                                    int32_t steps, int32_t S, const double* eps_x, const double* eps_y, double* out,
                                    void* workspace, size_t workspace_bytes);
/* handle-free, runs without a device: the one carve of the sampling call (also the window-batched entry's, with `steps` the
 * longest timeline of the call), measured.  0 for arguments outside 1 <= P <= d <= 128, steps >= 1, S >= 1, count >= 1. */
size_t gp_ssm_sample_workspace_bytes(int32_t d, int32_t steps, int32_t P, int32_t S, int32_t count);

/* The exact log marginal likelihood log p(y) of gp_sgpr_predict_source_ssm AND its gradient in the plan's parameter layout, in
 * O(N d^2): the forward walk with its history, then a Bryson-Frazier walk over every step that carries the score (ssm_smooth.hip,
 * DESIGN 3c-5).  Same scope and errors as gp_sgpr_predict_source_ssm; the timeline is the N training frames.
 *   order_host   HOST, N entries: a permutation of 0 .. N - 1, the training frames in stable ascending order of time
 *   loglik       one double (device): the bits gp_sgpr_predict_source_ssm writes with n = 0
 *   grad         [gp_sgpr_num_params] (device): d loglik / d [noise variance | theta_0 | ...], constrained parameters
 *   resid_grad   [N] (device) or null: d loglik / d Y in training-frame order (the chain to a mean function)
 *   workspace    gp_ssm_score_workspace_bytes(d, N, P, 1) bytes, 256-byte aligned; a short one is GP_ERR_BAD_ARG
 * Every check precedes the first launch.  float64 whatever the plan's precision.  Synchronises.  No atomics, every sum in a fixed
 * order: two calls are bit-identical. */
gp_status gp_sgpr_exact_loglik_grad(gp_sgpr_plan p, const double* params, const double* X, const double* Y, int32_t N,
                                    const int32_t* order_host, double* loglik, double* grad, double* resid_grad, void* workspace,
                                    size_t workspace_bytes);
/* handle-free, runs without a device: the one carve of the score call (the smoother's carve and the per-step terms), measured.
 * 0 for arguments outside 1 <= P <= d <= 128, steps >= 1, count >= 1. */
size_t gp_ssm_score_workspace_bytes(int32_t d, int32_t steps, int32_t P, int32_t count);

/* ---- many independent SGPRSS windows per launch sequence -------------------------------------------------------
 * replaces the window loop of AMT.optimize / SoSp.optimize (gpitch/transcription.py:265-288, gpitch/separation.py:279-313):
 * for each window, reset_model then model.optimize(maxiter) = a dozen-odd evaluations of SGPRSS.build_likelihood
 * (sgpr_ss.py:29-71) and its gradient.  Windows are independent; this plan evaluates W of them with one sequence of
 * launches (every kernel runs over a window index), so that N = 2001-frame windows fill the device.
 * All windows share max_N (= N), M and the kernel structure of `cfg`; contiguous layouts:
 *   params [W][gp_sgprb_num_params], X [W][N], Y [W][N], Z [W][M], bound_dev [W], grad [W][num_params] (may be NULL).
 * `count` <= W windows (the first `count` slots) are evaluated.  Asynchronous on the handle's stream; from the second
 * call with the same buffers the sequence is replayed from a hipGraph.  M <= 256: the largest inducing-point count of
 * the plan (gp_sgprb_set_inducing_counts gives each slot its own). */
gp_status gp_sgprb_create(gp_handle h, const gp_sgpr_config* cfg, int32_t num_windows, gp_sgprb_plan* out);
gp_status gp_sgprb_destroy(gp_sgprb_plan p);
int64_t gp_sgprb_num_params(gp_sgprb_plan p);
int32_t gp_sgprb_num_windows(gp_sgprb_plan p);
size_t gp_sgprb_workspace_bytes(gp_sgprb_plan p);
gp_status gp_sgprb_set_workspace(gp_sgprb_plan p, void* workspace, size_t bytes);
gp_status gp_sgprb_bound_grad(gp_sgprb_plan p, const double* params, const double* X, const double* Y, const double* Z,
                              int32_t count, double* bound_dev, double* grad);
gp_status gp_sgprb_set_graphs(gp_sgprb_plan p, int32_t enable);
gp_status gp_sgprb_eval_counts(gp_sgprb_plan p, int64_t* eager, int64_t* captured, int64_t* replayed);
/* Windows whose inducing-point counts differ (the drivers pick each window's Z from its own audio: init_liv).
 * counts_host[i] = inducing points of window slot i (1..M) for i < count; slots from `count` on take M.  Z rows beyond
 * counts[i] are ignored (never read).  Each window is evaluated as the exact M-point problem with an identity pad block
 * in Kuu and zero pad rows in Kuf: its bound, gradient and predictions are those of the counts[i]-point window up to
 * rounding, independent of the other slots.  Never called = every slot has M (today's results, bit for bit).  A change
 * of counts rebuilds the descriptors and the recorded graph at the next evaluation. */
gp_status gp_sgprb_set_inducing_counts(gp_sgprb_plan p, const int32_t* counts_host, int32_t count);
/* The rest of SoSp.optimize's loop body (gpitch/separation.py:300-313), window-batched: after a window's optimisation
 * the reference calls model.predict_f(X_i) (GPflow 0.5 SGPR.build_predict) and model.predict_s(X_i) (sgpr_ss.py:73-114).
 * gp_sgprb_predict_f: Xnew [count][n] (n <= N), mean / var [count][n]; runs the forward pass at `params` first.
 * gp_sgprb_predict_source: the exact GP on each window's N frames (N x N Cholesky per window, every launch of the blocked
 * factorisation carrying all windows); Xnew [count][n], mean / var [count][P][n]; workspace from
 * gp_sgprb_predict_source_workspace_bytes(p, count, n) (about 3 N^2 doubles per window), 256-byte aligned.
 * Both synchronise the stream and report a failed factorisation (GP_ERR_NOT_PD). */
gp_status gp_sgprb_predict_f(gp_sgprb_plan p, const double* params, const double* X, const double* Y, const double* Z,
                             const double* Xnew, int32_t n, int32_t count, double* mean, double* var);
size_t gp_sgprb_predict_source_workspace_bytes(gp_sgprb_plan p, int32_t count, int32_t n);
gp_status gp_sgprb_predict_source(gp_sgprb_plan p, const double* params, const double* X, const double* Y,
                                  const double* Xnew, int32_t n, int32_t count, double* mean, double* var,
                                  void* workspace, size_t workspace_bytes);
/* gp_sgpr_predict_source_sparse of the first `count` windows from ONE fused launch over all windows and sources: Xnew
 * [count][n] (any n >= 1), mean / var [count][P][n].  Honours gp_sgprb_set_inducing_counts: a slot with k < M points gives
 * the k-point window's result and its pad rows of Z are never read.  Synchronises; GP_ERR_NOT_PD as gp_sgprb_predict_f. */
gp_status gp_sgprb_predict_source_sparse(gp_sgprb_plan p, const double* params, const double* X, const double* Y,
                                         const double* Z, const double* Xnew, int32_t n, int32_t count, double* mean,
                                         double* var);

/* gp_sgpr_sample_source_sparse of the first `count` windows: Xnew [count][n], order_host [count][n + M] (HOST; a slot with
 * k <= M inducing points: its first n + k entries, a permutation of 0..n+k-1, checked before anything is enqueued),
 * eps_x [count][S][C][n], eps_z [count][S][C][M], eps_u [count][S][2][M], out [count][P][S][n].  Honours
 * gp_sgprb_set_inducing_counts: rows >= k of a slot's eps_z, eps_u, Z, W and WB are never read.  workspace:
 * gp_sgpr_sample_source_workspace_bytes(M, P, C, n, S, count).  Synchronises; GP_ERR_NOT_PD as gp_sgprb_predict_f. */
gp_status gp_sgprb_sample_source_sparse(gp_sgprb_plan p, const double* params, const double* X, const double* Y,
                                        const double* Z, const double* Xnew, int32_t n, int32_t count,
                                        const int32_t* order_host, int32_t S, const double* eps_x, const double* eps_z,
                                        const double* eps_u, double* out, void* workspace, size_t workspace_bytes);

/* gp_sgpr_predict_source_ssm of the first `count` windows from one launch sequence, one workgroup per window: params
 * [count][num_params], X / Y [count][N], Xnew [count][n], order_host [count][N + n] (HOST; window w's first steps_host[w]
 * entries), out_step_host [count][n], steps_host [count] (HOST), mean / var [count][P][n], loglik [count].  workspace:
 * gp_ssm_smooth_workspace_bytes(d, max_w steps_host[w], P, count).  float32 plans and ragged inducing counts are taken: neither
 * plays a part.  A window's bits are those of the one-window call, whatever `count`. */
gp_status gp_sgprb_predict_source_ssm(gp_sgprb_plan p, const double* params, const double* X, const double* Y,
                                      const double* Xnew, int32_t n, int32_t count, const int32_t* order_host,
                                      const int32_t* out_step_host, const int32_t* steps_host, double* mean, double* var,
                                      double* loglik, void* workspace, size_t workspace_bytes);

/* gp_sgpr_sample_source_ssm of the first `count` windows, one wavefront per (window, draw) in the walks: per-window arguments as
 * gp_sgprb_predict_source_ssm; eps_x [count][S][max_w steps_host[w]][d] (a window reads its first steps_host[w] steps),
 * eps_y [count][S][N], out [count][P][S][n].  workspace: gp_ssm_sample_workspace_bytes(d, max_w steps_host[w], P, S, count).
 * A (window, draw)'s bits are those of the one-window call on the same normals, whatever `count` and S. */
gp_status gp_sgprb_sample_source_ssm(gp_sgprb_plan p, const double* params, const double* X, const double* Y,
                                     const double* Xnew, int32_t n, int32_t count, const int32_t* order_host,
                                     const int32_t* out_step_host, const int32_t* steps_host, int32_t S, const double* eps_x,
                                     const double* eps_y, double* out, void* workspace, size_t workspace_bytes);

/* gp_sgpr_exact_loglik_grad of the first `count` windows, one workgroup per window in the walks: params [count][num_params],
 * X / Y [count][N], order_host [count][N] (HOST), loglik [count], grad [count][num_params], resid_grad [count][N] or null.
 * workspace: gp_ssm_score_workspace_bytes(d, N, P, count).  A window's bits are those of the one-window call, whatever `count`. */
gp_status gp_sgprb_exact_loglik_grad(gp_sgprb_plan p, const double* params, const double* X, const double* Y, int32_t count,
                                     const int32_t* order_host, double* loglik, double* grad, double* resid_grad, void* workspace,
                                     size_t workspace_bytes);

/* ---- many small, independent Pdgp models per launch sequence ------------------------------------------------------
 * replaces the loop  for m in models: m.optimize(method=AdamOptimizer(...), maxiter)  over single-pitch models trained
 * one by one (init_models.py:74-121; demo-modgp.py:44-45): each step is Pdgp.build_likelihood (pdgp.py:113-170) and its
 * gradient, then tf.train.AdamOptimizer's update, for EVERY model, as four launches whatever the number of models.
 * Whitened, float64, unsharded models only; per latent GP M <= 128, minibatch <= 1024 frames, kernels Matern12 / 32 / 52,
 * RBF, MercerMatern12sm, Matern32sm (others: GP_ERR_UNSUPPORTED; train them with gp_pdgp_*).
 * Latent GPs are listed model by model, each model's rows in the order [g_0..g_{P-1}, f_0..f_{P-1}].
 * Parameter vector: per model [ noise_var | per latent GP: theta | z | q_mu | q_sqrt (M x M) ], models concatenated. */
typedef struct {
  int32_t num_models;
  const int32_t* num_sources;     /* host, [num_models]: P */
  const int32_t* batch;           /* host, [num_models]: minibatch frames B (the pdgp.py:76-77 minibatch_size);
                                     NULL: a prediction-only plan (gp_pdgpb_predict) */
  const int32_t* nlin;            /* host, [num_models]: GP_NLIN_* */
  const double* num_data;         /* host, [num_models]: N (the ELBO's N / B scale, pdgp.py:166-170); unused when
                                     batch is NULL */
  const int32_t* M;               /* host, [sum 2 P]: inducing points per latent GP */
  const int32_t* kern_type;       /* host, [sum 2 P]: GP_KERN_* */
  const int32_t* partials;        /* host, [sum 2 P] */
  double jitter;                  /* pdgp.py:14 */
} gp_pdgpb_config;
gp_status gp_pdgpb_create(gp_handle h, const gp_pdgpb_config* cfg, gp_pdgpb_plan* out);
gp_status gp_pdgpb_destroy(gp_pdgpb_plan p);
int64_t gp_pdgpb_num_params(gp_pdgpb_plan p);
/* offsets of latent GP g (global index) in the parameter vector; a model's noise variance sits right before its first GP */
gp_status gp_pdgpb_layout(gp_pdgpb_plan p, int32_t g, int64_t* off_theta, int64_t* off_z, int64_t* off_qmu,
                          int64_t* off_qsqrt);
/* as gp_pdgp_set_grad_needs: skip the hyper-parameter / z gradients of a latent GP whose Params are all `.fixed` */
gp_status gp_pdgpb_set_grad_needs(gp_pdgpb_plan p, int32_t g, int32_t need_theta, int32_t need_z);
/* scratch sized by the batch's own shapes (about 6 M^2 + 6 M B doubles per latent GP); 256-byte aligned */
size_t gp_pdgpb_workspace_bytes(gp_pdgpb_plan p);
gp_status gp_pdgpb_set_workspace(gp_pdgpb_plan p, void* workspace, size_t bytes);
/* Pdgp.build_likelihood of every model (pdgp.py:133-170) on its minibatch and, when grad != NULL, dELBO / dparams.
 * x, y: every model's frames, concatenated (device); idx: [sum B] int32 device indices into x / y, model by model, each
 * model's frames in time order; elbo_dev: [num_models]. */
gp_status gp_pdgpb_objective(gp_pdgpb_plan p, const double* params, const double* x, const double* y, const int32_t* idx,
                             double* elbo_dev, double* grad);
/* `steps` Adam steps (gp_adam_step's update, demo-modgp.py:44-45) of every model: step s evaluates on
 * idx + s * sum B and moves model k with step size lr_t[s * num_models + k] = lr sqrt(1 - b2^t) / (1 - b1^t) of that
 * model's t.  A model whose Cholesky fails is frozen from that step on (free state, params and moments untouched) while
 * the others go on; gp_pdgpb_not_pd reports it. */
gp_status gp_pdgpb_adam(gp_pdgpb_plan p, double* free_state, double* params, const uint8_t* tcode, double* m, double* v,
                        const double* x, const double* y, const int32_t* idx, int32_t steps, const double* lr_t,
                        double beta1, double beta2, double eps);
/* per model: 0, or 1 + 128 row + pivot of its failed Cholesky with the smallest (latent GP row, pivot index) since the
 * status was last cleared (TF's InvalidArgumentError in the reference); synchronises the stream.  clear != 0 resets the
 * status afterwards. */
gp_status gp_pdgpb_not_pd(gp_pdgpb_plan p, int32_t* host_status, int32_t clear);
/* `steps` iterations of  m.optimize(method=NatGradAdam(gamma, ...))  of every model: gp_pdgpb_adam's evaluation, then the
 * natural-gradient step of gp_pdgp_natgrad_step (same map, same masks: the stored strict upper triangle of q_sqrt is neither
 * read nor written) on every latent GP flagged in step_gp_host (HOST, one int32 per latent GP of the plan in gp_pdgpb_layout's
 * order; NULL = all), then gp_pdgpb_adam's update on a gradient whose stepped q_mu / q_sqrt blocks read 0.  Two more launches
 * per iteration whatever the number of models (none when no GP is flagged); the list of stepped GPs is uploaded once per
 * call, and nothing synchronises between the iterations.  float64, no float atomics, bit-identical between calls; a model's
 * result does not depend on the other models.
 * Refusal, per model: when I - 2 gamma P of one of its GPs is not positive definite, none of that model's GPs is stepped and
 * its Adam update is frozen from that iteration on, exactly as after a failed Kuu; the other models go on.  The model's
 * refusal word — separate from the Kuu word of gp_pdgpb_not_pd, which a failed Kuu of the same evaluation raises as well —
 * lives in the workspace and is read by gp_pdgpb_natgrad_refused: per model 0, or 1 + 128 row + pivot of the refused GP with
 * the smallest (row, pivot); clear != 0 resets the words afterwards.  The words are zeroed when the plan is handed a workspace
 * it has not seen in the previous call and otherwise persist from call to call (a refused model stays frozen) until cleared;
 * gp_pdgpb_natgrad_refused before any gp_pdgpb_natgrad: GP_ERR_WORKSPACE.
 * workspace: gp_pdgpb_natgrad_workspace_bytes(plan) bytes (0 for a null or prediction-only plan), 256-byte aligned: the
 * refusal words, the list, and per latent GP the inverse factor of its reversed B and Lq^T g; measured by its own carve.
 * gp_pdgpb_workspace_bytes does not change.  Null pointer, gamma outside (0, 1], misaligned workspace, prediction-only plan:
 * GP_ERR_BAD_ARG; workspace too small: GP_ERR_WORKSPACE; nothing is enqueued then. */
size_t gp_pdgpb_natgrad_workspace_bytes(gp_pdgpb_plan p);
gp_status gp_pdgpb_natgrad(gp_pdgpb_plan p, double* free_state, double* params, const uint8_t* tcode, double* m, double* v,
                           const double* x, const double* y, const int32_t* idx, int32_t steps, const double* lr_t,
                           double beta1, double beta2, double eps, double gamma, const int32_t* step_gp_host,
                           void* workspace, size_t workspace_bytes);
gp_status gp_pdgpb_natgrad_refused(gp_pdgpb_plan p, int32_t* host_status, int32_t clear);
/* gp_pdgpb_natgrad with one length per latent GP and automatic halving (the rule of gp_pdgp_natgrad_step_adaptive, DESIGN.md
 * 3k): gamma_gp_host (HOST, one double in (0, 1] per latent GP of the plan in gp_pdgpb_layout's order) replaces `gamma`, and
 * halvings is in 0..10.  The same two launches per iteration: the form launch's workgroup of a GP forms B at gamma_r 2^-j,
 * factors it, and on a recorded non-positive pivot with j < halvings forms it again at half the length (Phi recomputed from
 * params / grad); the accepted length goes to the workspace and the apply launch reads it.  The model's refusal word
 * (gp_pdgpb_natgrad_refused, unchanged) is raised only when a GP's last length fails; the pivot in it is that length's.  At
 * j = 0 the arithmetic is gp_pdgpb_natgrad's: with nothing to halve the two entries write the same bits.  GPs and models decide
 * independently; every iteration starts from gamma_r again.
 * Counters per latent GP of the plan, in the workspace: the sum of j over the iterations whose step the GP took, and the
 * smallest length taken; a model frozen by a refusal or a failed Kuu counts nothing from then on.  They are cleared when the
 * plan is handed an adaptive workspace it has not seen in the previous adaptive call and otherwise persist from call to call.
 * gp_pdgpb_natgrad_counts copies them to the host (both arrays, one entry per latent GP, or both NULL; synchronises the stream)
 * and with clear != 0 resets them afterwards; a GP that took no step since the reset reports 0 and +infinity (the caller knows
 * gamma_r).  Before any gp_pdgpb_natgrad_adaptive: GP_ERR_WORKSPACE.
 * workspace: gp_pdgpb_natgrad_adaptive_workspace_bytes(plan) bytes (0 for a null or prediction-only plan): gp_pdgpb_natgrad's
 * regions, then per latent GP gamma_r, the accepted length, j and the counters.  Argument errors as gp_pdgpb_natgrad's; a
 * gamma outside (0, 1], a NULL gamma_gp_host or halvings outside 0..10: GP_ERR_BAD_ARG. */
size_t gp_pdgpb_natgrad_adaptive_workspace_bytes(gp_pdgpb_plan p);
gp_status gp_pdgpb_natgrad_adaptive(gp_pdgpb_plan p, double* free_state, double* params, const uint8_t* tcode, double* m,
                                    double* v, const double* x, const double* y, const int32_t* idx, int32_t steps,
                                    const double* lr_t, double beta1, double beta2, double eps, const double* gamma_gp_host,
                                    int32_t halvings, const int32_t* step_gp_host, void* workspace, size_t workspace_bytes);
gp_status gp_pdgpb_natgrad_counts(gp_pdgpb_plan p, int64_t* halvings_host, double* shortest_host, int32_t clear);
/* Tied parameters: slots of the parameter vector that are ONE parameter, in one model or across models (the
 * segments of one recording share their noise variance and kernels).  The objective is the sum of the models' ELBOs, so the
 * shared parameter's gradient is the sum over its slots.  With ties set, gp_pdgpb_adam, gp_pdgpb_natgrad and
 * gp_pdgpb_natgrad_adaptive launch pdgpb_tie_kernel once per iteration behind the backward pass and the natural-gradient
 * kernels: per group it sums `grad` over the members in the listed order (no atomics: bit-identical between calls) and writes
 * the sum into every member's slot; the caller gives all members the same free state, moments, transform code and step length,
 * so the unchanged Adam update moves them alike, bit for bit.  gp_pdgpb_objective is not changed: elbo and grad stay per model.
 * gp_pdgpb_set_ties (HOST arrays): group j is members[group_start[j] .. group_start[j + 1]), group_start[0] = 0, every group
 * with one member or more.  Checked before anything is uploaded: group_start ascends; every offset lies in [0,
 * gp_pdgpb_num_params), outside every q_mu / q_sqrt block (q(u) is never tied), and is named once (GP_ERR_BAD_ARG); the
 * workspace holds gp_pdgpb_ties_workspace_bytes(ngroups, group_start[ngroups], num_models) bytes and is 256-byte aligned
 * (GP_ERR_WORKSPACE).  A refused call leaves the plan and its earlier ties as they were.  The entry derives the tied sets — the
 * connected components of the models under "a group has slots in both", those of two models or more — uploads groups and sets,
 * zeroes the frozen words and synchronises the stream; the workspace stays the caller's and in use until the ties are replaced
 * or cleared.  ngroups = 0 clears the ties (the other arguments are ignored): the step entries then launch exactly what they
 * launch without this entry.  gp_pdgpb_workspace_bytes does not change.
 * A tied set stops together: when the Kuu status or the refusal word of one of its models is raised, the tie launch of that
 * iteration writes 1 + the lowest failed model's index into the sticky frozen word of every model of the set that has none
 * yet, and the Adam launch behind it skips those models from then on.  The words of gp_pdgpb_not_pd and
 * gp_pdgpb_natgrad_refused keep reporting real failures only.  gp_pdgpb_ties_frozen copies the frozen words to the host (one
 * per model; synchronises the stream), clear != 0 resets them afterwards; without ties: GP_ERR_WORKSPACE.
 * gp_pdgpb_ties_workspace_bytes needs no plan: the measured carve [group_start | members | set_start | set_models | frozen]
 * plus the batch margin; 0 when an argument is not positive. */
size_t gp_pdgpb_ties_workspace_bytes(int32_t ngroups, int64_t nmembers, int32_t nmodels);
gp_status gp_pdgpb_set_ties(gp_pdgpb_plan p, int32_t ngroups, const int32_t* group_start, const int64_t* members,
                            void* workspace, size_t bytes);
gp_status gp_pdgpb_ties_frozen(gp_pdgpb_plan p, int32_t* host_words, int32_t clear);
/* ---- prediction of many models: Pdgp.predict_act_n_com (pdgp.py:190-208) of every model at its own inputs --------------
 * A prediction-only plan is created by gp_pdgpb_create with cfg->batch == NULL (num_data is then ignored).  It has the
 * parameter layout of a training plan (gp_pdgpb_layout) and no training workspace: gp_pdgpb_workspace_bytes returns 0,
 * and gp_pdgpb_set_workspace, gp_pdgpb_objective and gp_pdgpb_adam return GP_ERR_BAD_ARG on it.  The prediction entries
 * return GP_ERR_BAD_ARG on a training plan.
 * gp_pdgpb_predict_prepare factors Kuu + jitter I of every latent GP and stores [L^-1 ; tril(Lq)^T L^-1] in the workspace
 * (one launch; a failed pivot goes to the per-model status that gp_pdgpb_not_pd reads).  gp_pdgpb_predict then predicts
 * every model at its frames of xnew (device, every model's inputs concatenated; xnew_off: host, [num_models + 1],
 * xnew_off[0] = 0, model k's frames [xnew_off[k], xnew_off[k + 1]), empty models allowed) with the parameters and
 * workspace of the last prepare, as often as wanted.  Outputs are model-major, offsets 64-bit: per model its 2P rows
 * [g_0..g_{P-1}, f_0..f_{P-1}] of n_k frames in fmean / fvar (GPflow conditional, full_cov = False) and its P rows
 * nlin(mean g_i) * mean f_i in mean_source (may be NULL).  Both entries wait until their descriptors are on the device;
 * the kernels run asynchronously on the handle's stream. */
size_t gp_pdgpb_predict_workspace_bytes(gp_pdgpb_plan p);
gp_status gp_pdgpb_predict_prepare(gp_pdgpb_plan p, const double* params, void* workspace, size_t bytes);
gp_status gp_pdgpb_predict(gp_pdgpb_plan p, const double* params, const double* xnew, const int64_t* xnew_off,
                           double* fmean, double* fvar, double* mean_source, void* workspace, size_t bytes);

/* The moments of gp_mpd_predict_moments for every model of a prediction-only plan, each with its own P, nonlinearity and
 * noise variance: pdgpb_pred_kernel leaves fmean / fvar in the workspace (they never cross to the host) and one more launch
 * forms, model-major with 64-bit offsets: smean / svar (per model P rows of n_k frames, the layout of mean_source) and
 * ymean / yvar / logp (per frame, concatenated as xnew).  ynew (device, concatenated as xnew; may be NULL) is needed for
 * logp only; every output may be NULL.  The workspace is the one given to gp_pdgpb_predict_prepare, which for this entry
 * must have gp_pdgpb_predict_moments_workspace_bytes(plan, latent_frames) bytes, latent_frames >= sum_k 2 P_k n_k of the
 * largest call (gp_pdgpb_predict_workspace_bytes plus two arrays of that many doubles); a call that needs more returns
 * GP_ERR_WORKSPACE.  Bit-identical between calls; a model's results depend neither on the other models of the call nor on
 * how its frames are split between calls.
 * Every model of the plan needs P_k <= 96 (the LDS staging of gp_mpd_predict_moments, 4 P doubles per frame, strided by
 * the plan's largest P_k); otherwise a call with frames returns GP_ERR_UNSUPPORTED before any launch.  gp_pdgpb_predict
 * stages nothing per source and has no such limit. */
size_t gp_pdgpb_predict_moments_workspace_bytes(gp_pdgpb_plan p, int64_t latent_frames);
gp_status gp_pdgpb_predict_moments(gp_pdgpb_plan p, const double* params, const double* xnew, const int64_t* xnew_off,
                                   const double* ynew, double* smean, double* svar, double* ymean, double* yvar, double* logp,
                                   void* workspace, size_t bytes);

/* Joint posterior draws of every latent GP and every source nlin(g_i) f_i of every model of a prediction-only plan
 * (Pdgp.sample_sources of each model, gpitch/pdgp.py:146-155 for the conditional the draws follow): gp_pdgp_sample's map per
 * latent GP, whitened, for all models in one launch sequence.  Per latent GP r of model k (rows [g_0..g_{P-1}, f_0..f_{P-1}],
 * M_r inducing inputs z_r, W_r = chol(Kuu_r + jitter I)^-1 as gp_pdgpb_predict_prepare left it):
 *   prior path along the merged sorted points (xnew_k | z_r) by the exact state-space recursion of gp_pdgp_sample
 *   (GP_KERN_MATERN12: 1 normal per point, GP_KERN_MATERN32: 2, GP_KERN_MERCER_MATERN12SM: 2 m);
 *   u0 = prior(z_r) + sqrt(jitter) eps_u[0];  beta = W^T (q_mu + tril(q_sqrt) eps_u[1] - W u0);
 *   draw_r(x*) = prior_r(x*) + K_r(x*, z_r) beta;   source_i = nlin_k(draw_i) * draw_{P+i}.
 * Call order: gp_pdgpb_create with cfg->batch == NULL, gp_pdgpb_predict_prepare, then this entry with the same parameters
 * and workspace as often as wanted; its buffers live behind the factors, so the workspace given to prepare must have
 * gp_pdgpb_sample_workspace_bytes(plan, xnew_off, S) bytes (the measured carve; 0 for a bad argument) for the largest call.
 * Arguments (everything model-major, offsets 64-bit):
 *   xnew, xnew_off  as gp_pdgpb_predict: model k has n_k = xnew_off[k + 1] - xnew_off[k] frames; empty models are allowed and
 *               only take their (M_r-entry) orders and eps_z / eps_u blocks; a call without frames launches nothing.
 *   order_host  HOST array, the merges of every latent GP back to back, models in order, rows as above: GP r of model k has
 *               n_k + M_r entries, a stable ascending argsort of (xnew_k | z_r); entry < n_k is a frame, n_k + i is z_r[i].
 *               Each is checked to be a permutation before anything is enqueued (GP_ERR_BAD_ARG, "permutation" in
 *               gp_last_error, otherwise): a bad entry never becomes a device address.
 *   eps_x, eps_z, eps_u (device): the GPs' blocks back to back in the same order, [S][c_r][n_k], [S][c_r][M_r], [S][2][M_r],
 *               indexed by the caller's own point order.
 *   latents     (device, required) per model 2 P_k rows of [S][n_k];  sources (device, may be NULL) per model P_k rows of
 *               [S][n_k], each model with its own nonlinearity.
 * Refusals, all before anything is enqueued: a training plan, a plan never prepared (or prepared with other parameters or
 * another workspace), a null pointer other than sources, S < 1: GP_ERR_BAD_ARG; a latent GP whose kernel has no sampler here
 * (GP_KERN_MATERN52, GP_KERN_RBF, GP_KERN_MATERN32SM), more than 32767 latent GPs with frames: GP_ERR_UNSUPPORTED; a workspace
 * shorter than gp_pdgpb_sample_workspace_bytes: GP_ERR_WORKSPACE.  A failed factorisation is in gp_pdgpb_not_pd's status.
 * The entry waits until its descriptors are on the device; the kernels run asynchronously on the handle's stream.
 * Determinism: no atomics, every sum has a fixed order.  Draw s of model k depends on its own eps and its own model only: it is
 * bit-identical whatever S, whatever other models share the call, and however the caller splits models and draws between
 * calls. */
size_t gp_pdgpb_sample_workspace_bytes(gp_pdgpb_plan p, const int64_t* xnew_off, int32_t S);
gp_status gp_pdgpb_sample(gp_pdgpb_plan p, const double* params, const double* xnew, const int64_t* xnew_off,
                          const int32_t* order_host, int32_t S, const double* eps_x, const double* eps_z, const double* eps_u,
                          double* latents, double* sources, void* workspace, size_t bytes);

/* ---- kernel learning from an isolated-note recording (the drivers' init_kernel(train=True) branch,
 *      gpitch/transcription.py:176-195, gpitch/separation.py:185-204) -------------------------------------------------
 * gp_segment_gram replaces samplecov.get_samples + comatrix (samplecov.py:5-53: one tf.matmul session call per segment):
 *   C_b = (1/K) sum_k s_k s_k^T,  s_k = y[start_host[b K + k] : start_host[b K + k] + L],  b < B,
 * written as B row-major L x L matrices (both triangles, exactly symmetric).  y holds all B recordings (recording b is
 * y[rec_off_host[b] : rec_off_host[b] + rec_len_host[b]]; start_host holds ABSOLUTE element offsets into y, int32, read
 * on the host and uploaded into the workspace); every segment must lie inside its own recording and y must not exceed
 * GP_SEGMENT_GRAM_MAX_Y_BYTES (the kernel addresses y through 32-bit buffer offsets): GP_ERR_BAD_ARG otherwise — split
 * the batch.  The sum over k runs in chunks of a fixed length, so C_b is bit-identical from run to run, from device to
 * device and whatever else shares the batch.  Workspace: gp_segment_gram_workspace_bytes(B, K, L), 256-byte aligned. */
#define GP_SEGMENT_GRAM_MAX_Y_BYTES (2147483648LL - 4096)
size_t gp_segment_gram_workspace_bytes(int32_t B, int32_t K, int32_t L);
gp_status gp_segment_gram(gp_handle h, const double* y, int64_t ny, const int64_t* rec_off_host, const int64_t* rec_len_host,
                          int32_t B, const int32_t* start_host, int32_t K, int32_t L, double* C, void* workspace,
                          size_t workspace_bytes);
/* samplecov.autocorr (samplecov.py:56-74), before its normalisation: r[j] = sum_{i < n-L} y[i] y[i+j], j < L (n > L),
 * a fixed-order reduction over i. */
gp_status gp_autocorr(gp_handle h, const double* y, int64_t n, int32_t L, double* r);
/* kernelfit.loss_func / approximate_kernel (kernelfit.py:28-51) for W problems in one launch, one wavefront each.
 * Problem w: points x[w ld + j], targets y[w ld + j], j < npts[w] <= ld; m_w = npar[w] <= m_max <= 64 partials; parameter
 * row p[w P ..], P = 2 + 2 m_max: [bias, lengthscale, v_1..v_{m_w}, f_1..f_{m_w}, padding];
 *   k(x) = (1 + sqrt(3)|x|/|l|) exp(-sqrt(3)|x|/|l|) sum_i |v_i| cos(2 pi |f_i| |x|)   (+ 0 |bias|),
 *   f[w] = sqrt(mean_j (k(x_j) - y_j)^2);  g[w P ..] = df/dp in the same layout (sign(p) of the |.|, 0 for the bias and
 *   the padding);  k[w ld + j] = k(x_j) when k != NULL.  npts / npar are device int32 arrays.  A problem's results depend
 * on its own row only (bit-identical whatever shares the launch). */
gp_status gp_kernfit_eval(gp_handle h, int32_t W, const double* x, const double* y, int64_t ld, const int32_t* npts,
                          const int32_t* npar, int32_t m_max, const double* p, double* f, double* g, double* k);

/* ---- measurement hooks (bench.py) ---------------------------------------------------------------
 * HIP-event timing of the dominant kernels on the handle's own stream.  Returns the accumulated time of
 * kernel class `which` since the last reset and the number of launches. */
enum { GP_TIMER_KUF_BUILD = 0,   /* cov_build_kernel<0,2>: stationary Kuf assembly (HBM-bound)                 */
       GP_TIMER_COND_A = 1,      /* gemm_f64_kernel<..,1>: A = L^-1 Kuf (tri-aware, M^2 N flops per GP); Q route: G = Q Kuf (2 M^2 N) */
       GP_TIMER_COND_LTA = 2,    /* gemm_f64_kernel<..,2>: Lq^T A column sums (tri-aware, M^2 N)               */
       GP_TIMER_NT_GEMM = 3,     /* gemm_f64_kernel<..,4>: H = A D A^T split-K over frames (M^2 N, symmetric)  */
       GP_TIMER_KUF_BAR = 4,     /* gemm_f64_kernel<..,3>: Kuf_bar = R (A D) (dense, 2 M^2 N)                  */
       GP_TIMER_CHOL = 5, GP_TIMER_LIK = 6, GP_TIMER_SMALL_GEMM = 7, GP_TIMER_HYPER = 8,
       GP_TIMER_KUF_BUILD_SM = 9, /* cov_build_kernel<1,..>: spectral-mixture Kuf (features + build)              */
       GP_TIMER_COUNT = 10 };
gp_status gp_timers_enable(gp_handle h, int32_t on);
gp_status gp_timers_reset(gp_handle h);
gp_status gp_timers_read(gp_handle h, int32_t which, double* total_ms, int64_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* GPITCH_ABI_H */
