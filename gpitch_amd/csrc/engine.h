// engine.h — batched sparse-GP conditional engine shared by the Pdgp / SGPR plans and the one-shot
// C-ABI operators.  Host-side orchestration only; all arithmetic is in the .hip kernels.
#pragma once
#include "common.h"
#include <functional>

// lik.hip helpers
size_t cond_finish_item_bytes();
void cond_finish_fill(void* host_item, const double* s1, int rb1, const double* s2, int rb2, const double* dot,
                      int rbdot, DevKern k, double* fmean, double* fvar);
gp_status launch_cond_finish(gp_handle h, const void* d_items, int count, int N);
size_t kl_item_bytes();
void kl_item_fill(void* host_item, const double* q_mu, const double* q_sqrt, int M, double* out, double* g_mu,
                  double* g_sqrt);
gp_status launch_kl_white(gp_handle h, const void* d_items, int count);
size_t klu_item_bytes();
void klu_item_fill(void* host_item, const double* q_mu, const double* q_sqrt, const double* L, const double* W,
                   const double* tr_part, int nrb, int M, double* out);
gp_status launch_kl_unwhite(gp_handle h, const void* d_items, int count);
gp_status launch_elbo_finish(gp_handle h, const double* lik_partials, int nblocks, const double* kl, int nkl,
                             double* elbo, double* g_noise);
gp_status launch_mean_source(gp_handle h, const double* fmean, int P, int n, int nlin, double* out);

// bwd.hip helpers
gp_status launch_rowdot_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM);
gp_status launch_sub_identity_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM);
gp_status launch_phi_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM);
gp_status launch_rank1_tril_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM);
gp_status launch_matvec_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int trans);
gp_status launch_batched_sum(gp_handle h, const double* v, int64_t stride, int n, int rows, double* out);   // out[r] = sum_n v[r * stride + n]
// The kernel-gradient chain under the Pdgp, SGPRSS and window backward passes (bwd.hip; formulas there).  Every plan stores
// its problems slot-major and keeps these twelve slots in this order; G (the Kuf_bar product) is filled and launched by the plan.
enum ChainSlot { CH_EH = 0, CH_WBAR, CH_LU, CH_RANK1, CH_R, CH_ALPHA, CH_G, CH_T2, CH_LBAR, CH_P, CH_T3, CH_S, CH_COUNT };
struct ChainSlots { GemmProblem* p[CH_COUNT]; };     // first record of every slot: host records to fill, device ones to launch
// slot q at base + off[q] bytes (a plan's region offsets from its first chain slot on), records from `first` on
static inline ChainSlots chain_slots(char* base, const size_t* off, int first = 0) {
  ChainSlots s;
  for (int q = 0; q < CH_COUNT; q++) s.p[q] = (GemmProblem*)(base + off[q]) + first;
  return s;
}
static inline ChainSlots chain_slots_run(GemmProblem* first) {      // the twelve slots as one run of records, one each
  ChainSlots s;
  for (int q = 0; q < CH_COUNT; q++) s.p[q] = first + q;
  return s;
}
// one matrix's buffers: M x M each but the vectors u, v, Lu, alpha; v is what the rank-1 term and alpha read (q_mu / ubar).
// The adjoint ends in H (T3) and E (Kuu_bar), which it is free to overwrite by then.
struct ChainBufs { const double *L, *W; double *E, *H; const double *u, *v; double *T1, *T2, *Wbar, *R, *Lu, *alpha; };
void gemm_problem_square(GemmProblem& r, int M);     // zeroed, M = N = K = lda = ldb = ldc = M
void chain_fill(const ChainSlots& host, int idx, int M, const ChainBufs& b);     // every slot's record idx but CH_G's
// each enqueues on h->stream over `count` records
gp_status launch_chain_e(gp_handle h, const GemmProblem* e, int count, int maxM);
gp_status launch_chain_r_alpha(gp_handle h, const GemmProblem* r, const GemmProblem* alpha, int count, int maxM);
gp_status launch_chain_wbar(gp_handle h, const ChainSlots& dev, int count, int maxM);
gp_status launch_chain_adjoint(gp_handle h, const ChainSlots& dev, int count, int maxM);
gp_status launch_chain_b_head(gp_handle h, const GemmProblem* binv, const GemmProblem* ubar, int count, int maxM);
gp_status launch_addvec_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM);
gp_status launch_tril_add_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM);
gp_status launch_hyper_contract(gp_handle h, DevKern k, const double* x1, int n1, const double* x2, int n2,
                                const double* G, int64_t ldg, const double* alpha, const double* gm, int symmetric,
                                const double* feat, double* partials, int* nparts, double* gz_partials,
                                const double* kvals = nullptr, int64_t ldk = 0, int g32 = 0);   // g32: G (and kvals) are float32 strips
gp_status launch_hyper_finish(gp_handle h, DevKern k, const double* partials, int nparts, const double* gv_sum,
                              double* g_theta, const double* gz_partials, int ncolblocks, int n1, double* g_z);
int hyper_num_sums(int m);
#define HY_THREADS 256      // frames per workgroup of the generic contraction: one inducing-input partial record per such block
// item forms (one launch for many contractions / finishes: the window-batched SGPR plan)
struct HyperItem {
  DevKern k;
  const double* x1; const double* x2; const double* G; const double* alpha; const double* gm;
  const double* f1; const double* f2; double* partials; double* gz;
  const double* kvals;            // the covariance strip itself (Mercer Kuf side, matrix-core form), or null
  int64_t ldg, ldk; int n1, n2, symmetric, g32;
  const double* gscale;           // Q route: G's columns are still to be scaled by 2 gscale[j] (Kuf_bar = G diag(2 gv)); else null
};
struct HyperFinishItem {
  DevKern k;
  const double* p_uf; const double* p_uu; const double* gv_sum;
  double* g_theta; const double* gz_uf; const double* gz_uu; double* g_z;
  int np_uf, np_uu, cb_uf, cb_uu, n1, pad;
};
// use_mfma: Mercer family, every item has kvals and no inducing-input gradient -> hyper_sm_rows_kernel over the items
// (g32_items: the items' strips are float32 — all of them, as their g32 fields say)
gp_status launch_hyper_contract_items(gp_handle h, int type, int m, const HyperItem* d_items, int count, int n1, int n2,
                                      int with_gz, int* nparts, int use_mfma = 0, const double* x2_shared = nullptr,
                                      int g32_items = 0, int lean_items = 0, int gscale_items = 0);
// would that launch (use_mfma, lean_items, float64 strips) take hyper_sm_rows_lean_kernel, the form that applies gscale?
bool hyper_lean_takes(int type, int m, int n1, int n2, int count);
// one pass over G for the P MercerMatern12sm kernels of a sum (bwd.hip; true = taken)
bool launch_hyper_contract_sum(gp_handle h, const DevKern* kernels, double* const* feats, double* const* partials, int P,
                               const double* x1, int n1, const double* x2, int n2, const double* G, int64_t ldg,
                               const double* alpha, const double* gm, int g32, int* nparts, gp_status* st);
gp_status launch_hyper_finish_items(gp_handle h, const HyperFinishItem* d_items, int count, int maxblocks);
size_t hyper_finish_item_bytes();
// partial records the Kuf-side contraction of an M x N strip may write (the largest over its kernel variants)
size_t hyper_kuf_records(int N, int M);

// kuf_scan.hip: the Kuf-side contraction of a Matern-3/2 / Matern-5/2 family by moment sums along ascending frames
struct KufScanItem {
  const double* A; const double* gv; const double* gm;      // M x N strip (ld lda), dELBO/dfvar, dELBO/dfmean (N each)
  const double* R; const double* alpha; const double* z;    // M x M (ld M), M, M
  const double* theta;                                      // [variance, lengthscale]
  double* mom; double* near; double* partials;              // moments [chunk][side][q][M + 1], near sums [chunk][2], records
  int64_t lda; int M, pad;
  // the far-field form of launch 1 only: the stored Kuf strip (ld lda), W, and afar.hip's tables of this step
  const double* Kuf; const double* W; const int* rng; const double* T; const double* Psi;
};
int kuf_scan_nq(int ktype);                // moment orders a kernel type needs (3 Matern-3/2, 4 Matern-5/2; 0: not a scan type)
int kuf_scan_chunks(int N);
size_t kuf_scan_moment_doubles(int N, int M, int ktype);
int kuf_scan_records(int M);                // partial records one GP leaves (never more than hyper_kuf_records gives it)
// all `count` GPs of one family (same kernel type) over the n ascending frames x: three launches, no Kuf_bar product.
// far: the first launch forms the moments and the near sums from the items' Kuf, W, rng, T and Psi instead of a pass over A
// (Matern-3/2 on the shapes afar_takes admits; every GP's A of this step came from launch_afar)
gp_status launch_kuf_scan(gp_handle h, int ktype, const KufScanItem* d_items, int count, int maxM, const double* x, int n, int far = 0);

// qfar.hip: the tables of the Q route's far field, one item per latent GP of the run
struct QfarItem {
  const double* z; const double* theta; const double* fz; const double* fx; const double* Q;   // z features [nf][M], x features [nf][N]
  int* rng; double* ref; double* T; double* Psi;     // [groups][2] near range, [groups][2] reference points, T, Psi (CondTask)
  int M, pad;
};
#define QFAR_GROUP 256       // frames per column group: the wave product's workgroup
struct QfarSizes { size_t rng, ref, T, Psi; };       // doubles
QfarSizes qfar_sizes(int M, int N, int m);
bool qfar_takes(int M, int N, int m);
// count GPs of one family (M, m) over the n ascending frames x: two launches on h->stream
gp_status launch_qfar_tables(gp_handle h, const QfarItem* d_items, int count, int M, int m, const double* x, int n);
// the second of them alone (lds 0: qfar_t_kernel, 1: qfar_t_lds_kernel — switches.h far_tables); the caller checks hipGetLastError
void launch_qfar_t(gp_handle h, const QfarItem* d_items, int count, int M, int nf, int n, bool lds);

// qbar.hip: the Q route's backward products Qbar = Kuf diag(2 gv) Kuf^T and v = Kuf gm from the same far field,
// one item per latent GP of the run: the stored strip, the likelihood's two rows, qfar.hip's tables of this step, the workspace
struct QbarItem {
  const double* Kuf; int64_t ldk; const double* gv; const double* gm;
  const double* z; const double* theta; const double* fz;           // z features [nf][M]
  const int* rng; const double* ref; const double* Psi;             // qfar.hip's ranges, reference points, Psi
  int* rng2; int* tS;                                               // the ranges widened to monotone; per 16-row tile S0, then Sa
  double* CnF; double* CFF; double* cn; double* cF;                 // per group: near x far [M][2 nf], far x far [2 nf][2 nf], B gm
  double* Um; double* Vp; double* Wv;                               // [M][nf], [M][nf], [M / 16][M][nf]
  double* Qbar; double* v;                                          // out: M x M (full, symmetric), M
  int M, pad;
};
#define QBAR_MAX_TILES 64    // 16-row tiles: M <= 1024
#define QBAR_MAX_NF 64       // features per point: m <= 32
struct QbarSizes { size_t rng2, tS, CnF, CFF, cn, cF, Um, Wv; };   // doubles (Vp as Um)
QbarSizes qbar_sizes(int M, int N, int m);
bool qbar_takes(int M, int N, int m);
// count GPs of one family (M, m) over n frames, behind the tables and the likelihood's gv / gm: four launches on h->stream
gp_status launch_qbar(gp_handle h, const QbarItem* d_items, int count, int M, int m, int n);

// afar.hip: the activations' A = W Kuf and colsum((Lq^T A)^2) from near rows plus an exact rank-4 far field,
// one item per latent GP of the run: the conditional's operands and outputs, C = tril(Lq)^T W, and the tables of this step
// W, C, T, q_mu are the matrix cores' A operand and the epilogue's weights (buffer loads): none of them may
// alias A, s1, s2 or dot, and nothing may write them while afar_prod_kernel runs — they are left by earlier launches of the stream.
struct AfarItem {
  const double* z; const double* theta; const double* W; const double* C; const double* Kuf; const double* q_mu;
  double* A; double* s1; double* s2; double* dot;    // the stored strip; ONE partial row each of colsum(A^2), colsum((C Kuf)^2), A^T q_mu
  int* rng; double* ref; double* T; double* Psi;     // [groups][2] near range, [groups][2] xmin / xmax, T [groups][M][8], Psi [4][N]
  int64_t ld; int M, pad;
};
#define AFAR_GROUP 256       // frames per column group: one workgroup of the tables' kernels, eight wavefronts of the product
struct AfarSizes { size_t rng, ref, T, Psi, C; };    // doubles
AfarSizes afar_sizes(int M, int N);
bool afar_takes(int M, int N);
// count GPs of one family (M) over the n ascending frames x, behind C: the tables' two launches and the product's one on h->stream
gp_status launch_afar(gp_handle h, const AfarItem* d_items, int count, int M, const double* x, int n);
// the tables' launch alone (tiled 0: afar_t_kernel, 1: afar_t_tiled_kernel — switches.h far_tables); the caller checks hipGetLastError
void launch_afar_t(gp_handle h, const AfarItem* d_items, int count, int M, int n, bool tiled);

// hfar.hip: the activations' H = A diag(2 gv) A^T and u = A gm from the stored A once and afar.hip's factors once
// (DESIGN.md 3.10), one item per latent GP of the run: the strips, W, the likelihood's two rows, afar.hip's tables of this
// step, the store of Y, and the split-K product's slabs and u partials, which launch_slab_reduce sums as it does the product's
struct HfarItem {
  const double* A; const double* Kuf; const double* W; const double* gv; const double* gm;
  const int* rng; const double* T; const double* Psi;      // [groups][2] near range, T [groups][M][8], Psi [4][N]
  double* Yn; double* Yf; double* up; int* flag;           // near columns [slot = tile + group][M][16], far columns [groups][M][4],
                                                            // A gm per group [groups][M], the check's verdict
  double* slabs; double* upart;                            // [nsplit][M][M] (lower 16 x 16 tiles written), [nsplit][M]
  int64_t ld; int M, gp;                                   // gp: the latent GP's index, for the status word
};
struct HfarSizes { size_t Yn, Yf, up, flag; };             // doubles
HfarSizes hfar_sizes(int M, int N);
bool hfar_takes(int M, int N);
// count GPs of one family (M) over n frames, behind afar.hip's launches of this step and the likelihood's gv / gm: three
// launches on h->stream.  charges: the scopes they open under the split-K product's timer (0: none — a dense launch remains)
gp_status launch_hfar(gp_handle h, const HfarItem* d_items, int count, int M, int n, int nsplit, int charges);

#define CB_NB 128          // panel width of the blocked Kuu factorisation
#define CB_MAX_PANELS 8    // M <= 1024

// The descriptor block of a batch of `count` conditionals whose blocked Kuu factorisation has `nblk` panels (0: not
// blocked): every region's offset and the total, from one walk (cond_batch_desc_layout).
struct CondDescLayout {
  size_t chol_ptrs, w_ptrs, Ms, lds, f1, f1u, f2, finish;
  size_t fq, finish_q;                                   // the Q route's product and finish items (CondBatch::q_desc; else f1's and finish's offsets)
  size_t cov_uu, cov_uf, feat_zuu, feat_zuf, feat_x;     // grouped covariance builds: Kuu + Kuf items, z / x feature items
  // blocked factorisation: per panel 2 pointer arrays, 1 size array, 4 GEMM problem arrays ...
  size_t blk_mats[CB_MAX_PANELS], blk_w[CB_MAX_PANELS], blk_M[CB_MAX_PANELS], blk_gemm[CB_MAX_PANELS][4];
  size_t diag_mats, diag_w, diag_M, diag_ld;             // ... and all panels' diagonal blocks as one batch
  size_t bytes;
};
CondDescLayout cond_batch_desc_layout(int count, int nblk, bool q_desc = false);

// One latent GP inside a batch of conditionals.
struct CondTask {
  DevKern kern;
  const double* z = nullptr; int M = 0;
  const double* q_mu = nullptr; const double* q_sqrt = nullptr;  // q_sqrt may be null (no variational covariance)
  // workspace (device)
  double* L = nullptr;    // M x M  Kuu -> chol
  double* W = nullptr;    // M x M  L^-1
  double* Tblk = nullptr; // 128 x M scratch (blocked inverse)
  double* Kuf = nullptr;  // M x N
  double* A = nullptr;    // M x N  W Kuf
  double* A2 = nullptr;   // M x N  W^T A (unwhitened only)
  double* W32 = nullptr;  // float32 strips only: M * M floats each, the float32 copies of W and tril(Lq)^T (gemm_wave_f32.hip)
  double* Lq32 = nullptr;
  double* feat = nullptr; // spectral-mixture features (2m x (M + N))
  double* feat_uu = nullptr; // the same for the Kuu build (2m x M), separate because the two builds overlap
  double* s1 = nullptr; double* s2 = nullptr; double* dot = nullptr;  // [rowblocks][N] partials
  double* fmean = nullptr; double* fvar = nullptr;                    // N each
  bool f32 = false;       // this GP's M x N strips (Kuf, A, A2) are float32 (per-GP precision: CondBatch::n64)
  // Q route (CondBatch::nq): Q = W^T (Lq Lq^T - I) W (M x M) and beta = W^T q_mu, which the caller's hook fills
  const double* Qm = nullptr; const double* beta = nullptr;
  // ... and, when the run takes the far-field form (CondBatch::q_far), qfar.hip's tables: two ints per
  // 256-frame group [kbeg, kend), T [group][M][2 nf], Psi [2 nf][N]
  const int* far_rng = nullptr; const double* far_T = nullptr; const double* far_Psi = nullptr;
};

struct CondBatch {
  std::vector<CondTask> tasks;
  int N = 0;
  int maxM = 0;
  // device descriptor storage (inside the caller's workspace: cond_batch_desc_bytes(tasks.size()) bytes)
  char* d_desc = nullptr;
  std::vector<char> h_desc;
  CondDescLayout off;     // offsets of the descriptor arrays inside d_desc (cond_batch_upload)
  bool uploaded = false;
  bool overlap = true;    // run the Kuu factorisation on the handle's helper stream next to the Kuf builds
  bool f32 = false;       // every task's M x N strips (Kuf, A) are float32 and the strip products run on the float32 matrix path
  // per-GP precision: tasks [0, n64) keep float64 strips, tasks [n64, G) have float32 ones (CondTask::f32); -1 = uniform
  // (all float64 or, with f32 set, all float32).  cond_batch_upload checks the order and sets it.
  int n64 = -1;
  bool wave_a = false, wave_lta = false;
  bool wave_a32 = false, wave_lta32 = false;   // the same for the float32 tasks (gemm_wave_f32.hip)   // A = W Kuf / Lq^T A of the float64 tasks take gemm_wave.hip's form (64-row partial rows)
  // grouped covariance builds (one launch per kernel family)
  struct Group { int type = 0, m = 0, first = 0, maxM = 0; bool f32 = false; std::vector<int> members; };
  std::vector<Group> groups;
  // blocked Kuu factorisation (engine.hip: cond_batch_factorize)
  bool blocked = false; int nblk = 0;
  // Q route: the tasks [q0, q0 + nq) — float64, whitened, Qm and beta set — form G = Q Kuf into their A strip
  // instead of A = W Kuf and Lq^T A when cond_batch_run is given a hook; set before cond_batch_upload
  int q0 = 0, nq = 0;
  bool q_far = false;     // the run's product is role 7 (near rows + far field) instead of role 6; the hook fills the tables too
  // activation far field: the tasks [a0, a0 + na) — float64, whitened, Matern-3/2 — leave A = W Kuf and Lq^T A
  // to the caller's hook (afar.hip), which fills the A strip and one partial row each of s1, s2 and dot; set before cond_batch_upload
  int a0 = 0, na = 0;
  bool q_desc = false;    // the descriptor block was sized with the routes' regions (cond_batch_desc_bytes(count, true))
  bool feat_ready = false;   // q_far: gp_handle_s::ev_feat was recorded behind the Kuf builds (their feature tables)
  bool diag_ready = false;   // set by a factorisation that recorded gp_handle_s::ev_diag after the diagonal blocks of W
};

int cond_batch_uniform(const CondBatch& cb, int N);
size_t cond_batch_desc_bytes(int count, bool q_desc = false);     // the largest layout of `count` tasks (CB_MAX_PANELS panels)
// carve the per-task buffers out of the arena (needs t.M and t.kern's type and partial count); on a measuring arena this
// is the task's size
bool cond_task_carve(GpArena& ar, CondTask& t, int N, bool whiten, bool f32 = false);
gp_status cond_batch_upload(gp_handle h, CondBatch& cb, bool whiten, double jitter);
// run: Kuu -> chol -> W ; Kuf ; A = W Kuf ; (A2 = W^T A) ; Lq^T A ; reductions -> fmean, fvar
// q_prepare: take the Q route for the tasks [q0, q0 + nq).  The hook is called once the factorisation is enqueued and the other
// tasks' strip products are; it enqueues what fills Qm and beta and makes h->stream wait for it.  Null: every task takes
// the Cholesky route (predictions always do).
// a_run: the tasks [a0, a0 + na) take the activation far field.  The hook is called once the factorisation has joined the main
// stream and enqueues their A strips and partial rows there.  Null: those tasks take the dense products.
gp_status cond_batch_run(gp_handle h, CondBatch& cb, const double* x, int N, bool whiten, double jitter,
                         bool reuse_factor = false, const std::function<gp_status()>* q_prepare = nullptr,
                         const std::function<gp_status()>* a_run = nullptr);
// steps 1-2 of cond_batch_run alone, on the current stream: Kuu + jitter I -> L, W of every task (the uploaded descriptors'),
// for a caller that needs the factorisation and no conditional (sample.hip)
gp_status cond_batch_factor(gp_handle h, CondBatch& cb);
