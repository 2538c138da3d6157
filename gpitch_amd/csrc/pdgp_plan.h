// pdgp_plan.h — Pdgp plan object shared by pdgp.hip (forward, bind) and pdgp_bwd.hip (backward descriptors, routes, schedule).
#pragma once
#include "engine.h"

static inline size_t pdgp_kl_region_bytes(int G) {
  const size_t a = kl_item_bytes(), b = klu_item_bytes();
  return gp_align_up((size_t)G * (a > b ? a : b), 256);
}

// The plan's `misc` descriptor block: [KL items][PDGP_BWD_SLOTS arrays of G GemmProblems][KL items of the unwhitened
// backward][G hyper-gradient finish items][2 G contraction items].  The backward pass uses the first S_COUNT slots
// (pdgp_bwd.hip, checked there), the last one holds the trace-term problems of the unwhitened KL.
#define PDGP_BWD_SLOTS 32
#define PDGP_KLTR_SLOT (PDGP_BWD_SLOTS - 1)
struct PdgpMiscLayout { size_t kl_items, bwd[PDGP_BWD_SLOTS], kltr, kl2, fin_items, hy_items, ks_items, qf_items, qb_items, af_items, hf_items, bytes; };
static inline PdgpMiscLayout pdgp_misc_layout(int G) {
  PdgpMiscLayout o;
  GpRegions region;
  o.kl_items = region(pdgp_kl_region_bytes(G));
  for (int s = 0; s < PDGP_BWD_SLOTS; s++) o.bwd[s] = region((size_t)G * sizeof(GemmProblem));
  o.kltr = o.bwd[PDGP_KLTR_SLOT];
  o.kl2 = region(pdgp_kl_region_bytes(G));
  o.fin_items = region((size_t)G * hyper_finish_item_bytes());
  o.hy_items = region((size_t)2 * G * sizeof(HyperItem));      // G Kuf-side items, then G Kuu-side items, same order
  o.ks_items = region((size_t)G * sizeof(KufScanItem));       // kuf_scan.hip: one per latent GP, in the families' item order
  o.qf_items = region((size_t)G * sizeof(QfarItem));          // qfar.hip: one per latent GP of the Q run
  o.qb_items = region((size_t)G * sizeof(QbarItem));          // qbar.hip: one per latent GP of the Q run
  o.af_items = region((size_t)G * sizeof(AfarItem));          // afar.hip: one per latent GP of the activation far-field run
  o.hf_items = region((size_t)G * sizeof(HfarItem));          // hfar.hip: one per latent GP of the run whose H comes from the factors
  o.bytes = region.off;
  return o;
}

struct PdgpGP {
  int M = 0, ktype = 0, m = 0;
  int need_theta = 1, need_z = 1;   // gp_pdgp_set_grad_needs
  int f32 = 0;                      // this GP's M x N strips are float32 (gp_pdgp_set_precision / gp_pdgp_set_gp_precision)
  int64_t off_theta = 0, off_z = 0, off_qmu = 0, off_qsqrt = 0;
  int fam = -1;                     // its family in hy_fams (pdgp_upload_bwd; -1: no kernel gradient asked)
  int np_uf = 0, np_uu = 0;         // GPs of an unbatched family: partial records its own contractions left this step
};

// How a kernel family gets its Kuf-side hyper-gradient sums.  Decided at bind (pdgp_bwd.hip: pdgp_select_routes),
// from shapes, kernel types, precision, the gradient needs, the switches and the two setters — never from the overlap level.
enum KufRoute {
  KUF_PRODUCT,   // Kuf_bar = R (A diag(2 gv)) stored, then the family's contraction
  KUF_FUSED,     // the contraction as that product's epilogue (gemm_strip.hip role 5): no strip, no contraction launch
  KUF_SCAN,      // moment sums along ascending frames (kuf_scan.hip): no product
  KUF_QFORM      // Kuf_bar = G diag(2 gv) + beta gm^T: no product, the contraction scales G's columns
};

struct BwdBufs {  // per-GP backward workspace (device)
  double* H = nullptr;      // M x M   A D A^T
  double* E = nullptr;      // M x M   Lq Lq^T - I
  double* T1 = nullptr;     // M x M   scratch
  double* T2 = nullptr;     // M x M   scratch
  double* Wbar = nullptr;   // M x M
  double* R = nullptr;      // M x M   W^T E
  double* Q = nullptr;      // M x M   R W = W^T E W: the Q route's forward operand (MercerMatern12sm GPs of a whitened float64 plan only)
  // the Q route's far field (qfar.hip): near ranges, reference points, T and Psi — carved with Q, in the plan's own arena
  int* qf_rng = nullptr; double* qf_ref = nullptr; double* qf_T = nullptr; double* qf_Psi = nullptr;
  // the same far field in the backward pass (qbar.hip): widened ranges, tile tables, per-group Gram blocks and
  // vectors, the recurrences' results — carved behind the tables
  int* qb_rng2 = nullptr; int* qb_tS = nullptr; double* qb_CnF = nullptr; double* qb_CFF = nullptr; double* qb_cn = nullptr;
  double* qb_cF = nullptr; double* qb_Um = nullptr; double* qb_Vp = nullptr; double* qb_Wv = nullptr;
  // the activations' far field (afar.hip): near ranges, xmin / xmax, T, Psi and C = tril(Lq)^T W — Matern-3/2 GPs
  // of a whitened float64 plan whose shape admits it
  int* af_rng = nullptr; double* af_ref = nullptr; double* af_T = nullptr; double* af_Psi = nullptr; double* af_C = nullptr;
  // H = A D A^T from the stored A once and those factors once (hfar.hip): Y's near columns by slot, its far
  // columns, the per-group A gm, the check's verdict — carved behind the tables, nothing else is carved over them
  double* hf_Yn = nullptr; double* hf_Yf = nullptr; double* hf_up = nullptr; int* hf_flag = nullptr;
  double* R32 = nullptr;    // float32 strips only: M * M floats, the float32 copy of R (gemm_wave_f32.hip)
  double* G = nullptr;      // M x N   K̄uf (dense part R (A D))
  double* u = nullptr;      // M       A gm
  double* upart = nullptr;  // nsplit x M   fused row-dot partials
  double* Lu = nullptr;     // M       L u
  double* alpha = nullptr;  // M       W^T q_mu
  double* hyp_part = nullptr;   // hyper-gradient partial sums (Kuf side)
  double* hyp_part_uu = nullptr;
  double* gz_part = nullptr;    // z-gradient partials
  double* gvsum = nullptr;      // sum_n gv
  double* ks_mom = nullptr;     // kuf_scan.hip: chunk moments / their prefix and suffix sums (eligible GPs only)
  double* ks_near = nullptr;    // kuf_scan.hip: [chunks][2] near-part sums
  // unwhitened model only: the equivalent whitened variational state q' = (W q_mu, W Lq) and its gradient
  double* qmu_w = nullptr; double* Lq_w = nullptr;       // M, M x M
  double* g_qmu_w = nullptr; double* g_Lq_w = nullptr;   // M, M x M
};

struct gp_pdgp_plan_s {
  gp_handle h = nullptr;
  int P = 0, G = 0, whiten = 1, nlin = 0, maxN = 0;
  int f32 = 0;               // gp_pdgp_set_precision: the M x N strips (Kuf, A, Kuf_bar) of EVERY latent GP are float32 (gemm_f32.hip)
  int n64 = 0;               // latent GPs [0, n64) keep float64 strips, [n64, G) have float32 ones (PdgpGP::f32): G, 0, or —
                             // gp_pdgp_set_gp_precision — in between (activation GPs float64, component GPs float32)
  double jitter = 1e-6;
  std::vector<PdgpGP> gps;
  int64_t nparams = 0;
  int maxM = 0, maxm = 0;
  // workspace
  void* ws = nullptr; size_t ws_bytes = 0;
  CondBatch cb;
  std::vector<BwdBufs> bw;
  std::vector<double*> tr_part;    // unwhitened KL: column-sum partials of (W Lq)^2
  double* fmean = nullptr; double* fvar = nullptr;   // [G][maxN]
  double* gFmu = nullptr; double* gFvar = nullptr;   // [G][maxN]
  double* kl = nullptr;                              // [G]
  double* lik_partials = nullptr;                    // [2 * blocks]
  double* slabs = nullptr;                           // split-K slabs
  char* d_misc = nullptr; PdgpMiscLayout off;        // KL items + backward problem arrays: off = pdgp_misc_layout(G)
  std::vector<char> h_misc;
  std::vector<char> h_fin_items;   // batched hyper-gradient finish (pdgp_bwd.hip)
  // Kuf-side and Kuu-side contractions grouped by kernel family: one launch per family and side over an item array (pdgp_bwd.hip)
  struct HyFamily {
    int type = 0, m = 0, first = 0, count = 0, M = 0, mfma = 0, f32 = 0; bool batched = false; bool scan_ws = false;
    int slot0 = -1;                  // its first slot in the compacted batch; -1: its GPs do not sit in one run of it
    KufRoute route = KUF_PRODUCT;
    bool scan_far = false;           // KUF_SCAN: its first launch takes the moments from afar.hip's factored A
    int np_uf = 0, np_uu = 0;        // batched family: partial records per GP.  np_uf is fixed at bind by the fused and scan routes;
                                     // the contractions report the others at launch
    std::vector<int> gps;
  };
  std::vector<HyFamily> hy_fams;
  // shape facts of the bound batch the routes and the launches share (pdgp_select_routes)
  bool contiguous = false;     // whitened, and every family sits in one run of the compacted batch
  bool any_scan = false;       // some family takes KUF_SCAN
  bool any_routed = false;     // some family's route is not KUF_PRODUCT: Kuf_bar is then issued family by family
  int kuf_uniform = 0;         // even n and every GP of the compacted batch M = maxM (R, A, G: arena buffers, even ld)
  int nt_uniform = 0;          // the split-K product: n a multiple of 4 and every latent GP M = maxM
  int k64 = 0;                 // float64 GPs of the compacted batch (they come first)
  double* qw_block = nullptr; size_t qw_doubles = 0;   // [q' | grad q'] of all GPs, contiguous (one memset)
  double* kl_dummy = nullptr;
  int nsplit = 1;
  int nK = 0;                 // number of GPs whose kernel gradients are needed (compacted batch)
  std::vector<int> kgps;      // their indices
  // cache keys for the descriptor upload
  const double* last_params = nullptr; const double* last_x = nullptr; double* last_grad = nullptr; int last_n = -1;
  bool bwd_carved = false;
  GemmProblem dummy_prob;      // sink for descriptor slots a GP does not need (pdgp_upload_bwd)
  // the ELBO's final reduction (and the noise-variance gradient it produces), handed to the backward pass: neither is
  // needed before the step ends, so it runs at the head of the helper stream's chain instead of between the last forward
  // product and Kuf_bar (pdgp_bwd.hip: pdgp_backward)
  struct { const double* lik_partials = nullptr; int nb = 0; const double* kl = nullptr; int nkl = 0; double* elbo = nullptr;
           double* g_noise = nullptr; bool pending = false; } fin;
  int overlap = 2;             // gp_pdgp_set_overlap: 0 one stream, 1 Kuu factorisation / Kuu-side backward on the helper
                               // stream, 2 also the H = A D A^T chain next to Kuf_bar
  bool frames_ascending = false;   // gp_pdgp_set_frames_ascending: the caller promises time-ordered batches
  bool era_ready = false;      // pdgp_prefetch_backward ran for the current evaluation
  // Q route (pdgp_bwd.hip pdgp_qform_select): gp_pdgp_set_qform's permission, and the run of latent GPs
  // [q0, q0 + nq) that takes it at the bound batch size (nq = 0: none); qk0 = the run's first slot in the compacted batch
  bool qform = false;
  int q0 = 0, nq = 0, qk0 = 0;
  // far field of the run's product: gp_pdgp_set_qform's second bit — the caller vouches that the inducing inputs
  // of every MercerMatern12sm GP ascend (they are fixed on this route) — and whether the bound run takes it
  bool q_zasc = false, q_far = false;
  // Qbar and v of the run from the far field as well: gp_pdgp_set_qform's third bit allows it, q_bar says
  // the bound run takes it — its problems then leave the split-K launch, which covers the other latent GPs
  bool q_bar_ok = false, q_bar = false;
  bool qbar_ahead = false;     // this backward pass has put those launches on the main stream (pdgp_backward)
  // activation far field (pdgp_bwd.hip pdgp_afar_select): gp_pdgp_set_far_act's permission — the caller vouches
  // that the inducing inputs of every Matern-3/2 GP ascend — and the run [a0, a0 + na) that takes it at the bound batch size
  bool afar_ok = false;
  int a0 = 0, na = 0;
  // the scan's moments from that far field (pdgp_select_routes): gp_pdgp_set_scan_far's permission, given by
  // default — it exists so that one handle can evaluate both forms
  bool scan_far_ok = true;
  // H and u of that run from the factored A (pdgp_select_routes): gp_pdgp_set_h_far's permission, given by
  // default; nhf = na when the bound gradient evaluation takes the form (the run is then [a0, a0 + na)), else 0; the latent
  // GPs left to the dense split-K product are the run [hd0, hd0 + hdn), possibly empty
  bool h_far_ok = true;
  int nhf = 0, hd0 = 0, hdn = 0;
  bool factor_valid = false;   // L / W hold the factorisation of the parameters last passed to gp_pdgp_predict
  // two-stage (pitch-sharded) evaluation: what gp_pdgp_elbo_begin staged for gp_pdgp_elbo_end
  int staged_n = 0; double* staged_grad = nullptr; const double* staged_params = nullptr;
  // GP-sharded plan (gp_pdgp_create_subset): this plan's G latent GPs are rows `grow[g]` of the whole model's 2 P latent
  // GPs (engine order [g_0..g_{P-1}, f_0..f_{P-1}]); P is the WHOLE model's source count (the likelihood's)
  bool subset = false;
  std::vector<int> grow;
  double* gF_full_mu = nullptr; double* gF_full_var = nullptr;   // [2 P][maxN]: d varexp / d fmean, fvar of every latent GP
};

// is latent GP g in the run that takes the Q route at the bound batch size?  (A family asks its route field instead.)
static inline bool pdgp_on_q_route(const gp_pdgp_plan_s* p, int g) { return g >= p->q0 && g < p->q0 + p->nq; }

