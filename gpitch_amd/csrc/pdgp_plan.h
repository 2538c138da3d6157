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
  int fam = -1;                     // its family in hy_fams (pdgp_build_families; -1: no kernel gradient asked)
  int np_uf = 0, np_uu = 0;         // GPs of an unbatched family: partial records its own contractions left this step
};

// How a kernel family gets its Kuf-side hyper-gradient sums.  Decided at bind (pdgp_bwd.hip: pdgp_decide_routes),
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

// What the caller said about the routes (DESIGN.md 3.04's table has every rule); written by pdgp_set_perm alone.
struct PdgpPerms {
  bool frames_ascending = false;                          // gp_pdgp_set_frames_ascending: every batch is in time order
  bool qform = false, q_zasc = false, q_bar_ok = false;   // gp_pdgp_set_qform's bits 0, 1 (the inducing inputs ascend), 2
  bool afar_ok = false;                                   // gp_pdgp_set_far_act (they ascend for the Matern-3/2 GPs too)
  bool scan_far_ok = true, h_far_ok = true;               // gp_pdgp_set_scan_far, gp_pdgp_set_h_far: one handle, both forms
};

// What the bound batch takes: written by pdgp_decide_routes (pdgp_bwd.hip) alone, at bind.  All zero: dense everywhere — and
// so are the backward pass's fields after a bind without a gradient.
struct PdgpRoutes {
  int q0 = 0, nq = 0, qk0 = 0;          // Q route (3.03): latent GPs [q0, q0 + nq); qk0 = the run's first slot in the compacted batch
  bool q_far = false, q_bar = false;    // the run's product (3.05) / its Qbar and v (3.06) from the far field; with q_bar its
                                        // problems leave the split-K launch, which covers the other latent GPs
  int a0 = 0, na = 0;                   // activation far field (3.07): latent GPs [a0, a0 + na).  The rest: the backward pass's
  int nhf = 0, hd0 = 0, hdn = 0;        // H from the factors (3.10): nhf = na when taken; [hd0, hd0 + hdn) is left to the dense product
  bool contiguous = false;              // whitened, and every family sits in one run of the compacted batch
  bool any_scan = false;                // some family takes KUF_SCAN
  bool any_routed = false;              // some family's route is not KUF_PRODUCT: Kuf_bar is then issued family by family
  int kuf_uniform = 0;                  // even n and every GP of the compacted batch M = maxM (R, A, G: arena buffers, even ld)
  int nt_uniform = 0;                   // the split-K product: n a multiple of 4 and every latent GP M = maxM
  int k64 = 0;                          // float64 GPs of the compacted batch (they come first)
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
    KufRoute route = KUF_PRODUCT;    // (route, scan_far and np_uf at bind: pdgp_decide_routes; the rest: pdgp_build_families)
    bool scan_far = false;           // KUF_SCAN: its first launch takes the moments from afar.hip's factored A
    int np_uf = 0, np_uu = 0;        // batched family: partial records per GP.  np_uf is fixed at bind by the fused and scan routes;
                                     // the contractions report the others at launch
    std::vector<int> gps;
  };
  std::vector<HyFamily> hy_fams;
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
  bool era_ready = false;      // pdgp_prefetch_backward ran for the current evaluation
  PdgpPerms perms;             // what the caller allowed (the setters)
  PdgpRoutes routes;           // what the bound batch takes (pdgp_decide_routes)
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
static inline bool pdgp_on_q_route(const gp_pdgp_plan_s* p, int g) { return g >= p->routes.q0 && g < p->routes.q0 + p->routes.nq; }

// a setter's body: a permission that changes drops the bind cache, since the routes and the descriptors depend on it
static inline gp_status pdgp_set_perm(gp_pdgp_plan_s* p, bool PdgpPerms::*field, bool value) {
  if (!p) return GP_ERR_BAD_ARG;
  if (p->perms.*field != value) { p->perms.*field = value; p->last_params = nullptr; }
  return GP_OK;
}

// Could latent GP g EVER take a route?  Switches, the plan's whitening, the GP's precision, kernel and M, the plan's largest
// batch: all fixed once the workspace is set.  pdgp_carve reserves a route's regions where its predicate holds, and
// pdgp_decide_routes asks the same predicate — not the carved pointers — so the two cannot disagree.
static inline bool pdgp_may_q(const gp_pdgp_plan_s* p, int g) {
  return gp_switches().qform != 0 && p->whiten && !p->gps[g].f32 && p->gps[g].ktype == GP_KERN_MERCER_MATERN12SM;
}
static inline bool pdgp_may_qfar(const gp_pdgp_plan_s* p, int g) {
  return pdgp_may_q(p, g) && gp_switches().qform_far != 0 && qfar_takes(p->gps[g].M, p->maxN, p->gps[g].m);
}
static inline bool pdgp_may_qbar(const gp_pdgp_plan_s* p, int g) {
  return pdgp_may_qfar(p, g) && gp_switches().qform_qbar != 0 && qbar_takes(p->gps[g].M, p->maxN, p->gps[g].m);
}
static inline bool pdgp_may_afar(const gp_pdgp_plan_s* p, int g) {
  return gp_switches().act_far != 0 && p->whiten && !p->gps[g].f32 && p->gps[g].ktype == GP_KERN_MATERN32 && afar_takes(p->gps[g].M, p->maxN);
}
static inline bool pdgp_may_hfar(const gp_pdgp_plan_s* p, int g) {
  return pdgp_may_afar(p, g) && gp_switches().h_far != 0 && hfar_takes(p->gps[g].M, p->maxN);
}
static inline bool pdgp_may_scan(const gp_pdgp_plan_s* p, int g) {
  return gp_switches().kuf_scan != 0 && p->whiten && !p->gps[g].f32 && kuf_scan_nq(p->gps[g].ktype) > 0;
}

// The one run that the members among g = 0 .. G - 1 form.  False: a member is disqualified (asked of members only, in order),
// or the members are not neighbours.  True: they are [*first, *first + *count) — count 0, first 0 when there is none.
template <class Member, class Disqualified>
static inline bool pdgp_single_run(int G, Member member, Disqualified disqualified, int* first, int* count) {
  int last = *first = *count = 0;
  for (int g = 0; g < G; g++) {
    if (!member(g)) continue;
    if (disqualified(g)) return false;
    if (*count == 0) *first = g;
    last = g; (*count)++;
  }
  return *count == 0 || last - *first + 1 == *count;
}

// pdgp_bwd.hip, for pdgp.hip.  A bind (pdgp_bind) runs: families (with a gradient), routes, forward and backward descriptors.
void pdgp_build_families(gp_pdgp_plan p);
void pdgp_decide_routes(gp_pdgp_plan p, int n, bool grad);
void pdgp_upload_qform(gp_pdgp_plan p, const double* params);
void pdgp_upload_afar(gp_pdgp_plan p, const double* params);
void pdgp_upload_bwd(gp_pdgp_plan p, const double* params, int n, double* grad);
gp_status pdgp_qform_prepare(gp_pdgp_plan p, const double* x, int n);
gp_status pdgp_qform_join(gp_pdgp_plan p);
gp_status pdgp_afar_run(gp_pdgp_plan p, const double* x, int n);
gp_status pdgp_prefetch_backward(gp_pdgp_plan p, int n, bool* kl_done);
gp_status pdgp_backward(gp_pdgp_plan p, const double* params, const double* x, int n, double* grad);

