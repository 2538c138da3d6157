// pdgp.hip — the Pdgp model plan: ELBO forward / backward and predictions behind the C-ABI.
// Mirrors gpitch/pdgp.py:48-208 (Pdgp.build_prior_kl :113-131, build_likelihood :133-170,
// predict_act / predict_com / predict_act_n_com :172-208).
#include "pdgp_plan.h"
#include <string.h>


extern "C" {

static gp_status pdgp_create_impl(gp_handle h, const gp_pdgp_config* cfg, const int32_t* gp_index, int32_t count,
                                  gp_pdgp_plan* out) {
  if (!h || !out) return GP_ERR_BAD_ARG;
  *out = nullptr;
  if (!cfg || cfg->num_sources < 1 || cfg->max_batch < 1 || !cfg->M_act || !cfg->M_com || !cfg->kern_type_act ||
      !cfg->kern_type_com || !cfg->partials_act || !cfg->partials_com || cfg->nlin < 0 || cfg->nlin > 2)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_create: bad config");
  if (gp_index) {
    if (count < 1 || count > 2 * cfg->num_sources) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_create_subset: bad count");
    for (int l = 0; l < count; l++)
      if (gp_index[l] < 0 || gp_index[l] >= 2 * cfg->num_sources || (l > 0 && gp_index[l] <= gp_index[l - 1]))
        return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_create_subset: gp_index must be strictly increasing in [0, 2 P)");
  }
  gp_pdgp_plan p = new gp_pdgp_plan_s();
  p->h = h; p->P = cfg->num_sources; p->G = gp_index ? count : 2 * p->P; p->whiten = cfg->whiten ? 1 : 0; p->nlin = cfg->nlin;
  p->maxN = cfg->max_batch; p->jitter = cfg->jitter;
  p->subset = gp_index != nullptr;
  if (gp_index) p->grow.assign(gp_index, gp_index + count);
  p->gps.resize(p->G);
  p->n64 = p->G;
  int64_t off = 1;  // [0] = noise variance
  for (int l = 0; l < p->G; l++) {
    PdgpGP& q = p->gps[l];
    const int g = gp_index ? gp_index[l] : l;      // row of the whole model's [g_0..g_{P-1}, f_0..f_{P-1}]
    const bool act = g < p->P;
    const int i = act ? g : g - p->P;
    q.M = act ? cfg->M_act[i] : cfg->M_com[i];
    q.ktype = act ? cfg->kern_type_act[i] : cfg->kern_type_com[i];
    q.m = act ? cfg->partials_act[i] : cfg->partials_com[i];
    const bool sm = gp_kern_has_partials(q.ktype);
    if (q.M < 1 || q.ktype < 0 || q.ktype > GP_KERN_LAST || (sm && (q.m < 1 || q.m > 32)) || (!sm && q.m != 0)) {
      delete p;
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_create: bad per-GP config");
    }
    q.off_theta = off; off += GP_THETA_LEN(q.m);
    q.off_z = off; off += q.M;
    q.off_qmu = off; off += q.M;
    // keep q_sqrt 16-byte aligned inside the vector so it can be a vectorised GEMM operand
    if (off & 1) off += 1;
    q.off_qsqrt = off; off += (int64_t)q.M * q.M;
    if (q.M > p->maxM) p->maxM = q.M;
    if (q.m > p->maxm) p->maxm = q.m;
  }
  p->nparams = off;
  *out = p;
  return GP_OK;
}

gp_status gp_pdgp_create(gp_handle h, const gp_pdgp_config* cfg, gp_pdgp_plan* out) {
  return pdgp_create_impl(h, cfg, nullptr, 0, out);
}

gp_status gp_pdgp_create_subset(gp_handle h, const gp_pdgp_config* cfg, const int32_t* gp_index, int32_t count,
                                gp_pdgp_plan* out) {
  if (!gp_index) return h ? gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_create_subset: gp_index is NULL") : GP_ERR_BAD_ARG;
  return pdgp_create_impl(h, cfg, gp_index, count, out);
}

gp_status gp_pdgp_destroy(gp_pdgp_plan p) {
  if (p && p->h && p->h->aux_stream) (void)hipStreamSynchronize(p->h->aux_stream);   // nothing of this plan still in flight
  if (p && p->h && p->h->side_stream) (void)hipStreamSynchronize(p->h->side_stream);
  delete p;
  return GP_OK;
}

gp_status gp_pdgp_set_grad_needs(gp_pdgp_plan p, int32_t g, int32_t need_theta, int32_t need_z) {
  if (!p || g < 0 || g >= p->G) return GP_ERR_BAD_ARG;
  if (p->gps[g].need_theta != (need_theta != 0) || p->gps[g].need_z != (need_z != 0)) {
    p->gps[g].need_theta = need_theta != 0;
    p->gps[g].need_z = need_z != 0;
    p->last_params = nullptr;   // force the backward descriptors to be rebuilt
  }
  return GP_OK;
}
gp_status gp_pdgp_set_precision(gp_pdgp_plan p, int32_t bits) {
  if (!p || (bits != 32 && bits != 64)) return GP_ERR_BAD_ARG;
  if (p->ws) return gp_fail(p->h, GP_ERR_BAD_ARG, "gp_pdgp_set_precision: call it before gp_pdgp_set_workspace");
  p->f32 = (bits == 32);
  p->cb.f32 = (bits == 32);
  for (auto& q : p->gps) q.f32 = p->f32;
  p->n64 = p->f32 ? 0 : p->G;
  return GP_OK;
}
// Per-GP strip precision: bits[g] in {32, 64} for the plan's latent GPs in engine order [g_0..g_{P-1}, f_0..f_{P-1}] (a subset
// plan: its own rows, same order); float64 GPs must precede float32 ones — the transcription model's use is "activation
// GPs (Matern-3/2 on a 16-kHz grid: cond(Kuu) ~ 1e9) float64, component GPs float32".
gp_status gp_pdgp_set_gp_precision(gp_pdgp_plan p, const int32_t* bits, int32_t count) {
  if (!p || !bits || count != p->G) return GP_ERR_BAD_ARG;
  if (p->ws) return gp_fail(p->h, GP_ERR_BAD_ARG, "gp_pdgp_set_gp_precision: call it before gp_pdgp_set_workspace");
  int n64 = 0;
  for (int g = 0; g < count; g++) {
    if (bits[g] != 32 && bits[g] != 64) return gp_fail(p->h, GP_ERR_BAD_ARG, "gp_pdgp_set_gp_precision: bits must be 32 or 64");
    if (bits[g] == 64) { if (n64 != g) return gp_fail(p->h, GP_ERR_UNSUPPORTED, "gp_pdgp_set_gp_precision: float64 latent GPs must precede float32 ones"); n64 = g + 1; }
  }
  for (int g = 0; g < count; g++) p->gps[g].f32 = (bits[g] == 32);
  p->n64 = n64;
  p->f32 = (n64 == 0);
  p->cb.f32 = (n64 == 0);
  return GP_OK;
}
gp_status gp_pdgp_set_overlap(gp_pdgp_plan p, int32_t level) {
  if (!p || level < 0 || level > 2) return GP_ERR_BAD_ARG;
  p->overlap = level;
  p->cb.overlap = (level >= 1);
  return GP_OK;
}
gp_status gp_pdgp_set_frames_ascending(gp_pdgp_plan p, int32_t ascending) { return pdgp_set_perm(p, &PdgpPerms::frames_ascending, ascending != 0); }
gp_status gp_pdgp_set_far_act(gp_pdgp_plan p, int32_t enable) { return pdgp_set_perm(p, &PdgpPerms::afar_ok, enable != 0); }
gp_status gp_pdgp_set_scan_far(gp_pdgp_plan p, int32_t enable) { return pdgp_set_perm(p, &PdgpPerms::scan_far_ok, enable != 0); }
gp_status gp_pdgp_set_h_far(gp_pdgp_plan p, int32_t enable) { return pdgp_set_perm(p, &PdgpPerms::h_far_ok, enable != 0); }
gp_status gp_pdgp_set_qform(gp_pdgp_plan p, int32_t enable) {
  // bit 0: the Q route is allowed; bit 1: every MercerMatern12sm GP's inducing inputs ascend (the far field of its product);
  // bit 2: the backward pass may form Qbar and v from that far field too
  const bool on = (enable & 1) != 0, zasc = on && (enable & 2) != 0, bar = zasc && (enable & 4) != 0;
  (void)pdgp_set_perm(p, &PdgpPerms::qform, on); (void)pdgp_set_perm(p, &PdgpPerms::q_zasc, zasc);
  return pdgp_set_perm(p, &PdgpPerms::q_bar_ok, bar);
}
// what the batch last bound takes (pdgp_decide_routes); the backward pass's forms: of a bind with a gradient
int32_t gp_pdgp_far_field(gp_pdgp_plan p) { return (p && p->routes.nq > 0 && p->routes.q_far) ? 1 : 0; }
int32_t gp_pdgp_far_field_backward(gp_pdgp_plan p) { return (gp_pdgp_far_field(p) && p->routes.q_bar) ? 1 : 0; }
int32_t gp_pdgp_far_field_act(gp_pdgp_plan p) { return (p && p->routes.na > 0) ? 1 : 0; }
int32_t gp_pdgp_h_far(gp_pdgp_plan p) { return (gp_pdgp_far_field_act(p) && p->last_grad && p->routes.nhf > 0) ? 1 : 0; }
int32_t gp_pdgp_scan_far(gp_pdgp_plan p) {
  if (!gp_pdgp_far_field_act(p) || !p->last_grad) return 0;
  for (const auto& fam : p->hy_fams) if (fam.route == KUF_SCAN && fam.scan_far) return 1;
  return 0;
}
// debug: the device's own ranges and reference points of the last evaluation for latent GP i of the run [g0, g0 + nrun), whose
// groups are `group` frames, copied to the host (tests compare them with the numpy rules).  Returns the groups written.
static int32_t pdgp_debug_ranges(gp_pdgp_plan p, int32_t i, int g0, int nrun, int group, int32_t cap_groups, int* BwdBufs::*d_rng,
                                 double* BwdBufs::*d_ref, int32_t* gp_index, int32_t* rng, double* ref) {
  if (!p->ws || i < 0 || i >= nrun || p->last_n <= 0 || !rng || !ref) return 0;
  const int ng = p->last_n / group;
  const BwdBufs& b = p->bw[g0 + i];
  if (ng <= 0 || ng > cap_groups || !(b.*d_rng) || !(b.*d_ref)) return 0;
  gp_handle h = p->h;
  if (hipStreamSynchronize(h->stream) != hipSuccess) return 0;
  if (h->aux_stream && hipStreamSynchronize(h->aux_stream) != hipSuccess) return 0;
  if (h->side_stream && hipStreamSynchronize(h->side_stream) != hipSuccess) return 0;
  if (hipMemcpy(rng, b.*d_rng, (size_t)2 * ng * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  if (hipMemcpy(ref, b.*d_ref, (size_t)2 * ng * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  if (gp_index) *gp_index = g0 + i;
  return ng;
}
int32_t gp_debug_pdgp_far_ranges(gp_pdgp_plan p, int32_t i, int32_t cap_groups, int32_t* gp_index, int32_t* rng, double* ref,
                                 int32_t* rng2, int32_t* s0, int32_t* sa) {
  if (!p) return 0;
  const PdgpRoutes& r = p->routes;
  const int ng = pdgp_debug_ranges(p, i, r.q0, r.q_far ? r.nq : 0, QFAR_GROUP, cap_groups, &BwdBufs::qf_rng, &BwdBufs::qf_ref, gp_index, rng, ref);
  if (ng > 0 && r.q_bar && rng2 && s0 && sa && p->bw[r.q0 + i].qb_rng2 && p->bw[r.q0 + i].qb_tS) {
    const BwdBufs& b = p->bw[r.q0 + i];
    const int nt = p->gps[r.q0 + i].M / 16;
    if (hipMemcpy(rng2, b.qb_rng2, (size_t)2 * ng * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (hipMemcpy(s0, b.qb_tS, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (hipMemcpy(sa, b.qb_tS + QBAR_MAX_TILES, (size_t)nt * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) return 0;
  }
  return ng;
}
int32_t gp_debug_pdgp_act_ranges(gp_pdgp_plan p, int32_t i, int32_t cap_groups, int32_t* gp_index, int32_t* rng, double* ref) {
  return p ? pdgp_debug_ranges(p, i, p->routes.a0, p->routes.na, AFAR_GROUP, cap_groups, &BwdBufs::af_rng, &BwdBufs::af_ref, gp_index, rng, ref) : 0;
}
int64_t gp_pdgp_num_params(gp_pdgp_plan p) { return p ? p->nparams : 0; }

gp_status gp_pdgp_layout(gp_pdgp_plan p, int32_t g, int64_t* off_theta, int64_t* off_z, int64_t* off_qmu,
                         int64_t* off_qsqrt) {
  if (!p || g < 0 || g >= p->G) return GP_ERR_BAD_ARG;
  if (off_theta) *off_theta = p->gps[g].off_theta;
  if (off_z) *off_z = p->gps[g].off_z;
  if (off_qmu) *off_qmu = p->gps[g].off_qmu;
  if (off_qsqrt) *off_qsqrt = p->gps[g].off_qsqrt;
  return GP_OK;
}

// Every buffer of the plan's workspace, in order, into the plan's own members.  gp_pdgp_workspace_bytes runs it on a
// throwaway copy of the plan and a measuring arena.
static bool pdgp_carve(gp_pdgp_plan_s* p, GpArena& ar) {
  p->cb.tasks.assign(p->G, CondTask());
  p->cb.q_desc = false;      // (the Q route's descriptor regions, the activation far field's finish records: only where a GP could take one)
  for (int g = 0; g < p->G; g++) if (pdgp_may_q(p, g) || pdgp_may_afar(p, g)) p->cb.q_desc = true;
  p->cb.d_desc = ar.take<char>(cond_batch_desc_bytes(p->G, p->cb.q_desc));
  p->off = pdgp_misc_layout(p->G);
  p->d_misc = ar.take<char>(p->off.bytes);
  p->fmean = ar.take<double>((size_t)p->G * p->maxN);
  p->fvar = ar.take<double>((size_t)p->G * p->maxN);
  p->gFmu = ar.take<double>((size_t)p->G * p->maxN);
  p->gFvar = ar.take<double>((size_t)p->G * p->maxN);
  if (p->subset) {
    p->gF_full_mu = ar.take<double>((size_t)2 * p->P * p->maxN);
    p->gF_full_var = ar.take<double>((size_t)2 * p->P * p->maxN);
  }
  p->kl = ar.take<double>((size_t)p->G * GP_KL_BLOCKS);
  p->lik_partials = ar.take<double>(2 * (size_t)mpd_lik_blocks(p->maxN) + 8);
  for (int g = 0; g < p->G; g++) {
    CondTask& t = p->cb.tasks[g];
    t.M = p->gps[g].M;
    t.kern = DevKern{p->gps[g].ktype, p->gps[g].m, nullptr};
    t.f32 = p->gps[g].f32 != 0;
    cond_task_carve(ar, t, p->maxN, p->whiten != 0, t.f32);
  }
  p->bw.assign(p->G, BwdBufs());
  p->tr_part.assign(p->G, nullptr);
  if (!p->whiten)
    for (int g = 0; g < p->G; g++) p->tr_part[g] = ar.take<double>((size_t)gemm_rowblocks(p->gps[g].M, 0) * p->gps[g].M);
  {
    p->nsplit = gemm_nt_nsplit(p->maxM, p->maxN, p->G);
    if (p->nsplit < 2) p->nsplit = 2;
    for (int g = 0; g < p->G; g++) {
      const size_t M = p->gps[g].M;
      BwdBufs& b = p->bw[g];
      b.H = ar.take<double>(M * M); b.E = ar.take<double>(M * M); b.T1 = ar.take<double>(M * M);
      b.T2 = ar.take<double>(M * M); b.Wbar = ar.take<double>(M * M); b.R = ar.take<double>(M * M);
      b.G = ar.take<double>(gp_strip_doubles(M, p->maxN, p->gps[g].f32 != 0));
      // (Q route: like the scan's arrays below, reserved before its setters have spoken)
      if (pdgp_may_q(p, g)) {
        b.Q = ar.take<double>(M * M);
        // (its far field's tables, where the shape admits them: T and Psi are 4 mpad (N / 256 + N / M) rows of M doubles.  They
        // would fit the b.G strip a Q-route GP never uses only while 4 mpad (1 / 256 + 1 / M) <= 1 — not at M = 64 — so they
        // have a home of their own at every shape)
        if (pdgp_may_qfar(p, g)) {
          const QfarSizes qs = qfar_sizes((int)M, p->maxN, p->gps[g].m);
          b.qf_rng = (int*)ar.take<double>(qs.rng); b.qf_ref = ar.take<double>(qs.ref);
          b.qf_T = ar.take<double>(qs.T); b.qf_Psi = ar.take<double>(qs.Psi);
          // (the backward pass's use of the same far field, DESIGN.md 3.06: sized for every range — the lengthscale is trained on
          // the device.  At M = 512, N = 32768, m = 20 it is 0.41 of the b.G strip; like the tables it has a home of its own)
          if (pdgp_may_qbar(p, g)) {
            const QbarSizes bs = qbar_sizes((int)M, p->maxN, p->gps[g].m);
            b.qb_rng2 = (int*)ar.take<double>(bs.rng2); b.qb_tS = (int*)ar.take<double>(bs.tS);
            b.qb_CnF = ar.take<double>(bs.CnF); b.qb_CFF = ar.take<double>(bs.CFF); b.qb_cn = ar.take<double>(bs.cn);
            b.qb_cF = ar.take<double>(bs.cF); b.qb_Um = ar.take<double>(bs.Um); b.qb_Vp = ar.take<double>(bs.Um);
            b.qb_Wv = ar.take<double>(bs.Wv);
          }
        }
      }
      // (activation far field: reserved before its setters have spoken, for the plan's largest
      // batch — at M = 512, N = 32768: 4 MB of T, 1 MB of Psi, 2 MB of C per GP beside two 134 MB strips.
      // The backward window reads rng, T and Psi again, with W and the Kuf strip (kuf_scan_far_moments_kernel):
      // each has a region of its own in this walk and in cond_task_carve, nothing of the backward pass is carved over them, and
      // its launches only read W and Kuf — they stay the forward pass's until the next step's forward pass rewrites them)
      if (pdgp_may_afar(p, g)) {
        const AfarSizes as = afar_sizes((int)M, p->maxN);
        b.af_rng = (int*)ar.take<double>(as.rng); b.af_ref = ar.take<double>(as.ref);
        b.af_T = ar.take<double>(as.T); b.af_Psi = ar.take<double>(as.Psi); b.af_C = ar.take<double>(as.C);
        // (H from the stored A and these factors, DESIGN.md 3.10: the ranges are the device's own every step, so the store of Y is
        // sized by its bound — M / 16 + N / 256 - 1 slots of M x 16, the four far columns and A gm per group: at M = 512,
        // N = 32768 10.4 + 2.1 + 0.5 MB per GP — reserved like the tables, before the setters have spoken)
        if (pdgp_may_hfar(p, g)) {
          const HfarSizes hs = hfar_sizes((int)M, p->maxN);
          b.hf_Yn = ar.take<double>(hs.Yn); b.hf_Yf = ar.take<double>(hs.Yf); b.hf_up = ar.take<double>(hs.up);
          b.hf_flag = (int*)ar.take<double>(hs.flag);
        }
      }
      b.R32 = p->gps[g].f32 ? ar.take<double>((M * M + 1) / 2) : nullptr;
      b.u = ar.take<double>(M); b.Lu = ar.take<double>(M); b.alpha = ar.take<double>(M);
      b.upart = ar.take<double>((size_t)p->nsplit * M);
      const size_t ns = hyper_num_sums(p->gps[g].m);
      const size_t colblocks = (p->maxN + 255) / 256 + 1;
      b.hyp_part = ar.take<double>(ns * hyper_kuf_records(p->maxN, (int)M));
      b.hyp_part_uu = ar.take<double>(ns * hyper_kuf_records((int)M, (int)M));
      b.gz_part = ar.take<double>(colblocks * M + ((M + 255) / 256 + 1) * M);
      // moment arrays of the scan form of the Kuf-side contraction (kuf_scan.hip), for the GPs whose shape and types admit it:
      // 2 NQ (M + 1) doubles per chunk of 64 frames, 12.6 MB per GP at N = 32768, M = 512.  gp_pdgp_set_frames_ascending and
      // gp_pdgp_set_grad_needs may both be called after the workspace is set, so the carve cannot wait for them: the arrays
      // are reserved whether or not the caller goes on to make the promise.  With kuf_scan=0 nothing is reserved.
      if (pdgp_may_scan(p, g)) {
        b.ks_mom = ar.take<double>(kuf_scan_moment_doubles(p->maxN, (int)M, p->gps[g].ktype));
        b.ks_near = ar.take<double>(2 * (size_t)kuf_scan_chunks(p->maxN));
      }
    }
    {  // sum_n gv per GP, contiguous so one launch fills all of them
      double* gvs = ar.take<double>(p->G + 8);
      for (int g = 0; g < p->G; g++) p->bw[g].gvsum = gvs + g;
    }
    size_t slab_total = 0;
    for (int g = 0; g < p->G; g++) slab_total += gp_align_up((size_t)p->nsplit * p->gps[g].M * p->gps[g].M * sizeof(double), 256) / sizeof(double);
    p->slabs = ar.take<double>(slab_total);
    if (!p->whiten) {
      auto ev = [](size_t c) { return (c + 1) & ~(size_t)1; };   // keep every piece 16-byte aligned
      size_t tot = 0;
      for (int g = 0; g < p->G; g++) { const size_t M = p->gps[g].M; tot += 2 * (ev(M) + ev(M * M)); }
      p->qw_block = ar.take<double>(tot); p->qw_doubles = tot;
      double* c = p->qw_block;
      for (int g = 0; g < p->G && c; g++) {
        const size_t M = p->gps[g].M;
        BwdBufs& b = p->bw[g];
        b.qmu_w = c; c += ev(M); b.Lq_w = c; c += ev(M * M); b.g_qmu_w = c; c += ev(M); b.g_Lq_w = c; c += ev(M * M);
      }
      p->kl_dummy = ar.take<double>((size_t)p->G * GP_KL_BLOCKS);
    }
  }
  return ar.ok;
}

size_t gp_pdgp_workspace_bytes(gp_pdgp_plan p) {
  if (!p) return 0;
  gp_pdgp_plan_s dry = *p;      // a throwaway copy takes the null pointers: the plan owns nothing a destructor releases
  return gp_measure([&](GpArena& ar) { pdgp_carve(&dry, ar); }) + GP_WS_TAIL_PLAN;
}

gp_status gp_pdgp_set_workspace(gp_pdgp_plan p, void* workspace, size_t bytes) {
  if (!p) return GP_ERR_BAD_ARG;
  if (!workspace || bytes < gp_pdgp_workspace_bytes(p) || (((uintptr_t)workspace) & 255))
    return gp_fail(p->h, GP_ERR_WORKSPACE, "gp_pdgp_set_workspace: workspace too small or not 256-byte aligned");
  GpArena ar(workspace, bytes);
  if (!pdgp_carve(p, ar)) return gp_fail(p->h, GP_ERR_WORKSPACE, "gp_pdgp_set_workspace: arena exhausted");
  p->ws = workspace; p->ws_bytes = bytes;
  p->last_params = nullptr; p->last_n = -1;
  return GP_OK;
}

}  // extern "C"

// (re)bind the parameter vector / batch to the device descriptors: task pointers, the families (with a gradient), the routes —
// which need both — then the forward descriptors, the backward ones, one upload
static gp_status pdgp_bind(gp_pdgp_plan p, const double* params, const double* x, int n, double* grad,
                           double* fmean, double* fvar) {
  gp_handle h = p->h;
  // (the batch pointers x / y are not part of any descriptor: a fresh minibatch tensor every step must not
  //  force a re-upload)
  const bool same = (p->last_params == params && p->last_n == n && p->last_grad == grad &&
                     p->cb.tasks[0].fmean == fmean);
  if (same && p->cb.uploaded) return GP_OK;
  for (int g = 0; g < p->G; g++) {
    CondTask& t = p->cb.tasks[g];
    const PdgpGP& q = p->gps[g];
    t.kern.theta = params + q.off_theta;
    t.z = params + q.off_z;
    t.q_mu = params + q.off_qmu;
    t.q_sqrt = params + q.off_qsqrt;
    t.fmean = fmean + (size_t)g * n;
    t.fvar = fvar + (size_t)g * n;
  }
  p->cb.N = n;
  p->cb.maxM = p->maxM;
  if (grad) pdgp_build_families(p);
  pdgp_decide_routes(p, n, grad != nullptr);
  const PdgpRoutes& rt = p->routes;
  p->cb.q0 = rt.q0; p->cb.nq = rt.nq; p->cb.q_far = rt.q_far; p->cb.a0 = rt.a0; p->cb.na = rt.na;     // (the one copy CondBatch gets)
  for (int g = 0; g < p->G; g++) {
    const bool q = pdgp_on_q_route(p, g);
    CondTask& t = p->cb.tasks[g];
    t.Qm = q ? p->bw[g].Q : nullptr;
    t.beta = q ? p->bw[g].alpha : nullptr;
    t.far_rng = (q && rt.q_far) ? p->bw[g].qf_rng : nullptr;
    t.far_T = (q && rt.q_far) ? p->bw[g].qf_T : nullptr;
    t.far_Psi = (q && rt.q_far) ? p->bw[g].qf_Psi : nullptr;
  }
  GP_CHECK(cond_batch_upload(h, p->cb, p->whiten != 0, p->jitter));
  // KL items
  p->h_misc.assign(p->off.bytes, 0);
  for (int g = 0; g < p->G; g++) {
    const PdgpGP& q = p->gps[g];
    const CondTask& t = p->cb.tasks[g];
    if (p->whiten) {
      kl_item_fill(p->h_misc.data() + p->off.kl_items + g * kl_item_bytes(), params + q.off_qmu, params + q.off_qsqrt,
                   q.M, p->kl + (size_t)g * GP_KL_BLOCKS, grad ? grad + q.off_qmu : nullptr, grad ? grad + q.off_qsqrt : nullptr);
    } else {
      klu_item_fill(p->h_misc.data() + p->off.kl_items + g * klu_item_bytes(), params + q.off_qmu, params + q.off_qsqrt,
                    t.L, t.W, p->tr_part[g], gemm_rowblocks(q.M, 0), q.M, p->kl + (size_t)g * GP_KL_BLOCKS);
      // trace term: column sums of squares of W Lq (its own descriptor slot, after the backward ones)
      GemmProblem& r = *(GemmProblem*)(p->h_misc.data() + p->off.kltr + g * sizeof(GemmProblem));
      memset(&r, 0, sizeof(r));
      r.A = t.W; r.lda = q.M; r.B = params + q.off_qsqrt; r.ldb = q.M; r.M = q.M; r.N = q.M; r.K = q.M; r.ldc = q.M;
      r.o0 = p->tr_part[g];
    }
  }
  pdgp_upload_qform(p, params);
  pdgp_upload_afar(p, params);
  if (grad) pdgp_upload_bwd(p, params, n, grad);
  GP_HIP_CHECK(h, hipMemcpyAsync(p->d_misc, p->h_misc.data(), p->off.bytes, hipMemcpyHostToDevice, h->stream));
  p->last_params = params; p->last_x = x; p->last_n = n; p->last_grad = grad;
  return GP_OK;
}

extern "C" {

// Shared body of gp_pdgp_elbo (xchg == NULL, one call) and of the two-stage pitch-sharded form:
//   stage 1 (begin): conditionals, per-frame partial sums [A | B | D] and sum of the local KL terms -> xchg[0..3n]
//   stage 2 (end)  : likelihood + gradients from the rank-summed xchg, local backward pass.
static gp_status pdgp_forward(gp_pdgp_plan p, const double* params, const double* x, const double* y, int n,
                              double* grad, double* xchg, double* fmean = nullptr, double* fvar = nullptr) {
  gp_handle h = p->h;
  p->factor_valid = false;   // an optimiser step normally follows: predictions must re-factorise
  GP_CHECK(pdgp_bind(p, params, x, n, grad, fmean ? fmean : p->fmean, fvar ? fvar : p->fvar));
  if (grad) GP_HIP_CHECK(h, hipMemsetAsync(grad, 0, (size_t)p->nparams * sizeof(double), h->stream));
  // (an ELBO takes the Q route with or without a gradient, so a step's ELBO is one number; predictions never do)
  const std::function<gp_status()> q_prepare = [&]() -> gp_status { return pdgp_qform_prepare(p, x, n); };
  // (so does the activations' far field: predictions keep the dense products)
  const std::function<gp_status()> a_run = [&]() -> gp_status { return pdgp_afar_run(p, x, n); };
  {
    const gp_status st = cond_batch_run(h, p->cb, x, n, p->whiten != 0, p->jitter, false, p->routes.nq > 0 ? &q_prepare : nullptr, p->routes.na > 0 ? &a_run : nullptr);
    // the Q run's product is enqueued (or the run failed): the guard joins the main stream ahead of everything that follows
    const gp_status sj = pdgp_qform_join(p);
    GP_CHECK(st); GP_CHECK(sj);
  }
  bool kl_done = false;   // the whitened KL kernel went to the helper stream with the backward prefetch
  if (grad) GP_CHECK(pdgp_prefetch_backward(p, n, &kl_done));
  if (kl_done) GP_HIP_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_era, 0));   // behind the forward strips: no stall
  if (xchg) {
    GP_CHECK(launch_mpd_lik(h, p->fmean, p->fvar, 1, n, y, n, p->P, p->nlin, params, 1.0, nullptr, nullptr, nullptr,
                            nullptr, nullptr, xchg, nullptr));
  }
  if (p->whiten) {
    if (!kl_done) GP_CHECK(launch_kl_white(h, p->d_misc + p->off.kl_items, p->G));
  } else {
    // gauss_kl(q_mu, q_sqrt, K = Kuu + jitter I) (pdgp.py:123-129): L and W of the conditional are reused
    // (one value per GP: the other partial-sum slots of the whitened layout stay zero)
    GP_HIP_CHECK(h, hipMemsetAsync(p->kl, 0, (size_t)p->G * GP_KL_BLOCKS * sizeof(double), h->stream));
    GemmFlags f;
    f.triA = TRI_LOWER; f.triB = TRI_LOWER; f.epilogue = EPI_COLSUMSQ;
    GP_CHECK(launch_gemm_batched(h, (const GemmProblem*)(p->d_misc + p->off.kltr), p->G, p->maxM, p->maxM, f));
    GP_CHECK(launch_kl_unwhite(h, p->d_misc + p->off.kl_items, p->G));
  }
  if (xchg) GP_CHECK(launch_finish_sum(h, p->kl, p->G * GP_KL_BLOCKS, 1, 1, xchg + 3 * (size_t)n, 1.0, 0));
  return GP_OK;
}

// GP-sharded plan: rows grow[l] of the whole model's gradient arrays -> this plan's compact [G][n] arrays
struct RowGather { int rows[64]; int count; };
__global__ void __launch_bounds__(256) rows_gather_kernel(const double* __restrict__ src_mu, const double* __restrict__ src_var,
                                                          double* __restrict__ dst_mu, double* __restrict__ dst_var,
                                                          RowGather rg, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x, l = blockIdx.y;
  if (i >= n) return;
  const size_t s = (size_t)rg.rows[l] * n + i, d = (size_t)l * n + i;
  dst_mu[d] = src_mu[s];
  dst_var[d] = src_var[s];
}

// full_mu / full_var / kl_total != NULL: the GP-sharded second stage (moments of ALL 2 P latent GPs, [2 P][n], and the
// whole model's KL sum as one device double)
static gp_status pdgp_finish(gp_pdgp_plan p, const double* params, const double* x, const double* y, int n,
                             double num_data, const double* xchg, double* elbo_dev, double* elbo_host, double* grad,
                             const double* full_mu = nullptr, const double* full_var = nullptr,
                             const double* kl_total = nullptr) {
  gp_handle h = p->h;
  int nb = 0;
  const double scale = num_data / (double)n;
  if (full_mu) {
    GP_CHECK(launch_mpd_lik(h, full_mu, full_var, 1, n, y, n, p->P, p->nlin, params, scale, nullptr, p->lik_partials, &nb,
                            grad ? p->gF_full_mu : nullptr, grad ? p->gF_full_var : nullptr, nullptr, nullptr));
    if (grad) {
      for (int l0 = 0; l0 < p->G; l0 += 64) {
        RowGather rg;
        rg.count = p->G - l0 < 64 ? p->G - l0 : 64;
        for (int l = 0; l < rg.count; l++) rg.rows[l] = p->grow[l0 + l];
        hipLaunchKernelGGL(rows_gather_kernel, dim3((n + 255) / 256, rg.count), dim3(256), 0, h->stream, p->gF_full_mu,
                           p->gF_full_var, p->gFmu + (size_t)l0 * n, p->gFvar + (size_t)l0 * n, rg, n);
        GP_HIP_CHECK(h, hipGetLastError());
      }
    }
  } else {
    GP_CHECK(launch_mpd_lik(h, p->fmean, p->fvar, 1, n, y, n, p->P, p->nlin, params, scale, nullptr, p->lik_partials, &nb,
                            grad ? p->gFmu : nullptr, grad ? p->gFvar : nullptr, nullptr, xchg));
  }
  const double* kl_one = kl_total ? kl_total : (xchg ? xchg + 3 * (size_t)n : nullptr);
  if (grad) {     // (pdgp_backward launches it)
    p->fin.lik_partials = p->lik_partials; p->fin.nb = nb; p->fin.elbo = elbo_dev; p->fin.g_noise = grad; p->fin.pending = true;
    if (kl_one) { p->fin.kl = kl_one; p->fin.nkl = 1; } else { p->fin.kl = p->kl; p->fin.nkl = p->G * GP_KL_BLOCKS; }
    GP_CHECK(pdgp_backward(p, params, x, n, grad));
    if (p->fin.pending) return gp_fail(h, GP_ERR_HIP, "pdgp_backward left the ELBO reduction behind");
  } else if (kl_one) GP_CHECK(launch_elbo_finish(h, p->lik_partials, nb, kl_one, 1, elbo_dev, nullptr));
  else GP_CHECK(launch_elbo_finish(h, p->lik_partials, nb, p->kl, p->G * GP_KL_BLOCKS, elbo_dev, nullptr));
  if (elbo_host) {
    GP_HIP_CHECK(h, hipMemcpyAsync(elbo_host, elbo_dev, sizeof(double), hipMemcpyDeviceToHost, h->stream));
    GP_CHECK(check_not_pd(h));
  }
  return GP_OK;
}

gp_status gp_pdgp_elbo(gp_pdgp_plan p, const double* params, const double* x, const double* y, int32_t n,
                       double num_data, double* elbo_dev, double* elbo_host, double* grad) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->ws) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgp_elbo: workspace not set");
  if (!params || !x || !y || !elbo_dev || n < 1 || n > p->maxN) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_elbo: bad argument");
  if (p->subset) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_elbo: a GP-sharded plan is evaluated with gp_pdgp_cond_begin / _end");
  GP_CHECK(pdgp_forward(p, params, x, y, n, grad, nullptr));
  return pdgp_finish(p, params, x, y, n, num_data, nullptr, elbo_dev, elbo_host, grad);
}

gp_status gp_pdgp_elbo_begin(gp_pdgp_plan p, const double* params, const double* x, const double* y, int32_t n,
                             double* grad, double* exchange) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->ws) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgp_elbo_begin: workspace not set");
  if (!params || !x || !y || !exchange || n < 1 || n > p->maxN) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_elbo_begin: bad argument");
  if (p->subset) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_elbo_begin: a GP-sharded plan is evaluated with gp_pdgp_cond_begin / _end");
  p->staged_n = 0;
  GP_CHECK(pdgp_forward(p, params, x, y, n, grad, exchange));
  p->staged_n = n; p->staged_grad = grad; p->staged_params = params;
  return GP_OK;
}

/* GP-sharded evaluation (SURVEY section 8e option 2): see include/gpitch_abi.h */
gp_status gp_pdgp_cond_begin(gp_pdgp_plan p, const double* params, const double* x, int32_t n, double* grad,
                             double* fmean_local, double* fvar_local, double* kl_local_sum) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->ws) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgp_cond_begin: workspace not set");
  if (!p->subset) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_cond_begin: not a gp_pdgp_create_subset plan");
  if (!params || !x || !fmean_local || !fvar_local || !kl_local_sum || n < 1 || n > p->maxN)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_cond_begin: bad argument");
  p->staged_n = 0;
  GP_CHECK(pdgp_forward(p, params, x, nullptr, n, grad, nullptr, fmean_local, fvar_local));
  GP_CHECK(launch_finish_sum(h, p->kl, p->G * GP_KL_BLOCKS, 1, 1, kl_local_sum, 1.0, 0));
  p->staged_n = n; p->staged_grad = grad; p->staged_params = params;
  return GP_OK;
}

gp_status gp_pdgp_cond_end(gp_pdgp_plan p, const double* params, const double* x, const double* y, int32_t n,
                           double num_data, const double* fmean_full, const double* fvar_full, const double* kl_total,
                           double* elbo_dev, double* elbo_host, double* grad) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->subset) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_cond_end: not a gp_pdgp_create_subset plan");
  if (!params || !x || !y || !fmean_full || !fvar_full || !kl_total || !elbo_dev)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_cond_end: bad argument");
  if (p->staged_n != n || p->staged_grad != grad || p->staged_params != params)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_cond_end: no matching gp_pdgp_cond_begin (same params, n and grad required)");
  p->staged_n = 0;
  return pdgp_finish(p, params, x, y, n, num_data, nullptr, elbo_dev, elbo_host, grad, fmean_full, fvar_full, kl_total);
}

gp_status gp_pdgp_elbo_end(gp_pdgp_plan p, const double* params, const double* x, const double* y, int32_t n,
                           double num_data, const double* exchange, double* elbo_dev, double* elbo_host, double* grad) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!params || !x || !y || !exchange || !elbo_dev) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_elbo_end: bad argument");
  if (p->staged_n != n || p->staged_grad != grad || p->staged_params != params)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_elbo_end: no matching gp_pdgp_elbo_begin (same params, n and grad required)");
  p->staged_n = 0;
  return pdgp_finish(p, params, x, y, n, num_data, exchange, elbo_dev, elbo_host, grad);
}

static gp_status pdgp_predict_impl(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, double* fmean,
                                   double* fvar, double* mean_source, bool reuse_factor) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->ws) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgp_predict: workspace not set");
  if (!params || !xnew || !fmean || !fvar || n < 1 || n > p->maxN) return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_predict: bad argument");
  if (p->subset && mean_source)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_predict: a GP-sharded plan holds single latent GPs, not (activation, component) pairs: mean_source must be NULL");
  if (reuse_factor && !p->factor_valid)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_predict_reuse: no factorisation to reuse (call gp_pdgp_predict first)");
  GP_CHECK(pdgp_bind(p, params, xnew, n, nullptr, fmean, fvar));
  GP_CHECK(cond_batch_run(h, p->cb, xnew, n, p->whiten != 0, p->jitter, reuse_factor));
  if (mean_source) GP_CHECK(launch_mean_source(h, fmean, p->P, n, p->nlin, mean_source));
  gp_status st = check_not_pd(h);
  p->factor_valid = (st == GP_OK);
  return st;
}

gp_status gp_pdgp_predict(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, double* fmean,
                          double* fvar, double* mean_source) {
  return pdgp_predict_impl(p, params, xnew, n, fmean, fvar, mean_source, false);
}

gp_status gp_pdgp_predict_reuse(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, double* fmean,
                                double* fvar, double* mean_source) {
  return pdgp_predict_impl(p, params, xnew, n, fmean, fvar, mean_source, true);
}

// the conditionals into the plan's own fmean / fvar ([2P][n], never copied out), then the moments kernel on them
static gp_status pdgp_predict_moments_impl(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n,
                                           const double* ynew, int32_t with_noise, double* smean, double* svar, double* ymean,
                                           double* yvar, double* logp, bool reuse_factor) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (!p->ws) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgp_predict_moments: workspace not set");
  if (p->subset)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_predict_moments: a GP-sharded plan holds only some of the 2P rows (assemble them and call gp_mpd_predict_moments)");
  if (!params || !xnew || n < 1 || n > p->maxN || (logp && !ynew))
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_predict_moments: bad argument (logp needs ynew)");
  if (reuse_factor && !p->factor_valid)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_predict_moments_reuse: no factorisation to reuse (call gp_pdgp_predict or gp_pdgp_predict_moments first)");
  GP_CHECK(pdgp_bind(p, params, xnew, n, nullptr, p->fmean, p->fvar));
  GP_CHECK(cond_batch_run(h, p->cb, xnew, n, p->whiten != 0, p->jitter, reuse_factor));
  GP_CHECK(launch_mpd_moments(h, p->fmean, p->fvar, 1, n, ynew, n, p->P, p->nlin, params, with_noise != 0, smean, svar, ymean,
                              yvar, logp));
  gp_status st = check_not_pd(h);
  p->factor_valid = (st == GP_OK);
  return st;
}

gp_status gp_pdgp_predict_moments(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, const double* ynew,
                                  int32_t with_noise, double* smean, double* svar, double* ymean, double* yvar, double* logp) {
  return pdgp_predict_moments_impl(p, params, xnew, n, ynew, with_noise, smean, svar, ymean, yvar, logp, false);
}

gp_status gp_pdgp_predict_moments_reuse(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n,
                                        const double* ynew, int32_t with_noise, double* smean, double* svar, double* ymean,
                                        double* yvar, double* logp) {
  return pdgp_predict_moments_impl(p, params, xnew, n, ynew, with_noise, smean, svar, ymean, yvar, logp, true);
}

// Joint posterior draws (sample.hip).  Every argument, the host array `order` included, is checked before anything is
// enqueued.  The plain form factorises every Kuu at `params` without a conditional (n is not bounded by the plan's batch:
// the descriptors are bound for min(n, max_batch) frames, which only the factorisation's choice of path looks at).
static gp_status pdgp_sample_impl(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, const int32_t* order_host,
                                  int32_t S, const double* eps_x, const double* eps_z, const double* eps_u, double* latents,
                                  double* sources, void* workspace, size_t workspace_bytes, bool reuse_factor) {
  if (!p) return GP_ERR_BAD_ARG;
  gp_handle h = p->h;
  if (p->subset)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_sample: a GP-sharded plan holds only some of the 2P latent GPs");
  if (!params || !xnew || !order_host || !eps_x || !eps_z || !eps_u || !latents || !workspace || n < 1 || S < 1)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_sample: bad argument (n >= 1, S >= 1, no null pointers but sources)");
  if (!p->ws) return gp_fail(h, GP_ERR_WORKSPACE, "gp_pdgp_sample: workspace not set");
  if (reuse_factor && !p->factor_valid)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_pdgp_sample_reuse: no factorisation to reuse (call gp_pdgp_sample or gp_pdgp_predict first)");
  std::vector<PsmGP> gps(p->G);
  for (int g = 0; g < p->G; g++) {
    const PdgpGP& q = p->gps[g];
    gps[g] = PsmGP{DevKern{q.ktype, q.m, params + q.off_theta}, params + q.off_z, p->cb.tasks[g].W, params + q.off_qmu,
                   params + q.off_qsqrt, q.M};
  }
  GP_CHECK(pdgp_sample_check(h, gps.data(), p->G, n, S, order_host, workspace, workspace_bytes));
  if (!reuse_factor) {
    p->factor_valid = false;
    GP_CHECK(pdgp_bind(p, params, xnew, n < p->maxN ? n : p->maxN, nullptr, p->fmean, p->fvar));
    GP_CHECK(cond_batch_factor(h, p->cb));
  }
  GP_CHECK(pdgp_sample_run(h, gps.data(), p->P, p->whiten != 0, p->nlin, p->jitter, xnew, n, S, order_host, eps_x, eps_z, eps_u,
                           latents, sources, workspace, workspace_bytes));
  gp_status st = check_not_pd(h);
  if (!reuse_factor) p->factor_valid = (st == GP_OK);
  return st;
}

gp_status gp_pdgp_sample(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, const int32_t* order_host,
                         int32_t S, const double* eps_x, const double* eps_z, const double* eps_u, double* latents,
                         double* sources, void* workspace, size_t workspace_bytes) {
  return pdgp_sample_impl(p, params, xnew, n, order_host, S, eps_x, eps_z, eps_u, latents, sources, workspace, workspace_bytes,
                          false);
}

gp_status gp_pdgp_sample_reuse(gp_pdgp_plan p, const double* params, const double* xnew, int32_t n, const int32_t* order_host,
                               int32_t S, const double* eps_x, const double* eps_z, const double* eps_u, double* latents,
                               double* sources, void* workspace, size_t workspace_bytes) {
  return pdgp_sample_impl(p, params, xnew, n, order_host, S, eps_x, eps_z, eps_u, latents, sources, workspace, workspace_bytes,
                          true);
}

size_t gp_pdgp_sample_workspace_bytes(int32_t G, int32_t maxM, int32_t C, int32_t n, int32_t S) {
  return pdgp_sample_workspace_bytes(G, maxM, C, n, S);
}

}  // extern "C"
