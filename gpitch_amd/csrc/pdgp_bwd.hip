// pdgp_bwd.hip — host orchestration of the Pdgp ELBO's reverse pass: descriptor slots, the Q route's host code and guard
// kernel, the bind-time descriptor upload and the backward schedule.  The algebra, the element-wise helpers and the
// contraction kernels it launches are in bwd.hip, and so is the kernel-gradient chain (Wbar, R and alpha, the Cholesky
// adjoint: engine.h ChainSlot), which this plan shares with sgpr.hip and sgpr_batch.hip.
#include "pdgp_plan.h"
#include <string.h>
#include <stdlib.h>

// ---------------------------------------------------------------------------------------------
// orchestration
// slots below S_E are batched over all latent GPs, slots from S_E on over the GPs whose kernel gradients are needed.
// S_CHAIN: the first of the shared chain's CH_COUNT slots (engine.h ChainSlot), S_CHAIN + CH_x each; this file names the three
// it launches itself.  S_QW_* / S_GQ_* / S_WB_*: unwhitened model only (see pdgp_backward).
enum BwdSlot { S_H = 0, S_U, S_HLQ, S_QW_MU, S_QW_L, S_GQ_MU, S_GQ_L,
               S_E, S_CHAIN, S_R = S_CHAIN + CH_R, S_ALPHA = S_CHAIN + CH_ALPHA, S_G = S_CHAIN + CH_G, S_WB_R1 = S_CHAIN + CH_COUNT, S_WB_L,
               // Q route, entry i = latent GP q0 + i: E, R, beta and Q = R W of the forward pass (filled whether or
               // not a gradient is asked), then T = W Qbar, H = T W^T and u = W v of the backward pass
               S_QE, S_QR, S_QALPHA, S_QQ, S_QT, S_QHH, S_QU,
               // activation far field, entry i = latent GP a0 + i: C = tril(Lq)^T W of the forward pass
               S_AC,
               S_COUNT };
static_assert(S_COUNT <= PDGP_KLTR_SLOT, "pdgp_plan.h: the backward slots must stay below the KL trace slot");
static inline const GemmProblem* slot_probs(gp_pdgp_plan p, int slot) { return (const GemmProblem*)(p->d_misc + p->off.bwd[slot]); }
// record i of a slot's host copy, zeroed and square
static inline GemmProblem& host_prob(gp_pdgp_plan p, int slot, int i, int M) {
  GemmProblem& r = *((GemmProblem*)(p->h_misc.data() + p->off.bwd[slot]) + i);
  gemm_problem_square(r, M);
  return r;
}

// ---- Q route --------------------------------------------------------------------------------------------------------
// With E = Lq Lq^T - I, Q = W^T E W and beta = W^T q_mu the whitened conditional is
//   fmean = Kuf^T beta,  fvar = kdiag + colsum(Kuf o G),  G = Q Kuf                      (one dense strip product)
// and its reverse pass
//   Kuf_bar = G diag(2 gv) + beta gm^T        (no product: the contraction reads G and scales its columns)
//   Qbar = Kuf diag(2 gv) Kuf^T, v = Kuf gm   (the split-K product on Kuf);  H = W Qbar W^T, u = W v: the chain's H and u.
// Which latent GPs take it at n frames: pdgp_decide_routes.
// the forward pass's descriptors of the Q run (pdgp_bind, with or without a gradient)
void pdgp_upload_qform(gp_pdgp_plan p, const double* params) {
  for (int i = 0; i < p->routes.nq; i++) {
    const int g = p->routes.q0 + i;
    const PdgpGP& q = p->gps[g];
    const CondTask& t = p->cb.tasks[g];
    const BwdBufs& b = p->bw[g];
    const int M = q.M;
    auto P = [&](int slot) -> GemmProblem& { return host_prob(p, slot, i, M); };
    const double* q_sqrt = params + q.off_qsqrt;
    { GemmProblem& r = P(S_QE); r.A = q_sqrt; r.B = q_sqrt; r.C = b.E; }
    { GemmProblem& r = P(S_QR); r.A = t.W; r.B = b.E; r.C = b.R; }
    { GemmProblem& r = P(S_QALPHA); r.A = t.W; r.v0 = params + q.off_qmu; r.o0 = b.alpha; }
    // (the guard reads L through v0: qform_guard_kernel)
    { GemmProblem& r = P(S_QQ); r.A = b.R; r.B = t.W; r.C = b.Q; r.v0 = t.L; }
    if (p->routes.q_far) {     // (feature tables: cov_item_fill's layout of t.feat — z first, then the frames)
      QfarItem& it = *(QfarItem*)(p->h_misc.data() + p->off.qf_items + i * sizeof(QfarItem));
      const size_t nfz = gp_align_up((size_t)2 * sm_mpad(q.m) * M, 32);
      it = QfarItem{t.z, t.kern.theta, t.feat, t.feat + nfz, b.Q, b.qf_rng, b.qf_ref, b.qf_T, b.qf_Psi, M, 0};
    }
  }
}

// Guard of the Q route: Q inverts Kuu + jitter I explicitly, so its error grows with cond_2 of that matrix (not its root), and
// the lengthscale is trained on the device.  c = ||L||_F^2 ||W||_F^2 = tr(K) tr(K^-1) >= cond_2(K); above GP_QFORM_COND_MAX M^2
// (switches.h; or not finite) the handle's status word is raised, as the scan's frame check does, and the next host-scalar call fails.
__global__ void __launch_bounds__(256) qform_guard_kernel(const GemmProblem* __restrict__ probs, int g0, double cmax, int32_t* status) {
  const GemmProblem p = probs[blockIdx.x];
  const double* L = p.v0;
  const double* W = p.B;
  double sl = 0.0, sw = 0.0;
  for (int idx = threadIdx.x; idx < p.M * p.M; idx += 256)      // (the lower triangles: above them L still holds Kuu)
    if (idx % p.M <= idx / p.M) { sl = fma(L[idx], L[idx], sl); sw = fma(W[idx], W[idx], sw); }
  __shared__ double red[2][4];
  for (int o = 32; o > 0; o >>= 1) { sl += __shfl_down(sl, o, 64); sw += __shfl_down(sw, o, 64); }
  if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = sl; red[1][threadIdx.x >> 6] = sw; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double c = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) * ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3]));
    if (!(c <= cmax * (double)p.M * (double)p.M)) { status[0] = 4; status[1] = 0; status[2] = g0 + (int)blockIdx.x; }
  }
}

// The same verdict from row-wise loads (switch far_tables): 1024 threads per GP, wavefront w takes the rows
// r = w, w + 16, ... four at a time, a lane the entries 2 l, 2 l + 1 (+ 128 k) of each up to the diagonal as one 16-byte load
// of L and one of W (M even and both 16-byte aligned; else 8-byte loads), eight independent loads and four accumulators per
// matrix in flight, no integer division.  Entries above the diagonal are not requested, and the odd one beside the diagonal
// is zeroed in the registers.  A fixed order — lane sums, the wavefront's shuffle tree, the sixteen wavefronts in turn — and
// no atomics: two runs agree bit for bit.  The order is not qform_guard_kernel's, so c may differ from its c in the last
// bits; c is compared with the bound and reaches no output.
typedef double qg_d2 __attribute__((ext_vector_type(2)));
__global__ void __launch_bounds__(1024) qform_guard_rows_kernel(const GemmProblem* __restrict__ probs, int g0, double cmax, int32_t* status) {
  const GemmProblem p = probs[blockIdx.x];
  const double* L = p.v0;
  const double* W = p.B;
  const int M = p.M, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool wide = (M & 1) == 0 && ((((uintptr_t)L) | ((uintptr_t)W)) & 15) == 0;
  double sl[4] = {0.0, 0.0, 0.0, 0.0}, sw[4] = {0.0, 0.0, 0.0, 0.0};
  for (int rb = wave; rb < M; rb += 64) {
    const int rtop = min(rb + 48, M - 1);                        // the longest of the four rows
    for (int k = lane; 2 * k <= rtop; k += 64) {
      qg_d2 l[4], w[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int r = rb + 16 * u;
        l[u] = w[u] = qg_d2{0.0, 0.0};
        if (r < M && 2 * k <= r) {
          const size_t o = (size_t)r * M + 2 * k;
          if (wide) { l[u] = *(const qg_d2*)(L + o); w[u] = *(const qg_d2*)(W + o); }
          else { l[u].x = L[o]; w[u].x = W[o]; if (2 * k + 1 <= r) { l[u].y = L[o + 1]; w[u].y = W[o + 1]; } }
          if (2 * k + 1 > r) { l[u].y = 0.0; w[u].y = 0.0; }
        }
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        sl[u] = fma(l[u].x, l[u].x, sl[u]); sl[u] = fma(l[u].y, l[u].y, sl[u]);
        sw[u] = fma(w[u].x, w[u].x, sw[u]); sw[u] = fma(w[u].y, w[u].y, sw[u]);
      }
    }
  }
  double tl = (sl[0] + sl[1]) + (sl[2] + sl[3]), tw = (sw[0] + sw[1]) + (sw[2] + sw[3]);
  __shared__ double red[2][16];
  for (int o = 32; o > 0; o >>= 1) { tl += __shfl_down(tl, o, 64); tw += __shfl_down(tw, o, 64); }
  if (lane == 0) { red[0][wave] = tl; red[1][wave] = tw; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double al = red[0][0], aw = red[1][0];
    for (int q = 1; q < 16; q++) { al += red[0][q]; aw += red[1][q]; }
    const double c = al * aw;
    if (!(c <= cmax * (double)M * (double)M)) { status[0] = 4; status[1] = 0; status[2] = g0 + (int)blockIdx.x; }
  }
}

// far_wait: the far field's tables (qfar.hip) follow Q and precede the guard — the guard is one workgroup per GP and, beside
// the other GPs' strip products, the longest link of this chain, while the tables are what the product waits for.  They read
// the feature tables of the Kuf builds, which the main stream has enqueued: on the helper stream (far_wait) they first wait
// for the event cond_batch_run left behind those builds.  tables_done: recorded between the tables and the guard — the product
// reads Q and the tables, not the guard's verdict.
gp_status pdgp_qform_join(gp_pdgp_plan p);
static gp_status qform_chain(gp_pdgp_plan p, const double* x, int n, bool far_wait, hipEvent_t tables_done = nullptr) {
  gp_handle h = p->h;
  const int nq = p->routes.nq, maxM = p->maxM;
  GP_CHECK(launch_chain_e(h, slot_probs(p, S_QE), nq, maxM));
  GP_CHECK(launch_chain_r_alpha(h, slot_probs(p, S_QR), slot_probs(p, S_QALPHA), nq, maxM));
  GemmFlags f; f.triB = TRI_LOWER;        // Q = R W
  GP_CHECK(launch_gemm_batched(h, slot_probs(p, S_QQ), nq, maxM, maxM, f));
  if (p->routes.q_far) {
    if (far_wait && hipStreamWaitEvent(h->stream, h->ev_feat, 0) != hipSuccess) return gp_fail(h, GP_ERR_HIP, "event hand-over to the helper stream failed");
    GP_CHECK(launch_qfar_tables(h, (const QfarItem*)(p->d_misc + p->off.qf_items), nq, maxM, p->gps[p->routes.q0].m, x, n));
  }
  if (tables_done && hipEventRecord(tables_done, h->stream) != hipSuccess) return gp_fail(h, GP_ERR_HIP, "event hand-over from the helper stream failed");
  if (gp_switches().far_tables != 0)
    hipLaunchKernelGGL(qform_guard_rows_kernel, dim3(nq), dim3(1024), 0, h->stream, slot_probs(p, S_QQ), p->routes.q0, (double)GP_QFORM_COND_MAX, h->d_status);
  else
    hipLaunchKernelGGL(qform_guard_kernel, dim3(nq), dim3(256), 0, h->stream, slot_probs(p, S_QQ), p->routes.q0, (double)GP_QFORM_COND_MAX, h->d_status);
  if (hipGetLastError() != hipSuccess) return gp_fail(h, GP_ERR_HIP, "qform guard launch failed");
  return GP_OK;
}

// E, R, beta, Q, the far field's tables and the guard of the Q run: cond_batch_run's hook (pdgp.hip).  On the helper stream when the plan overlaps
// (behind the factorisation it has just run, beside the other GPs' strip products), else in line.  From the helper stream
// h->stream waits here for Q and the tables only (ev_q, recorded ahead of the guard); the guard's event (ev_guard) is waited
// for by pdgp_qform_join, which pdgp_forward calls once the product is enqueued: the status word is complete before anything
// of the step's tail and before any host-scalar read, with or without a gradient.
gp_status pdgp_qform_prepare(gp_pdgp_plan p, const double* x, int n) {
  gp_handle h = p->h;
  h->guard_pending = false;
  if (p->routes.nq <= 0) return GP_OK;
  bool aux = (n >= 4096) && p->overlap >= 2 && h->aux_stream && !h->aux_active;
  if (aux && p->routes.q_far && !p->cb.feat_ready) aux = false;
  if (aux && !h->ev_q && hipEventCreateWithFlags(&h->ev_q, hipEventDisableTiming) != hipSuccess) { h->ev_q = nullptr; aux = false; }
  if (aux && !h->ev_guard && hipEventCreateWithFlags(&h->ev_guard, hipEventDisableTiming) != hipSuccess) { h->ev_guard = nullptr; aux = false; }
  gp_status st;
  { GpStreamScope on(h, aux ? h->aux_stream : nullptr); st = qform_chain(p, x, n, aux, aux ? h->ev_q : nullptr); }
  hipError_t e = hipSuccess;
  if (aux) {
    // (whatever the chain enqueued on the helper stream is joined, also when it failed half way)
    e = hipEventRecord(h->ev_guard, h->aux_stream);
    if (e == hipSuccess) h->guard_pending = true;
    if (e == hipSuccess && st == GP_OK) e = hipStreamWaitEvent(h->stream, h->ev_q, 0);
    if (st != GP_OK) (void)pdgp_qform_join(p);
  }
  GP_CHECK(st);
  if (e != hipSuccess) return gp_fail(h, GP_ERR_HIP, "event hand-over from the helper stream failed");
  return GP_OK;
}

// h->stream waits for the guard that pdgp_qform_prepare left on the helper stream (nothing to do when it ran in line)
gp_status pdgp_qform_join(gp_pdgp_plan p) {
  gp_handle h = p->h;
  if (!h->guard_pending) return GP_OK;
  h->guard_pending = false;
  if (hipStreamWaitEvent(h->stream, h->ev_guard, 0) != hipSuccess) return gp_fail(h, GP_ERR_HIP, "event hand-over from the helper stream failed");
  return GP_OK;
}

// ---- activation far field ---------------------------------------------------------------------------
// A Matern-3/2 Kuf is exactly semiseparable along sorted inputs, so A = W Kuf and Lq^T A = (Lq^T W) Kuf need, per 256-frame
// group, only the rows of Kuf near the group plus two M x 2 tables per factor (afar.hip).  Nothing is inverted that the Cholesky
// route does not invert, and the backward pass reads the same A strip.  Which latent GPs take it at n frames: pdgp_decide_routes.
// the forward pass's descriptors of that run (pdgp_bind, with or without a gradient)
void pdgp_upload_afar(gp_pdgp_plan p, const double* params) {
  for (int i = 0; i < p->routes.na; i++) {
    const int g = p->routes.a0 + i;
    const PdgpGP& q = p->gps[g];
    const CondTask& t = p->cb.tasks[g];
    const BwdBufs& b = p->bw[g];
    const int M = q.M;
    GemmProblem& r = host_prob(p, S_AC, i, M);
    r.A = params + q.off_qsqrt; r.B = t.W; r.C = b.af_C;
    AfarItem& it = *(AfarItem*)(p->h_misc.data() + p->off.af_items + i * sizeof(AfarItem));
    it = AfarItem{t.z, t.kern.theta, t.W, b.af_C, t.Kuf, t.q_mu, t.A, t.s1, t.s2, t.dot,
                  b.af_rng, b.af_ref, b.af_T, b.af_Psi, gp_strip_ld(p->cb.N, false), M, 0};
  }
}

// C = tril(Lq)^T W, the tables and the product of the run: cond_batch_run's hook (pdgp.hip), on the main stream behind W
gp_status pdgp_afar_run(gp_pdgp_plan p, const double* x, int n) {
  gp_handle h = p->h;
  if (p->routes.na <= 0) return GP_OK;
  GemmFlags f;
  f.transA = 1; f.triA = TRI_UPPER; f.triB = TRI_LOWER;
  GP_CHECK(launch_gemm_batched(h, slot_probs(p, S_AC), p->routes.na, p->maxM, p->maxM, f));
  return launch_afar(h, (const AfarItem*)(p->d_misc + p->off.af_items), p->routes.na, p->maxM, x, n);
}

// E = Lq Lq^T - I (ERA_E) and R = W^T E, alpha = W^T q_mu (ERA_R) over the compacted batch without the Q run, whose E, R and
// beta the forward pass has left: the slots before the run, then those behind it (no run: qk0 = nq = 0, the whole batch)
enum { ERA_E = 1, ERA_R = 2 };
static gp_status pdgp_era(gp_pdgp_plan p, int parts) {
  gp_handle h = p->h;
  const int maxM = p->maxM, behind = p->routes.qk0 + p->routes.nq;
  const int s0[2] = {0, behind}, cnt[2] = {p->routes.qk0, p->nK - behind};
  for (int r = 0; r < 2; r++) {
    if (cnt[r] <= 0) continue;
    if (parts & ERA_E) GP_CHECK(launch_chain_e(h, slot_probs(p, S_E) + s0[r], cnt[r], maxM));
    if (parts & ERA_R) GP_CHECK(launch_chain_r_alpha(h, slot_probs(p, S_R) + s0[r], slot_probs(p, S_ALPHA) + s0[r], cnt[r], maxM));
  }
  return GP_OK;
}

// The compacted batch (the latent GPs whose kernel gradients are asked) and its kernel families — same type, partial count and
// precision, in kgps order; one contraction launch per family and side.  Host work on the plan alone, ahead of the routes.
void pdgp_build_families(gp_pdgp_plan p) {
  p->kgps.clear();
  for (int g = 0; g < p->G; g++) if (p->gps[g].need_theta || p->gps[g].need_z) p->kgps.push_back(g);
  p->nK = (int)p->kgps.size();
  p->hy_fams.clear();
  for (auto& q : p->gps) q.fam = -1;
  for (size_t s = 0; s < p->kgps.size(); s++) {
    const int g = p->kgps[s];
    const PdgpGP& q = p->gps[g];
    const int key_m = gp_kern_has_partials(q.ktype) ? q.m : 0;
    int fi = -1;
    for (size_t f = 0; f < p->hy_fams.size(); f++)
      if (p->hy_fams[f].type == q.ktype && p->hy_fams[f].m == key_m && p->hy_fams[f].f32 == q.f32) fi = (int)f;
    if (fi < 0) { gp_pdgp_plan_s::HyFamily nf; nf.type = q.ktype; nf.m = key_m; nf.M = q.M; nf.f32 = q.f32; nf.batched = true; p->hy_fams.push_back(nf); fi = (int)p->hy_fams.size() - 1; }
    gp_pdgp_plan_s::HyFamily& fam = p->hy_fams[fi];
    fam.gps.push_back(g);
    p->gps[g].fam = fi;
    if (q.M != fam.M || q.need_z || !q.need_theta) fam.batched = false;   // the per-GP path handles those
  }
  int nitems = 0;
  for (auto& fam : p->hy_fams) {
    fam.first = nitems; fam.count = (int)fam.gps.size(); nitems += fam.count;
    fam.mfma = (gp_kern_is_mercer(fam.type) && fam.batched) ? 1 : 0;
    fam.scan_ws = true;
    for (int g : fam.gps) if (!pdgp_may_scan(p, g)) fam.scan_ws = false;
    int s0 = -1;             // its first slot, when its GPs sit in one run of the compacted batch
    for (size_t s = 0; s < p->kgps.size(); s++) if (p->kgps[s] == fam.gps[0]) s0 = (int)s;
    for (size_t i = 0; i < fam.gps.size(); i++)
      if (s0 < 0 || s0 + (int)i >= (int)p->kgps.size() || p->kgps[s0 + i] != fam.gps[i]) { s0 = -1; break; }
    fam.slot0 = s0;
  }
}

// Every route of the bound batch (DESIGN.md 3.04's table), once per bind: from shapes, types, precision, the gradient needs, the
// switches and the permissions — never from the overlap level or the schedule's switches (scan_side, kufbar_split): every level
// must give the same bits.  Writes p->routes and the families' route, scan_far and np_uf; launches nothing, reads no device
// memory.  A decision may rest on the ones above it, never on one below.  Whether a GP's workspace has a route's regions is
// asked of the pdgp_may_* predicate that carved them, not of the pointers: nothing the predicates read can change once the
// workspace is set (pdgp_plan.h), so an item never gets a null table.
void pdgp_decide_routes(gp_pdgp_plan p, int n, bool grad) {
  const GpSwitches& sw = gp_switches();
  const PdgpPerms& pm = p->perms;
  const int G = p->G, maxM = p->maxM;
  PdgpRoutes& r = p->routes;
  r = PdgpRoutes();
  auto kernel_is = [p](int type) { return [p, type](int g) { return p->gps[g].ktype == type; }; };
  int first = 0, cnt = 0, m = -1, qk0 = 0;
  // 1. The Q run (3.03): ALL MercerMatern12sm GPs of a whitened plan, float64, trained hyper-parameters over fixed inducing inputs,
  // one partial count, one run — as every other family of the compacted batch is, since Kuf_bar is then issued family by family
  // — and the wave product and the lean contraction, the one kernel that applies the column scale, take the shape
  auto q_bad = [&](int g) {
    const PdgpGP& q = p->gps[g];
    const bool bad = q.f32 || !q.need_theta || q.need_z || !pdgp_may_q(p, g) || (m >= 0 && q.m != m);
    m = q.m;
    return bad;
  };
  auto families_distinct = [&]() {       // in the compacted batch; counts the slots ahead of the run on its way
    struct Key { int type, m, f32; };
    std::vector<Key> seen;
    for (int g = 0; g < G; g++) {
      const PdgpGP& q = p->gps[g];
      if (!(q.need_theta || q.need_z)) continue;
      if (g < first) qk0++;
      const Key k{q.ktype, gp_kern_has_partials(q.ktype) ? q.m : 0, q.f32};
      if (!seen.empty() && seen.back().type == k.type && seen.back().m == k.m && seen.back().f32 == k.f32) continue;
      for (const Key& s : seen) if (s.type == k.type && s.m == k.m && s.f32 == k.f32) return false;
      seen.push_back(k);
    }
    return true;
  };
  if (sw.qform && pm.qform && p->whiten && pdgp_single_run(G, kernel_is(GP_KERN_MERCER_MATERN12SM), q_bad, &first, &cnt) && cnt > 0 &&
      families_distinct() && cond_batch_uniform(p->cb, n) && gemm_wave_takes(6, maxM, n, 1) && hyper_lean_takes(GP_KERN_MERCER_MATERN12SM, m, maxM, n, cnt)) {
    r.q0 = first; r.nq = cnt; r.qk0 = qk0;
    // 2. its product's far field (3.05): frames and inducing inputs both promised ascending, the switch, the shape, the tables
    r.q_far = sw.qform_far != 0 && pm.frames_ascending && pm.q_zasc && gemm_wave_takes(7, maxM, n, 1) && qfar_takes(maxM, n, m);
    for (int g = first; g < first + cnt; g++) r.q_far = r.q_far && pdgp_may_qfar(p, g) && p->gps[g].M == maxM;
    // 3. Qbar and v from the same far field (3.06): the switch, the caller's bit, the shape, the workspace — and the latent GPs left
    // to the split-K product are one non-empty run of its float64 problems, so it stays one launch
    r.q_bar = r.q_far && sw.qform_qbar != 0 && pm.q_bar_ok && qbar_takes(maxM, n, m) && (first == 0 || first + cnt == p->n64) && p->n64 > cnt;
    for (int g = first; g < first + cnt; g++) r.q_bar = r.q_bar && pdgp_may_qbar(p, g);
  }
  // 4. The activations' run (3.07): ALL Matern-3/2 GPs of a whitened plan, float64, over fixed inducing inputs, of the batch's one
  // M, in one run, none of them on the Q route; frames promised ascending
  auto a_bad = [&](int g) { const PdgpGP& q = p->gps[g]; return q.f32 || q.need_z || q.M != maxM || !pdgp_may_afar(p, g) || pdgp_on_q_route(p, g); };
  if (sw.act_far && pm.afar_ok && p->whiten && pm.frames_ascending && pdgp_single_run(G, kernel_is(GP_KERN_MATERN32), a_bad, &first, &cnt) &&
      cnt > 0 && cond_batch_uniform(p->cb, n) && afar_takes(maxM, n)) { r.a0 = first; r.na = cnt; }
  if (!grad) return;
  auto on_a_run = [&r](int g) { return g >= r.a0 && g < r.a0 + r.na; };
  r.nt_uniform = ((n & 3) == 0) ? 1 : 0;
  for (const PdgpGP& q : p->gps) if (q.M != maxM) r.nt_uniform = 0;
  r.kuf_uniform = ((n & 1) == 0) ? 1 : 0;
  for (int g : p->kgps) {          // (slots of the compacted batch keep the GPs' order: its float64 GPs come first)
    if (p->gps[g].M != maxM) r.kuf_uniform = 0;
    if (!p->gps[g].f32) r.k64++;
  }
  r.contiguous = p->whiten && !p->hy_fams.empty();
  for (const auto& fam : p->hy_fams) if (fam.slot0 < 0) r.contiguous = false;
  // 5. Each family's Kuf route.  Priority: the Q run's family, the scan, the fused epilogue, else the stored product.  The scan and
  // the fused form need every family in one run of the compacted batch, since Kuf_bar is then issued family by family;
  // fam.batched says one M, hyper-parameter gradients of every GP, no inducing-input gradient.
  //   scan : Matern-3/2 / Matern-5/2 over frames the caller promised ascending (kuf_scan.hip), float64 strips, M <= 1024.
  //          Matern-1/2 (kink at 0) and RBF (not semiseparable) have no such form.
  //   fused: a stationary family that wants Kuf_bar for two sums per GP only: they come out of the product's epilogue
  //          (gemm_strip.hip role 5; whole tiles) and neither the strip nor the separate contraction exists.
  for (auto& fam : p->hy_fams) {
    fam.route = KUF_PRODUCT; fam.np_uf = fam.np_uu = 0; fam.scan_far = false;
    if (r.nq > 0 && fam.gps[0] == r.q0) {
      fam.route = KUF_QFORM;
    } else if (r.contiguous && sw.kuf_scan != 0 && pm.frames_ascending && fam.batched && !fam.f32 && fam.scan_ws &&
               kuf_scan_nq(fam.type) > 0 && fam.M <= 1024) {
      fam.route = KUF_SCAN; fam.np_uf = kuf_scan_records(fam.M);
      r.any_scan = true;
      // its moments from the factored A (3.09): a Matern-3/2 family all of whose GPs are in the activations' run at this batch
      // size (that run's conditions — float64, one M, n a multiple of 256 — come with it), in a plan of float64 strips throughout
      fam.scan_far = sw.scan_far != 0 && pm.scan_far_ok && fam.type == GP_KERN_MATERN32 && r.na > 0;
      for (int g : fam.gps) if (!on_a_run(g)) fam.scan_far = false;
      for (const PdgpGP& q : p->gps) if (q.f32) fam.scan_far = false;
    } else if (r.contiguous && r.kuf_uniform && fam.batched && !fam.mfma && fam.M == maxM &&
               (fam.f32 ? gemm_f32_fused_contraction_ok(maxM, n, fam.type) : gemm_strip_fused_contraction_ok(maxM, n, fam.type))) {
      fam.route = KUF_FUSED;
      fam.np_uf = !fam.f32 ? gemm_fused_contraction_records(maxM, n, fam.type)
                           : gemm_wave_f32_takes(5, maxM, n, r.kuf_uniform) ? (maxM / 64) * (n / 64) : (maxM / 128) * (n / 128);
    }
    if (fam.route != KUF_PRODUCT) r.any_routed = true;
  }
  // 6. H and u of the activations' run from the stored A once and its factors once (3.10): the switch, gp_pdgp_set_h_far, a plan of
  // float64 strips throughout, the workspace — and the latent GPs left to the dense split-K product (neither in this run nor in
  // the Q run when qbar.hip has its Qbar) are one run of the batch, or none
  bool hf = sw.h_far != 0 && pm.h_far_ok && r.na > 0 && p->n64 == G && hfar_takes(maxM, n);
  for (const PdgpGP& q : p->gps) if (q.f32) hf = false;
  for (int g = r.a0; g < r.a0 + r.na; g++) if (!pdgp_may_hfar(p, g)) hf = false;
  auto left_dense = [&](int g) { return !on_a_run(g) && !(r.q_bar && pdgp_on_q_route(p, g)); };
  if (hf && pdgp_single_run(G, left_dense, [](int) { return false; }, &first, &cnt)) { r.nhf = r.na; r.hd0 = first; r.hdn = cnt; }
}
// do the family's Kuf-side partial sums come with its Kuf_bar step (no contraction launch of its own)?
static inline bool kuf_sums_with_step(const gp_pdgp_plan_s::HyFamily& fam) { return fam.route == KUF_FUSED || fam.route == KUF_SCAN; }

// the backward pass's descriptors (pdgp_bind with a gradient, behind the families and the routes)
void pdgp_upload_bwd(gp_pdgp_plan p, const double* params, int n, double* grad) {
  const int G = p->G;
  p->h_fin_items.clear();       // the descriptor block is rewritten: force a fresh upload of the finish items
  const bool white = p->whiten != 0;
  size_t slab_off = 0;
  int kslot = 0;
  for (int g = 0; g < G; g++) {
    const PdgpGP& q = p->gps[g];
    const CondTask& t = p->cb.tasks[g];
    const BwdBufs& b = p->bw[g];
    const int M = q.M;
    const int64_t ldN = gp_strip_ld(n, q.f32 != 0);     // this GP's strips: float64 or float32 (per-GP precision)
    // unwhitened model: the chain runs on the equivalent whitened state q' = (W q_mu, W Lq) and its gradient
    // buffers; pdgp_backward maps the result back (see there)
    const double* q_mu = white ? params + q.off_qmu : b.qmu_w;
    const double* q_sqrt = white ? params + q.off_qsqrt : b.Lq_w;
    double* g_mu = white ? grad + q.off_qmu : b.g_qmu_w;
    double* g_sqrt = white ? grad + q.off_qsqrt : b.g_Lq_w;
    const double* gm = p->gFmu + (size_t)g * n;
    const double* gv = p->gFvar + (size_t)g * n;
    const bool kneed = (q.need_theta || q.need_z);
    auto P = [&](int slot) -> GemmProblem& {
      // E, Kuf_bar and the unwhitened additions to Wbar are batched, as the chain is, over the GPs that need kernel gradients only
      const bool kchain = (slot >= S_E);
      if (kchain && !kneed) { memset(&p->dummy_prob, 0, sizeof(p->dummy_prob)); return p->dummy_prob; }
      return host_prob(p, slot, kchain ? kslot : g, M);
    };
    { GemmProblem& r = P(S_H); r.A = t.A; r.lda = ldN; r.B = t.A; r.ldb = ldN; r.K = n; r.v1 = gv; r.C = b.H;
      r.o2 = p->slabs + slab_off; slab_off += gp_align_up((size_t)p->nsplit * M * M * sizeof(double), 256) / sizeof(double);
      // fused u = A gm: partials per K-slice in o1, result in o0 and accumulated into grad q_mu (xa)
      r.v2 = gm; r.o1 = b.upart; r.o0 = b.u; r.xa = g_mu;
      // Q route: the same product on Kuf gives Qbar (into T2) and v = Kuf gm (into Lu); H and u follow from S_QT / S_QHH / S_QU
      if (pdgp_on_q_route(p, g)) { r.A = t.Kuf; r.B = t.Kuf; r.C = b.T2; r.o0 = b.Lu; r.xa = nullptr; } }
    if (pdgp_on_q_route(p, g)) {
      auto PQ = [&](int slot) -> GemmProblem& { return host_prob(p, slot, g - p->routes.q0, M); };
      { GemmProblem& r = PQ(S_QT); r.A = t.W; r.B = b.T2; r.C = b.T1; }
      { GemmProblem& r = PQ(S_QHH); r.A = b.T1; r.B = t.W; r.C = b.H; }
      { GemmProblem& r = PQ(S_QU); r.A = t.W; r.v0 = b.Lu; r.o0 = b.u; r.o1 = g_mu; }
      if (p->routes.q_bar) {   // Qbar and v from the far field (qbar.hip) into the same T2 and Lu; the split-K launch skips this GP
        QbarItem& it = *(QbarItem*)(p->h_misc.data() + p->off.qb_items + (g - p->routes.q0) * sizeof(QbarItem));
        it = QbarItem{t.Kuf, ldN, gv, gm, t.z, t.kern.theta, t.feat, b.qf_rng, b.qf_ref, b.qf_Psi, b.qb_rng2, b.qb_tS,
                      b.qb_CnF, b.qb_CFF, b.qb_cn, b.qb_cF, b.qb_Um, b.qb_Vp, b.qb_Wv, b.T2, b.Lu, M, 0};
      }
    }
    { GemmProblem& r = P(S_U); r.A = t.A; r.lda = ldN; r.N = n; r.v0 = gm; r.o0 = b.u; r.o1 = g_mu; r.a_f32 = q.f32; }
    { GemmProblem& r = P(S_HLQ); r.A = b.H; r.B = q_sqrt; r.C = g_sqrt; }
    if (!white) {
      const double* qm = params + q.off_qmu;
      const double* qs = params + q.off_qsqrt;
      { GemmProblem& r = P(S_QW_MU); r.A = t.W; r.v0 = qm; r.o0 = b.qmu_w; }
      { GemmProblem& r = P(S_QW_L); r.A = t.W; r.B = qs; r.C = b.Lq_w; }
      { GemmProblem& r = P(S_GQ_MU); r.A = t.W; r.v0 = b.g_qmu_w; r.o0 = grad + q.off_qmu; }
      { GemmProblem& r = P(S_GQ_L); r.A = t.W; r.B = b.g_Lq_w; r.C = grad + q.off_qsqrt; }
      { GemmProblem& r = P(S_WB_R1); r.C = b.Wbar; r.v0 = b.g_qmu_w; r.v1 = qm; }
      { GemmProblem& r = P(S_WB_L); r.A = b.g_Lq_w; r.B = qs; r.C = b.Wbar; }
      kl_item_fill(p->h_misc.data() + p->off.kl2 + g * kl_item_bytes(), b.qmu_w, b.Lq_w, M, p->kl_dummy + (size_t)g * GP_KL_BLOCKS, b.g_qmu_w,
                   b.g_Lq_w);
    }
    { GemmProblem& r = P(S_E); r.A = q_sqrt; r.B = q_sqrt; r.C = b.E; }
    if (kneed)
      chain_fill(chain_slots(p->h_misc.data(), &p->off.bwd[S_CHAIN]), kslot, M,
                 ChainBufs{t.L, t.W, b.E, b.H, b.u, q_mu, b.T1, b.T2, b.Wbar, b.R, b.Lu, b.alpha});
    { GemmProblem& r = P(S_G); r.A = b.R; r.B = t.A; r.ldb = ldN; r.N = n; r.v1 = gv; r.C = b.G; r.ldc = ldN; r.xb = b.R32;
      // (read only by the form that contracts Kuf_bar with dK/dtheta in its epilogue — gemm_strip.hip role 5)
      r.kern = t.kern; r.xa = params + q.off_z; r.v0 = b.alpha; r.v2 = gm; r.o0 = b.hyp_part; }
    if (kneed) kslot++;
  }
  for (int i = 0; i < p->routes.nhf; i++) {      // hfar.hip's items: the product's own slabs and u partials, which the slab reduction sums
    const int g = p->routes.a0 + i;
    const CondTask& t = p->cb.tasks[g];
    const BwdBufs& b = p->bw[g];
    const GemmProblem& r = *((const GemmProblem*)(p->h_misc.data() + p->off.bwd[S_H]) + g);
    HfarItem& it = *(HfarItem*)(p->h_misc.data() + p->off.hf_items + i * sizeof(HfarItem));
    it = HfarItem{t.A, t.Kuf, t.W, p->gFvar + (size_t)g * n, p->gFmu + (size_t)g * n, b.af_rng, b.af_T, b.af_Psi,
                  b.hf_Yn, b.hf_Yf, b.hf_up, b.hf_flag, r.o2, r.o1, gp_strip_ld(n, false), p->gps[g].M, g};
  }
  // Kuf-side contractions: the families' item arrays.  x2 stays null in the items: the frames of the batch come with the launch
  // (their pointer may change from step to step without a descriptor upload).
  {
    HyperItem* items = (HyperItem*)(p->h_misc.data() + p->off.hy_items);
    KufScanItem* sitems = (KufScanItem*)(p->h_misc.data() + p->off.ks_items);
    for (auto& fam : p->hy_fams) {
      int pos = fam.first;
      for (int g : fam.gps) {
        const PdgpGP& q = p->gps[g];
        const CondTask& t = p->cb.tasks[g];
        const BwdBufs& bb = p->bw[g];
        {    // the same GP's record for the scan form (kuf_scan.hip), used only on that route
          KufScanItem& si = sitems[pos];
          memset(&si, 0, sizeof(si));
          si.A = t.A; si.lda = gp_strip_ld(n, q.f32 != 0); si.gv = p->gFvar + (size_t)g * n; si.gm = p->gFmu + (size_t)g * n;
          si.R = bb.R; si.alpha = bb.alpha; si.z = params + q.off_z; si.theta = t.kern.theta;
          si.mom = bb.ks_mom; si.near = bb.ks_near; si.partials = bb.hyp_part; si.M = q.M;
          if (fam.route == KUF_SCAN && fam.scan_far) { si.Kuf = t.Kuf; si.W = t.W; si.rng = bb.af_rng; si.T = bb.af_T; si.Psi = bb.af_Psi; }
        }
        HyperItem& it = items[pos++];
        memset(&it, 0, sizeof(it));
        const int64_t ldN = gp_strip_ld(n, q.f32 != 0);
        it.k = t.kern; it.x1 = params + q.off_z; it.n1 = q.M; it.x2 = nullptr; it.n2 = n; it.G = bb.G; it.ldg = ldN;
        it.alpha = bb.alpha; it.gm = p->gFmu + (size_t)g * n; it.symmetric = 0; it.partials = bb.hyp_part; it.gz = nullptr;
        it.kvals = t.Kuf; it.ldk = ldN; it.g32 = q.f32;
        if (fam.route == KUF_QFORM) { it.G = t.A; it.gscale = p->gFvar + (size_t)g * n; }     // Q route: G = Q Kuf, in A's strip
        if (gp_kern_is_mercer(q.ktype) && t.feat) {
          it.f1 = t.feat;
          it.f2 = t.feat + gp_align_up((size_t)2 * sm_mpad(q.m) * q.M, 32);
        }
        // its Kuu-side twin (contraction of Kuu_bar = E with dK(z, z)): G entries further on
        HyperItem& iu = items[G + pos - 1];
        memset(&iu, 0, sizeof(iu));
        iu.k = t.kern; iu.x1 = params + q.off_z; iu.n1 = q.M; iu.x2 = iu.x1; iu.n2 = q.M; iu.G = bb.E; iu.ldg = q.M;
        iu.symmetric = 1; iu.partials = bb.hyp_part_uu;
        if (gp_kern_is_mercer(q.ktype) && t.feat) { iu.f1 = t.feat; iu.f2 = t.feat; }
      }
    }
  }
}

// R = W^T (Lq Lq^T - I) and alpha = W^T q_mu depend on the parameters and on W only: when the helper stream exists they
// are enqueued on it during the FORWARD pass.  The helper stream is in order: they follow whatever cond_batch_run's hooks have
// put there, which with a Q run is the factorisation, E, R, beta, Q, the far field's tables and the GUARD (qform_chain), so
// they start when the guard ends.  pdgp_forward makes the main stream wait for ev_era ahead of the
// likelihood, since the whitened KL terms (parameters only) ride along here and the ELBO needs them: the prefetch is on the
// forward pass's path, and so is everything in front of it on the helper stream.  The backward pass finds R and alpha ready.
gp_status pdgp_prefetch_backward(gp_pdgp_plan p, int n, bool* kl_done) {
  gp_handle h = p->h;
  p->era_ready = false;
  if (kl_done) *kl_done = false;
  if (!(p->whiten && p->nK > 0 && n >= 4096 && p->overlap >= 2 && h->aux_stream && !h->aux_active)) return GP_OK;
  if (!h->ev_era && hipEventCreateWithFlags(&h->ev_era, hipEventDisableTiming) != hipSuccess) { h->ev_era = nullptr; return GP_OK; }
  gp_status st;
  {
    GpStreamScope on(h, h->aux_stream);
    st = pdgp_era(p, ERA_E | ERA_R);
    if (st == GP_OK && kl_done) {
      st = launch_kl_white(h, p->d_misc + p->off.kl_items, p->G);
      *kl_done = (st == GP_OK);
    }
  }
  hipError_t e = hipEventRecord(h->ev_era, h->aux_stream);
  GP_CHECK(st);
  if (e != hipSuccess) return gp_fail(h, GP_ERR_HIP, "hipEventRecord on the helper stream failed");
  p->era_ready = true;
  return GP_OK;
}

// ---- the backward pass's steps: each enqueues on h->stream, wherever the schedule (pdgp_backward) has pointed it ----------
struct BwdCall { gp_pdgp_plan p; const double* params; const double* x; int n; double* grad;
                 bool qbar_ahead; };      // this pass has put the far-field Qbar's launches on the main stream (pdgp_backward)
typedef gp_pdgp_plan_s::HyFamily HyFamily;

// conditional(whiten=False) + gauss_kl(q_mu, q_sqrt, K) (pdgp.py:123-129, 147-155) is the whitened model at
//   q_mu' = W q_mu,  Lq' = W Lq      (W = chol(Kuu + jitter I)^-1),
// so the whitened chain runs on (q_mu', Lq') with gradient buffers (g', G'), and afterwards
//   grad q_mu = W^T g',  grad q_sqrt = tril(W^T G'),  Wbar += tril(g' q_mu^T + G' Lq^T).
static gp_status bwd_unwhitened_head(const BwdCall& c) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  GP_HIP_CHECK(h, hipMemsetAsync(p->qw_block, 0, p->qw_doubles * sizeof(double), h->stream));
  GP_CHECK(launch_matvec_batched(h, slot_probs(p, S_QW_MU), p->G, p->maxM, 0));
  GemmFlags f; f.triA = TRI_LOWER; f.triB = TRI_LOWER; f.triC = TRI_LOWER;
  GP_CHECK(launch_gemm_batched(h, slot_probs(p, S_QW_L), p->G, p->maxM, p->maxM, f));
  return launch_kl_white(h, p->d_misc + p->off.kl2, p->G);   // accumulates -dKL/dq' into (g', G')
}
static gp_status bwd_unwhitened_tail(const BwdCall& c) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  GP_CHECK(launch_matvec_batched(h, slot_probs(p, S_GQ_MU), p->G, p->maxM, 1));
  GemmFlags f; f.transA = 1; f.triA = TRI_UPPER; f.triB = TRI_LOWER; f.triC = TRI_LOWER;
  return launch_gemm_batched(h, slot_probs(p, S_GQ_L), p->G, p->maxM, p->maxM, f);
}

// sum_n gv (the kdiag term) and the ELBO's final reduction (pdgp.hip: pdgp_finish): wanted only when the step ends
static gp_status bwd_late_sums(const BwdCall& c) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  GP_CHECK(launch_batched_sum(h, p->gFvar, (int64_t)c.n, c.n, p->G, p->bw[0].gvsum));
  if (p->fin.pending) {
    p->fin.pending = false;
    GP_CHECK(launch_elbo_finish(h, p->fin.lik_partials, p->fin.nb, p->fin.kl, p->fin.nkl, p->fin.elbo, p->fin.g_noise));
  }
  return GP_OK;
}

static gp_status bwd_qbar(const BwdCall& c) {
  gp_pdgp_plan p = c.p;
  return launch_qbar(p->h, (const QbarItem*)(p->d_misc + p->off.qb_items), p->routes.nq, p->maxM, p->gps[p->routes.q0].m, c.n);
}

// H = A diag(2 gv) A^T (symmetric, split-K over the frames; u = A gm and grad q_mu += u are fused into it), grad q_sqrt
static gp_status bwd_h_chain(const BwdCall& c) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  const int G = p->G, maxM = p->maxM, n64 = p->n64;     // latent GPs [0, n64): float64 strips, [n64, G): float32 strips
  GemmFlags f;
  if (p->routes.nhf > 0) {     // the activations' run from the stored A once and its factors once (hfar.hip), the dense product on the others
    if (p->routes.q_bar && !c.qbar_ahead) GP_CHECK(bwd_qbar(c));
    if (p->routes.hdn > 0) GP_CHECK(launch_gemm_nt_reduce_batched(h, slot_probs(p, S_H) + p->routes.hd0, p->routes.hdn, maxM, c.n, p->nsplit, 1, 1, 2.0, p->routes.nt_uniform));
    GP_CHECK(launch_hfar(h, (const HfarItem*)(p->d_misc + p->off.hf_items), p->routes.nhf, maxM, c.n, p->nsplit,
                        p->routes.hdn == 0 ? gemm_nt_reduce_charges(maxM, c.n, p->nsplit, p->routes.nt_uniform) : 0));
    GP_CHECK(launch_slab_reduce(h, slot_probs(p, S_H) + p->routes.a0, p->routes.nhf, maxM, p->nsplit, 1, 1.0));      // (Y carries the factor 2)
    if (p->routes.q_bar && c.qbar_ahead) GP_HIP_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_q, 0));
  } else if (p->routes.q_bar) {       // the Q run's Qbar and v from its far field (four launches, no timer class); the product on the other run
    const int rest0 = (p->routes.q0 == 0) ? p->routes.nq : 0;
    if (!c.qbar_ahead) GP_CHECK(bwd_qbar(c));
    GP_CHECK(launch_gemm_nt_reduce_batched(h, slot_probs(p, S_H) + rest0, n64 - p->routes.nq, maxM, c.n, p->nsplit, 1, 1, 2.0, p->routes.nt_uniform));
    // (pdgp_backward put them on the main stream, beside this product: S_QT waits for them here)
    if (c.qbar_ahead) GP_HIP_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_q, 0));
  } else if (n64 > 0) GP_CHECK(launch_gemm_nt_reduce_batched(h, slot_probs(p, S_H), n64, maxM, c.n, p->nsplit, 1, 1, 2.0, p->routes.nt_uniform));
  if (n64 < G) GP_CHECK(launch_gemm_f32_nt_reduce_batched(h, slot_probs(p, S_H) + n64, G - n64, maxM, c.n, p->nsplit, 1, 1, 2.0, p->routes.nt_uniform));
  if (p->routes.nq > 0) {      // Q route: that product gave Qbar and v; H = (W Qbar) W^T, u = W v, grad q_mu += u
    f = GemmFlags(); f.triA = TRI_LOWER;
    GP_CHECK(launch_gemm_batched(h, slot_probs(p, S_QT), p->routes.nq, maxM, maxM, f));
    f = GemmFlags(); f.transB = 1; f.triB = TRI_UPPER;
    GP_CHECK(launch_gemm_batched(h, slot_probs(p, S_QHH), p->routes.nq, maxM, maxM, f));
    GP_CHECK(launch_matvec_batched(h, slot_probs(p, S_QU), p->routes.nq, maxM, 0));
  }
  // grad q_sqrt += tril(H Lq)
  f = GemmFlags(); f.triB = TRI_LOWER; f.triC = TRI_LOWER; f.beta = 1.0;
  return launch_gemm_batched(h, slot_probs(p, S_HLQ), G, maxM, maxM, f);
}

// T1 = E H;  Wbar = tril(T1 L^T) + tril(mu (L u)^T)
static gp_status bwd_wbar_chain(const BwdCall& c) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  const int nK = p->nK, maxM = p->maxM;
  GP_CHECK(launch_chain_wbar(h, chain_slots(p->d_misc, &p->off.bwd[S_CHAIN]), nK, maxM));
  if (!p->whiten) {      // Wbar += tril(g' q_mu^T + G' Lq^T)
    GP_CHECK(launch_rank1_tril_batched(h, slot_probs(p, S_WB_R1), nK, maxM));
    GemmFlags f; f.triA = TRI_LOWER; f.transB = 1; f.triB = TRI_UPPER; f.triC = TRI_LOWER; f.beta = 1.0;
    GP_CHECK(launch_gemm_batched(h, slot_probs(p, S_WB_L), nK, maxM, maxM, f));
  }
  return GP_OK;
}

// The Kuu side: Lbar = -tril(W^T Wbar W^T); P = Phi(L^T Lbar); S = W^T P W, and the contraction of Kuu_bar with
// dK(z, z)/d(theta, z), partial sums only: one launch per kernel family (24 launches of a few workgroups each otherwise:
// 2.6 ms at the end of the helper stream's chain), per GP where a family is mixed
static gp_status bwd_kuu_side(const BwdCall& c) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  const int nK = p->nK, maxM = p->maxM;
  GP_CHECK(launch_chain_adjoint(h, chain_slots(p->d_misc, &p->off.bwd[S_CHAIN]), nK, maxM));
  for (auto& fam : p->hy_fams)
    if (fam.batched)
      GP_CHECK(launch_hyper_contract_items(h, fam.type, fam.m, (const HyperItem*)(p->d_misc + p->off.hy_items) + p->G + fam.first,
                                           fam.count, fam.M, fam.M, 0, &fam.np_uu));
  for (int g : p->kgps) {
    PdgpGP& q = p->gps[g];
    if (p->hy_fams[q.fam].batched) continue;
    const CondTask& t = p->cb.tasks[g];
    const BwdBufs& bb = p->bw[g];
    const double* z = c.params + q.off_z;
    const int cb_uf = (c.n + HY_THREADS - 1) / HY_THREADS;
    double* gz_uu = q.need_z ? bb.gz_part + (size_t)cb_uf * q.M : nullptr;
    GP_CHECK(launch_hyper_contract(h, t.kern, z, q.M, z, q.M, bb.E, q.M, nullptr, nullptr, 1, t.feat, bb.hyp_part_uu, &q.np_uu, gz_uu));
  }
  return GP_OK;
}

// Kuf_bar (dense part) = R (A diag(2 gv)) of `count` slots of the compacted batch from slot0 on.  `fused`: they are that
// family's, and its Kuf-side contraction is the product's epilogue, nothing stored (one precision per family).
static gp_status bwd_kuf_product(const BwdCall& c, int slot0, int count, const HyFamily* fused = nullptr) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  const int maxM = p->maxM, k64 = p->routes.k64;
  GemmFlags f;
  f.big_tiles = 1; f.scale_mode = 1; f.alpha = 2.0; f.timer = GP_TIMER_KUF_BAR; f.role = 3;
  f.uniform_aligned = p->routes.kuf_uniform;
  f.a32_ok = 1;          // (float32 GPs: b.R32 is in every problem's xb)
  if (fused) {
    f.role = 5; f.epilogue = 0; f.aux_x = c.x; f.aux_ktype = fused->type;
    if (fused->f32) return launch_gemm_f32_role(h, slot_probs(p, S_G) + slot0, count, maxM, c.n, f);
    return launch_gemm_batched(h, slot_probs(p, S_G) + slot0, count, maxM, c.n, f);
  }
  const int c64 = (slot0 < k64) ? ((slot0 + count <= k64) ? count : k64 - slot0) : 0;
  if (c64 > 0) GP_CHECK(launch_gemm_batched(h, slot_probs(p, S_G) + slot0, c64, maxM, c.n, f));
  if (c64 < count) GP_CHECK(launch_gemm_f32_role(h, slot_probs(p, S_G) + slot0 + c64, count - c64, maxM, c.n, f));
  return GP_OK;
}

// One family's Kuf_bar step, by its route.  scan_to_side: the scan's three launches go to the side stream if it is to be had.
static gp_status bwd_kuf_bar_step(const BwdCall& c, const HyFamily& fam, bool scan_to_side) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  switch (fam.route) {
    case KUF_QFORM: return GP_OK;      // Kuf_bar = G diag(2 gv) + beta gm^T needs no product: the contraction scales G's columns
    case KUF_SCAN: {
      auto scan = [&]() { return launch_kuf_scan(h, fam.type, (const KufScanItem*)(p->d_misc + p->off.ks_items) + fam.first, fam.count, fam.M, c.x, c.n, fam.scan_far ? 1 : 0); };
      bool side;
      GP_CHECK(gp_on_side(h, scan_to_side, &side, scan));
      return side ? GP_OK : scan();
    }
    case KUF_FUSED: return bwd_kuf_product(c, fam.slot0, fam.count, &fam);
    case KUF_PRODUCT: break;
  }
  return bwd_kuf_product(c, fam.slot0, fam.count);
}

// One family's Kuf-side contraction of Kuf_bar with dK/dtheta over all frames: one launch over its item array (built at
// bind), or GP by GP where the family is mixed (inducing-input gradients, several sizes)
static gp_status bwd_contract(const BwdCall& c, HyFamily& fam) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  if (fam.batched)
    return launch_hyper_contract_items(h, fam.type, fam.m, (const HyperItem*)(p->d_misc + p->off.hy_items) + fam.first, fam.count,
                                       fam.M, c.n, 0, &fam.np_uf, fam.mfma, c.x, fam.f32, 1, fam.route == KUF_QFORM ? 1 : 0);
  for (int g : fam.gps) {
    PdgpGP& q = p->gps[g];
    const CondTask& t = p->cb.tasks[g];
    const BwdBufs& bb = p->bw[g];
    const int64_t ldN = gp_strip_ld(c.n, q.f32 != 0);
    GP_CHECK(launch_hyper_contract(h, t.kern, c.params + q.off_z, q.M, c.x, c.n, bb.G, ldN, bb.alpha, p->gFmu + (size_t)g * c.n, 0, t.feat,
                                   bb.hyp_part, &q.np_uf, q.need_z ? bb.gz_part : nullptr, t.Kuf, ldN, q.f32));
  }
  return GP_OK;
}

// All partial sums (Kuf side, Kuu side) are in: ONE finish launch adds them into the gradient vector (48 tiny launches at
// the end of every step otherwise).  The item array is re-uploaded only when it changes.
static gp_status bwd_finish(const BwdCall& c) {
  gp_pdgp_plan p = c.p; gp_handle h = p->h;
  std::vector<HyperFinishItem> items;
  int maxblocks = 0;
  for (int g : p->kgps) {
    const PdgpGP& q = p->gps[g];
    const HyFamily& fam = p->hy_fams[q.fam];
    const CondTask& t = p->cb.tasks[g];
    const BwdBufs& bb = p->bw[g];
    const int cb_uf = (c.n + HY_THREADS - 1) / HY_THREADS, cb_uu = (q.M + HY_THREADS - 1) / HY_THREADS;
    HyperFinishItem it;
    memset(&it, 0, sizeof(it));
    it.k = t.kern; it.p_uf = bb.hyp_part; it.p_uu = bb.hyp_part_uu;
    it.np_uf = fam.batched ? fam.np_uf : q.np_uf; it.np_uu = fam.batched ? fam.np_uu : q.np_uu;
    it.gv_sum = bb.gvsum; it.g_theta = c.grad + q.off_theta; it.n1 = q.M;
    if (q.need_z) {
      it.gz_uf = bb.gz_part; it.cb_uf = cb_uf; it.gz_uu = bb.gz_part + (size_t)cb_uf * q.M; it.cb_uu = cb_uu;
      it.g_z = c.grad + q.off_z;
    }
    const int blocks = 2 + 2 * t.kern.m + (q.need_z ? (q.M + 255) / 256 : 0);
    if (blocks > maxblocks) maxblocks = blocks;
    items.push_back(it);
  }
  const size_t bytes = items.size() * sizeof(HyperFinishItem);
  char* d_items = p->d_misc + p->off.fin_items;
  if (p->h_fin_items.size() != bytes || memcmp(p->h_fin_items.data(), items.data(), bytes) != 0) {
    p->h_fin_items.assign((const char*)items.data(), (const char*)items.data() + bytes);
    GP_HIP_CHECK(h, hipMemcpyAsync(d_items, p->h_fin_items.data(), bytes, hipMemcpyHostToDevice, h->stream));
  }
  return launch_hyper_finish_items(h, (const HyperFinishItem*)d_items, (int)items.size(), maxblocks);
}

// The helper stream's chain: [the H chain when forked early,] the Kuu side [, the late sums: at the END of the chain — ahead
// of the split-K product they delayed it]
static gp_status bwd_helper_chain(const BwdCall& c, bool early_fork) {
  if (early_fork) { GP_CHECK(bwd_h_chain(c)); GP_CHECK(bwd_wbar_chain(c)); }
  GP_CHECK(bwd_kuu_side(c));
  return early_fork ? bwd_late_sums(c) : GP_OK;
}

// With exactly two families — the transcription model: stationary activations, spectral-mixture components — in
// contiguous runs of the compacted batch, Kuf_bar is issued family by family and the first family's contraction runs on the
// side stream UNDERNEATH the second family's product instead of after it.  Which goes first (switches.h kufbar_split;
// -1 = by precision): with float64 strips the stationary family — its contraction (an HBM read, next to no arithmetic)
// goes underneath the spectral-mixture product, whose float64 MFMA holds the vector ALU, and the long contraction has the
// device to itself afterwards; with float32 strips the spectral-mixture family — its vector-ALU contraction then runs
// beside the other family's float32 matrix product, which leaves the vector ALU free (cfg3 3.90 -> 3.80 ms, headline
// 19.47 / 19.56 the other way round).  False: no such pair, or the switch says no.
static bool bwd_two_family_order(gp_pdgp_plan p, HyFamily** first, HyFamily** second) {
  if (p->hy_fams.size() != 2 || p->hy_fams[0].mfma == p->hy_fams[1].mfma) return false;
  HyFamily* sm = &p->hy_fams[p->hy_fams[0].mfma ? 0 : 1];
  HyFamily* other = &p->hy_fams[p->hy_fams[0].mfma ? 1 : 0];
  if (sm->slot0 < 0 || other->slot0 < 0) return false;
  int mode = gp_switches().kufbar_split;
  if (mode < 0) mode = sm->f32 ? 1 : 2;
  if (mode < 1) return false;
  *first = (mode == 2) ? other : sm;
  *second = (mode == 2) ? sm : other;
  return true;
}

// The schedule: which step goes to the helper stream (gp_aux_fork .. gp_aux_end), which to the side stream (gp_on_side), and in
// which order.  The routes were chosen at bind; overlap, scan_side and kufbar_split move launches between streams and
// reorder independent ones, never add or drop one that changes a bit.
gp_status pdgp_backward(gp_pdgp_plan p, const double* params, const double* x, int n, double* grad) {
  gp_handle h = p->h;
  BwdCall c{p, params, x, n, grad, false};
  const bool white = p->whiten != 0;
  if (!white) GP_CHECK(bwd_unwhitened_head(c));
  // Everything that hangs off H = A diag(2 gv) A^T — grad q_sqrt, Wbar, the whole Kuu side — is independent of the
  // Kuf_bar product, which needs only R = W^T (Lq Lq^T - I) and alpha = W^T q_mu.  With early_fork the H chain
  // (the split-K product included) goes to the helper stream and the main stream starts Kuf_bar right away; the late sums
  // go to the end of the helper stream's chain when there is one, and run up front otherwise.
  const bool early_fork = white && p->nK > 0 && n >= 4096 && p->overlap >= 2;
  if (!early_fork) { GP_CHECK(bwd_late_sums(c)); GP_CHECK(bwd_h_chain(c)); }
  if (p->nK == 0) return white ? GP_OK : bwd_unwhitened_tail(c);

  const bool pre = p->era_ready;   // E, R, alpha were computed on the helper stream during the forward pass
  p->era_ready = false;
  if (pre) GP_HIP_CHECK(h, hipStreamWaitEvent(h->stream, h->ev_era, 0));
  else GP_CHECK(pdgp_era(p, ERA_E));
  if (!early_fork) GP_CHECK(bwd_wbar_chain(c));
  if (!pre) GP_CHECK(pdgp_era(p, ERA_R));
  // From here two independent chains remain: the Kuf side (the big Kuf_bar product and its contraction with dK/dtheta over
  // all frames) and the Kuu side (the Cholesky adjoint, six M x M products, and its contraction over M x M).  The Kuu side
  // is ~1.4 ms of small launches: it runs on the helper stream underneath Kuf_bar.
  // With a scan family (switches.h scan_side; measurements: DESIGN.md 3.02) the scan's launches go to the side stream, beside
  // the other families' Kuf_bar product.  The side stream serves ONE fork per backward pass — gp_side_begin refuses until
  // gp_side_join — so only the first taker gets it: a further scan family, or a contraction that asks after it, stays in line.
  const bool scan_side = p->routes.any_scan && gp_switches().scan_side != 0 && n >= 4096 && p->overlap >= 2;
  const bool forked = n >= 4096 && p->overlap >= 1 && gp_aux_fork(h);
  HyFamily *first = nullptr, *second = nullptr;
  const bool two = forked && p->overlap >= 2 && bwd_two_family_order(p, &first, &second);
  // When the H chain goes to the helper stream, the far-field Qbar runs on the MAIN stream, beside the other
  // GPs' split-K product instead of in front of it, and the helper stream picks it up by an event before S_QT; a first
  // family that contracts by the scan is issued ahead of it, so that the side stream starts at once.  qform_qbar = 2 keeps
  // the launches on the helper stream.  The same launches either way, the same bits.
  bool first_issued = false;
  if (forked && early_fork && p->routes.q_bar && gp_switches().qform_qbar != 2 &&
      (h->ev_q || hipEventCreateWithFlags(&h->ev_q, hipEventDisableTiming) == hipSuccess)) {
    hipStream_t helper = h->stream;       // (not a GpStreamScope: the main stream may be the null stream, which it reads as "stay")
    h->stream = h->main_stream_saved;
    gp_status st = GP_OK;
    if (two && first->route == KUF_SCAN) { st = bwd_kuf_bar_step(c, *first, scan_side); first_issued = true; }
    if (st == GP_OK) st = bwd_qbar(c);
    h->stream = helper;
    if (st != GP_OK || hipEventRecord(h->ev_q, h->main_stream_saved) != hipSuccess) {
      (void)gp_aux_end(h);
      return st != GP_OK ? st : gp_fail(h, GP_ERR_HIP, "event hand-over to the helper stream failed");
    }
    c.qbar_ahead = true;
  }
  if (forked) {
    const gp_status st = bwd_helper_chain(c, early_fork);
    const gp_status se = gp_aux_end(h);
    GP_CHECK(st); GP_CHECK(se);
  } else if (early_fork) {
    GP_CHECK(bwd_late_sums(c));
  }
  if (two) {
    const bool pending = !kuf_sums_with_step(*first);     // first's contraction is still to run once its step is through
    bool side = false;
    if (!first_issued) GP_CHECK(bwd_kuf_bar_step(c, *first, scan_side));
    if (pending) GP_CHECK(gp_on_side(h, true, &side, [&]() { return bwd_contract(c, *first); }));
    GP_CHECK(bwd_kuf_bar_step(c, *second, scan_side));
    if (pending && !side) GP_CHECK(bwd_contract(c, *first));
    if (!kuf_sums_with_step(*second)) GP_CHECK(bwd_contract(c, *second));
  } else {
    // one product over the whole batch, or family by family when some family has a route of its own; then the families'
    // contractions side by side: the matrix-core ones on this stream, the others (short, HBM-bound) on the side stream
    if (p->routes.any_routed) { for (const auto& fam : p->hy_fams) GP_CHECK(bwd_kuf_bar_step(c, fam, scan_side)); }
    else GP_CHECK(bwd_kuf_product(c, 0, p->nK));
    if (!forked) {       // (no helper stream to be had)
      if (early_fork) { GP_CHECK(bwd_h_chain(c)); GP_CHECK(bwd_wbar_chain(c)); }
      GP_CHECK(bwd_kuu_side(c));
    }
    bool side = false;
    GP_CHECK(gp_on_side(h, p->hy_fams.size() > 1 && forked && p->overlap >= 2, &side, [&]() -> gp_status {
      for (auto& fam : p->hy_fams) if (!fam.mfma && !kuf_sums_with_step(fam)) GP_CHECK(bwd_contract(c, fam));
      return GP_OK;
    }));
    for (auto& fam : p->hy_fams) if ((!side || fam.mfma) && !kuf_sums_with_step(fam)) GP_CHECK(bwd_contract(c, fam));
  }
  if (!white) GP_CHECK(bwd_unwhitened_tail(c));
  GP_CHECK(gp_side_join(h));
  GP_CHECK(gp_aux_join(h));
  return bwd_finish(c);
}
