// hyper_debug.hip — gp_debug_hyper_contract: ONE launch of a kernel-gradient contraction host entry (bwd.hip) on the caller's
// buffers, for the operator tests (tests/test_gpu_hyper.py).  No arithmetic of its own and no kernel: the plain records are
// copied into HyperItems / HyperFinishItems, uploaded into the caller's device workspace on the handle's stream, the
// spectral-mixture feature tables are built as the plans build them (launch_sm_features, the layout hyper_item_fill of bwd.hip
// assumes) and the launcher that `entry` selects is called once.  Nothing is synchronised.
// Also the two host-only queries of the sizing rules: gp_debug_hyper_records, gp_debug_hyper_lean_takes.
#include "common.h"
#include "engine.h"
#include <string.h>
#include <vector>

// the header and the tests size the workspace at 160 bytes per record
static_assert(sizeof(HyperItem) <= 160 && sizeof(HyperFinishItem) <= 160,
              "gp_debug_hyper_contract: include/gpitch_abi.h promises 160 bytes of workspace per record");

extern "C" int64_t gp_debug_hyper_records(int32_t N, int32_t M) {
  if (N <= 0 || M <= 0) return -1;
  return (int64_t)hyper_kuf_records(N, M);
}

extern "C" int32_t gp_debug_hyper_lean_takes(int32_t type, int32_t m, int32_t n1, int32_t n2, int32_t count) {
  if (m <= 0 || n1 <= 0 || n2 <= 0) return 0;
  return hyper_lean_takes(type, m, n1, n2, count) ? 1 : 0;
}

static bool hyd_kern_ok(const gp_kernel_desc& k) {
  if (k.type < 0 || k.type > GP_KERN_LAST || !k.theta) return false;
  if (gp_kern_has_partials(k.type)) return k.num_partials >= 1 && k.num_partials <= 32;
  return k.num_partials == 0;
}

// the record as hyper_item_fill (bwd.hip) lays it out: f2 behind f1 at gp_align_up(2 mpad n1, 32) doubles, or f1 itself when x2 is x1
static void hyd_item(HyperItem* it, const gp_debug_hyper_item& s, const double* feat) {
  memset((void*)it, 0, sizeof(HyperItem));
  const DevKern k = dev_kern(&s.kern);
  const int mp = gp_kern_is_mercer(k.type) ? sm_mpad(k.m) : 0;
  it->k = k; it->x1 = s.x1; it->x2 = s.x2; it->G = (const double*)s.G; it->alpha = s.alpha; it->gm = s.gm;
  it->f1 = feat;
  it->f2 = (s.x2 == s.x1 || !feat) ? feat : feat + gp_align_up((size_t)2 * mp * s.n1, 32);
  it->partials = s.partials; it->gz = s.gz; it->kvals = (const double*)s.kvals;
  it->ldg = s.ldg; it->ldk = s.ldk; it->n1 = s.n1; it->n2 = s.n2; it->symmetric = s.symmetric; it->g32 = s.g32;
  it->gscale = s.gscale;
}

extern "C" gp_status gp_debug_hyper_contract(gp_handle h, int32_t entry, const gp_debug_hyper_item* items,
                                             const gp_debug_hyper_finish* fins, int32_t count, const gp_debug_hyper_flags* fl,
                                             void* workspace, size_t workspace_bytes, int32_t* nparts, int32_t* taken) {
  if (!h) return GP_ERR_BAD_ARG;
  if (nparts) *nparts = 0;
  if (taken) *taken = 0;
  if (entry < 0 || entry > 4 || count <= 0 || count > 4096 || !fl) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: bad argument");
  if (!workspace || (((uintptr_t)workspace) & 15) != 0 || workspace_bytes < (size_t)count * 160)
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_debug_hyper_contract: workspace too small or not 16-byte aligned");

  // ---- the two finishes -------------------------------------------------------------------------------------------------
  if (entry >= 3) {
    if (!fins || (entry == 3 && count != 1)) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: finish records");
    std::vector<HyperFinishItem> hf((size_t)count);
    memset((void*)hf.data(), 0, hf.size() * sizeof(HyperFinishItem));
    int maxblocks = 0;
    for (int i = 0; i < count; i++) {
      const gp_debug_hyper_finish& s = fins[i];
      if (!hyd_kern_ok(s.kern) || !s.g_theta || s.np_uf < 0 || s.np_uu < 0 || s.cb_uf < 0 || s.cb_uu < 0 || s.n1 < 0 ||
          (s.np_uf > 0 && !s.p_uf) || (s.np_uu > 0 && !s.p_uu) || (s.cb_uf > 0 && !s.gz_uf) || (s.cb_uu > 0 && !s.gz_uu))
        return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: bad finish record");
      HyperFinishItem& d = hf[(size_t)i];
      d.k = dev_kern(&s.kern); d.p_uf = s.p_uf; d.p_uu = s.p_uu; d.gv_sum = s.gv_sum; d.g_theta = s.g_theta;
      d.gz_uf = s.gz_uf; d.gz_uu = s.gz_uu; d.g_z = s.g_z;
      d.np_uf = s.np_uf; d.np_uu = s.np_uu; d.cb_uf = s.cb_uf; d.cb_uu = s.cb_uu; d.n1 = s.n1;
      const int blocks = 2 + 2 * d.k.m + (d.g_z ? (s.n1 + 255) / 256 : 0);     // as the plans size the grid: by the largest record
      if (blocks > maxblocks) maxblocks = blocks;
    }
    if (entry == 3) {
      const gp_debug_hyper_finish& s = fins[0];
      if (s.np_uu != 0 || s.cb_uu != 0) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_hyper_contract: the single finish has no Kuu side");
      if (nparts) *nparts = s.np_uf;
      return launch_hyper_finish(h, dev_kern(&s.kern), s.p_uf, s.np_uf, s.gv_sum, s.g_theta, s.gz_uf, s.cb_uf, s.n1, s.g_z);
    }
    HyperFinishItem* d_fin = (HyperFinishItem*)workspace;
    GP_HIP_CHECK(h, hipMemcpyAsync(d_fin, hf.data(), hf.size() * sizeof(HyperFinishItem), hipMemcpyHostToDevice, h->stream));
    if (nparts) *nparts = maxblocks;
    return launch_hyper_finish_items(h, d_fin, count, maxblocks);
  }

  // ---- the contractions -------------------------------------------------------------------------------------------------
  if (!items) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: no records");
  const int n1 = items[0].n1, n2 = (entry == 1 && fl->x2_shared) ? fl->n2_shared : items[0].n2;
  if (n1 <= 0 || n2 <= 0) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: empty problem");
  std::vector<const double*> feat((size_t)count, nullptr);
  for (int i = 0; i < count; i++) {
    const gp_debug_hyper_item& s = items[i];
    const bool shared_x2 = (entry == 1 && !s.x2);
    if (!hyd_kern_ok(s.kern) || !s.x1 || !s.G || !s.partials || s.n1 != n1 || (!shared_x2 && s.n2 != n2) || s.ldg < n2 ||
        (shared_x2 && !fl->x2_shared) || (!s.x2 && entry != 1) || (s.kvals && s.ldk < n2) || (s.symmetric && (s.x2 != s.x1 || n1 != n2)) ||
        (s.alpha == nullptr) != (s.gm == nullptr) || s.feat_from >= i || s.feat_from < -1)
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: bad record");
    if (entry != 2 && (s.kern.type != items[0].kern.type || s.kern.num_partials != items[0].kern.num_partials))
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: one launch is one kernel family");
    if (gp_kern_is_mercer(s.kern.type)) {
      if (s.feat_from >= 0) {
        // a shared table is the table of the SAME kernel over the same inputs: the caller's promise
        feat[(size_t)i] = feat[(size_t)s.feat_from];
      } else {
        if (!s.feat || (((uintptr_t)s.feat) & 15) != 0) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: feature workspace");
        const double* x2 = shared_x2 ? fl->x2_shared : s.x2;
        GP_CHECK(launch_sm_features(h, dev_kern(&s.kern), s.x1, n1, x2, n2, s.feat));
        feat[(size_t)i] = s.feat;
      }
      if (!feat[(size_t)i]) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: feature table of a record without one");
    }
  }
  int np = 0;
  if (entry == 0) {
    if (count != 1) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: entry 0 takes one record");
    const gp_debug_hyper_item& s = items[0];
    if (s.gscale) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_hyper_contract: the single-record entry applies no column scale");
    GP_CHECK(launch_hyper_contract(h, dev_kern(&s.kern), s.x1, n1, s.x2, n2, (const double*)s.G, s.ldg, s.alpha, s.gm, s.symmetric,
                                   feat[0], s.partials, &np, s.gz, (const double*)s.kvals, s.ldk, s.g32));
    if (taken) *taken = 1;
  } else if (entry == 1) {
    const int type = items[0].kern.type, m = items[0].kern.num_partials;
    const bool rows = fl->use_mfma && gp_kern_is_mercer(type) && !fl->with_gz;
    for (int i = 0; i < count; i++) {
      const gp_debug_hyper_item& s = items[i];
      // what the item kernels read without asking (engine.h: "every item has kvals and no inducing-input gradient"; the
      // matrix-core forms read alpha and gm of every row and column; g32_items / gscale_items speak for ALL items)
      if (fl->with_gz && !s.gz) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: with_gz needs gz in every record");
      if (rows && (!s.kvals || !s.alpha || !s.gm || s.symmetric))
        return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: the matrix-core forms need kvals, alpha and gm in every record");
      if (rows && ((s.g32 != 0) != (fl->g32_items != 0))) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: g32_items and the records disagree");
      // lean_items is the caller's promise that hyper_sm_rows_lean_kernel's 16-byte loads are whole: the launcher sees only
      // the device array, so nothing checks it there (launch_hyper_contract checks the same for its one record)
      const uintptr_t amask = fl->g32_items ? 7 : 15;
      if (rows && fl->lean_items && hyper_lean_takes(type, m, n1, n2, count) &&
          ((s.ldg & 1) || (s.ldk & 1) || (((uintptr_t)s.G) & amask) || (((uintptr_t)s.kvals) & amask)))
        return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: lean_items promises 16-byte aligned strips with even strides");
      if ((s.gscale != nullptr) != (fl->gscale_items != 0)) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: gscale_items and the records disagree");
    }
    std::vector<HyperItem> hi((size_t)count);
    for (int i = 0; i < count; i++) hyd_item(&hi[(size_t)i], items[i], feat[(size_t)i]);
    HyperItem* d_items = (HyperItem*)workspace;
    GP_HIP_CHECK(h, hipMemcpyAsync(d_items, hi.data(), hi.size() * sizeof(HyperItem), hipMemcpyHostToDevice, h->stream));
    GP_CHECK(launch_hyper_contract_items(h, type, m, d_items, count, n1, n2, fl->with_gz, &np, fl->use_mfma, fl->x2_shared, fl->g32_items,
                                         fl->lean_items, fl->gscale_items));
    if (taken) *taken = 1;
  } else {
    // one G for the kernels of a sum: the shared operands are record 0's
    if (count > 8) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: at most 8 kernels in a sum");
    const gp_debug_hyper_item& s0 = items[0];
    DevKern kerns[8]; double* feats[8]; double* parts[8];
    for (int i = 0; i < count; i++) {
      const gp_debug_hyper_item& s = items[i];
      if (s.x1 != s0.x1 || s.x2 != s0.x2 || s.G != s0.G || s.ldg != s0.ldg || s.alpha != s0.alpha || s.gm != s0.gm || s.g32 != s0.g32 ||
          s.symmetric || s.gz || s.gscale)
        return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_hyper_contract: the kernels of a sum share x1, x2, G, alpha and gm");
      kerns[i] = dev_kern(&s.kern); feats[i] = const_cast<double*>(feat[(size_t)i]); parts[i] = s.partials;
    }
    gp_status st = GP_OK;
    const bool took = launch_hyper_contract_sum(h, kerns, feats, parts, count, s0.x1, n1, s0.x2, n2, (const double*)s0.G, s0.ldg, s0.alpha,
                                                s0.gm, s0.g32, &np, &st);
    if (taken) *taken = took ? 1 : 0;
    if (!took) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_hyper_contract: the sum kernel does not take this launch");
    GP_CHECK(st);
  }
  if (nparts) *nparts = np;
  return GP_OK;
}
