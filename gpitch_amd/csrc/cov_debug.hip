// cov_debug.hip — gp_debug_cov_build: ONE launch of a covariance-build host entry (cov.hip) on the caller's buffers, for the
// operator tests (tests/test_gpu_cov.py).  No arithmetic of its own and no kernel: the plain records are copied into CovItems /
// FeatItems exactly as the plans fill them (cov_item_fill; the feature records of cond_batch_upload in engine.hip), uploaded
// into the caller's device workspace on the handle's stream, and handed to the launcher that `entry` selects.  What ran is
// reported from cov_items_form, the same function the launcher decides by.  Nothing is synchronised.
#include "common.h"
#include <string.h>
#include <vector>

// the header and the tests size the workspace at 192 bytes per record: one CovItem, one FeatItem for its rows, one for its columns
static_assert(sizeof(CovItem) + 2 * sizeof(FeatItem) <= 192,
              "gp_debug_cov_build: include/gpitch_abi.h promises 192 bytes of workspace per record");
static_assert(sizeof(CovItem) % 16 == 0 && sizeof(FeatItem) % 8 == 0, "gp_debug_cov_build: the three record arrays follow each other");

static bool cvd_kern_ok(const gp_kernel_desc& k) {
  if (k.type < 0 || k.type > GP_KERN_LAST || !k.theta) return false;
  if (gp_kern_has_partials(k.type)) return k.num_partials >= 1 && k.num_partials <= 32;
  return k.num_partials == 0;
}

extern "C" gp_status gp_debug_cov_build(gp_handle h, int32_t entry, const gp_debug_cov_item* items, int32_t count,
                                        const double* x2_shared, int32_t n2_shared, int32_t engine_strips, void* workspace,
                                        size_t workspace_bytes, int32_t* form, int32_t* row_seg) {
  if (!h) return GP_ERR_BAD_ARG;
  if (form) *form = 0;
  if (row_seg) *row_seg = 0;
  if (entry < 0 || entry > 2 || !items || count <= 0 || count > 4096 || engine_strips < 0 || engine_strips > 2 ||
      (x2_shared && n2_shared <= 0))
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_cov_build: bad argument");
  for (int i = 0; i < count; i++) {
    const gp_debug_cov_item& s = items[i];
    const bool shared = s.n2 < 0;
    if (!cvd_kern_ok(s.kern) || !s.x1 || !s.out || s.n1 <= 0 || s.n2 == 0 || (shared && (entry != 1 || !x2_shared || s.x2)) ||
        s.ld < (shared ? n2_shared : (s.x2 ? s.n2 : s.n1)) || (!shared && !s.x2 && s.n2 != s.n1))
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_cov_build: bad record");
    if (gp_kern_is_mercer(s.kern.type) && (!s.feat || (((uintptr_t)s.feat) & 15) != 0))
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_cov_build: feature workspace");
  }

  // ---- one record by value ----------------------------------------------------------------------------------------------
  if (entry == 0) {
    if (count != 1) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_cov_build: entry 0 takes one record");
    const gp_debug_cov_item& s = items[0];
    return launch_kernel_build(h, dev_kern(&s.kern), s.x1, s.n1, s.x2, s.n2, (double*)s.out, s.ld, s.accumulate, s.diag_add, s.feat, 0,
                               s.f32out);
  }

  // ---- the kernels of a sum in one pass -----------------------------------------------------------------------------------
  if (entry == 2) {
    const gp_debug_cov_item& s0 = items[0];
    std::vector<DevKern> kerns((size_t)count);
    std::vector<double*> feats((size_t)count);
    for (int i = 0; i < count; i++) {
      const gp_debug_cov_item& s = items[i];
      if (s.x1 != s0.x1 || s.x2 != s0.x2 || s.n1 != s0.n1 || s.n2 != s0.n2 || s.out != s0.out || s.ld != s0.ld ||
          s.diag_add != s0.diag_add || s.f32out != s0.f32out)
        return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_cov_build: the kernels of a sum share x1, x2, out, ld, diag_add and f32out");
      kerns[(size_t)i] = dev_kern(&s.kern); feats[(size_t)i] = s.feat;
    }
    for (int i = 0; i < count; i++) GP_CHECK(launch_sm_features(h, kerns[(size_t)i], s0.x1, s0.n1, s0.x2, s0.n2, feats[(size_t)i]));
    gp_status st = GP_OK;
    const bool took = launch_kernel_build_sum(h, kerns.data(), feats.data(), count, s0.x1, s0.n1, s0.x2, s0.n2, (double*)s0.out, s0.ld,
                                              s0.diag_add, s0.f32out, &st);
    if (!took) {
      if (form) *form = -1;
      return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_cov_build: the sum kernel does not take this launch");
    }
    return st;
  }

  // ---- the grouped build of one kernel family -----------------------------------------------------------------------------
  const int type = items[0].kern.type, m = items[0].kern.num_partials;
  const bool mercer = gp_kern_is_mercer(type);
  const int mp = mercer ? sm_mpad(m) : 0;
  int max_n1 = 0, max_n2 = 0, max_nx = 0;
  for (int i = 0; i < count; i++) {
    const gp_debug_cov_item& s = items[i];
    if (s.kern.type != type || (mercer ? sm_mpad(s.kern.num_partials) != mp : s.kern.num_partials != m))
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_cov_build: one launch is one kernel family and one padded partial count");
    const int n2 = s.n2 < 0 ? n2_shared : (s.x2 ? s.n2 : s.n1);
    if (s.n1 > max_n1) max_n1 = s.n1;
    if (n2 > max_n2) max_n2 = n2;
    if ((s.n2 < 0 || (s.x2 && s.x2 != s.x1)) && n2 > max_nx) max_nx = n2;
    // engine_strips is a promise the launcher cannot check on the device array.  The lean form, which only that promise
    // admits, stores 16 bytes unasked and loads whole 128-column blocks of the frames unguarded while the launcher looks at
    // n2_shared alone: a record with frames of its own (n2 >= 0) is refused here, and no caller in the library passes one
    if (engine_strips && (s.n2 >= 0 || (s.ld & 1) || (((uintptr_t)s.out) & 15) || (s.f32out != 0) != (engine_strips == 2) ||
                          s.accumulate || s.diag_add != 0.0))
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_cov_build: engine_strips promises strips of the shared frames, 16-byte aligned, even strides");
  }
  const CovItemsForm cf = cov_items_form(type, m, count, max_n1, max_n2, x2_shared != nullptr, n2_shared, engine_strips);
  // the matrix-core forms neither accumulate nor add a diagonal
  if (cf.form != 0)
    for (int i = 0; i < count; i++)
      if (items[i].accumulate || items[i].diag_add != 0.0)
        return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_cov_build: the matrix-core forms write plain Kuf strips");
  if (!workspace || (((uintptr_t)workspace) & 15) != 0 || workspace_bytes < (size_t)count * 192)
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_debug_cov_build: workspace too small or not 16-byte aligned");

  const size_t cov_bytes = (size_t)count * sizeof(CovItem), feat_bytes = (size_t)count * sizeof(FeatItem);
  std::vector<char> hd(cov_bytes + 2 * feat_bytes, 0);
  CovItem* ci = (CovItem*)hd.data();
  FeatItem* fz = (FeatItem*)(hd.data() + cov_bytes);
  FeatItem* fx = (FeatItem*)(hd.data() + cov_bytes + feat_bytes);
  for (int i = 0; i < count; i++) {
    const gp_debug_cov_item& s = items[i];
    const DevKern k = dev_kern(&s.kern);
    cov_item_fill(&ci[i], k, s.x1, s.n1, s.x2, s.n2, (double*)s.out, s.ld, s.accumulate, s.diag_add, s.feat, s.f32out);
    if (!mercer) continue;
    double* fcol = s.feat + gp_align_up((size_t)2 * mp * s.n1, 32);
    fz[i] = FeatItem{k, s.x1, s.feat, s.n1, 0};
    if (s.n2 < 0) fx[i] = FeatItem{k, nullptr, fcol, -1, 0};                 // the launch's shared frames
    else if (s.x2 && s.x2 != s.x1) fx[i] = FeatItem{k, s.x2, fcol, s.n2, 0};
    else fx[i] = FeatItem{k, s.x1, s.feat, 0, 0};                            // K(x1): the row table serves both sides
  }
  char* dd = (char*)workspace;
  GP_HIP_CHECK(h, hipMemcpyAsync(dd, hd.data(), hd.size(), hipMemcpyHostToDevice, h->stream));
  if (mercer) {
    GP_CHECK(launch_sm_features_items(h, (const FeatItem*)(dd + cov_bytes), count, max_n1, mp, nullptr, 0));
    if (max_nx > 0)
      GP_CHECK(launch_sm_features_items(h, (const FeatItem*)(dd + cov_bytes + feat_bytes), count, max_nx, mp, x2_shared, x2_shared ? n2_shared : 0));
  }
  if (form) *form = cf.form;
  if (row_seg) *row_seg = cf.form ? cf.row_seg : 0;
  return launch_kernel_build_items(h, type, m, (const CovItem*)dd, count, max_n1, max_n2, x2_shared, n2_shared, engine_strips);
}
