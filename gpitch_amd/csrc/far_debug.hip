// far_debug.hip — gp_debug_far_tables: ONE launch of a far field's table kernel (afar.hip / qfar.hip) on the caller's buffers,
// for the operator tests (tests/test_gpu_far_tables.py).  No arithmetic of its own and no kernel: the plain arguments are
// copied into an AfarItem / a QfarItem as the plans fill them (pdgp_upload_afar, pdgp_upload_qform), uploaded into the caller's
// device workspace on the handle's stream, and handed to the launcher that the switch far_tables chooses between.  The cols
// kernels are not launched: the ranges and reference points are the caller's.  Nothing is synchronised.
#include "engine.h"
#include <string.h>

static_assert(sizeof(AfarItem) <= 256 && sizeof(QfarItem) <= 256, "gp_debug_far_tables: include/gpitch_abi.h promises 256 bytes of workspace");

static bool fd_al16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

extern "C" gp_status gp_debug_far_tables(gp_handle h, int32_t which, int32_t form, const double* X, const double* X2, const double* z,
                                         const double* theta, const double* fz, int32_t* rng, double* ref, double* T, int32_t M,
                                         int32_t N, int32_t nf, void* workspace, size_t workspace_bytes) {
  if (!h) return GP_ERR_BAD_ARG;
  if (which < 0 || which > 1 || form < 0 || form > 1 || !X || !z || !theta || !rng || !ref || !T || M <= 0 || M > 1024 || N <= 0 ||
      !fd_al16(X))
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_far_tables: bad argument");
  if (!workspace || !fd_al16(workspace) || workspace_bytes < 256)
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_debug_far_tables: workspace too small or not 16-byte aligned");
  if (which == 0) {
    if (!X2 || !fd_al16(X2) || fz || nf != 0 || (M % 16) != 0 || (N % AFAR_GROUP) != 0)
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_far_tables: the activations' tables take W and C, M a multiple of 16, whole 256-frame groups");
    AfarItem it;
    memset(&it, 0, sizeof(it));
    it.z = z; it.theta = theta; it.W = X; it.C = X2; it.rng = rng; it.ref = ref; it.T = T; it.M = M;
    GP_HIP_CHECK(h, hipMemcpyAsync(workspace, &it, sizeof(it), hipMemcpyHostToDevice, h->stream));
    launch_afar_t(h, (const AfarItem*)workspace, 1, M, N, form != 0);
  } else {
    if (X2 || !fz || !fd_al16(fz) || nf <= 0 || nf > 64 || (nf % 8) != 0 || (M % 64) != 0 || (N % QFAR_GROUP) != 0)
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_far_tables: the Q route's tables take Q and the z features, M a multiple of 64, nf of 8, whole 256-frame groups");
    QfarItem it;
    memset(&it, 0, sizeof(it));
    it.z = z; it.theta = theta; it.fz = fz; it.Q = X; it.rng = rng; it.ref = ref; it.T = T; it.M = M;
    GP_HIP_CHECK(h, hipMemcpyAsync(workspace, &it, sizeof(it), hipMemcpyHostToDevice, h->stream));
    launch_qfar_t(h, (const QfarItem*)workspace, 1, M, nf, N, form != 0);
  }
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}
