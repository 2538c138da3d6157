// predict_sparse.hip — the sparse per-source posterior of an SGPRSS window in ONE fused launch (gfx950).
//
// Beside gpitch/sgpr_ss.py:43-53 (the state L, LB, c of the collapsed bound) and :73-114 (the exact per-source posterior
// this is the cheap companion of): GPflow 0.5 SGPR.build_predict with the one kernel K_p in place of the sum,
//   tmp1_p = W K_p(Z, Xnew),  tmp2_p = WB tmp1_p          (W = L^-1, WB = LB^-1: what sgpr_common leaves in the plan)
//   smean_p = tmp2_p^T c,     svar_p = Kdiag_p + sum_m tmp2_p^2 - sum_m tmp1_p^2
// A workgroup takes one (window, source, tile of T new frames):
//   1. K_p(Z, x*) of its T frames is built straight into LDS (frame-major, M values per frame) with the entry arithmetic
//      of cov.hip (cov_entry.h): an entry equals what launch_kernel_build writes.  The Z feature table of a Mercer kernel is
//      the plan's (current after the forward pass); the T frames' features are computed here, once per workgroup.  The
//      build itself is sps_tile.h's, shared with sample.hip.
//   2. tmp1 = W tile on v_mfma_f64_16x16x4_f64.  A wavefront owns 16 frames — both products act on a frame's column alone,
//      so nothing crosses wavefronts after the build.  Row blocks run from the last to the first and overwrite the tile
//      in place: block rb reads blocks kb <= rb only (the zero blocks above W's diagonal are skipped).
//   3. tmp2 = WB tmp1 the same way; it is never stored.
//   4. sum tmp1^2, sum tmp2^2 and tmp2^T c per frame: a lane adds its own rows in loop order, then the four lanes of a frame
//      are added in a fixed order.  A frame's result depends on nothing but its own column: bit-identical between calls
//      and whatever other frames share the launch.
//   5. two doubles per (source, frame) leave.
// HBM traffic: W, WB, c, Z (+ its features) and x* in — the M x M factors stay in L2 across tiles — 2 P n doubles out.
// float64 throughout, whatever the plan's strip precision.  M <= SPS_MAX_M; tails in M (zero rows, never read from Z, W
// or WB) and in n (frames past the end repeat the last one and are not written) are handled here.
#include "common.h"
#include "cov_entry.h"
#include "sps_tile.h"

typedef double sps_d4 __attribute__((ext_vector_type(4)));

template <int MPAD>
__global__ void __launch_bounds__(256) sgpr_source_sparse_kernel(const SrcSparseItem* __restrict__ items, int nwin, int n,
                                                                 int T, int S) {
  extern __shared__ double sps_lds[];
  const SpsLds lds = sps_lds_carve<MPAD>(sps_lds);
  double* buf = lds.buf;
  const SrcSparseItem it = items[(size_t)blockIdx.y * nwin + blockIdx.z];
  const int tid = threadIdx.x;
  const int kz = it.kz, Mp = (kz + 15) & ~15, ldw = it.ldw;
  const int type = it.k.type, m = it.k.m;
  const double* __restrict__ th = it.k.theta;
  const int j0 = blockIdx.x * T;

  // ---- 1. the tile (sps_tile.h) -------------------------------------------------------------------------------------
  sps_build_tile<MPAD>(lds, it.k, it.z, it.fz, kz, it.xnew, n, j0, T, S);

  // ---- 2.-4. the two triangular products and the per-frame sums, one wavefront per 16 frames ---------------------------
  const int lane = tid & 63, wave = tid >> 6, lc = lane & 15, kq = lane >> 4;
  double* col = buf + (size_t)(16 * wave + lc) * S;       // this lane's frame: B[k][j = lc] = col[k]
  const int nrb = Mp >> 4;
  double p1 = 0.0, p2 = 0.0, pd = 0.0;
  {
    const double* __restrict__ Wm = it.W;
    for (int rb = nrb - 1; rb >= 0; rb--) {
      const int row = 16 * rb + lc;                       // A[i = lc][k = kq]
      const bool row_on = row < kz;
      const double* wr = Wm + (size_t)(row_on ? row : 0) * ldw;
      sps_d4 acc = sps_d4{0.0, 0.0, 0.0, 0.0};
      for (int kb = 0; kb <= rb; kb++) {
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int k = 16 * kb + 4 * s + kq;
          const double af = (row_on && k < kz) ? wr[k] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af, col[k], acc, 0, 0, 0);
        }
      }
      // element r: row 16 rb + kq + 4 r of this lane's frame; later (smaller) row blocks read blocks kb < rb only
#pragma unroll
      for (int r = 0; r < 4; r++) { p1 = fma(acc[r], acc[r], p1); col[16 * rb + kq + 4 * r] = acc[r]; }
    }
  }
  __syncthreads();                                        // tmp1 is whole (a lane's column was written by its wavefront's lanes)
  {
    const double* __restrict__ Wm = it.WB;
    for (int rb = nrb - 1; rb >= 0; rb--) {
      const int row = 16 * rb + lc;
      const bool row_on = row < kz;
      const double* wr = Wm + (size_t)(row_on ? row : 0) * ldw;
      sps_d4 acc = sps_d4{0.0, 0.0, 0.0, 0.0};
      for (int kb = 0; kb <= rb; kb++) {
#pragma unroll
        for (int s = 0; s < 4; s++) {
          const int k = 16 * kb + 4 * s + kq;
          const double af = (row_on && k < kz) ? wr[k] : 0.0;
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(af, col[k], acc, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int orow = 16 * rb + kq + 4 * r;
        const double cv = (orow < kz) ? it.c[orow] : 0.0;
        p2 = fma(acc[r], acc[r], p2);
        pd = fma(acc[r], cv, pd);
      }
    }
  }
  // the four lanes (kq = 0..3) of a frame, in a fixed order
  p1 += __shfl_xor(p1, 16, 64); p1 += __shfl_xor(p1, 32, 64);
  p2 += __shfl_xor(p2, 16, 64); p2 += __shfl_xor(p2, 32, 64);
  pd += __shfl_xor(pd, 16, 64); pd += __shfl_xor(pd, 32, 64);
  // ---- 5. ------------------------------------------------------------------------------------------------------------
  const int j = j0 + 16 * wave + lc;
  if (kq == 0 && j < n) {
    const double kd = cov_kdiag(type, m, th);             // the source's OWN Kdiag (sgpr_ss.py:101 uses the sum kernel's)
    it.mean[j] = pd;
    it.var[j] = (kd + p2) - p1;
  }
}

// d_items: device array [P][nwin] (kernel-major); every item's kz <= M (the plan's inducing-point count, <= SPS_MAX_M);
// max_mpad: the largest sm_mpad() among the Mercer kernels of the launch (0: none)
gp_status launch_sgpr_source_sparse(gp_handle h, const SrcSparseItem* d_items, int P, int nwin, int M, int n, int max_mpad) {
  if (M < 1 || M > SPS_MAX_M) return gp_fail(h, GP_ERR_UNSUPPORTED, "sparse source posterior: M must be in [1, 1024]");
  if (P < 1 || P > 65535 || nwin < 1 || nwin > 65535 || n < 1) return gp_fail(h, GP_ERR_BAD_ARG, "sparse source posterior: bad launch shape");
  GpTimerScope ts(h, GP_TIMER_COND_A);
  return sps_dispatch_mpad(h, max_mpad, "sparse source posterior: num_partials must be in [1, 32]", [&](auto mpad) -> gp_status {
    const int T = sps_tile_frames(M), S = sps_stride(M);
    const size_t lds = sps_lds_bytes(M, decltype(mpad)::value);
    GP_HIP_CHECK(h, hipFuncSetAttribute((const void*)sgpr_source_sparse_kernel<decltype(mpad)::value>,
                                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((sgpr_source_sparse_kernel<decltype(mpad)::value>), dim3((n + T - 1) / T, P, nwin), dim3(4 * T), lds, h->stream,
                       d_items, nwin, n, T, S);
    GP_HIP_CHECK(h, hipGetLastError());
    return GP_OK;
  });
}
