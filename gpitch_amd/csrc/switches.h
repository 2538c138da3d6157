// switches.h — every run-time switch of libgpitch_hip.so, in one place.
//
// All of them select between forms that give the SAME results (bit-identical where DESIGN.md says so, rounding-level
// otherwise); they exist for same-box A/B measurements and are read ONCE per process from ONE environment variable:
//
//     GPITCH_AMD_SWITCHES="name=value,name=value,..."        e.g.  GPITCH_AMD_SWITCHES=strip_wave=0,kufbar_split=1
//
//   name            default  meaning
//   strip_wave        1      gemm_wave.hip: float64 strip products with a 64 x 64 tile per wavefront, no LDS (0: gemm_strip.hip)
//   strip_wave_roles  46     bit (1 << role) — which roles (1 A = W Kuf, 2 Lq^T A, 3 Kuf_bar, 5 Kuf_bar + contraction) take it
//   strip_wave_f32    46     gemm_wave_f32.hip: the same form for float32 strips, a bitmask 1 << role (0: gemm_strip_f32.hip / gemm_f32.hip)
//   strip_lean        1      gemm_strip.hip / gemm_strip_f32.hip: the lean 128 x 128 LDS tiles (0: gemm.hip / gemm_f32.hip's)
//   hyper_fuse        1      a stationary family's Kuf-side contraction as the epilogue of its Kuf_bar product
//   kufbar_split     -1      Kuf_bar per kernel family: 2 stationary family first, 1 spectral-mixture family first, 0 one launch, -1: 1 with float32 strips, else 2
//   cond_a_early      1      first row-block of A = W Kuf underneath the block-row inverse of the Kuu factorisation
//   blocked_256       1      M in (128, 256] with long batches: resident factor + blocked inverse (0: one fused kernel)
//   cov_sum           1      SGPRSS: the kernel sum K = sum_p K_p built in one pass (0: one accumulate launch per kernel)
//   hyper_sum         1      SGPRSS: the P kernels' Kuf-side contractions in one pass over Kuf_bar
//   kuf_scan          1      kuf_scan.hip: a Matern-3/2 / Matern-5/2 family with fixed inducing inputs and ascending frames contracts Kuf_bar by moment sums, no Kuf_bar product (0: the product)
//   chol_cluster      1      chol_cluster.hip: M x M factor + inverse (128 <= M <= 512, M % 32 == 0) by a cluster of 17 / 5 / 2 workgroups per matrix, up to 128 per launch (0: chol.hip)
//   aux_priority      1      the handle's helper stream is created with the highest stream priority (0: default priority)
//   gemm_tile32       320    generic M x M products with fewer 64 x 64 tiles than this in the launch take 32 x 32 tiles (0: never)
//   nt_cover          0      split-K product: workgroups the K-slices are chosen to cover (0: 1024 below 128 output tiles in the launch, else 2048)
//   scan_side         1      a kuf_scan family's three launches go to the side stream, beside the other families' Kuf_bar product (0: ahead of it on the main stream)
//   qform             1      a whitened MercerMatern12sm family with fixed inducing inputs forms G = Q Kuf, Q = W^T (Lq Lq^T - I) W, instead of A, Lq^T A and the Kuf_bar product
//                            (gemm_wave.hip role 6; the caller enables it per plan, gp_pdgp_set_qform).  Q inverts Kuu explicitly: a guard on ||L||_F^2 ||W||_F^2
//                            >= cond_2(Kuu + jitter I) raises the handle's status word above GP_QFORM_COND_MAX M^2 (below; DESIGN.md 3.03 has the ladder behind the value) (0: the Cholesky route)
//   qform_far         1      the Q route's product contracts only the rows near each 256-frame group and adds a rank-4 mpad far field (gemm_wave.hip role 7, qfar.hip)
//                            when the frames and the family's inducing inputs are both promised ascending (0: role 6, the dense product)
//   qform_qbar        1      a family whose product took that far field forms Qbar = Kuf diag(2 gv) Kuf^T and v = Kuf gm from it too (qbar.hip);
//                            the split-K product then covers the other latent GPs only (0: it covers every latent GP;
//                            2: the new launches stay on the helper stream, in front of that product, instead of the main stream beside it)
//   act_far           1      a whitened Matern-3/2 family with fixed inducing inputs and ascending frames forms A = W Kuf and colsum((Lq^T A)^2) per 256-frame group from the
//                            rows of Kuf near the group plus an exact rank-4 far field (afar.hip; the caller enables it per plan, gp_pdgp_set_far_act;
//                            strips of 2^20 entries or more) (0: the two dense products)
//   scan_far          1      a kuf_scan family whose A afar.hip formed this step takes its chunk moments and near sums from the same factors (W's near columns, T,
//                            the near rows of Kuf, Psi: kuf_scan_far_moments_kernel; gp_pdgp_set_scan_far can withhold it per plan) (0: the pass over A)
//   h_far             1      the run whose A afar.hip formed takes H = A diag(2 gv) A^T and u = A gm from the stored A once and the same factors once (hfar.hip,
//                            DESIGN.md 3.10; a float64 plan; gp_pdgp_set_h_far can withhold it per plan) (0: the dense split-K product)
//   far_tables        1      the far fields' table kernels and the Q route's guard in their staged forms: afar_t_tiled_kernel (afar.hip) and
//                            qfar_t_lds_kernel (qfar.hip) pass each entering 16-row tile through LDS once per workgroup and write byte-identical tables;
//                            qform_guard_rows_kernel (pdgp_bwd.hip) sums the lower triangles row-wise with 1024 threads per GP — the same verdict, c may differ
//                            in its last bits (0: afar_t_kernel, qfar_t_kernel, qform_guard_kernel)
//   ssm_wide          0      ssm_smooth.hip: 1 = every state dimension takes the two-wavefront walks (128 rows, two per SIMD pair); 0: d <= 64 takes one
//                            wavefront with a row of P per lane (the same sums in the same order: the extra rows and columns are zeros)
//
// Unknown names are reported once on stderr and ignored.
#pragma once
struct GpSwitches {
  int strip_wave = 1, strip_wave_f32 = (1 << 1) | (1 << 2) | (1 << 3) | (1 << 5), strip_wave_roles = (1 << 1) | (1 << 2) | (1 << 3) | (1 << 5), strip_lean = 1, hyper_fuse = 1, kufbar_split = -1,
      cond_a_early = 1, blocked_256 = 1, cov_sum = 1, hyper_sum = 1, chol_cluster = 1, aux_priority = 1, gemm_tile32 = 320, nt_cover = 0, kuf_scan = 1, scan_side = 1, qform = 1, qform_far = 1, qform_qbar = 1, act_far = 1, scan_far = 1, h_far = 1, far_tables = 1, ssm_wide = 0;
};
// qform guard: the Q route is admitted while c = ||L||_F^2 ||W||_F^2 = tr(K) tr(K^-1) <= GP_QFORM_COND_MAX * M^2 for K = Kuu + jitter I.
// cond_2(K) <= c, and c / M^2 is (mean eigenvalue) x (mean inverse eigenvalue), so for one spectrum c grows with M^2 and the bound with
// it.  Ladder (tests/test_qform_cpu.py): up to c / M^2 = 4 (cond_2 ~ 100-160) the Q route's deviation from a long-double
// restatement stays within 5 x the Cholesky route's and below 1e-14 of scale; the benchmark's components sit at 1.1 - 2.7.
#define GP_QFORM_COND_MAX 4.0
const GpSwitches& gp_switches();     // abi.hip
