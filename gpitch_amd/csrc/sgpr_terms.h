// sgpr_terms.h — the SGPRSS scalar and element formulas (gpitch/sgpr_ss.py:56-68 and their derivatives), once, for the
// one-window kernels (sgpr.hip) and the window-batched ones (sgpr_batch.hip).  Device only.  The kernels keep their own
// reductions and grids — those differ and decide the bits — and hand the reduced sums in.
#pragma once
#include "common.h"

// B = H / s2 + I, entry (i, j); inv = 1 / s2
__device__ __forceinline__ double sgpr_B_entry(double h, double inv, int i, int j) { return h * inv + (i == j ? 1.0 : 0.0); }

// E2 = (I - Binv - ubar ubar^T) / s2, entry idx = (i, j)
__device__ __forceinline__ double sgpr_E2_entry(const double* Binv, const double* ubar, double inv, int64_t idx, int i, int j) {
  return inv * ((i == j ? 1.0 : 0.0) - Binv[idx] - ubar[i] * ubar[j]);
}

// The collapsed bound from logd = sum log diag LB, csq = |c|^2, scal[1] = sum err^2 and scal[2] = tr(A' A'^T); one thread.
// Leaves the bound in scal[0] and the kernel sum's Kdiag per point in scal[3].
__device__ __forceinline__ double sgpr_bound_scalar(const double* params, int P, const int* toff, const int* ktype, const int* km,
                                                    int reg, int N, double s2, double logd, double csq, double* scal) {
  double kd = 0.0, vabs = 0.0;
  for (int p = 0; p < P; p++) {
    const double* th = params + toff[p];
    double v = th[0];
    vabs += fabs(v);
    if (gp_kern_kdiag_energy(ktype[p])) {
      double s = 0.0;
      for (int q = 0; q < km[p]; q++) s += th[2 + q];
      v *= s;
    }
    kd += v;
  }
  const double LOG2PI = 1.8378770664093453;
  double b = -0.5 * N * LOG2PI;          // sgpr_ss.py:56
  b += -logd;                            // :57  (output_dim = 1)
  b -= 0.5 * N * log(s2);                // :58
  b += -0.5 * scal[1] / s2;              // :59
  b += 0.5 * csq;                        // :60
  b += -0.5 * (N * kd) / s2;             // :61
  b += 0.5 * scal[2] / s2;               // :62  tr(A A^T) with A = A'/sigma
  if (reg) b -= 1000.0 * vabs;           // :64-68
  scal[0] = b;
  scal[3] = kd;
  return b;
}

// The noise-variance gradient (into g_noise[0] and scal[5]) and dF/dkd (scal[4]) from t_bh = tr(Binv H), t_uhu = ubar^T H ubar,
// t_uu = ubar.u and the bound's scal[1..3]; one thread.  The formula: sgpr.hip, above sgpr_noise_partial_kernel.
__device__ __forceinline__ void sgpr_noise_grad_scalar(double t_bh, double t_uhu, double t_uu, double s, int N, double* scal,
                                                       double* g_noise) {
  const double trBH = -0.5 * t_bh - 0.5 * t_uhu;
  const double trH = scal[2];   // sum colsumsq(A') = tr(H)
  const double g = -trBH / (s * s) - t_uu / (s * s) - 0.5 * trH / (s * s) - 0.5 * N / s + 0.5 * scal[1] / (s * s) +
                   0.5 * N * scal[3] / (s * s);
  g_noise[0] = g;
  scal[4] = -0.5 * N / s;
  scal[5] = g;
}
