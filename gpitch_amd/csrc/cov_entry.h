// cov_entry.h — the arithmetic of ONE covariance entry, one spectral-mixture feature pair and one Kdiag value, shared by
// every kernel that has to produce the values cov.hip's builds write (cov.hip itself; predict_sparse.hip, which builds
// its K_p(Z, x*) tile in LDS instead of a strip in HBM).  Device-only; include after common.h.
#pragma once
#include "common.h"

__device__ __forceinline__ double stat_profile(int type, double r2, double var, const double* __restrict__ etab) {
  // r2 is the literal expansion; the kernels below follow GPflow 0.5 Stationary subclasses
  if (type == GP_KERN_RBF) return var * gp_exp_neg(-r2 * 0.5, etab);
  double r = gp_sqrt_pos(__dadd_rn(r2, 1e-12));
  if (type == GP_KERN_MATERN12) return var * gp_exp_neg(-r, etab);
  if (type == GP_KERN_MATERN32) {
    const double s3 = 1.7320508075688772;
    return var * (1.0 + s3 * r) * gp_exp_neg(-s3 * r, etab);
  }
  // Matern52
  const double s5 = 2.23606797749979;
  return var * (1.0 + s5 * r + (5.0 / 3.0) * (r * r)) * gp_exp_neg(-s5 * r, etab);
}

__device__ __forceinline__ double r2_expand(double a, double aa, double b, double bb) {
  return __dadd_rn(__dadd_rn(-2.0 * __dmul_rn(a, b), aa), bb);
}

// spectral-mixture feature pair of partial p < m at x: sqrt(e_p) cos(2 pi f_p x), sqrt(e_p) sin(2 pi f_p x)
__device__ __forceinline__ void cov_sm_feature(const double* __restrict__ th, int m, int p, double x, double* c, double* s) {
  const double e = th[2 + p], fr = th[2 + m + p];
  const double arg = __dmul_rn(__dmul_rn(6.283185307179586, fr), x);
  sincos(arg, s, c);
  const double se = __dsqrt_rn(e);
  *c *= se; *s *= se;
}

// Mercer (feature) form: var * env(r) * acc, acc = Phi(z)^T Phi(x) summed in feature order, r = sqrt(r2 + 1e-12);
// env 0: Matern-1/2 (MercerMatern12sm), otherwise Matern-5/2 (the Matern52 x MercerCosMix product, GPflow Matern52.K profile)
__device__ __forceinline__ double cov_mercer_entry(int env, double var, double a, double aa, double b, double bb, double acc,
                                                   const double* __restrict__ etab) {
  const double r = gp_sqrt_pos(__dadd_rn(r2_expand(a, aa, b, bb), 1e-12));
  if (env == 0) return var * gp_exp_neg(-r, etab) * acc;
  const double s5 = 2.23606797749979;
  return var * ((1.0 + s5 * r + (5.0 / 3.0) * (r * r)) * gp_exp_neg(-s5 * r, etab)) * acc;
}

// broadcast form, Matern12sm (m12sm.py:46-56) / Matern32sm (kernels.py:232-247): r = sqrt((x - x' + 1e-12)^2)
__device__ __forceinline__ double cov_broadcast_entry(int type, const double* __restrict__ th, int m, double var, double ls,
                                                      double xa, double xb) {
  const double d = __dadd_rn(__dadd_rn(xa, -xb), 1e-12);
  const double r = __dsqrt_rn(__dmul_rn(d, d));
  double s = 0.0;
  for (int p = 0; p < m; p++)
    s += th[2 + p] * cos(__dmul_rn(__dmul_rn(6.283185307179586, th[2 + m + p]), r));
  if (type == GP_KERN_MATERN12SM) return var * exp(-(r / ls)) * s;
  // Matern32sm: r1 = sqrt(3) r / l, (1 + r1) exp(-r1) sum_k variance_k cos(2 pi f_k r)
  const double r1 = 1.7320508075688772 * (r / ls);
  return var * ((1.0 + r1) * exp(-r1)) * s;
}

// Kdiag of one kernel: variance, times the summed energies where the family's diagonal carries them
__device__ __forceinline__ double cov_kdiag(int type, int m, const double* __restrict__ th) {
  double v = th[0];
  if (gp_kern_kdiag_energy(type)) {
    double s = th[2];
    for (int p = 1; p < m; p++) s += th[2 + p];
    v = v * s;
  }
  return v;
}

// ---- separable envelope: which 16-row tiles of a Mercer Kuf strip are written in product form ----------------------------
// With a = z / l of a tile's rows in [tile_lo, tile_hi] and b = x / l of a wavefront's CVM_SEP_COLS columns in [bmin, bmax],
// the tile is separable when every a lies at least CVM_SEP above every b, or below (cov.hip has the argument and the error
// bound).  One definition for the builders (cov.hip) and for the range rule of the Q route's far field (qfar.hip), which must
// call an entry far only where the builder wrote it as a product.
#define CVM_SEP 1.0                  // |z - x| / lengthscale at least this for every entry of a tile
#define CVM_SEP_COLS 32              // columns of one builder wavefront (16 * CVM_CT of cov.hip)
__device__ __forceinline__ bool cov_sep_cols_ok(double senv, double bmin, double bmax) { return senv * (bmax - bmin) < 300.0; }
__device__ __forceinline__ bool cov_sep_above(bool cols_ok, double tile_lo, double bmax) { return cols_ok && (tile_lo - bmax >= CVM_SEP); }
__device__ __forceinline__ bool cov_sep_below(bool cols_ok, double bmin, double tile_hi) { return cols_ok && (bmin - tile_hi >= CVM_SEP); }
