// gh_quad.h — 20-point Gauss-Hermite expectations of the reference's nonlinearities, shared by lik.hip (one model)
// and pdgp_batch.hip (many models).  hermgauss1d gpitch/likelihoods.py:33-45, nonlinearities gpitch/methods.py:216-233.
#pragma once
#include "common.h"

#define GH_POINTS 20

// numpy.polynomial.hermite.hermgauss(20) as exact float64 hex literals (data of the reference's
// algorithm: gpflow.quadrature.hermgauss at likelihoods.py:35)
__constant__ double c_gh_x[GH_POINTS] = {
    -0x1.58cc7ca59b160p+2, -0x1.26a2bbb67f55ep+2, -0x1.f8ee072f5de17p+1, -0x1.ac867f9b566b1p+1,
    -0x1.64f798cfeaf13p+1, -0x1.20a2fcf426dedp+1, -0x1.bd10ceb867454p+0, -0x1.3bec6b39e4f51p+0,
    -0x1.7996281385f71p-1, -0x1.f67530743d203p-3, 0x1.f67530743d203p-3, 0x1.7996281385f71p-1,
    0x1.3bec6b39e4f51p+0, 0x1.bd10ceb867454p+0, 0x1.20a2fcf426dedp+1, 0x1.64f798cfeaf13p+1,
    0x1.ac867f9b566b1p+1, 0x1.f8ee072f5de17p+1, 0x1.26a2bbb67f55ep+2, 0x1.58cc7ca59b160p+2};
// hermgauss weights / sqrt(pi) (likelihoods.py:37)
__constant__ double c_gh_w[GH_POINTS] = {
    0x1.1b3b45ae1f142p-43, 0x1.10e7d83542f1ap-32, 0x1.072c77c84087ep-24, 0x1.276bdd4d669f2p-18,
    0x1.0e2b15190024dp-13, 0x1.dfc024629beb1p-10, 0x1.caae5f0667278p-7, 0x1.f7dc3610551aep-5,
    0x1.4b3dfdef813b4p-3, 0x1.0b0d563a28706p-2, 0x1.0b0d563a28706p-2, 0x1.4b3dfdef813b4p-3,
    0x1.f7dc3610551aep-5, 0x1.caae5f0667278p-7, 0x1.dfc024629beb1p-10, 0x1.0e2b15190024dp-13,
    0x1.276bdd4d669f2p-18, 0x1.072c77c84087ep-24, 0x1.10e7d83542f1ap-32, 0x1.1b3b45ae1f142p-43};

__device__ __forceinline__ void nlin_eval(int nlin, double x, double& s, double& ds) {
  const double PI = 3.141592653589793;
  if (nlin == GP_NLIN_LOGISTIC) {          // methods.py:216-218
    s = 1.0 / (1.0 + exp(-2.0 * (x - PI)));
    ds = 2.0 * s * (1.0 - s);
  } else if (nlin == GP_NLIN_SOFTPLUS) {   // methods.py:220-222 (naive form, as the reference)
    s = log(exp(x) + 1.0);
    ds = 1.0 / (1.0 + exp(-x));
  } else {                                 // methods.py:232-233
    double d = x - PI;
    s = exp(-2.0 * d * d);
    ds = -4.0 * d * s;
  }
}

struct Quad {
  double E1, E2, dE1m, dE1s, dE2m, dE2s;
};

__device__ __forceinline__ Quad gh_quad(int nlin, double mg, double vg, bool want_grad) {
  Quad q = {0, 0, 0, 0, 0, 0};
  const double sd = sqrt(2.0 * vg);
#pragma unroll 4
  for (int hh = 0; hh < GH_POINTS; hh++) {
    const double xh = c_gh_x[hh], wh = c_gh_w[hh];
    double s, ds;
    nlin_eval(nlin, xh * sd + mg, s, ds);
    q.E1 = fma(s, wh, q.E1);
    q.E2 = fma(s * s, wh, q.E2);
    if (want_grad) {
      const double t1 = wh * ds, t2 = 2.0 * wh * s * ds;
      q.dE1m += t1;
      q.dE1s = fma(t1, xh, q.dE1s);
      q.dE2m += t2;
      q.dE2s = fma(t2, xh, q.dE2s);
    }
  }
  return q;
}

// ---------------------------------------------------------------------------------------------------------------
// Prediction side: E1, E2 exactly as gh_quad forms them (same operations in the same order) and the rule's own variance of
// nlin(g), V = sum_h w_h (nlin(x_h) - E1)^2 >= 0.  The 20 values stay in registers (both loops fully unrolled), so each
// node's exp() work is done once.
struct QuadV {
  double E1, E2, V;
};

__device__ __forceinline__ QuadV gh_quad_var(int nlin, double mg, double vg) {
  double s[GH_POINTS];
  QuadV q = {0, 0, 0};
  const double sd = sqrt(2.0 * vg);
#pragma unroll
  for (int hh = 0; hh < GH_POINTS; hh++) {
    const double xh = c_gh_x[hh], wh = c_gh_w[hh];
    double ds;
    nlin_eval(nlin, xh * sd + mg, s[hh], ds);
    q.E1 = fma(s[hh], wh, q.E1);
    q.E2 = fma(s[hh] * s[hh], wh, q.E2);
  }
#pragma unroll
  for (int hh = 0; hh < GH_POINTS; hh++) {
    const double d = s[hh] - q.E1;
    q.V = fma(c_gh_w[hh], d * d, q.V);
  }
  return q;
}

// Moments of one frame by MOM_LANES lanes (lane l takes the sources l, l + MOM_LANES, ...), shared by mpd_moments_kernel
// (lik.hip) and pdgpb_pred_moments_kernel (pdgp_batch.hip).  Fm / Fv: the model's 2P rows, element (row c, this frame) at
// [c * cs + fo]; smean / svar: P rows, element (i, this frame) at [i * ld + oo]; ymean / yvar / logp: the frame's own slot;
// yvar takes the noise variance only when add_noise.
// Each lane writes the moments of its sources and parks a_i = E1_i m_f_i, E2_i, v_f_i + m_f_i^2 and svar_i in LDS (sm: 4 P
// doubles of this frame); after the barrier lane 0 replays mpd_lik_kernel's sequential accumulation over i = 0..P-1 (same
// order, same fused operations) and adds up the variances in source order.  Called by every thread of the workgroup
// (`live` = false for the lanes of a frame beyond the end): it holds a __syncthreads().
#define MOM_LANES 16
__device__ __forceinline__ void mpd_moments_frame(const double* __restrict__ Fm, const double* __restrict__ Fv, int64_t cs,
                                                  int64_t fo, bool live, int l, int P, int nlin, const double* noise, bool add_noise,
                                                  const double* y, double* __restrict__ smean, double* __restrict__ svar,
                                                  int64_t ld, int64_t oo, double* ymean, double* yvar, double* logp,
                                                  double* sm) {
  double* sa = sm;
  double* se = sa + P;
  double* sc = se + P;
  double* sv = sc + P;
  if (live) {
    for (int i = l; i < P; i += MOM_LANES) {
      const double mg = Fm[i * cs + fo], vg = Fv[i * cs + fo];
      const double mf = Fm[(i + P) * cs + fo], vf = Fv[(i + P) * cs + fo];
      const QuadV q = gh_quad_var(nlin, mg, vg);
      const double a = q.E1 * mf;
      const double v = fma(q.V, mf * mf, q.E2 * vf);
      sa[i] = a;
      se[i] = q.E2;
      sc[i] = vf + mf * mf;
      sv[i] = v;
      if (smean) smean[i * ld + oo] = a;
      if (svar) svar[i * ld + oo] = v;
    }
  }
  __syncthreads();
  if (live && l == 0 && (ymean || yvar || logp)) {
    double A = 0.0, B = 0.0, Cpair = 0.0, S = 0.0;
    for (int i = 0; i < P; i++) {
      const double a = sa[i];
      Cpair = fma(a, A, Cpair);
      A += a;
      B = fma(se[i], sc[i], B);
      S += sv[i];
    }
    if (ymean) *ymean = A;
    if (yvar) *yvar = add_noise ? S + noise[0] : S;
    if (logp) {
      const double Y = y[0], s2 = noise[0];
      const double C = 2.0 * Cpair;
      const double resid = Y * Y - 2.0 * Y * A + B + C;
      const double LOG2PI = 1.8378770664093453;
      *logp = -0.5 * ((1.0 / s2) * resid + LOG2PI + log(s2));
    }
  }
}
