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
