"""Modulated-GP likelihood — gpitch/likelihoods.py:279-447 (MpdLik), with hermgauss1d (:33-45) and
log_lik_exp (:47-68) executed by csrc/lik.hip through gp_mpd_varexp."""
import ctypes as C

import numpy as np

from . import _lib
from .methods import nlin_code
from .param import Param, Parameterized, transforms


class MpdLik(Parameterized):
    '''Modulated GP likelihood'''

    def __init__(self, nlinfun, num_sources):
        self.variance = Param(1., transforms.positive)   # likelihoods.py:283
        self.nlinfun = nlinfun
        self.num_sources = num_sources
        self.num_gauss_hermite_points = 20

    def logp(self, F, Y):
        """likelihoods.py:287-323: log N(y | sum_i nlin(g_i) f_i, variance).  (Not on the ELBO path;
        a host-side formula.)"""
        F = np.asarray(F, dtype=np.float64)
        P = self.num_sources
        mean = np.zeros(F.shape[0])
        for i in range(P):
            mean = mean + self.nlinfun(F[:, i]) * F[:, i + P]
        y = np.asarray(Y, dtype=np.float64)[:, 0]
        v = self.variance.value[0]
        return (-0.5 * np.log(2 * np.pi) - 0.5 * np.log(v) - 0.5 * (y - mean) ** 2 / v).reshape(-1, 1)

    def variational_expectations(self, Fmu, Fvar, Y):
        """likelihoods.py:325-447.  Fmu, Fvar: N x 2P with columns [g_0..g_{P-1}, f_0..f_{P-1}]."""
        h = _lib.default_handle()
        Fmu = np.ascontiguousarray(Fmu, dtype=np.float64)
        Fvar = np.ascontiguousarray(Fvar, dtype=np.float64)
        N = Fmu.shape[0]
        P = self.num_sources
        if Fmu.shape != (N, 2 * P) or Fvar.shape != (N, 2 * P):
            raise ValueError("Fmu/Fvar must be N x 2*num_sources")
        dmu, dvar = h.to_device(Fmu), h.to_device(Fvar)
        dy = h.to_device(np.asarray(Y, dtype=np.float64).reshape(-1))
        nv = h.to_device(self.variance.value)
        out = h.empty(N)
        h.check(h.lib.gp_mpd_varexp(h.h, dmu.data_ptr(), dvar.data_ptr(), dy.data_ptr(), N, P, nlin_code(self.nlinfun),
                                    nv.data_ptr(), out.data_ptr(), None))
        return out.cpu().numpy().reshape(-1, 1)

    # ------------------------------------------------------------------------------------------
    # prediction side: the same quadrature applied to the posterior (csrc/lik.hip mpd_moments_kernel)
    def _moments(self, Fmu, Fvar, Y=None, sources=False, y=False, logp=False, noise=True):
        """gp_mpd_predict_moments on host arrays (N x 2P, the column layout of variational_expectations); only the
        requested arrays are computed and copied back: (smean, svar) P x N, (ymean, yvar) N, logp N, else None"""
        Fmu = np.ascontiguousarray(Fmu, dtype=np.float64)
        Fvar = np.ascontiguousarray(Fvar, dtype=np.float64)
        N = Fmu.shape[0]
        P = self.num_sources
        if Fmu.ndim != 2 or Fmu.shape != (N, 2 * P) or Fvar.shape != (N, 2 * P):
            raise ValueError("Fmu/Fvar must be N x 2*num_sources")
        if logp:
            Y = np.asarray(Y, dtype=np.float64).reshape(-1)
            if Y.size != N:
                raise ValueError("Y has %d values for %d rows of Fmu" % (Y.size, N))
        h = _lib.default_handle()
        dmu, dvar = h.to_device(Fmu), h.to_device(Fvar)
        dy = h.to_device(Y) if logp else None
        nv = h.to_device(self.variance.value) if (noise or logp) else None
        sm, sv = (h.empty(P, N), h.empty(P, N)) if sources else (None, None)
        ym, yv = (h.empty(N), h.empty(N)) if y else (None, None)
        lp = h.empty(N) if logp else None
        ptr = lambda t: None if t is None else t.data_ptr()
        h.check(h.lib.gp_mpd_predict_moments(h.h, dmu.data_ptr(), dvar.data_ptr(), ptr(dy), N, P, nlin_code(self.nlinfun),
                                             ptr(nv), ptr(sm), ptr(sv), ptr(ym), ptr(yv), ptr(lp)))
        host = lambda t: None if t is None else t.cpu().numpy()
        return host(sm), host(sv), host(ym), host(yv), host(lp)

    def predict_mean_and_var(self, Fmu, Fvar):
        """GPflow Likelihood.predict_mean_and_var: mean and variance of y (N x 1 each) under q, the nonlinearity
        integrated by the 20-point rule of variational_expectations; the variance includes the noise variance."""
        _, _, ym, yv, _ = self._moments(Fmu, Fvar, y=True)
        return ym.reshape(-1, 1), yv.reshape(-1, 1)

    def predict_sources(self, Fmu, Fvar):
        """posterior mean and variance of every source nlin(g_i) f_i: two lists of P arrays, N x 1"""
        sm, sv, _, _, _ = self._moments(Fmu, Fvar, sources=True)
        P = self.num_sources
        return [sm[i].reshape(-1, 1) for i in range(P)], [sv[i].reshape(-1, 1) for i in range(P)]

    def expected_log_density(self, Fmu, Fvar, Y):
        """E_q[log p(y_n | g, f)] per frame (N x 1): variational_expectations' values, by the prediction kernel"""
        return self._moments(Fmu, Fvar, Y, logp=True)[4].reshape(-1, 1)
