"""Fitting a pitch's component kernel to its sampled covariance — gpitch/kernelfit.py:28-87.

`fit` takes row 0 of a note's sampled covariance (samplecov.get_cov) and fits
    k(x) = (1 + sqrt(3)|x|/|l|) exp(-sqrt(3)|x|/|l|) sum_i |v_i| cos(2 pi |f_i| |x|)
to it by L-BFGS-B on the RMSE, starting from the FFT peaks of the recording (init_cparam(scaled=False)).  The objective
and its gradient are evaluated on the device for many problems in one launch (gp_kernfit_eval); `fit_many` advances
every problem's L-BFGS-B together through lbfgsb_batch.minimize_many (one launch per round), `learn_kernels` is the
drivers' `init_kernel(train=True)` branch (transcription.py:176-195) in one call.

Deliberate deviation: the optimiser is given the analytic gradient.  The reference gives none, so scipy differentiates
forward with an absolute step of 1e-8; its iterates could not be reproduced anyway (ulp-level differences in f grow by
1e8 in the difference quotient), and the fits end at the same RMSE to within a fraction of a percent with 10-30 times
fewer evaluations.  Kept from the reference: the Matern-3/2 envelope of the fit (the kernel it initialises,
MercerMatern12sm, has a Matern-1/2 one), the bias entry p[0] that is multiplied by 0, the Python 2 split
m = (len(p) - 2) // 2 and tol=1e-12 (ftol = gtol = 1e-12).
"""
import numpy as np

from . import _lib, lbfgsb_batch
from .methods import find_ideal_f0, init_cparam

TOL = 1e-12


def _npartials(p):
    return (np.asarray(p).size - 2) // 2


class KernfitBatch(object):
    """W fitting problems resident on the device: points xs[w], targets ys[w] (1-D), partial counts ms[w].
    Calling it with W parameter vectors (problem w's first 2 + 2 ms[w] entries are used) evaluates every problem in one
    gp_kernfit_eval launch and returns (f (W,), [g_w]) with g_w of the length of the vector passed (0 past 2 + 2 m_w),
    plus the fitted kernels (list of (n_w,)) when want_k."""

    def __init__(self, xs, ys, ms, handle=None):
        h = handle or _lib.default_handle()
        self.h = h
        torch = h.torch
        self.W = len(xs)
        self.n = [int(np.asarray(x).size) for x in xs]
        self.ms = [int(m) for m in ms]
        self.ld = max(max(self.n), 1)
        self.m_max = max(self.ms + [0])
        self.P = 2 + 2 * self.m_max
        X = np.zeros((self.W, self.ld))
        Y = np.zeros((self.W, self.ld))
        for w in range(self.W):
            X[w, :self.n[w]] = np.asarray(xs[w], dtype=np.float64).reshape(-1)
            Y[w, :self.n[w]] = np.asarray(ys[w], dtype=np.float64).reshape(-1)
        self.x = h.to_device(X)
        self.y = h.to_device(Y)
        self.npts = torch.as_tensor(np.array(self.n, dtype=np.int32), device=h.device)
        self.npar = torch.as_tensor(np.array(self.ms, dtype=np.int32), device=h.device)
        self.p = h.zeros(self.W, self.P)
        self.f = h.empty(self.W)
        self.g = h.empty(self.W, self.P)
        self.k = None

    def __call__(self, ps, want_k=False):
        torch = self.h.torch
        rows = np.zeros((self.W, self.P))
        for w in range(self.W):
            q = 2 + 2 * self.ms[w]
            rows[w, :q] = np.asarray(ps[w], dtype=np.float64).reshape(-1)[:q]
        self.p.copy_(torch.from_numpy(rows))
        if want_k and self.k is None:
            self.k = self.h.empty(self.W, self.ld)
        kp = _lib._ptr(self.k) if want_k else None
        self.h.check(self.h.lib.gp_kernfit_eval(self.h.h, self.W, _lib._ptr(self.x), _lib._ptr(self.y), self.ld,
                                                _lib._ptr(self.npts), _lib._ptr(self.npar), self.m_max, _lib._ptr(self.p),
                                                _lib._ptr(self.f), _lib._ptr(self.g), kp))
        f = self.f.cpu().numpy()
        G = self.g.cpu().numpy()
        gs = []
        for w in range(self.W):
            g = np.zeros(np.asarray(ps[w]).size)
            q = 2 + 2 * self.ms[w]
            g[:q] = G[w, :q]
            gs.append(g)
        if not want_k:
            return f, gs
        K = self.k.cpu().numpy()
        return f, gs, [K[w, :self.n[w]].copy() for w in range(self.W)]


def approximate_kernel(p, x, handle=None):
    """kernelfit.py:40-51: k(x) at the points x (same shape as x)"""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    x = np.asarray(x, dtype=np.float64)
    b = KernfitBatch([x], [np.zeros(x.size)], [_npartials(p)], handle)
    return b([p], want_k=True)[2][0].reshape(x.shape)


def loss_func(p, x, y, handle=None):
    """kernelfit.py:28-33: sqrt(mean((k(x) - y)^2))"""
    p = np.asarray(p, dtype=np.float64).reshape(-1)
    b = KernfitBatch([x], [y], [_npartials(p)], handle)
    return float(b([p])[0][0])


def _minimize_many(xs, ys, p0s, handle=None):
    """L-BFGS-B (tol 1e-12) on every problem, all evaluated together; returns the list of minimisers (raw, signed)"""
    p0s = [np.asarray(p0, dtype=np.float64).reshape(-1) for p0 in p0s]
    batch = KernfitBatch(xs, ys, [_npartials(p0) for p0 in p0s], handle)
    if lbfgsb_batch.available():
        def fg(X, active):
            return batch([X[i] for i in range(len(p0s))])
        runs = lbfgsb_batch.minimize_many(fg, p0s, ftol=TOL, gtol=TOL)
        return [r.x.copy() for r in runs]
    # scipy without the reverse-communication routine: one minimisation after the other (same iterates)
    from scipy.optimize import minimize
    out = []
    for w, p0 in enumerate(p0s):
        one = KernfitBatch([xs[w]], [ys[w]], [_npartials(p0)], batch.h)

        def fg1(p):
            f, gs = one([p])
            return float(f[0]), gs[0]
        out.append(minimize(fg1, p0, jac=True, method="L-BFGS-B", tol=TOL).x.copy())
    return out


def optimize_kern(x, y, p0, handle=None):
    """kernelfit.py:54-58: |argmin| of loss_func from p0"""
    phat = _minimize_many([x], [y], [p0], handle)[0]
    return np.sqrt(phat ** 2).copy()


def fit_many(kerns, audios, file_names, max_par, fs, handle=None):
    """`fit` for many notes, every L-BFGS-B advancing together (one gp_kernfit_eval launch per round).  `fs` is one rate
    or one per note.  Returns the list of fit()'s results; each is bit-identical to fit() on that note alone."""
    W = len(kerns)
    fss = list(fs) if np.ndim(fs) else [fs] * W
    xks, ys, p0s = [], [], []
    for w in range(W):
        kern = np.asarray(kerns[w], dtype=np.float64)
        n = kern.size
        xks.append(np.linspace(0., (n - 1.) / fss[w], n).reshape(-1, 1))
        ys.append(kern)
        if0 = find_ideal_f0([file_names[w]])[0]
        init_f, init_v = init_cparam(y=audios[w], fs=fss[w], maxh=max_par, ideal_f0=if0, scaled=False)[0:2]
        p0s.append(np.hstack((np.array([0., 1.]), init_v, init_f)))
    h = handle or _lib.default_handle()
    pstars = [np.sqrt(p ** 2).copy() for p in _minimize_many(xks, ys, p0s, h)]
    shapes = KernfitBatch(xks, [np.zeros(x.size) for x in xks], [_npartials(p) for p in p0s], h)
    k_init = shapes(p0s, want_k=True)[2]
    k_approx = shapes(pstars, want_k=True)[2]
    out = []
    for w in range(W):
        m = _npartials(pstars[w])
        params = [pstars[w][1], pstars[w][2:m + 2], pstars[w][m + 2:]]
        out.append((params, k_init[w].reshape(xks[w].shape), k_approx[w].reshape(xks[w].shape)))
    return out


def fit(kern, audio, file_name, max_par, fs, handle=None):
    """kernelfit.py:61-87: ([lengthscale, variances, frequencies], kern_init, kern_approx)"""
    return fit_many([kern], [audio], [file_name], max_par, fs, handle)[0]


def learn_kernels(ys, names, fs, covsize=441, num_sam=10000, max_par=20, handle=None):
    """The drivers' train branch (transcription.py:176-195, separation.py:185-204) for all training notes at once:
    sampled covariance (samplecov.get_cov_many), kernel fit (fit_many).  Returns (params, kern_sampled, sampled_cov):
    params = [lengthscales, variances, frequencies] (lists over notes, ready for
    init_kern_com(..., len_fixed=False)), kern_sampled = [xkern, skern] (lists of (covsize, 1)), sampled_cov the list
    of (covsize, covsize) covariances."""
    from . import samplecov
    W = len(ys)
    fss = list(fs) if np.ndim(fs) else [fs] * W
    h = handle or _lib.default_handle()
    covs, skern, _ = samplecov.get_cov_many(ys, num_sam, covsize, h)
    fits = fit_many(skern, ys, names, max_par, fss, h)
    params = [[r[0][0] for r in fits], [r[0][1] for r in fits], [r[0][2] for r in fits]]
    xkern = [np.linspace(0., (covsize - 1.) / fss[w], covsize).reshape(-1, 1) for w in range(W)]
    return params, [xkern, skern], covs
