"""float64 restatement of the sparse per-source posterior (SGPRSS.predict_s_sparse, gp_sgpr_predict_source_sparse), built
from the oracle's sgpr_common, K and Kdiag: GPflow 0.5 SGPR.build_predict with the one kernel K_p in place of the sum,

    tmp1_p = L^-1 K_p(Z, Xnew),  tmp2_p = LB^-1 tmp1_p,  smean_p = tmp2_p^T c,
    svar_p = Kdiag_p(Xnew) + sum_m tmp2_p^2 - sum_m tmp1_p^2

with L, LB, c as in sgpr_ss.py:43-53.  Shared by the CPU and GPU tests of the sparse posterior."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gpflow05 as orc


def sparse_source(Xnew, X, Y, Z, kern_list, noise_var):
    """(list of P means (n, D), list of P variances (n, D)); zero mean function (pass Y - mean_function(X))"""
    Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1, 1)
    err, Kdg, L, A, AAT, LB, c = orc.sgpr_common(X, Y, Z, kern_list, noise_var)
    D = Y.shape[1]
    means, variances = [], []
    for kp in kern_list:
        tmp1 = solve_triangular(L, orc.K(kp, Z, Xnew), lower=True)
        tmp2 = solve_triangular(LB, tmp1, lower=True)
        means.append(tmp2.T.dot(c))
        var = orc.Kdiag(kp, Xnew) + np.sum(np.square(tmp2), 0) - np.sum(np.square(tmp1), 0)
        variances.append(np.tile(np.reshape(var, (-1, 1)), (1, D)))
    return means, variances


def problem(N, M, P, seed, npart=2):
    """the inputs of tests/test_gpu_sgpr.py's _problem: P decaying sinusoids, MercerMatern12sm kernels, Z on the frame grid"""
    rng = np.random.RandomState(seed)
    fs = 16000.
    X = np.linspace(0, (N - 1) / fs, N).reshape(-1, 1)
    kl = []
    Y = np.zeros((N, 1))
    for p in range(P):
        f0 = 220. * 2 ** (p * 4 / 12.)
        Y += np.sin(2 * np.pi * f0 * X) * np.exp(-((X - X.mean()) / (0.3 * np.ptp(X) + 1e-9)) ** 2)
        kl.append({"type": "mercer_matern12sm", "variance": 1.0 + 0.1 * p, "lengthscales": 0.05 + 0.02 * p,
                   "energy": [0.6, 0.4] if npart == 2 else list(np.linspace(1.0, 0.2, npart) / npart),
                   "frequency": [f0 * (q + 1) for q in range(npart)]})
    Y += 0.05 * rng.randn(N, 1)
    Z = X[:: max(N // M, 1)][:M].copy()
    return X, Y, Z, kl
