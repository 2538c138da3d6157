"""References for the simulation smoother (SGPRSS.sample_s_ssm, gp_sgpr_sample_source_ssm), shared by its CPU and GPU tests, on
the helpers and cases of ssm_smooth_ref:

  gains         the gain walk: the covariance recursion of the Kalman filter alone (no data): g_j and F_j of the observed steps
  draw          the numpy restatement of the map: three walks of one d-vector per draw, all draws at once
  linear_part   the map's linear part A, column by column from unit normals: [P n] x [steps d + N]
  dense_joint   the dense exact GP on the idealised kernels: the mean [P n] and the full covariance [P n] x [P n] of all
                sources at all new frames

Rows of a [P n] axis are source-major: p * n + i."""
import numpy as np
from scipy.linalg import cho_solve, cholesky

import ssm_smooth_ref as R


def gains(X, Xnew, kl, noise):
    X = np.asarray(X, dtype=np.float64).reshape(-1)
    Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1)
    N = X.size
    order, out_step, T = R.timeline(X, Xnew)
    v, ell, src, feat = R._state(kl)
    d = v.size
    t = np.array([X[o] if o < N else Xnew[o - N] for o in order])
    H = np.stack([R._hrow(feat, tj) for tj in t])
    phi, q, G, F = np.ones((T, d)), np.zeros((T, d)), np.zeros((T, d)), np.ones(T)
    Pc = np.diag(v)
    for j in range(T):
        if j > 0:
            dt = max(t[j] - t[j - 1], 0.0)
            phi[j] = np.exp(-dt / ell)
            q[j] = v * (-np.expm1(-2.0 * dt / ell))
            Pc = phi[j][:, None] * Pc * phi[j][None, :] + np.diag(q[j])
        if order[j] < N:
            G[j] = Pc.dot(H[j])
            F[j] = H[j].dot(G[j]) + noise
            Pc = Pc - np.outer(G[j], G[j]) / F[j]
    return {"order": order, "out_step": out_step, "steps": T, "N": N, "d": d, "v": v, "src": src, "H": H, "phi": phi, "q": q,
            "G": G, "F": F, "noise": noise, "P": len(kl)}


def draw(gn, Y, eps_x, eps_y):
    """out [P][S][n] of the map for one output column Y (N,), eps_x (S, steps, d), eps_y (S, N)"""
    Y = np.asarray(Y, dtype=np.float64).reshape(-1)
    eps_x, eps_y = np.asarray(eps_x, dtype=np.float64), np.asarray(eps_y, dtype=np.float64)
    order, T, N, d, v = gn["order"], gn["steps"], gn["N"], gn["d"], gn["v"]
    H, phi, q, G, F = gn["H"], gn["phi"], gn["q"], gn["G"], gn["F"]
    S = eps_x.shape[0]
    assert eps_x.shape == (S, T, d) and eps_y.shape == (S, N)
    sigma = np.sqrt(gn["noise"])
    # 1. forward: the prior path plus the filter mean of its residual, folded
    c = np.zeros((S, T))
    w = np.sqrt(v) * eps_x[:, 0]
    for j in range(T):
        if j > 0:
            w = phi[j] * w + np.sqrt(q[j]) * eps_x[:, j]
        o = order[j]
        if o < N:
            c[:, j] = (Y[o] - sigma * eps_y[:, o] - w.dot(H[j])) / F[j]
            w = w + G[j] * c[:, j:j + 1]
    # 2. backward
    r = np.zeros((S, T, d))
    rc = np.zeros((S, d))
    for j in range(T - 1, -1, -1):
        if j < T - 1:
            rc = phi[j + 1] * rc
        if order[j] < N:
            rc = rc - H[j] * (rc.dot(G[j]) / F[j])[:, None] + H[j] * c[:, j:j + 1]
        r[:, j] = rc
    # 3. forward: the posterior path
    out = np.zeros((gn["P"], S, T))
    z = np.sqrt(v) * eps_x[:, 0] + v * r[:, 0]
    for j in range(T):
        if j > 0:
            z = phi[j] * z + np.sqrt(q[j]) * eps_x[:, j] + q[j] * r[:, j]
        for p in range(gn["P"]):
            m = gn["src"] == p
            out[p, :, j] = z[:, m].dot(H[j][m])
    return out[:, :, gn["out_step"]]


def linear_part(gn, Y):
    """A [P n][steps d + N]: column k = draw(unit normal k) - draw(0); the eps_x entries step-major, then eps_y"""
    T, d, N = gn["steps"], gn["d"], gn["N"]
    K = T * d + N
    E = np.eye(K)
    out = draw(gn, Y, E[:, :T * d].reshape(K, T, d), E[:, T * d:])
    zero = draw(gn, Y, np.zeros((1, T, d)), np.zeros((1, N)))
    A = out - zero                                   # [P][K][n]
    return np.transpose(A, (0, 2, 1)).reshape(-1, K)


def dense_joint(X, Y, Xnew, kl, noise):
    """(mean [P n], covariance [P n][P n]) of all sources at all new frames, idealised kernels"""
    X = np.asarray(X, dtype=np.float64).reshape(-1)
    Y = np.asarray(Y, dtype=np.float64).reshape(-1)
    Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1)
    N, n, P = X.size, Xnew.size, len(kl)
    L = cholesky(sum(R.k_ideal(k, X, X) for k in kl) + noise * np.eye(N), lower=True)
    Kx = np.vstack([R.k_ideal(k, Xnew, X) for k in kl])                       # [P n][N]
    prior = np.zeros((P * n, P * n))
    for p, k in enumerate(kl):
        prior[p * n:(p + 1) * n, p * n:(p + 1) * n] = R.k_ideal(k, Xnew, Xnew)
    return Kx.dot(cho_solve((L, True), Y)), prior - Kx.dot(cho_solve((L, True), Kx.T))


def case_index(prefix):
    """the index of the case of ssm_smooth_ref.CASES whose id starts with `prefix` ("d4-N37-mixed")"""
    hits = [i for i in range(len(R.CASES)) if R.case_id(i).startswith(prefix + "-s")]
    assert len(hits) == 1, prefix
    return hits[0]


def random_eps(gn, S, seed):
    rng = np.random.RandomState(seed)
    return rng.randn(S, gn["steps"], gn["d"]), rng.randn(S, gn["N"])
