"""numpy restatement of the two routes a whitened MercerMatern12sm latent GP can take through the engine, in
whatever float type the inputs have (float64, or numpy's long double as the yardstick):

  Cholesky route  A = W Kuf,  fmean = A^T q_mu,  fvar = kdiag - colsum(A^2) + colsum((Lq^T A)^2),
                  H = A D A^T,  u = A gm,  Kuf_bar = R (A D) + alpha gm^T          (R = W^T E, alpha = W^T q_mu, D = diag(2 gv))
  Q route         G = Q Kuf,  fmean = Kuf^T beta,  fvar = kdiag + colsum(Kuf o G),
                  Qbar = Kuf D Kuf^T, v = Kuf gm,  H = W Qbar W^T,  u = W v,  Kuf_bar = G D + beta gm^T
with W = chol(Kuu + jitter I)^-1, E = Lq Lq^T - I, Q = W^T E W, beta = alpha.  Factor and inverse are written out (numpy's
LAPACK calls take no long double)."""
import numpy as np

JITTER = 1e-6


def covariances(kern, z, x, dtype=np.float64):
    """(Kuu without jitter, Kuf, kdiag) of a mercer_matern12sm kernel dict: the oracle's arithmetic (euclid_dist's expansion,
    r = sqrt(r2 + 1e-12), features on the unscaled inputs) in `dtype`"""
    z = np.asarray(z, dtype).reshape(-1, 1)
    x = np.asarray(x, dtype).reshape(-1, 1)
    var, ls = dtype(kern["variance"]), dtype(kern["lengthscales"])
    e = [dtype(v) for v in kern["energy"]]
    f = [dtype(v) for v in kern["frequency"]]
    two_pi = 2 * np.arccos(dtype(-1))

    def feats(a):
        return np.vstack([np.sqrt(ek) * np.cos(two_pi * fk * a.T) for ek, fk in zip(e, f)] +
                         [np.sqrt(ek) * np.sin(two_pi * fk * a.T) for ek, fk in zip(e, f)])

    def K(a, b):
        a1, b1 = a / ls, b / ls
        r2 = -2 * (a1 @ b1.T) + np.sum(a1 * a1, 1)[:, None] + np.sum(b1 * b1, 1)[None, :]
        return var * np.exp(-np.sqrt(r2 + dtype(1e-12))) * (feats(a).T @ feats(b))
    return K(z, z), K(z, x), np.full(x.shape[0], var * sum(e), dtype)


def chol_and_inverse(K):
    """(L, W = L^-1) of a symmetric positive definite matrix, in its own float type"""
    M = K.shape[0]
    L = np.zeros_like(K)
    for j in range(M):
        d = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j, j] = d
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / d
    W = np.zeros_like(K)
    for i in range(M):
        W[i, :i] = -(L[i, :i] @ W[:i, :i]) / L[i, i]
        W[i, i] = 1 / L[i, i]
    return L, W


def cholesky_route(Kuu, Kuf, kdiag, q_mu, q_sqrt, gm, gv, jitter=JITTER):
    dt = Kuu.dtype.type
    M = Kuu.shape[0]
    L, W = chol_and_inverse(Kuu + dt(jitter) * np.eye(M, dtype=Kuu.dtype))
    Lq = np.tril(q_sqrt)
    A = W @ Kuf
    LTA = Lq.T @ A
    fmean = A.T @ q_mu
    fvar = (kdiag - np.sum(A * A, 0)) + np.sum(LTA * LTA, 0)
    AD = A * (2 * gv)[None, :]
    E = Lq @ Lq.T - np.eye(M, dtype=Kuu.dtype)
    R, alpha = W.T @ E, W.T @ q_mu
    return dict(fmean=fmean, fvar=fvar, H=AD @ A.T, u=A @ gm, Kuf_bar=R @ AD + np.outer(alpha, gm), L=L, W=W)


def q_route(Kuu, Kuf, kdiag, q_mu, q_sqrt, gm, gv, jitter=JITTER):
    dt = Kuu.dtype.type
    M = Kuu.shape[0]
    L, W = chol_and_inverse(Kuu + dt(jitter) * np.eye(M, dtype=Kuu.dtype))
    Lq = np.tril(q_sqrt)
    E = Lq @ Lq.T - np.eye(M, dtype=Kuu.dtype)
    Q, beta = (W.T @ E) @ W, W.T @ q_mu
    G = Q @ Kuf
    fmean = Kuf.T @ beta
    fvar = kdiag + np.sum(Kuf * G, 0)
    Qbar = (Kuf * (2 * gv)[None, :]) @ Kuf.T
    v = Kuf @ gm
    return dict(fmean=fmean, fvar=fvar, H=(W @ Qbar) @ W.T, u=W @ v, Kuf_bar=G * (2 * gv)[None, :] + np.outer(beta, gm),
                L=L, W=W)


def cond_bound(L, W):
    """the guard's quantity: ||L||_F^2 ||W||_F^2 = tr(K) tr(K^-1) >= cond_2(K) for K = L L^T"""
    return float(np.sum(np.tril(L) ** 2) * np.sum(np.tril(W) ** 2))
