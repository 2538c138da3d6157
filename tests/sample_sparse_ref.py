"""float64 restatement of the joint posterior draws of the SGPRSS sources (SGPRSS.sample_s_sparse,
gp_sgpr_sample_source_sparse), built on the oracle's sgpr_common and K: Matheron's rule under the optimal q(u) of the
collapsed bound, with an exact first-order prior sampler along the merged, sorted points t = (Xnew | Z).

    source p, component c (a_k = 2k, b_k = 2k + 1 of partial k; Matern12: one component), per draw:
        s_(1) = sqrt(v) eps_(1),   s_(j) = exp(-D_j / l) s_(j-1) + sqrt(v (-expm1(-2 D_j / l))) eps_(j),   D_j = t_(j) - t_(j-1)
        prior_p(t) = sum_k sqrt(e_k) (a_k cos 2 pi f_k t + b_k sin 2 pi f_k t)               (Matern12: s itself)
    u0   = sum_p prior_p(Z) + sqrt(jitter) eps_u[0]
    beta = L^-T (LB^-T (c + eps_u[1]) - L^-1 u0)
    sample_p(x*) = prior_p(x*) + K_p(Z, x*)^T beta

eps_x (S, C, n), eps_z (S, C, M), eps_u (S, 2, M) are indexed by the caller's point order; C = sum_p components_p.  The map
is affine in eps; joint_cov is the closed-form covariance its linear part reproduces.  Shared by the CPU and GPU tests."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gpflow05 as orc

JITTER = 1e-6
SUPPORTED = ("mercer_matern12sm", "matern12sm", "matern12")


def components(kern):
    if kern["type"] not in SUPPORTED:
        raise NotImplementedError(kern["type"])
    return 1 if kern["type"] == "matern12" else 2 * len(kern["frequency"])


def merged_order(xnew, z):
    return np.argsort(np.concatenate([np.ravel(xnew), np.ravel(z)]), kind="stable")


def prior_paths(kern, t, order, eps):
    """eps (S, c, T) in the caller's point order -> prior_p at the T points, (S, T) in the caller's order"""
    v, ls = float(kern["variance"]), float(kern["lengthscales"])
    S, c, T = eps.shape
    ts = t[order]
    es = eps[:, :, order]
    st = np.empty((S, c, T))
    st[:, :, 0] = np.sqrt(v) * es[:, :, 0]
    for j in range(1, T):
        d = (ts[j] - ts[j - 1]) / ls
        st[:, :, j] = np.exp(-d) * st[:, :, j - 1] + np.sqrt(v * (-np.expm1(-2. * d))) * es[:, :, j]
    if kern["type"] == "matern12":
        ps = st[:, 0, :]
    else:
        ps = np.zeros((S, T))
        for k, (e, f) in enumerate(zip(kern["energy"], kern["frequency"])):
            arg = 2 * np.pi * f * ts
            ps += np.sqrt(e) * (st[:, 2 * k, :] * np.cos(arg) + st[:, 2 * k + 1, :] * np.sin(arg))
    out = np.empty((S, T))
    out[:, order] = ps
    return out


def sample_sources(Xnew, X, Y, Z, kern_list, noise_var, eps_x, eps_z, eps_u):
    """(P, S, n) draws for the one-column residual Y (pass Y - mean_function(X)); Xnew in any order"""
    Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1, 1)
    n, M, S = Xnew.shape[0], Z.shape[0], eps_x.shape[0]
    err, Kdg, L, A, AAT, LB, c = orc.sgpr_common(X, Y, Z, kern_list, noise_var)
    t = np.concatenate([Xnew.ravel(), Z.ravel()])
    order = merged_order(Xnew, Z)
    prior_x, u0, off = [], np.sqrt(JITTER) * eps_u[:, 0, :], 0
    for kp in kern_list:
        cp = components(kp)
        pr = prior_paths(kp, t, order, np.concatenate([eps_x[:, off:off + cp], eps_z[:, off:off + cp]], axis=2))
        prior_x.append(pr[:, :n])
        u0 = u0 + pr[:, n:]
        off += cp
    rhs = c.reshape(1, M) + eps_u[:, 1, :]                                   # (S, M)
    inner = solve_triangular(LB, rhs.T, lower=True, trans='T') - solve_triangular(L, u0.T, lower=True)
    beta = solve_triangular(L, inner, lower=True, trans='T')                 # (M, S)
    # K_p(Z, x*)^T, the orientation the sparse predictor builds: Matern12sm's r = |z - x* + 1e-12| is not symmetric in it
    return np.stack([prior_x[p] + orc.K(kp, Z, Xnew).T.dot(beta).T for p, kp in enumerate(kern_list)])


def joint_cov(Xnew, X, Y, Z, kern_list, noise_var):
    """closed-form joint posterior covariance of (f_1*, ..., f_P*) under q(u): block (p, r) =
    delta_pr K_p(x*, x*) - tmp1_p^T tmp1_r + tmp2_p^T tmp2_r, (P n, P n); and max_p Kdiag_p"""
    Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1, 1)
    err, Kdg, L, A, AAT, LB, c = orc.sgpr_common(X, Y, Z, kern_list, noise_var)
    t1 = [solve_triangular(L, orc.K(kp, Z, Xnew), lower=True) for kp in kern_list]
    t2 = [solve_triangular(LB, a, lower=True) for a in t1]
    P, n = len(kern_list), Xnew.shape[0]
    cov = np.empty((P * n, P * n))
    for p in range(P):
        for r in range(P):
            blk = t2[p].T.dot(t2[r]) - t1[p].T.dot(t1[r])
            if p == r:
                blk = blk + orc.K(kern_list[p], Xnew)
            cov[p * n:(p + 1) * n, r * n:(r + 1) * n] = blk
    return cov, max(float(orc.Kdiag(kp, Xnew).max()) for kp in kern_list)


def eps_shapes(kern_list, n, M, S):
    C = sum(components(k) for k in kern_list)
    return (S, C, n), (S, C, M), (S, 2, M)


def identity_eps(kern_list, n, M):
    """one draw per eps coordinate: the three arrays whose draw i has a one in coordinate i (eps_x, then eps_z, then eps_u)
    and zeros elsewhere.  sample(eps) - sample(0) over these draws is the linear part T, one column per coordinate."""
    shx, shz, shu = eps_shapes(kern_list, n, M, 1)
    nx, nz, nu = int(np.prod(shx)), int(np.prod(shz)), int(np.prod(shu))
    S = nx + nz + nu
    eye = np.eye(S)
    return (eye[:, :nx].reshape((S,) + shx[1:]).copy(), eye[:, nx:nx + nz].reshape((S,) + shz[1:]).copy(),
            eye[:, nx + nz:].reshape((S,) + shu[1:]).copy())


def smallest_problem(shuffle=False):
    """the inputs that pin the mathematics: problem(300, 12, 2, 0), noise 0.3, 40 sorted uniform points of the window with
    three of them set equal to Z[1:4] (optionally shuffled)"""
    from sparse_source_ref import problem
    X, Y, Z, kl = problem(300, 12, 2, 0)
    rng = np.random.RandomState(1)
    Xs = np.sort(rng.uniform(X.min(), X.max(), 40))
    Xs[[7, 19, 31]] = Z[1:4, 0]
    Xs = np.sort(Xs)
    if shuffle:
        Xs = Xs[rng.permutation(40)]
    return X, Y, Z, kl, 0.3, Xs.reshape(-1, 1)
