"""Reference for the score of the exact likelihood (SGPRSS.exact_log_likelihood_and_grad, gp_sgpr_exact_loglik_grad), shared by
its CPU and GPU tests: a numpy restatement, in plain loops, of the walk in DESIGN 3c-5.

  score         (loglik, grad, S, gres) of one output column: grad over [noise | theta_0 | theta_1 | ...] with
                theta_p = [variance, lengthscale, e.., f..]; S the sum of the absolute per-step contributions to every entry (its
                cancellation scale); gres = d loglik / d y in training-frame order
  dense_score   torch autograd (float64) through the dense log N(y | 0, K + s2 I) on the idealised kernels (ssm_smooth_ref.k_ideal)

The problems are ssm_smooth_ref's CASES; Xnew plays no part (the timeline is the N training frames, every step observed).

The walk.  Forward as ssm_smooth_ref.smooth, keeping a^-, P^-, g, e, F per step.  Backward j = N - 1 .. 0 from r = 0, Nm = 0:
  1. (j + 1 < N; r, Nm of step j + 1 after its update, before propagation)  P+ = P^-_j - g g^T / F,  a+ = a^-_j + g e / F,
     phi = phi_(j+1):   gphi[j+1][i] = r_i a+_i + sum_k (r_i r_k - Nm_ik) phi_k P+_ik,   gq[j+1][i] = (r_i^2 - Nm_ii) / 2;
     then r <- phi r, Nm <- phi Nm phi
  2. k = g / F, u = Nm k, kr = k.r, ku = k.u, uu = e / F - kr, Fb = (uu^2 - (1 / F + ku)) / 2:
     gs2 += Fb,  gres[j] = -uu,  gh[j] = uu a^- + P^- (uu r + u + Fb h) + Fb g
  3. Nm <- Nm - h u^T - u h^T + h h^T (ku + 1 / F),  r <- r - h kr + h e / F
  4. after j = 0: gv0[i] = (r_i^2 - Nm_ii) / 2
Chain (coordinates i of source p, D_j = t_j - t_(j-1), D_0 = 0):
  d/d noise = gs2;  d/d v_p = sum_(j,i) gq[j][i] (1 - phi^2) + sum_i gv0[i];
  d/d l_p = sum_(j,i) (gphi[j][i] - 2 v_p phi gq[j][i]) phi D_j / l_p^2;
  d/d e_k = sum_j (gh_c h_c + gh_s h_s) / (2 e_k);  d/d f_k = sum_j 2 pi t_j (gh_s h_c - gh_c h_s)"""
import numpy as np

import ssm_smooth_ref as R

CASES, case, case_id, kernels = R.CASES, R.case, R.case_id, R.kernels


def param_vector(noise, kl):
    v = [noise]
    for k in kl:
        v += [k["variance"], k["lengthscales"]] + list(k["energy"]) + list(k["frequency"])
    return np.array(v, dtype=np.float64)


def score(X, Y, kl, noise):
    """(loglik, grad [nparams], S [nparams], gres [N]) for one output column Y (N,)"""
    X = np.asarray(X, dtype=np.float64).reshape(-1)
    Y = np.asarray(Y, dtype=np.float64).reshape(-1)
    N = X.size
    order = np.argsort(X, kind="stable")
    t, y = X[order], Y[order]
    v, ell, src, feat = R._state(kl)
    d = v.size
    H = np.stack([R._hrow(feat, tj) for tj in t])
    phis, dts = np.ones((N, d)), np.zeros(N)
    am, Pm, gs, es, Fs = np.zeros((N, d)), np.zeros((N, d, d)), np.zeros((N, d)), np.zeros(N), np.ones(N)
    a, Pc, loglik = np.zeros(d), np.diag(v), 0.0
    for j in range(N):
        if j > 0:
            dts[j] = max(t[j] - t[j - 1], 0.0)
            phi = np.exp(-dts[j] / ell)
            phis[j] = phi
            a = phi * a
            Pc = phi[:, None] * Pc * phi[None, :] + np.diag(v * (-np.expm1(-2.0 * dts[j] / ell)))
        am[j], Pm[j] = a, Pc
        h = H[j]
        g = Pc.dot(h)
        F = h.dot(g) + noise
        e = y[j] - h.dot(a)
        loglik += -0.5 * (np.log(2 * np.pi * F) + e * e / F)
        a = a + g * (e / F)
        Pc = Pc - np.outer(g, g) / F
        gs[j], es[j], Fs[j] = g, e, F
    gphi, gq, gh, gres = np.zeros((N, d)), np.zeros((N, d)), np.zeros((N, d)), np.zeros(N)
    fb = np.zeros(N)
    r, Nm = np.zeros(d), np.zeros((d, d))
    for j in range(N - 1, -1, -1):
        g, e, F, h = gs[j], es[j], Fs[j], H[j]
        if j + 1 < N:
            Pp = Pm[j] - np.outer(g, g) / F
            ap = am[j] + g * (e / F)
            phi = phis[j + 1]
            gphi[j + 1] = r * ap + ((np.outer(r, r) - Nm) * phi[None, :] * Pp).sum(1)
            gq[j + 1] = 0.5 * (r * r - np.diag(Nm))
            r = phi * r
            Nm = phi[:, None] * Nm * phi[None, :]
        k = g / F
        u = Nm.dot(k)
        kr, ku = k.dot(r), k.dot(u)
        uu = e / F - kr
        Fb = 0.5 * (uu * uu - (1.0 / F + ku))
        fb[j] = Fb
        gres[j] = -uu
        gh[j] = uu * am[j] + Pm[j].dot(uu * r + u + Fb * h) + Fb * g
        Nm = Nm - np.outer(h, u) - np.outer(u, h) + np.outer(h, h) * (ku + 1.0 / F)
        r = r - h * kr + h * (e / F)
    gv0 = 0.5 * (r * r - np.diag(Nm))
    # ---- the chain: per entry the list of its per-step contributions
    grad, S = [fb.sum()], [np.abs(fb).sum()]
    c0 = 0
    for p, kp in enumerate(kl):
        cp = 1 if kp["type"] == "matern12" else 2 * len(kp["frequency"])
        sl = slice(c0, c0 + cp)
        vp, lp = kp["variance"], kp["lengthscales"]
        phi = phis[:, sl]
        terms_v = np.concatenate([(gq[:, sl] * (1.0 - phi * phi)).ravel(), gv0[sl]])
        terms_l = ((gphi[:, sl] - 2.0 * vp * phi * gq[:, sl]) * phi * dts[:, None] / (lp * lp)).ravel()
        grad += [terms_v.sum(), terms_l.sum()]
        S += [np.abs(terms_v).sum(), np.abs(terms_l).sum()]
        ge, gf, se, sf = [], [], [], []
        for q in range(cp // 2 if cp > 1 else 0):
            c, s = c0 + 2 * q, c0 + 2 * q + 1
            te = (gh[:, c] * H[:, c] + gh[:, s] * H[:, s]) / (2.0 * kp["energy"][q])
            tf = 2 * np.pi * t * (gh[:, s] * H[:, c] - gh[:, c] * H[:, s])
            ge.append(te.sum()); se.append(np.abs(te).sum())
            gf.append(tf.sum()); sf.append(np.abs(tf).sum())
        grad += ge + gf
        S += se + sf
        c0 += cp
    back = np.empty(N)
    back[order] = gres
    return loglik, np.array(grad), np.array(S), back


def dense_score(X, Y, kl, noise):
    """(loglik, grad [nparams], gres [N]) by torch autograd (float64) of the dense Gaussian on the idealised kernels"""
    import torch
    x = torch.tensor(np.asarray(X, dtype=np.float64).reshape(-1))
    y = torch.tensor(np.asarray(Y, dtype=np.float64).reshape(-1), requires_grad=True)
    par = torch.tensor(param_vector(noise, kl), requires_grad=True)
    diff = x[:, None] - x[None, :]
    K = par[0] * torch.eye(x.numel(), dtype=torch.float64)
    o = 1
    for k in kl:
        env = par[o] * torch.exp(-diff.abs() / par[o + 1])
        m = len(k["frequency"])
        if k["type"] == "matern12":
            K = K + env
        else:
            K = K + env * sum(par[o + 2 + q] * torch.cos((2 * np.pi * par[o + 2 + m + q]) * diff) for q in range(m))
        o += 2 + 2 * m
    L = torch.linalg.cholesky(K)
    alpha = torch.cholesky_solve(y[:, None], L)[:, 0]
    ll = -0.5 * y.dot(alpha) - torch.log(torch.diagonal(L)).sum() - 0.5 * x.numel() * np.log(2 * np.pi)
    ll.backward()
    return float(ll.detach()), par.grad.numpy().copy(), y.grad.numpy().copy()


def bar(ref, S, rel=1e-8, floor=1e-3):
    """per entry: rel * max(|ref_i|, S_i, floor), the smoother's rule with the cancellation scale added"""
    return rel * np.maximum(np.maximum(np.abs(ref), S), floor)


# The worst ratio |restatement - dense autograd| / bar over a case's entries, measured on the CPU by
# tests/test_ssm_score_cpu.py::test_restatement_matches_dense_autograd (rounded up), which prints it beside the figure it
# measures and holds every case within a tenth of the bar (ratio <= 0.1).  No case comes near a tenth: the largest is 6e-6.
DENSE_RATIO = {
    "d1-N37-mixed-s0.3": 1.0e-07,
    "d2-N37-mixed-s0.1": 9.0e-08,
    "d4-N37-mixed-s0.03": 1.2e-06,
    "d60-N37-mixed-s0.01": 2.3e-06,
    "d63-N37-mixed-s0.3": 5.5e-07,
    "d64-N37-mixed-s0.1": 4.8e-07,
    "d65-N37-mixed-s0.03": 1.7e-06,
    "d127-N37-mixed-s0.1": 1.4e-06,
    "d128-N37-mixed-s0.01": 1.3e-06,
    "d4-N1-mixed-s0.1": 5.0e-08,
    "d65-N1-same-s0.1": 4.9e-08,
    "d4-N2-mixed-s0.03": 4.2e-07,
    "d64-N2-same-s0.3": 1.4e-07,
    "d60-N300-same-s0.01": 5.9e-06,
    "d65-N300-mixed-s0.1": 1.2e-06,
    "d4-N300-mixed-s0.001": 4.4e-07,
    "d60-N37-gap-s0.03": 2.1e-06,
    "d65-N37-dup-s0.1": 1.1e-06,
    "d4-N37-dup-s0.3": 1.7e-07,
}
