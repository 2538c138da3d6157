"""The Q route of a whitened MercerMatern12sm latent GP (tests/qform_ref.py restates it in numpy), on the CPU:
A. against autograd through the oracle's conditional: fmean, fvar, and the reverse pass's H, u and Kuf_bar (the last one
   contracted with dK/dtheta, as the engine uses it);
B. a lengthscale ladder against a long-double restatement of the same route on the same float64 covariances, up to the
   largest lengthscale the engine's guard admits — the evidence for GP_QFORM_COND_MAX (gpitch_amd/csrc/switches.h)."""
import os
import re

import numpy as np
import pytest

import qform_ref as qf

BAR = 1e-9                 # of a block's scale: the project's bar for two float64 forms of one quantity
LADDER_ABS = 1e-10         # of scale, against long double
LADDER_REL = 10.0          # x the Cholesky route's own deviation from long double


def _midi2freq(m):
    return 440.0 * 2.0 ** ((m - 69) / 12.0)


def _kern(ls, m, midi=60):
    f0 = _midi2freq(midi)
    return {"type": "mercer_matern12sm", "variance": 1.0, "lengthscales": ls, "energy": [1.0 / m] * m,
            "frequency": [(k + 1) * f0 for k in range(m)]}


def _state(M, N, seed):
    """variational state by gpitch_amd.synth.make_problem's recipe, and upstream gradients of both signs"""
    rq = np.random.RandomState(seed)
    q_mu = 0.3 * rq.randn(M)
    q_sqrt = np.tril(np.eye(M) + 0.05 * rq.randn(M, M))
    return q_mu, q_sqrt, rq.randn(N), 0.5 * rq.randn(N)


def _guard_max():
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "gpitch_amd", "csrc", "switches.h")).read()
    return float(re.search(r"#define\s+GP_QFORM_COND_MAX\s+([0-9.eE+-]+)", src).group(1))


def test_q_route_against_autograd():
    import torch
    from oracle import gpflow05 as orc
    from oracle.backend import TorchBackend
    tb = TorchBackend()
    M, N, m = 64, 256, 3
    z = (np.arange(M) * 0.004).reshape(-1, 1)
    # frames across the inducing grid, none ON it: at a coincident pair r = sqrt(r2 + 1e-12) = 1e-6 and dr/dl = -r2 / (r l) turns the
    # rounding of the expanded r2 (~1e-16) into 1e-10 per entry, and autograd's own lengthscale sum is then good to 1.5e-9
    # only (against long double; the Q route's stays within 3e-10 of it)
    x = ((np.arange(N) + 0.37) * (z[-1, 0] / N)).reshape(-1, 1)
    kern = _kern(0.1, m)
    q_mu, q_sqrt, gm, gv = _state(M, N, 3)
    Kuu, Kuf, kdiag = qf.covariances(kern, z, x)
    got = qf.q_route(Kuu, Kuf, kdiag, q_mu, q_sqrt, gm, gv)

    T = lambda a: torch.tensor(np.asarray(a, dtype=np.float64), requires_grad=True)
    tk = dict(kern)
    tk["variance"], tk["lengthscales"] = T(kern["variance"]), T(kern["lengthscales"])
    tk["energy"], tk["frequency"] = [T(e) for e in kern["energy"]], [T(f) for f in kern["frequency"]]
    theta = [tk["variance"], tk["lengthscales"]] + tk["energy"] + tk["frequency"]
    t_mu, t_sq = T(q_mu.reshape(-1, 1)), T(q_sqrt[:, :, None])
    fmean, fvar = orc.conditional(torch.tensor(x), torch.tensor(z), tk, t_mu, q_sqrt=t_sq, whiten=True, xp=tb)
    ref_mean, ref_var = fmean.detach().numpy().reshape(-1), fvar.detach().numpy().reshape(-1)

    def close(name, a, b):
        scale = max(np.abs(b).max(), 1e-300)
        dev = np.abs(a - b).max() / scale
        print("%s: %.2e of scale" % (name, dev))
        assert dev <= BAR, (name, dev)
    close("fmean", got["fmean"], ref_mean)
    close("fvar", got["fvar"], ref_var)

    # the reverse pass of S = gm . fmean + gv . fvar:  dS/dq_mu = u,  dS/dq_sqrt = tril(H Lq)
    S = torch.sum(torch.tensor(gm) * fmean.reshape(-1)) + torch.sum(torch.tensor(gv) * fvar.reshape(-1))
    g_mu, g_sq = torch.autograd.grad(S, [t_mu, t_sq], retain_graph=True)
    close("u", got["u"], g_mu.numpy().reshape(-1))
    close("tril(H Lq)", np.tril(got["H"] @ np.tril(q_sqrt)), np.tril(g_sq.numpy()[:, :, 0]))
    # H itself, against the Cholesky route's A D A^T formed from the oracle's triangular solve
    A = np.linalg.solve(np.linalg.cholesky(Kuu + qf.JITTER * np.eye(M)), Kuf)
    close("H", got["H"], (A * (2.0 * gv)) @ A.T)
    # Kuf_bar contracted with dKuf/dtheta: autograd of S through Kuf alone (Kuu held constant)
    Kuf_t = orc.K(tk, torch.tensor(z), torch.tensor(x), tb)
    Lm = torch.tensor(np.linalg.cholesky(Kuu + qf.JITTER * np.eye(M)))
    At = tb.trsm(Lm, Kuf_t, lower=True)
    Lq = torch.tensor(np.tril(q_sqrt))
    LTA = Lq.T @ At
    S2 = torch.sum(torch.tensor(gm) * (At.T @ torch.tensor(q_mu))) + torch.sum(torch.tensor(gv) * (torch.sum(LTA * LTA, 0) - torch.sum(At * At, 0)))
    ref_th = np.array([float(g) for g in torch.autograd.grad(S2, theta, retain_graph=True)])
    got_th = np.array([float(g) for g in torch.autograd.grad(torch.sum(torch.tensor(got["Kuf_bar"]) * Kuf_t), theta)])
    for k in range(len(theta)):
        close("Kuf_bar : dK/dtheta[%d]" % k, got_th[k:k + 1], ref_th[k:k + 1])


def test_ladder_up_to_the_guard():
    """z on the benchmark's 4 ms grid, 20 partials of midi 60, 128 inducing points, 512 frames across them.  Both routes get
    the SAME float64 covariances (so what is measured is the route, not how the inputs round), once in float64 and once
    cast to long double; the printed lines are the guard threshold's evidence."""
    LD = np.longdouble
    M, N, m = 128, 512, 20
    z = np.arange(M) * 0.004
    x = np.linspace(0.0, z[-1], N)
    q_mu, q_sqrt, gm, gv = _state(M, N, 1)
    cmax = _guard_max()
    admitted = []
    for ls in (0.01, 0.03, 0.1, 0.2, 0.3, 0.4, 0.5, 0.7):
        cov = qf.covariances(_kern(ls, m), z, x)
        ld = tuple(a.astype(LD) for a in cov)
        chol = qf.cholesky_route(*cov, q_mu, q_sqrt, gm, gv)
        qrt = qf.q_route(*cov, q_mu, q_sqrt, gm, gv)
        ref = qf.cholesky_route(*ld, q_mu.astype(LD), q_sqrt.astype(LD), gm.astype(LD), gv.astype(LD))
        bound = qf.cond_bound(chol["L"], chol["W"])
        kappa = np.linalg.cond(cov[0] + qf.JITTER * np.eye(M))
        ok = bound <= cmax * M * M
        line = "l %-5g cond_2 %8.3g  tr(K) tr(K^-1) %9.3g = %6.3g M^2  %s |" % (ls, kappa, bound, bound / (M * M), "admitted" if ok else "REFUSED ")
        worst = 0.0
        for name in ("fmean", "fvar", "H", "u", "Kuf_bar"):
            scale = float(np.abs(ref[name]).max())
            dc = float(np.abs(chol[name] - ref[name]).max()) / scale
            dq = float(np.abs(qrt[name] - ref[name]).max()) / scale
            line += " %s %.1e / %.1e" % (name, dc, dq)
            if ok:
                assert dq <= LADDER_ABS, (ls, name, dq)
                assert dq <= LADDER_REL * dc, (ls, name, dq, dc)
                worst = max(worst, dq / dc)
        print(line + (" | worst ratio %.1f" % worst if ok else ""))
        admitted.append(ok)
    # the ladder reaches the guard: its last rung, and only that one, is past the threshold
    assert admitted == [True] * 7 + [False], admitted
