"""float64 restatement of the natural-gradient step on one variational posterior q(u) = N(q_mu, Lq Lq^T), Lq = tril(q_sqrt)
(Pdgp.optimize(method=NatGradAdam(...)), gp_pdgp_natgrad_step), in two host routes of the same map.

    g = d ELBO / d q_mu,  G_L = tril(d ELBO / d q_sqrt),  G^ = d ELBO / d S  (S = Lq Lq^T;  G_L = tril(2 G^ Lq))

    step          the closed form the device evaluates
                    Phi = tril(Lq^T G_L),  P = (Phi + Phi^T - diag Phi) / 2 = Lq^T G^ Lq,  B = I - 2 gamma P
                    B = U U^T (U upper: Cholesky of the index-reversed matrix),  Lq' = Lq U^-T,  q_mu' = q_mu + gamma Lq' Lq'^T g
    step_natural  the textbook update in natural parameters theta_1 = S^-1 m, theta_2 = -S^-1 / 2:
                    theta_1 += gamma (g - 2 G^ q_mu),  theta_2 += gamma G^,  S' = (-2 theta_2)^-1,  m' = S' theta_1
                  (G^ = Lq^-T P Lq^-1 by triangular solves; Lq' = chol(S') with the column signs of Lq)

Their difference measures the conditioning of the inputs: `step` never inverts Lq, `step_natural` does.  Both leave the strict
upper triangle of the stored M x M block as it is and raise NotPositiveDefinite when B (equivalently S'^-1) is not positive
definite.  Shared by tests/test_natgrad_cpu.py and tests/test_gpu_natgrad.py.

three_iter_bar(shape, gamma), the bar of the GPU file's three-iteration comparison against the restatement driven by the
oracle's autograd gradients: the device gradient may differ from autograd by GRAD_REL of the gradient's scale, Param by Param
(tests/test_gpu_pdgp.py: atol = 2e-7 * scale).  test_natgrad_cpu.py::test_three_iteration_sensitivity perturbs the autograd
gradient of every variational Param by that much (random signs, a fresh draw per iteration) on the comparison's own problems
and step lengths and prints the change of q after three restated iterations, relative to max(|q|, 1e-3) Param by Param.
THREE_ITER_CHANGE holds what it printed, rounded up; ten times that is the bar, and the CPU test asserts that the measurement
still stays within the table.

CONJ_GRAD_BAR, the bar on the stepped component GP's gradient (q_mu and tril(q_sqrt) together, 2-norm) after one gamma = 1 step
of the conjugate problems, relative to its norm before the step: the restatement, with the oracle's autograd gradient, reaches
3.9e-16 (P = 1) and 2.2e-16 (P = 2) (test_natgrad_cpu.py::test_conjugate_step_in_numpy, which asserts the bar itself);
ten times the larger."""
import numpy as np
from scipy.linalg import solve_triangular

GRAD_REL_SOURCE = "test_gpu_pdgp.py"      # ... atol=<GRAD_REL> * scale: the bound between the device gradient and autograd
THREE_ITER_SHAPES = [0, 1]                # rows of pdgp_sample_ref.SHAPES: (12, 10, 1) and (50, 64, 3)
THREE_ITER_GAMMAS = [0.1, 1.0]
THREE_ITER_CHANGE = {(0, 0.1): 1.5e-7, (0, 1.0): 5.6e-6, (1, 0.1): 3.7e-6, (1, 1.0): 7.3e-6}
CONJ_GRAD_BAR = 3.9e-15


def three_iter_bar(shape, gamma):
    return 10.0 * THREE_ITER_CHANGE[(shape, gamma)]


def grad_rel():
    """the constant of tests/test_gpu_pdgp.py's gradient comparison, read from the file"""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), GRAD_REL_SOURCE)).read()
    found = set(re.findall(r"assert_allclose\(gg\.reshape\(rg\.shape\), rg, rtol=0, atol=([0-9.e-]+) \* scale", src))
    assert len(found) == 1, found
    return float(found.pop())


def perturbed(grads, P, rel, rng):
    """a copy of a gradient dict with every variational Param's gradient moved by rel * max|gradient|, random signs"""
    out = dict(grads)
    for names in variational_names(P):
        for n in names:
            out[n] = grads[n] + rel * np.abs(grads[n]).max() * np.sign(rng.randn(*grads[n].shape))
    return out


class NotPositiveDefinite(np.linalg.LinAlgError):
    """B = I - 2 gamma P is not positive definite: the step is too long"""


def _mat(q_sqrt):
    a = np.asarray(q_sqrt, dtype=np.float64)
    return a[:, :, 0] if a.ndim == 3 else a


def _put(q_sqrt, Lnew):
    """tril(q_sqrt) <- Lnew, the strict upper triangle kept, in q_sqrt's own shape"""
    a = np.array(q_sqrt, dtype=np.float64, copy=True)
    m = a[:, :, 0] if a.ndim == 3 else a
    il = np.tril_indices(m.shape[0])
    m[il] = Lnew[il]
    return a


def sym_P(q_sqrt, G_L):
    """P = Lq^T G^ Lq from the lower triangles alone"""
    Lq, GL = np.tril(_mat(q_sqrt)), np.tril(_mat(G_L))
    Phi = np.tril(Lq.T.dot(GL))
    return 0.5 * (Phi + Phi.T - np.diag(np.diag(Phi)))


def B_matrix(q_sqrt, G_L, gamma):
    P = sym_P(q_sqrt, G_L)
    return np.eye(P.shape[0]) - 2.0 * gamma * P


def step(q_mu, q_sqrt, g, G_L, gamma):
    """(q_mu', q_sqrt') in the shapes given"""
    Lq = np.tril(_mat(q_sqrt))
    M = Lq.shape[0]
    B = B_matrix(q_sqrt, G_L, gamma)
    try:
        C = np.linalg.cholesky(B[::-1, ::-1])
    except np.linalg.LinAlgError:
        raise NotPositiveDefinite("I - 2 gamma P is not positive definite at gamma = %g" % gamma)
    U = C[::-1, ::-1]                                            # upper triangular, B = U U^T
    Lnew = solve_triangular(U, Lq.T, lower=False).T               # Lq U^-T
    mu = np.asarray(q_mu, dtype=np.float64)
    gv = np.asarray(g, dtype=np.float64).reshape(M)
    mu_new = mu.reshape(M) + gamma * Lnew.dot(Lnew.T.dot(gv))
    return mu_new.reshape(mu.shape), _put(q_sqrt, np.tril(Lnew))


def step_natural(q_mu, q_sqrt, g, G_L, gamma):
    """the same map by the natural-parameter route"""
    Lq = np.tril(_mat(q_sqrt))
    M = Lq.shape[0]
    P = sym_P(q_sqrt, G_L)
    X = solve_triangular(Lq, P, lower=True, trans='T')            # Lq^-T P
    Ghat = solve_triangular(Lq, X.T, lower=True, trans='T').T     # Lq^-T P Lq^-1
    Ghat = 0.5 * (Ghat + Ghat.T)
    Linv = solve_triangular(Lq, np.eye(M), lower=True)
    Sinv = Linv.T.dot(Linv)
    mu = np.asarray(q_mu, dtype=np.float64)
    m = mu.reshape(M)
    gv = np.asarray(g, dtype=np.float64).reshape(M)
    th1 = Sinv.dot(m) + gamma * (gv - 2.0 * Ghat.dot(m))
    th2 = -0.5 * Sinv + gamma * Ghat
    try:
        Cs = np.linalg.cholesky(-2.0 * th2)
    except np.linalg.LinAlgError:
        raise NotPositiveDefinite("S'^-1 is not positive definite at gamma = %g" % gamma)
    Ci = solve_triangular(Cs, np.eye(M), lower=True)
    Snew = Ci.T.dot(Ci)
    Lnew = np.linalg.cholesky(0.5 * (Snew + Snew.T)) * np.sign(np.diag(Lq))[None, :]
    return Snew.dot(th1).reshape(mu.shape), _put(q_sqrt, Lnew)


def variational_names(P):
    """[(q_mu name, q_sqrt name)] of helpers.oracle_elbo_and_grads / model_grad_dict, rows [g_0..g_{P-1}, f_0..f_{P-1}]"""
    return ([("q_mu_act%d" % i, "q_sqrt_act%d" % i) for i in range(P)] +
            [("q_mu_com%d" % i, "q_sqrt_com%d" % i) for i in range(P)])


def step_problem(prob, grads, gamma, rows=None):
    """a copy of the oracle-format problem with `step` applied to the latent GPs `rows` (default: all), from a gradient dict
    keyed as helpers.oracle_elbo_and_grads / helpers.model_grad_dict"""
    P = prob["P"]
    out = dict(prob)
    for k in ("q_mu_act", "q_mu_com", "q_sqrt_act", "q_sqrt_com"):
        out[k] = [np.array(a, copy=True) for a in prob[k]]
    for r, (nm, ns) in enumerate(variational_names(P)):
        if rows is not None and r not in rows:
            continue
        km, ks, i = ("q_mu_act", "q_sqrt_act", r) if r < P else ("q_mu_com", "q_sqrt_com", r - P)
        out[km][i], out[ks][i] = step(prob[km][i], prob[ks][i], grads[nm], grads[ns], gamma)
    return out


def iterate(prob, gamma, iters, grad_fn, rows=None):
    """`iters` restated iterations: grad_fn(problem) -> gradient dict"""
    for _ in range(iters):
        prob = step_problem(prob, grad_fn(prob), gamma, rows)
    return prob


def q_distance(a, b):
    """largest difference of the variational Params of two problems, relative to max(|q|, 1e-3) Param by Param (the 1e-8
    rule's scale)"""
    worst = 0.0
    for k in ("q_mu_act", "q_mu_com", "q_sqrt_act", "q_sqrt_com"):
        for u, v in zip(a[k], b[k]):
            u, v = np.asarray(u), np.asarray(v)
            if k.startswith("q_sqrt"):
                u, v = np.tril(_mat(u)), np.tril(_mat(v))
            worst = max(worst, np.abs(u - v).max() / max(np.abs(v).max(), 1e-3))
    return worst


# ---- problems of the GPU file ------------------------------------------------------------------------------------------------
# (Ma, Mc, P) of pdgp_sample_ref.SHAPES rows 0, 1, 2, 4, 5: below one 16-row tile; 50 / 64 (64: the last size the LDS-resident
# factorisation takes); unequal and no multiple of 16 or 32; 512 (the largest size whose panel the one-workgroup factorisation
# keeps in LDS) and 528 (the first it does not, and a last 32-row block of 16 rows).  (33, 65, 1) adds the first sizes past one
# and two 32 x 32 tiles, and 65 the first size of the factorisation's global-memory form.
# (5, 6, 33) has 66 latent GPs: more than one form / apply launch's records hold (64), so the step runs in two chunks around one
# factorisation launch.
STEP_SHAPES = [0, 1, 2, 4, 5]
EXTRA_SHAPE = (33, 65, 1, 2, 520, 140)       # Ma, Mc, P, m, N, seed
MANY_SHAPE = (5, 6, 33, 2, 96, 150)


def shape_problem(k):
    import pdgp_sample_ref as psr
    if k in ("extra", "many"):
        Ma, Mc, P, m, N, seed = EXTRA_SHAPE if k == "extra" else MANY_SHAPE
        return psr.problem(Ma, Mc, P, m, N, seed=seed)
    return psr.shape_problem(k)[0]


def unwhitened_problem():
    import pdgp_sample_ref as psr
    return psr.unwhitened_problem()[0]


def conjugate_problem(P):
    """the known-answer problems: P = 1 (12, 10) and P = 2 (50, 64) of pdgp_sample_ref, with data that carries signal
    (y = 0.5 sin + noise at noise variance 0.05) so that the data term, not only the KL term, shapes the optimum"""
    import pdgp_sample_ref as psr
    prob = psr.problem(12, 10, 1, 2, 204, seed=400) if P == 1 else psr.problem(50, 64, 2, 2, 512, seed=401)
    x = prob["x"]
    rng = np.random.RandomState(402 + P)
    prob["y"] = 0.5 * np.sin(2 * np.pi * 261.6 * x) + 0.05 * rng.randn(*x.shape)
    prob["noise_var"] = 0.05
    return prob


def refusal_problem():
    """a state whose natural-gradient step of length REFUSAL_GAMMA is refused, on the smallest shape.  B = (1 - gamma) I +
    gamma Lq^T (I + Lambda) Lq with Lambda = -2 d(data term) / d S in whitened coordinates, so the KL term alone never refuses
    a step: it takes a data term whose d / d S has an eigenvalue above 1 / 2.  The activation's likelihood is not conjugate:
    y = the component's own posterior mean (the data ask for nlin(g) = 1) under an activation at g = -3 with a narrow q
    (q_sqrt scaled by 0.1) makes E[log p] grow with var(g), and a noise variance of 1e-4 makes that growth large:
    the smallest eigenvalue of B at gamma = 1 is -0.10, and +0.89 at gamma = 0.1 (test_natgrad_cpu.py)."""
    import pdgp_sample_ref as psr
    from oracle import gpflow05 as orc
    prob = psr.problem(12, 10, 1, 2, 204, seed=400)
    fm, _ = orc.conditional(prob["x"], prob["zc"][0], prob["kern_com"][0], prob["q_mu_com"][0], prob["q_sqrt_com"][0], True,
                            full_cov=False)
    prob["y"] = np.asarray(fm, dtype=np.float64).reshape(-1, 1).copy()
    prob["noise_var"] = 1e-4
    Lk = np.linalg.cholesky(orc.K(prob["kern_act"][0], prob["za"][0]) + 1e-6 * np.eye(12))
    prob["q_mu_act"] = [solve_triangular(Lk, -3.0 * np.ones((12, 1)), lower=True)]
    prob["q_sqrt_act"] = [0.1 * a for a in prob["q_sqrt_act"]]
    return prob


REFUSAL_GAMMA = 1.0
REFUSAL_SMALL_GAMMA = 0.1
