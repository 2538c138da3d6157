"""float64 restatement of the natural-gradient step with a length per role and automatic halving (NatGradAdam(gamma,
gamma_com=..., halvings=...), gp_pdgp_natgrad_step_adaptive, gp_pdgpb_natgrad_adaptive), on top of
tests/natgrad_ref.py: a latent GP takes natgrad_ref.step at the first of gamma, gamma / 2, ..., gamma / 2^halvings whose
B = I - 2 gamma P is positive definite, by the test that step applies (the Cholesky factorisation of the reversed B) and
nothing else.  Shared by tests/test_natgrad_adaptive_cpu.py and the two GPU files.

HALVING_TABLE: the family halving_problem(noise_var), measured on the CPU with the oracle's autograd gradients
(test_natgrad_adaptive_cpu.py re-derives it): 2 lambda_max(P) of the activation GP and the halvings a step from gamma = 1
needs.  The component GP has 2 lambda_max = 0.22 in all three and never halves."""
import numpy as np

import natgrad_ref as ng

HALVING_TABLE = [(1e-4, 1.0999, 1), (6e-6, 2.8331, 2), (1e-6, 12.0528, 4)]     # noise_var, 2 lambda_max(P) activation, halvings
# the same recipe at the sizes where the kernels' tiles end (sized_halving_problem): Ma, Mc, N, seed, noise_var, halvings of the
# activation GP from gamma = 1.  Measured on the CPU with the oracle's autograd gradients: 2 lambda_max(P) of the activation GP is
# 1 + 3.08e-5 / noise_var at 33 / 65 and 1 + 1.90e-5 / noise_var at 128 / 127 (the component GPs: 0.60 and 0.72, never halved);
# the noise levels put it at 1.30, 5.70, 2.90 and 5.70, away from the powers of two.
SIZED_HALVING_TABLE = [(33, 65, 520, 140, 1e-4, 1), (33, 65, 520, 140, 6.55e-6, 3), (128, 127, 2816, 160, 1e-5, 2),
                       (128, 127, 2816, 160, 4.03e-6, 3)]
EDGE_MARGIN = 0.05           # the deciding eigenvalues of B lie at least this far from zero, on their sides


def adaptive_step(q_mu, q_sqrt, g, G_L, gamma, halvings):
    """(q_mu', q_sqrt', j): natgrad_ref.step at gamma 2^-j for the smallest j in 0..halvings it accepts; NotPositiveDefinite
    when it accepts none"""
    for j in range(halvings + 1):
        try:
            mu, sq = ng.step(q_mu, q_sqrt, g, G_L, gamma * 2.0 ** -j)
            return mu, sq, j
        except ng.NotPositiveDefinite:
            pass
    raise ng.NotPositiveDefinite("I - 2 gamma P is not positive definite at gamma = %g, the last of %d halvings"
                                 % (gamma * 2.0 ** -halvings, halvings))


def step_problem_adaptive(prob, grads, gamma_act, gamma_com, halvings, rows=None):
    """(a copy of the oracle-format problem with adaptive_step applied to the latent GPs `rows` (default: all), [j per latent
    GP, 0 for one not stepped]), rows [g_0..g_{P-1}, f_0..f_{P-1}]; gamma_com None: gamma_act for every GP"""
    P = prob["P"]
    out = dict(prob)
    for k in ("q_mu_act", "q_mu_com", "q_sqrt_act", "q_sqrt_com"):
        out[k] = [np.array(a, copy=True) for a in prob[k]]
    js = [0] * (2 * P)
    for r, (nm, ns) in enumerate(ng.variational_names(P)):
        if rows is not None and r not in rows:
            continue
        km, ks, i = ("q_mu_act", "q_sqrt_act", r) if r < P else ("q_mu_com", "q_sqrt_com", r - P)
        gamma = gamma_act if (r < P or gamma_com is None) else gamma_com
        out[km][i], out[ks][i], js[r] = adaptive_step(prob[km][i], prob[ks][i], grads[nm], grads[ns], gamma, halvings)
    return out, js


def halving_problem(noise_var):
    """natgrad_ref.refusal_problem() with its noise variance replaced"""
    prob = ng.refusal_problem()
    prob["noise_var"] = float(noise_var)
    return prob


def sized_halving_problem(Ma, Mc, N, seed, noise_var):
    """natgrad_ref.refusal_problem()'s recipe on pdgp_sample_ref.problem(Ma, Mc, 1, 2, N, seed): y = the component's own
    posterior mean, the activation at g = -3 with q_sqrt scaled by 0.1, and the noise variance given.  N = 520 and 2816 leave
    260 and 256 frames: a full batch also for the batched entry."""
    import pdgp_sample_ref as psr
    from oracle import gpflow05 as orc
    from scipy.linalg import solve_triangular
    prob = psr.problem(Ma, Mc, 1, 2, N, seed=seed)
    fm, _ = orc.conditional(prob["x"], prob["zc"][0], prob["kern_com"][0], prob["q_mu_com"][0], prob["q_sqrt_com"][0], True,
                            full_cov=False)
    prob["y"] = np.asarray(fm, dtype=np.float64).reshape(-1, 1).copy()
    prob["noise_var"] = float(noise_var)
    Lk = np.linalg.cholesky(orc.K(prob["kern_act"][0], prob["za"][0]) + 1e-6 * np.eye(Ma))
    prob["q_mu_act"] = [solve_triangular(Lk, -3.0 * np.ones((Ma, 1)), lower=True)]
    prob["q_sqrt_act"] = [0.1 * a for a in prob["q_sqrt_act"]]
    return prob


def deciding_eigenvalues(q_sqrt, G_L, halvings, gamma=1.0):
    """(smallest eigenvalue of B at the last refused length, or None when halvings = 0; at the accepted length)"""
    low = lambda g: np.linalg.eigvalsh(ng.B_matrix(q_sqrt, G_L, g)).min()
    return (low(gamma * 2.0 ** -(halvings - 1)) if halvings > 0 else None), low(gamma * 2.0 ** -halvings)


def two_lambda_max(q_sqrt, G_L):
    return 2.0 * np.linalg.eigvalsh(ng.sym_P(q_sqrt, G_L)).max()


def halvings_needed(two_lmax, gamma=1.0):
    """the smallest j with gamma 2^-j * 2 lambda_max < 1"""
    j = 0
    while gamma * 2.0 ** -j * two_lmax >= 1.0:
        j += 1
    return j
