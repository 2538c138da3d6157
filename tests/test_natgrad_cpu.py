"""Natural-gradient steps on q(u) of a Pdgp, host side: the closed form of tests/natgrad_ref.py against the textbook
natural-parameter route and against torch autograd carried through the expectation-parameter map; its fixed point at gamma = 1;
the refusal of a step whose B is not positive definite; the conditioning of the GPU file's inputs; the measurements the GPU
file's bars are derived from; and the host-only parts of the product (argument checks, refusals before any device work)."""
import numpy as np
import pytest

import natgrad_ref as ng

MS = (1, 7, 33)
GAMMAS = (0.05, 0.5, 1.0)


def _random_inputs(M, seed):
    """(q_mu, q_sqrt, g, G_L, G^): a random state with junk in the stored strict upper triangle, and the gradient of a concave
    objective (G^ negative definite, so every step length in (0, 1] is admissible)"""
    rng = np.random.RandomState(seed)
    q_mu = rng.randn(M, 1)
    q_sqrt = np.tril(np.eye(M) + 0.3 * rng.randn(M, M))
    q_sqrt[np.triu_indices(M, 1)] = rng.randn(M * (M - 1) // 2)
    A = rng.randn(M, M)
    Ghat = -A.dot(A.T) / M - 0.1 * np.eye(M)
    g = rng.randn(M, 1)
    G_L = np.tril(2.0 * Ghat.dot(np.tril(q_sqrt)))
    return q_mu, q_sqrt[:, :, None].copy(), g, G_L[:, :, None].copy(), Ghat


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("gamma", GAMMAS)
def test_closed_form_is_the_textbook_update(M, gamma):
    q_mu, q_sqrt, g, G_L, _ = _random_inputs(M, 10 + M)
    mu_a, sq_a = ng.step(q_mu, q_sqrt, g, G_L, gamma)
    mu_b, sq_b = ng.step_natural(q_mu, q_sqrt, g, G_L, gamma)
    d_mu, d_sq = np.abs(mu_a - mu_b).max(), np.abs(sq_a - sq_b).max()
    print("M = %d, gamma = %g: closed form against natural parameters: q_mu %.2e, q_sqrt %.2e" % (M, gamma, d_mu, d_sq))
    assert d_mu <= 1e-11 * max(np.abs(mu_b).max(), 1.0) and d_sq <= 1e-11 * max(np.abs(sq_b).max(), 1.0)
    assert mu_a.shape == q_mu.shape and sq_a.shape == q_sqrt.shape


@pytest.mark.parametrize("M", MS)
@pytest.mark.parametrize("gamma", GAMMAS)
def test_closed_form_against_autograd_through_the_expectation_parameters(M, gamma):
    """The natural gradient with respect to the natural parameters is the plain gradient with respect to the expectation
    parameters eta = (m, S + m m^T).  torch differentiates an objective written in (m, L) once directly, for the (g, G_L) the
    closed form takes, and once through eta -> (m, chol(eta_2 - m m^T)), for the update of theta; the two updates agree."""
    import torch
    torch.manual_seed(M)
    q_mu, q_sqrt, _, _, _ = _random_inputs(M, 40 + M)
    Lq = np.tril(q_sqrt[:, :, 0])
    Lq = Lq * np.sign(np.diag(Lq))[None, :]           # chol() below returns a positive diagonal: start from one
    q_sqrt = ng._put(q_sqrt, Lq)
    rng = np.random.RandomState(70 + M)
    A = rng.randn(M, M)
    H = A.dot(A.T) / M + 0.5 * np.eye(M)
    b = rng.randn(M)
    Ht, bt = torch.tensor(H), torch.tensor(b)

    def objective(m, L):
        """a data term linear in (m, S + m m^T) minus the whitened KL: concave, the shape of a component GP's ELBO"""
        S = L @ L.T
        return bt @ m - 0.5 * (m @ Ht @ m + torch.trace(Ht @ S)) - 0.5 * (torch.trace(S) + m @ m - M - torch.logdet(S))

    m = torch.tensor(q_mu.reshape(M), requires_grad=True)
    L = torch.tensor(Lq, requires_grad=True)
    objective(m, torch.tril(L)).backward()
    g, G_L = m.grad.numpy().reshape(M, 1), np.tril(L.grad.numpy())[:, :, None]
    mu_a, sq_a = ng.step(q_mu, q_sqrt, g, G_L, gamma)

    S0 = Lq.dot(Lq.T)
    e1 = torch.tensor(q_mu.reshape(M), requires_grad=True)
    e2 = torch.tensor(S0 + q_mu.reshape(M, 1) * q_mu.reshape(1, M), requires_grad=True)
    S = e2 - torch.outer(e1, e1)
    objective(e1, torch.linalg.cholesky(0.5 * (S + S.T))).backward()
    Sinv = np.linalg.inv(S0)
    th1 = Sinv.dot(q_mu.reshape(M)) + gamma * e1.grad.numpy()
    th2 = -0.5 * Sinv + gamma * 0.5 * (e2.grad.numpy() + e2.grad.numpy().T)
    S1 = np.linalg.inv(-2.0 * th2)
    mu_b, L_b = S1.dot(th1), np.linalg.cholesky(0.5 * (S1 + S1.T))
    d_mu, d_sq = np.abs(mu_a.reshape(M) - mu_b).max(), np.abs(np.tril(sq_a[:, :, 0]) - L_b).max()
    print("M = %d, gamma = %g: closed form against autograd through eta: q_mu %.2e, q_sqrt %.2e" % (M, gamma, d_mu, d_sq))
    assert d_mu <= 1e-10 * max(np.abs(mu_b).max(), 1.0) and d_sq <= 1e-10 * max(np.abs(L_b).max(), 1.0)


def test_gamma_one_lands_on_the_optimum_of_a_quadratic_objective():
    """ELBO = b^T m - (m^T H m + tr(H S)) / 2 - KL(N(m, S) || N(0, I)): the optimum is S* = (I + H)^-1, m* = S* b, and one
    step of length 1 from anywhere lands on it, with a zero gradient there"""
    M = 7
    q_mu, q_sqrt, _, _, _ = _random_inputs(M, 5)
    rng = np.random.RandomState(6)
    A = rng.randn(M, M)
    H = A.dot(A.T) / M + 0.5 * np.eye(M)
    b = rng.randn(M, 1)

    def grads(q_mu, q_sqrt):
        L = np.tril(q_sqrt[:, :, 0])
        Ghat = -0.5 * H - 0.5 * (np.eye(M) - np.linalg.inv(L.dot(L.T)))
        return b - H.dot(q_mu) - q_mu, np.tril(2.0 * Ghat.dot(L))[:, :, None]

    g, G_L = grads(q_mu, q_sqrt)
    mu1, sq1 = ng.step(q_mu, q_sqrt, g, G_L, 1.0)
    S_opt = np.linalg.inv(np.eye(M) + H)
    L1 = np.tril(sq1[:, :, 0])
    assert np.abs(L1.dot(L1.T) - S_opt).max() <= 1e-13
    assert np.abs(mu1 - S_opt.dot(b)).max() <= 1e-13
    g1, G1 = grads(mu1, sq1)
    assert np.abs(g1).max() <= 1e-12 and np.abs(G1).max() <= 1e-12
    mu2, sq2 = ng.step(mu1, sq1, g1, G1, 1.0)            # a fixed point
    assert np.abs(mu2 - mu1).max() <= 1e-13 and np.abs(sq2 - sq1).max() <= 1e-13


def test_a_B_that_is_not_positive_definite_is_detected():
    """d ELBO / d S with a positive direction: B = I - 2 gamma Lq^T G^ Lq loses definiteness once gamma passes
    1 / (2 lambda_max(Lq^T G^ Lq)); both routes refuse there and both step just below it"""
    M = 7
    q_mu, q_sqrt, g, _, _ = _random_inputs(M, 3)
    Lq = np.tril(q_sqrt[:, :, 0])
    v = np.random.RandomState(4).randn(M, 1)
    Ghat = 2.0 * v.dot(v.T) / float(v.T.dot(v)[0, 0]) - 0.2 * np.eye(M)
    G_L = np.tril(2.0 * Ghat.dot(Lq))[:, :, None]
    lam = np.linalg.eigvalsh(Lq.T.dot(Ghat).dot(Lq)).max()
    edge = 1.0 / (2.0 * lam)
    assert 0.0 < edge < 1.0
    assert np.linalg.eigvalsh(ng.B_matrix(q_sqrt, G_L, 1.0)).min() < 0.0
    for route in (ng.step, ng.step_natural):
        with pytest.raises(ng.NotPositiveDefinite):
            route(q_mu, q_sqrt, g, G_L, 1.0)
        with pytest.raises(ng.NotPositiveDefinite):
            route(q_mu, q_sqrt, g, G_L, 1.05 * edge)
        route(q_mu, q_sqrt, g, G_L, 0.9 * edge)


@pytest.mark.parametrize("M", MS)
def test_the_strict_upper_triangle_is_untouched(M):
    q_mu, q_sqrt, g, G_L, _ = _random_inputs(M, 20 + M)
    iu = np.triu_indices(M, 1)
    for route in (ng.step, ng.step_natural):
        _, sq = route(q_mu, q_sqrt, g, G_L, 0.5)
        assert np.array_equal(sq[:, :, 0][iu], q_sqrt[:, :, 0][iu])
        assert M == 1 or np.abs(sq - q_sqrt).max() > 0
    # ... and junk there, or in the gradient's, changes nothing below it
    G2 = G_L.copy()
    G2[:, :, 0][iu] = 7.0
    q2 = q_sqrt.copy()
    q2[:, :, 0][iu] = -3.0
    a, b = ng.step(q_mu, q_sqrt, g, G_L, 0.5), ng.step(q_mu, q2, g, G2, 0.5)
    assert np.array_equal(a[0], b[0]) and np.array_equal(np.tril(a[1][:, :, 0]), np.tril(b[1][:, :, 0]))


_oracle_cache = {}


def _oracle_grads(key, prob, whiten=True):
    """the oracle's autograd gradient at a problem of the GPU file, computed once"""
    from helpers import oracle_elbo_and_grads
    if key not in _oracle_cache:
        _oracle_cache[key] = oracle_elbo_and_grads(prob, whiten=whiten)
    return _oracle_cache[key]


def _gpu_cases():
    cases = [(k, ng.shape_problem(k), True) for k in ng.STEP_SHAPES + ["extra", "many"]]
    return cases + [("unwhitened", ng.unwhitened_problem(), False)]


def test_gpu_shapes_are_well_conditioned():
    """Conditioning is a condition on the inputs: at every shape and step length the GPU file uses, the closed form and the
    natural-parameter route (which inverts Lq and S) agree to a tenth of the 1e-8 rule"""
    for key, prob, whiten in _gpu_cases():
        _, grads = _oracle_grads(key, prob, whiten)
        for gamma in (0.1, 1.0):
            a = ng.step_problem(prob, grads, gamma)
            P = prob["P"]
            worst = 0.0
            for r, (nm, ns) in enumerate(ng.variational_names(P)):
                km, ks, i = ("q_mu_act", "q_sqrt_act", r) if r < P else ("q_mu_com", "q_sqrt_com", r - P)
                mu_b, sq_b = ng.step_natural(prob[km][i], prob[ks][i], grads[nm], grads[ns], gamma)
                for u, v in ((a[km][i], mu_b), (a[ks][i], sq_b)):
                    worst = max(worst, np.abs(u - v).max() / max(np.abs(u).max(), 1e-3))
            print("shape %s, gamma = %g: host routes differ by %.2e of max(|q|, 1e-3); a tenth of the rule is 1e-9"
                  % (key, gamma, worst))
            assert worst <= 1e-9, (key, gamma, worst)


def test_three_iteration_sensitivity():
    """what the GPU file's three-iteration bar is derived from (natgrad_ref.THREE_ITER_CHANGE)"""
    from helpers import oracle_elbo_and_grads
    rel = ng.grad_rel()
    assert rel == 2e-7
    for k in ng.THREE_ITER_SHAPES:
        prob = ng.shape_problem(k)
        for gamma in ng.THREE_ITER_GAMMAS:
            rng = np.random.RandomState(7)
            exact = ng.iterate(prob, gamma, 3, lambda p: oracle_elbo_and_grads(p)[1])
            moved = ng.iterate(prob, gamma, 3, lambda p: ng.perturbed(oracle_elbo_and_grads(p)[1], p["P"], rel, rng))
            change = ng.q_distance(moved, exact)
            print("shape %d, gamma = %g: a gradient off by %.0e of its scale moves q by %.2e after three iterations; "
                  "recorded %.1e, bar %.1e" % (k, gamma, rel, change, ng.THREE_ITER_CHANGE[(k, gamma)],
                                                ng.three_iter_bar(k, gamma)))
            assert change <= ng.THREE_ITER_CHANGE[(k, gamma)]


def _com_grad_norm(grads, i):
    return np.sqrt(np.sum(grads["q_mu_com%d" % i] ** 2) + np.sum(np.tril(grads["q_sqrt_com%d" % i][:, :, 0]) ** 2))


@pytest.mark.parametrize("P", (1, 2))
def test_conjugate_step_in_numpy(P):
    """the GPU file's known answer on the restatement: with everything but one component GP's q(u) fixed, one step of length 1
    zeroes that GP's gradient (the figure CONJ_GRAD_BAR is derived from), a second one moves nothing, and the ELBO rises"""
    from helpers import oracle_elbo_and_grads
    prob = ng.conjugate_problem(P)
    i = P - 1
    f0, g0 = oracle_elbo_and_grads(prob)
    p1 = ng.step_problem(prob, g0, 1.0, rows=[P + i])
    f1, g1 = oracle_elbo_and_grads(p1)
    ratio = _com_grad_norm(g1, i) / _com_grad_norm(g0, i)
    p2 = ng.step_problem(p1, g1, 1.0, rows=[P + i])
    print("P = %d: ELBO %.6f -> %.6f; gradient of the stepped GP after / before the step: %.2e (bar of the GPU file %.1e); "
          "a second step moves q by %.2e" % (P, f0, f1, ratio, ng.CONJ_GRAD_BAR, ng.q_distance(p2, p1)))
    assert ratio <= ng.CONJ_GRAD_BAR
    assert ng.q_distance(p2, p1) <= 1e-8
    assert f1 > f0
    for k in ("q_mu_act", "q_sqrt_act"):                       # fixed GPs are skipped
        assert all(np.array_equal(a, b) for a, b in zip(p1[k], prob[k]))
    if P == 2:
        assert np.array_equal(p1["q_mu_com"][0], prob["q_mu_com"][0])


def test_the_refusal_state_is_refused_on_the_cpu_first():
    from helpers import oracle_elbo_and_grads
    prob = ng.refusal_problem()
    _, grads = oracle_elbo_and_grads(prob)
    low = np.linalg.eigvalsh(ng.B_matrix(prob["q_sqrt_act"][0], grads["q_sqrt_act0"], ng.REFUSAL_GAMMA)).min()
    ok = np.linalg.eigvalsh(ng.B_matrix(prob["q_sqrt_act"][0], grads["q_sqrt_act0"], ng.REFUSAL_SMALL_GAMMA)).min()
    com = np.linalg.eigvalsh(ng.B_matrix(prob["q_sqrt_com"][0], grads["q_sqrt_com0"], ng.REFUSAL_GAMMA)).min()
    print("smallest eigenvalue of B: activation GP %.3f at gamma = %g and %.3f at gamma = %g; component GP %.3f"
          % (low, ng.REFUSAL_GAMMA, ok, ng.REFUSAL_SMALL_GAMMA, com))
    assert low < -0.05 and ok > 0.5 and com > 0.5            # far from the edge on either side: rounding cannot flip it
    with pytest.raises(ng.NotPositiveDefinite):
        ng.step_problem(prob, grads, ng.REFUSAL_GAMMA)
    ng.step_problem(prob, grads, ng.REFUSAL_SMALL_GAMMA)


# ---- host-only parts of the product ------------------------------------------------------------------------------------------
def _model(shard=None):
    from gpitch_amd import kernels as K
    from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
    from gpitch_amd.pdgp import Pdgp
    x = np.arange(64).reshape(-1, 1) / 16000.
    z = [[x[::8].copy(), x[::4].copy()], [x[::2].copy(), x[::16].copy()]]
    act = [K.Matern32(1, variance=3.5, lengthscales=1.0), K.Matern32(1, variance=2.0, lengthscales=0.1)]
    com = [MercerMatern12sm(1, energy=np.ones(2) / 2., frequency=110. * np.arange(1, 3), variance=0.9, lengthscales=0.07)
           for _ in range(2)]
    return Pdgp(x, np.zeros_like(x), z, [act, com], shard=shard)


def test_natgradadam_arguments():
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    o = NatGradAdam()
    assert (o.gamma, o.learning_rate, o.beta1, o.beta2, o.epsilon) == (0.1, 0.001, 0.9, 0.999, 1e-8)
    o = NatGradAdam(1, 0.0025, 0.8, 0.99, 1e-7)
    assert (o.gamma, o.learning_rate, o.beta1, o.beta2, o.epsilon) == (1.0, 0.0025, 0.8, 0.99, 1e-7)
    assert not isinstance(o, AdamOptimizer)
    for bad in (0, 0.0, -0.1, 1.0000001, 2, float("nan"), float("inf"), None, "0.1", True):
        with pytest.raises(ValueError):
            NatGradAdam(gamma=bad)


def test_one_of_a_pair_fixed_is_refused_before_any_device_work():
    from gpitch_amd.train import NatGradAdam
    m = _model()
    m.q_sqrt_act[1].fixed = True
    with pytest.raises(ValueError) as ei:
        m.optimize(method=NatGradAdam(0.5), maxiter=1)
    assert "activation GP 1" in str(ei.value) and m._plan is None
    m.q_sqrt_act[1].fixed = False
    m.q_mu_com[0].fixed = True
    with pytest.raises(ValueError) as ei:
        m.optimize(method=NatGradAdam(0.5), maxiter=1)
    assert "component GP 0" in str(ei.value) and m._plan is None
    m.q_sqrt_com[0].fixed = True                               # both fixed: skipped, not refused
    assert m._natgrad_gps(NatGradAdam(0.5)) == [1, 1, 0, 1]
    o = NatGradAdam(0.5)
    o.gamma = 1.5                                              # a token changed after it was made
    with pytest.raises(ValueError):
        m.optimize(method=o, maxiter=1)
    assert m._plan is None


def test_sharded_models_are_refused_before_any_device_work():
    from gpitch_amd.train import NatGradAdam
    for shard in ((0, 2), ("gp", 1, 4)):
        m = _model(shard=shard)
        with pytest.raises(NotImplementedError) as ei:
            m.optimize(method=NatGradAdam(), maxiter=1)
        assert "unsharded" in str(ei.value) and "one GPU" in str(ei.value)
        assert m._plan is None


def test_optimize_many_still_takes_adam_only():
    from gpitch_amd.pdgp_batch import check_batchable
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    models = [_model(), _model()]
    check_batchable(models, method=AdamOptimizer())
    with pytest.raises(NotImplementedError):
        check_batchable(models, method=NatGradAdam())


def test_workspace_bytes_is_exported():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    assert lib.gp_pdgp_natgrad_workspace_bytes(None) == 0
