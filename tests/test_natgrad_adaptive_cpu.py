"""NatGradAdam with a step length per role and automatic halving, the parts that need no GPU: the token's
arguments, the halving family of tests/natgrad_adaptive_ref.py re-derived from the oracle's autograd gradients with the margins
the GPU files rely on, the restatement adaptive_step against natgrad_ref.step, and the host-only parts of the product."""
import numpy as np
import pytest

import natgrad_adaptive_ref as nga
import natgrad_ref as ng


# ---- the token ---------------------------------------------------------------------------------------------------------------
def test_the_defaults_and_the_five_old_attributes():
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    o = NatGradAdam()
    assert (o.gamma, o.learning_rate, o.beta1, o.beta2, o.epsilon) == (0.1, 0.001, 0.9, 0.999, 1e-8)
    assert o.gamma_com is None and o.halvings == 0 and type(o.halvings) is int and not o.adaptive()
    o = NatGradAdam(1, 0.0025, 0.8, 0.99, 1e-7, gamma_com=1, halvings=10)
    assert (o.gamma, o.learning_rate, o.beta1, o.beta2, o.epsilon) == (1.0, 0.0025, 0.8, 0.99, 1e-7)
    assert o.gamma_com == 1.0 and type(o.gamma_com) is float and o.halvings == 10 and o.adaptive()
    assert NatGradAdam(halvings=1).adaptive() and NatGradAdam(gamma_com=0.1).adaptive()
    assert not isinstance(o, AdamOptimizer)
    assert NatGradAdam(0.25, gamma_com=1.0).role_gammas(2) == [0.25, 0.25, 1.0, 1.0]
    assert NatGradAdam(0.25, halvings=3).role_gammas(1) == [0.25, 0.25]


def test_the_new_arguments_are_keyword_only_and_validated():
    from gpitch_amd.train import NatGradAdam
    with pytest.raises(TypeError):
        NatGradAdam(0.1, 0.001, 0.9, 0.999, 1e-8, 1.0)
    for bad in (0, 0.0, -0.1, 1.0000001, 2, float("nan"), float("inf"), "0.1", True, False):
        with pytest.raises(ValueError):
            NatGradAdam(gamma_com=bad)
    for bad in (-1, 11, 1.0, 2.5, "2", None, True, False, float("nan")):
        with pytest.raises(ValueError):
            NatGradAdam(halvings=bad)
    for bad in (0, 1.5, float("nan"), float("inf"), None, "0.1", True):     # gamma keeps its validation beside them
        with pytest.raises(ValueError):
            NatGradAdam(gamma=bad, gamma_com=1.0, halvings=2)


# ---- the halving family ------------------------------------------------------------------------------------------------------
_family = {}


def _family_case(noise_var):
    if noise_var not in _family:
        from helpers import oracle_elbo_and_grads
        prob = nga.halving_problem(noise_var)
        _family[noise_var] = (prob, oracle_elbo_and_grads(prob)[1])
    return _family[noise_var]


@pytest.mark.parametrize("noise_var,two_lmax,halvings", nga.HALVING_TABLE)
def test_the_halving_table_from_the_oracle(noise_var, two_lmax, halvings):
    """2 lambda_max(P) of the activation GP as tabulated; the smallest eigenvalue of B = I - 2 gamma P at the last refused and the
    first accepted length is at least EDGE_MARGIN from zero on its side, so that rounding cannot flip an outcome on the
    device; the component GP never halves, even at gamma = 1"""
    prob, grads = _family_case(noise_var)
    got = nga.two_lambda_max(prob["q_sqrt_act"][0], grads["q_sqrt_act0"])
    print("noise_var %g: 2 lambda_max(P) of the activation GP %.4f (table %.4f)" % (noise_var, got, two_lmax))
    assert abs(got - two_lmax) <= 5e-4 * two_lmax
    assert nga.halvings_needed(got) == halvings
    low = lambda gamma: np.linalg.eigvalsh(ng.B_matrix(prob["q_sqrt_act"][0], grads["q_sqrt_act0"], gamma)).min()
    refused, accepted = low(2.0 ** -(halvings - 1)), low(2.0 ** -halvings)
    print("   smallest eigenvalue of B at gamma = 2^-%d: %.3f, at 2^-%d: %.3f" % (halvings - 1, refused, halvings, accepted))
    assert refused <= -nga.EDGE_MARGIN and accepted >= nga.EDGE_MARGIN
    for j in range(halvings):
        assert low(2.0 ** -j) <= -nga.EDGE_MARGIN
    com = nga.two_lambda_max(prob["q_sqrt_com"][0], grads["q_sqrt_com0"])
    assert abs(com - 0.22) <= 0.01
    assert np.linalg.eigvalsh(ng.B_matrix(prob["q_sqrt_com"][0], grads["q_sqrt_com0"], 1.0)).min() >= nga.EDGE_MARGIN


@pytest.mark.parametrize("noise_var,two_lmax,halvings", nga.HALVING_TABLE)
def test_adaptive_step_is_the_plain_step_at_the_accepted_length(noise_var, two_lmax, halvings):
    prob, grads = _family_case(noise_var)
    args = (prob["q_mu_act"][0], prob["q_sqrt_act"][0], grads["q_mu_act0"], grads["q_sqrt_act0"])
    for budget in (halvings, 10):
        mu, sq, j = nga.adaptive_step(*args, 1.0, budget)
        assert j == halvings
        mu0, sq0 = ng.step(*args, 2.0 ** -halvings)
        assert np.array_equal(mu, mu0) and np.array_equal(sq, sq0)
    with pytest.raises(ng.NotPositiveDefinite):
        nga.adaptive_step(*args, 1.0, halvings - 1)
    # from a length that is accepted as it is: no halving, whatever the budget
    mu, sq, j = nga.adaptive_step(*args, 2.0 ** -halvings, 3)
    assert j == 0 and np.array_equal(mu, mu0) and np.array_equal(sq, sq0)
    want, js = nga.step_problem_adaptive(prob, grads, 1.0, None, halvings)
    assert js == [halvings, 0]
    assert np.array_equal(want["q_mu_act"][0], mu0)
    mc, sc = ng.step(prob["q_mu_com"][0], prob["q_sqrt_com"][0], grads["q_mu_com0"], grads["q_sqrt_com0"], 1.0)
    assert np.array_equal(want["q_mu_com"][0], mc) and np.array_equal(want["q_sqrt_com"][0], sc)
    per_role, js = nga.step_problem_adaptive(prob, grads, 2.0 ** -halvings, 1.0, 0)
    assert js == [0, 0] and ng.q_distance(per_role, want) == 0.0


@pytest.mark.parametrize("Ma,Mc,N,seed,noise_var,halvings", nga.SIZED_HALVING_TABLE)
def test_the_sized_halving_table_from_the_oracle(Ma, Mc, N, seed, noise_var, halvings):
    """the batch file's halving models at 33 / 65 and 128 / 127: the halvings as tabulated, the deciding eigenvalues of B at
    least EDGE_MARGIN from zero on their sides, the component GP accepted at gamma = 1"""
    from helpers import oracle_elbo_and_grads
    prob = nga.sized_halving_problem(Ma, Mc, N, seed, noise_var)
    assert prob["x"].shape[0] <= 1024
    grads = oracle_elbo_and_grads(prob)[1]
    got = nga.two_lambda_max(prob["q_sqrt_act"][0], grads["q_sqrt_act0"])
    refused, accepted = nga.deciding_eigenvalues(prob["q_sqrt_act"][0], grads["q_sqrt_act0"], halvings)
    print("%d / %d, noise_var %g: 2 lambda_max(P) %.4f, smallest eigenvalue of B %.3f at 2^-%d, %.3f at 2^-%d"
          % (Ma, Mc, noise_var, got, refused, halvings - 1, accepted, halvings))
    assert nga.halvings_needed(got) == halvings
    assert refused <= -nga.EDGE_MARGIN and accepted >= nga.EDGE_MARGIN
    assert nga.deciding_eigenvalues(prob["q_sqrt_com"][0], grads["q_sqrt_com0"], 0)[1] >= nga.EDGE_MARGIN


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


def test_the_host_refusals_come_before_any_device_work():
    from gpitch_amd.train import NatGradAdam
    tok = lambda: NatGradAdam(0.5, gamma_com=1.0, halvings=4)
    m = _model()
    m.q_sqrt_act[1].fixed = True
    with pytest.raises(ValueError) as ei:
        m.optimize(method=tok(), maxiter=1)
    assert "activation GP 1" in str(ei.value) and m._plan is None
    m.q_sqrt_act[1].fixed = False
    m.q_mu_com[0].fixed = True
    m.q_sqrt_com[0].fixed = True                               # both fixed: skipped, not refused
    assert m._natgrad_gps(tok()) == [1, 1, 0, 1]
    for name, bad in (("gamma", 1.5), ("gamma_com", 0.0), ("gamma_com", float("nan")), ("gamma_com", "1"), ("halvings", 11),
                      ("halvings", -1), ("halvings", 2.0), ("halvings", True)):
        o = tok()
        setattr(o, name, bad)                                  # a token changed after it was made
        with pytest.raises(ValueError):
            m.optimize(method=o, maxiter=1)
        assert m._plan is None
    for shard in ((0, 2), ("gp", 1, 4)):
        s = _model(shard=shard)
        with pytest.raises(NotImplementedError) as ei:
            s.optimize(method=tok(), maxiter=1)
        assert "unsharded" in str(ei.value) and s._plan is None


def test_the_scope_checks_of_optimize_many():
    from gpitch_amd.pdgp_batch import check_batchable, check_batchable_natgrad
    from gpitch_amd.train import NatGradAdam
    models = [_model(), _model()]
    tok = NatGradAdam(0.5, gamma_com=1.0, halvings=4)
    models_out, flags = check_batchable_natgrad(models, tok)
    assert flags == [[1, 1, 1, 1], [1, 1, 1, 1]]
    with pytest.raises(NotImplementedError):
        check_batchable(models, method=tok)                    # the Adam path's scope check keeps refusing it
    tok.halvings = 12
    with pytest.raises(ValueError):
        check_batchable_natgrad(models, tok)
    assert all(m._plan is None for m in models)


def test_the_new_symbols_are_exported():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    assert lib.gp_pdgp_natgrad_adaptive_workspace_bytes(None) == 0
    assert lib.gp_pdgpb_natgrad_adaptive_workspace_bytes(None) == 0
    for name in ("gp_pdgp_natgrad_adaptive_workspace_bytes", "gp_pdgp_natgrad_step_adaptive", "gp_pdgp_natgrad_counts",
                 "gp_pdgpb_natgrad_adaptive_workspace_bytes", "gp_pdgpb_natgrad_adaptive", "gp_pdgpb_natgrad_counts"):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name
