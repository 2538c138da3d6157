"""NatGradAdam with a step length per role and automatic halving on the device (gp_pdgp_natgrad_step_adaptive, csrc/natgrad.hip;
DESIGN.md 3k) against tests/natgrad_adaptive_ref.py: nothing to halve changes nothing, a length per role, the halving family at
its three noise levels, an exhausted budget, and — at the ABI, with a synthetic gradient — every tile edge and both launch
chunks with GPs that need 0, 1, 2 and 3 halvings side by side.  Full batch unless stated, so an iteration is deterministic."""
import ctypes as C

import numpy as np
import pytest

import natgrad_adaptive_ref as nga
import natgrad_ref as ng
from helpers import model_grad_dict

pytestmark = pytest.mark.gpu

Q_NAMES = ("q_mu_act", "q_mu_com", "q_sqrt_act", "q_sqrt_com")
STATE = ("_params", "_free", "_adam_m", "_adam_v")


def _model(prob, gp_handle, **kw):
    from gpitch_amd.synth import pdgp_from_problem
    return pdgp_from_problem(prob, whiten=True, handle=gp_handle, **kw)


def _fix_all_but_q(m):
    m.likelihood.variance.fixed = True
    m.za.fixed = True
    m.zc.fixed = True
    for k in list(m.kern_act) + list(m.kern_com):
        for p in k.theta_params():
            p.fixed = True


def _device_grads(m):
    m._pack()
    m._elbo(True)
    return model_grad_dict(m)


def _model_q(m):
    return dict(q_mu_act=[q.value for q in m.q_mu_act], q_mu_com=[q.value for q in m.q_mu_com],
                q_sqrt_act=[q.value for q in m.q_sqrt_act], q_sqrt_com=[q.value for q in m.q_sqrt_com])


def _state(m):
    return [getattr(m, n).cpu().numpy().copy() for n in STATE]


# ---- 1. nothing to halve is nothing changed -----------------------------------------------------------------------------------
def test_nothing_to_halve_is_bit_identical_to_the_plain_token(gp_handle):
    from gpitch_amd.train import NatGradAdam
    prob = ng.shape_problem(1)
    out = []
    for method in (NatGradAdam(0.1, 0.01), NatGradAdam(0.1, 0.01, halvings=4)):
        m = _model(prob, gp_handle, minibatch_size=100)
        rng = np.random.RandomState(5)
        m.x.rng = rng
        m.y.rng = rng
        res = m.optimize(method=method, maxiter=3)
        out.append((_state(m), rng.get_state(), res))
    (s0, r0, res0), (s1, r1, res1) = out
    for a, b in zip(s0, s1):
        assert np.array_equal(a, b)
    assert r0[0] == r1[0] and np.array_equal(r0[1], r1[1]) and r0[2:] == r1[2:]
    assert res0.fun == res1.fun and np.array_equal(res0.x, res1.x)
    assert "natgrad" not in res0
    assert res1.natgrad == {"halvings": [0] * 6, "shortest_gamma": [0.1] * 6}


# ---- 2. a length per role ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ng.STEP_SHAPES + ["extra", "many"])
def test_a_length_per_role_follows_the_restatement(gp_handle, key):
    from gpitch_amd.train import NatGradAdam
    prob = ng.shape_problem(key)
    twin = _model(prob, gp_handle)
    _fix_all_but_q(twin)
    grads = _device_grads(twin)
    want, js = nga.step_problem_adaptive(prob, grads, 0.1, 1.0, 0)
    m = _model(prob, gp_handle)
    _fix_all_but_q(m)
    res = m.optimize(method=NatGradAdam(0.1, gamma_com=1.0), maxiter=1)
    P = prob["P"]
    d = ng.q_distance(dict(prob, **_model_q(m)), want)
    print("%s: q after one per-role step differs from the restatement by %.2e" % (key, d))
    assert d <= 1e-8
    assert res.natgrad == {"halvings": [0] * (2 * P), "shortest_gamma": [0.1] * P + [1.0] * P}
    # ... and not by the step every GP would take at the activations' length
    assert ng.q_distance(ng.step_problem(prob, grads, 0.1), want) > 1e-4


# ---- 3. halving --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("noise_var,two_lmax,halvings", nga.HALVING_TABLE)
def test_a_step_that_is_too_long_is_halved_until_it_is_not(gp_handle, noise_var, two_lmax, halvings):
    from gpitch_amd.train import NatGradAdam
    prob = nga.halving_problem(noise_var)
    grads = _device_grads(_model(prob, gp_handle))
    got = nga.two_lambda_max(prob["q_sqrt_act"][0], grads["q_sqrt_act0"])
    print("noise_var %g: 2 lambda_max(P) of the activation GP from the device gradient %.4f (table %.4f)" % (noise_var, got, two_lmax))
    want = dict(prob)
    for k in Q_NAMES:
        want[k] = list(prob[k])
    want["q_mu_act"][0], want["q_sqrt_act"][0] = ng.step(prob["q_mu_act"][0], prob["q_sqrt_act"][0], grads["q_mu_act0"],
                                                         grads["q_sqrt_act0"], 2.0 ** -halvings)
    want["q_mu_com"][0], want["q_sqrt_com"][0] = ng.step(prob["q_mu_com"][0], prob["q_sqrt_com"][0], grads["q_mu_com0"],
                                                         grads["q_sqrt_com0"], 1.0)
    runs = []
    for _ in range(2):
        m = _model(prob, gp_handle)
        res = m.optimize(method=NatGradAdam(1.0, 1e-6, halvings=4), maxiter=1)
        runs.append(_state(m))
        d = ng.q_distance(dict(prob, **_model_q(m)), want)
        print("   q differs from natgrad_ref.step at 2^-%d / 1 by %.2e" % (halvings, d))
        assert d <= 1e-8
        assert res.natgrad == {"halvings": [halvings, 0], "shortest_gamma": [2.0 ** -halvings, 1.0]}
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---- 4. exhausted ------------------------------------------------------------------------------------------------------------
def test_an_exhausted_budget_refuses_the_step_and_changes_nothing(gp_handle):
    """noise 1e-6 needs four halvings from gamma = 1.  A numerical refusal through the handle's status word: nothing here
    faults the device."""
    from gpitch_amd import _lib
    from gpitch_amd.train import NatGradAdam
    prob = nga.halving_problem(1e-6)
    m = _model(prob, gp_handle)
    m._pack()
    before = _state(m)
    with pytest.raises(_lib.NotPositiveDefiniteError) as ei:
        m.optimize(method=NatGradAdam(1.0, 0.01, halvings=3), maxiter=2)
    msg = str(ei.value)
    assert "too long" in msg and "activation GP 0" in msg and "gamma = 0.125" in msg and "halvings = 3" in msg, msg
    assert "more halvings" in msg
    for a, b in zip(_state(m), before):
        assert np.array_equal(a, b)
    for k in Q_NAMES:
        assert all(np.array_equal(a, b) for a, b in zip(_model_q(m)[k], prob[k]))
    res = m.optimize(method=NatGradAdam(1.0, 0.01, halvings=4), maxiter=1)
    assert np.isfinite(res.fun) and res.natgrad == {"halvings": [4, 0], "shortest_gamma": [2.0 ** -4, 1.0]}
    assert np.abs(m.q_mu_act[0].value - prob["q_mu_act"][0]).max() > 0
    assert np.abs(_state(m)[2]).max() > 0                    # Adam ran beside it


# ---- 5. every tile edge and both chunks, at the ABI ---------------------------------------------------------------------------
# 2 lambda_max(P_r) per class of GP: j = 0 (below 0.8), 1 (in (1.2, 1.7)), 2 (in (2.4, 3.3)), 3 (in (4.8, 6.6)) from gamma = 1
_TARGET = {0: 0.5, 1: 1.45, 2: 2.85, 3: 5.7}
_RANGE = {0: (0.0, 0.8), 1: (1.2, 1.7), 2: (2.4, 3.3), 3: (4.8, 6.6)}


def _big_problem():
    """M = 528 (no LDS panel, a last 32-row block of 16 rows) beside 64"""
    import pdgp_sample_ref as psr
    return psr.problem(528, 64, 1, 2, 2112, seed=160)


def _synthetic(prob, pattern, seed):
    """per latent GP (g, G_L) with 2 lambda_max(P) on the class's target: G_L = tril(2 G^ Lq) of a random symmetric G^ with
    eigenvalues of both signs, scaled"""
    P = prob["P"]
    rng = np.random.RandomState(seed)
    out = []
    for r in range(2 * P):
        q_sqrt = (prob["q_sqrt_act"][r] if r < P else prob["q_sqrt_com"][r - P])[:, :, 0]
        M = q_sqrt.shape[0]
        Lq = np.tril(q_sqrt)
        A = rng.randn(M, M)
        Gh = A + A.T
        Pm = Lq.T.dot(Gh).dot(Lq)
        lmax = np.linalg.eigvalsh(0.5 * (Pm + Pm.T)).max()
        assert lmax > 0
        Gh *= _TARGET[pattern[r]] / (2.0 * lmax)
        G_L = np.tril(2.0 * Gh.dot(Lq))
        g = rng.randn(M, 1) * 0.1
        got = nga.two_lambda_max(q_sqrt, G_L)
        lo, hi = _RANGE[pattern[r]]
        assert lo < got < hi, (r, got)                       # the margins, on the host
        out.append((g, G_L[:, :, None]))
    return out


@pytest.mark.parametrize("key", ("many", "extra", "big"))
def test_every_tile_edge_and_both_chunks_at_the_abi(gp_handle, key):
    from gpitch_amd import _lib
    prob = _big_problem() if key == "big" else ng.shape_problem(key)
    P = prob["P"]
    G = 2 * P
    # a mixed pattern; "many": GP 64 and 65 (the second chunk) halve twice and three times
    pattern = [(1, 0, 2, 3, 0, 1)[r % 6] for r in range(G)]
    if key == "many":
        pattern[64], pattern[65] = 2, 3
    if key == "big":
        pattern = [3, 1]
    syn = _synthetic(prob, pattern, 170)
    m = _model(prob, gp_handle)
    m._pack()
    h = m._handle
    grad = np.zeros(m._nparams)
    for r, ((o_th, o_z, o_mu, o_sq), (g, G_L)) in enumerate(zip(m._layout, syn)):
        M = g.shape[0]
        grad[o_mu:o_mu + M] = g.reshape(-1)
        grad[o_sq:o_sq + M * M] = G_L.reshape(-1)
    m._grad.copy_(h.torch.as_tensor(grad))
    nbytes = h.lib.gp_pdgp_natgrad_adaptive_workspace_bytes(m._plan)
    assert nbytes > h.lib.gp_pdgp_natgrad_workspace_bytes(m._plan)
    ws = h.workspace(nbytes)
    gam = (C.c_double * G)(*([1.0] * G))

    def call(gammas=gam, halvings=3, ptr=None, size=None):
        return h.lib.gp_pdgp_natgrad_step_adaptive(m._plan, m._params.data_ptr(), m._free.data_ptr(), m._grad.data_ptr(), gammas,
                                                   halvings, None, ws.data_ptr() if ptr is None else ptr,
                                                   ws.numel() if size is None else size)
    before = m._params.cpu().numpy().copy()
    assert call(halvings=11) == _lib.GP_ERR_BAD_ARG and call(halvings=-1) == _lib.GP_ERR_BAD_ARG
    assert call(gammas=(C.c_double * G)(*([1.0] * (G - 1) + [1.5]))) == _lib.GP_ERR_BAD_ARG
    assert call(gammas=None) == _lib.GP_ERR_BAD_ARG
    assert call(size=nbytes // 2) == _lib.GP_ERR_WORKSPACE
    assert call(ptr=ws.data_ptr() + 8) == _lib.GP_ERR_BAD_ARG
    h.sync()
    assert np.array_equal(m._params.cpu().numpy(), before)
    h.check(h.lib.gp_pdgp_natgrad_counts(m._plan, ws.data_ptr(), None, None, 1))
    h.check(call())
    h.check(h.lib.gp_check_not_pd(h.h))
    hv, sg = (C.c_int64 * G)(), (C.c_double * G)()
    h.check(h.lib.gp_pdgp_natgrad_counts(m._plan, ws.data_ptr(), hv, sg, 0))
    assert list(hv) == pattern
    assert list(sg) == [2.0 ** -j for j in pattern]
    after_grad, after_params, after_free = m._grad.cpu().numpy(), m._params.cpu().numpy(), m._free.cpu().numpy()
    for (o_th, o_z, o_mu, o_sq), (g, G_L) in zip(m._layout, syn):
        M = g.shape[0]
        assert not np.any(after_grad[o_mu:o_mu + M]) and not np.any(after_grad[o_sq:o_sq + M * M])
        assert np.array_equal(after_params[o_mu:o_mu + M], after_free[o_mu:o_mu + M])
        assert np.array_equal(after_params[o_sq:o_sq + M * M], after_free[o_sq:o_sq + M * M])
    m._unpack()
    got = _model_q(m)
    worst = 0.0
    for r, (g, G_L) in enumerate(syn):
        km, ks, i = ("q_mu_act", "q_sqrt_act", r) if r < P else ("q_mu_com", "q_sqrt_com", r - P)
        mu, sq, j = nga.adaptive_step(prob[km][i], prob[ks][i], g, G_L, 1.0, 3)
        assert j == pattern[r]
        for a, b in ((got[km][i], mu), (np.tril(got[ks][i][:, :, 0]), np.tril(sq[:, :, 0]))):
            err = np.abs(a - b).max() / max(np.abs(b).max(), 1e-3)
            worst = max(worst, err)
            assert err <= 1e-8, (key, r, pattern[r], err)
    print("%s: worst relative difference from adaptive_step %.2e" % (key, worst))
