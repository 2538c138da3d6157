"""The frame-chunked oracle forms (tests/helpers.py) equal the whole-batch oracle they restate: the Pdgp ELBO and its
gradient, the Pdgp predictions, the SGPRSS bound, its gradient and predict_f.  CPU only; N = 5000 in chunks of 1024
leaves a ragged last chunk of 904 frames."""
import numpy as np
import pytest

from helpers import (oracle_elbo_and_grads, oracle_elbo_and_grads_chunked, oracle_predict_act_n_com_chunked,  # noqa: E402
                     oracle_sgpr_bound_chunked, oracle_sgpr_bound_and_grads_chunked, oracle_sgpr_predict_f_chunked)

N, CHUNK = 5000, 1024
RTOL = 1e-12
# kernel lengthscale gradients: each is a sum over N x M covariance entries whose terms, amplified near r = 0 by the
# derivative of GPflow's sqrt(r^2 + 1e-12) distance, cancel down to the result, so its last digits follow the order in
# which autograd sums frames — which chunking changes.  Measured (seeds 4-6 below, 5000 frames in chunks of 1024): up to
# 6.0e-7 relative (com1, seed 6), 1.6e-9 in the SGPRSS case; every other entry within 1.3e-11 of its block's largest.
LS_RTOL = 5e-6
# the other gradient entries (relative to their block's largest entry) carry the same summation-order rounding at a smaller
# amplification: inducing inputs and kernel variances, measured up to 6.4e-12 (seeds 4-6); the rest <= 1e-13
GRAD_RTOL = 5e-11


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


@pytest.mark.parametrize("seed", [4, 5, 6])
def test_pdgp_elbo_and_gradient_chunked_equal_whole_batch(seed):
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, 64, 2, num_partials=3, seed=seed)
    f, g = oracle_elbo_and_grads(prob)
    fc, gc = oracle_elbo_and_grads_chunked(prob, chunk=CHUNK)
    assert abs(fc - f) <= RTOL * abs(f), (fc, f)
    assert sorted(gc) == sorted(g)
    bad = {k: _rel(gc[k], v) for k, v in g.items() if _rel(gc[k], v) > (LS_RTOL if k.endswith("lengthscales") else GRAD_RTOL)}
    assert not bad, bad


def test_pdgp_predictions_chunked_equal_whole_batch():
    from gpitch_amd.synth import make_problem
    from oracle import gpflow05 as orc
    prob = make_problem(N, 64, 2, num_partials=3, seed=5)
    x = prob["x"]
    ref = orc.pdgp_predict_act_n_com(x, prob["za"], prob["zc"], prob["kern_act"], prob["kern_com"], prob["q_mu_act"],
                                     prob["q_sqrt_act"], prob["q_mu_com"], prob["q_sqrt_com"])
    got = oracle_predict_act_n_com_chunked(prob, x, chunk=CHUNK)
    for got_l, ref_l in zip(got, ref):
        assert len(got_l) == len(ref_l) == 2
        for a, b in zip(got_l, ref_l):
            assert a.shape == b.shape == (N, 1)
            assert _rel(a, b) <= RTOL


@pytest.mark.parametrize("reg", [False, True])
def test_sgpr_bound_gradient_and_predictions_chunked_equal_whole_batch(reg):
    from oracle import gpflow05 as orc
    from test_gpu_sgpr import _problem, _torch_bound_and_grads
    X, Y, Z, kl = _problem(N, 96, 2, 9)
    b = orc.sgpr_bound(X, Y, Z, kl, 0.3, reg=reg)
    bc = oracle_sgpr_bound_chunked(X, Y, Z, kl, 0.3, reg=reg, chunk=CHUNK)
    assert abs(bc - b) <= RTOL * abs(b), (bc, b)
    bt, g = _torch_bound_and_grads(X, Y, Z, kl, 0.3, reg=reg)
    btc, gc = oracle_sgpr_bound_and_grads_chunked(X, Y, Z, kl, 0.3, reg=reg, chunk=CHUNK)
    assert abs(btc - bt) <= RTOL * abs(bt), (btc, bt)
    assert gc.shape == g.shape
    ls = np.zeros(g.shape, dtype=bool)
    o = 1
    for d in kl:                              # [noise, then per kernel: variance, lengthscales, energies, frequencies]
        ls[o + 1] = True
        o += 2 + len(d["energy"]) + len(d["frequency"])
    assert o == g.size
    assert np.all(np.abs(gc - g)[ls] <= LS_RTOL * np.abs(g[ls])), (gc, g)
    assert np.abs(gc - g)[~ls].max() <= GRAD_RTOL * np.abs(g[~ls]).max(), (gc, g)
    Xs = X[::3] + 1e-5
    m, v = orc.sgpr_predict_f(Xs, X, Y, Z, kl, 0.3)
    mc, vc = oracle_sgpr_predict_f_chunked(Xs, X, Y, Z, kl, 0.3, chunk=CHUNK)
    assert mc.shape == m.shape and vc.shape == v.shape
    assert _rel(mc, m) <= RTOL and _rel(vc, v) <= RTOL
