"""optimize_many / PdgpBatch.optimize with a NatGradAdam token that carries a length per role or a halving budget
(gp_pdgpb_natgrad_adaptive: pdgpb_ng_form_adaptive_kernel and pdgpb_ng_apply_adaptive_kernel, csrc/pdgp_batch.hip):
nothing to halve against the plain token's call bit for bit; a length per role and the halving family against the same models
trained one at a time by Pdgp.optimize (whose own step tests/test_gpu_natgrad_adaptive.py holds against the restatement); a
halving and an exhausted model between two ordinary ones; the counters per model; the entry's own checks.

Bars as tests/test_gpu_pdgp_batch_natgrad.py states them: the 1e-8 rule on variational Params, 1e-9 relative on the others,
equality where two runs of the same kernels are compared.  The batched entry evaluates its own gradient, so a halving is
planted by the data: natgrad_adaptive_ref.sized_halving_problem puts the halving family's recipe on 33 / 65 and 128 / 127
inducing points (one row past a 32-row block and past the size of the LDS-resident factorisation; the size limit, where the LDS
block is full and B is formed again over the factor), at noise levels that ask for 1, 2 and 3 halvings with margins checked on
the host."""
import copy

import numpy as np
import pytest

import natgrad_adaptive_ref as nga
import natgrad_ref as ng
import pdgp_sample_ref as psr
from helpers import pdgp_from_problem

pytestmark = pytest.mark.gpu


def _qkeys(m):
    return [p for lst in (m.q_mu_act, m.q_mu_com, m.q_sqrt_act, m.q_sqrt_com) for p in lst]


def _hkeys(m):
    ps = [m.likelihood.variance]
    for k in list(m.kern_act) + list(m.kern_com):
        ps += k.theta_params()
    return ps + list(m.za) + list(m.zc)


def _rule(a, b):
    return np.abs(a - b).max() <= 1e-8 * max(np.abs(b).max(), 1e-3)


def _state(m):
    """everything a call may change in a model, as comparable values"""
    mom = m._adam_state()
    return dict(params=[p.value.copy() for p in _hkeys(m) + _qkeys(m)],
                mom=None if mom is None else [(a.copy(), b.copy()) for a, b in mom], t=m._adam_t,
                rng=(str(m.x.rng.get_state()), str(m.y.rng.get_state())))


def _assert_same_state(a, b):
    assert a["t"] == b["t"] and a["rng"] == b["rng"]
    for u, v in zip(a["params"], b["params"]):
        np.testing.assert_array_equal(u, v)
    assert (a["mom"] is None) == (b["mom"] is None)
    for (um, uv), (vm, vv) in zip(a["mom"] or [], b["mom"] or []):
        np.testing.assert_array_equal(um, vm)
        np.testing.assert_array_equal(uv, vv)


def _assert_trained_alike(models, twins, t):
    for k, (m, tw) in enumerate(zip(models, twins)):
        for a, b in zip(_qkeys(m), _qkeys(tw)):
            assert _rule(a.value, b.value), (k, np.abs(a.value - b.value).max())
        for a, b in zip(_hkeys(m), _hkeys(tw)):
            np.testing.assert_allclose(a.value, b.value, rtol=1e-9, atol=0)
        assert str(m.x.rng.get_state()) == str(tw.x.rng.get_state())
        assert m._adam_t == tw._adam_t == t


def _z_fixed(m):
    """(z free amplifies the rounding difference between the batch's and the single-model path's gradient kernels under Adam
    whatever the token: tests/test_gpu_pdgp_batch_natgrad.py)"""
    m.za.fixed = True
    m.zc.fixed = True
    return m


def _sized_models():
    """M from 5 to 128: 5 / 6 (66 latent GPs), 12 / 10, 50 / 64, 33 / 65 and 128 / 127 (on a minibatch of 256 of its 2990 frames)"""
    probs = [(ng.shape_problem("many"), None), (psr.shape_problem(0)[0], None), (psr.shape_problem(1)[0], None),
             (ng.shape_problem("extra"), None), (psr.problem(128, 127, 1, 2, 2990, seed=160), 256)]
    return [_z_fixed(pdgp_from_problem(p, minibatch_size=mb)) for p, mb in probs]


# ---- 1. nothing to halve is nothing changed ------------------------------------------------------------------------------------
def test_nothing_to_halve_is_bit_identical_to_the_plain_tokens_call(gp_handle):
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    a = _sized_models()
    b = copy.deepcopy(a)
    ra = optimize_many(a, method=NatGradAdam(0.1, 0.01), maxiter=3)
    rb = optimize_many(b, method=NatGradAdam(0.1, 0.01, halvings=4), maxiter=3)
    for m, n, x, y in zip(a, b, ra, rb):
        assert x.success and y.success
        _assert_same_state(_state(m), _state(n))
        np.testing.assert_array_equal(x.x, y.x)
        np.testing.assert_array_equal(x.jac, y.jac)
        assert x.fun == y.fun and "natgrad" not in x
        G = 2 * m.num_sources
        assert y.natgrad == {"halvings": [0] * G, "shortest_gamma": [0.1] * G}


# ---- 2. a length per role, against the models trained one at a time ---------------------------------------------------------------
def test_a_length_per_role_matches_the_models_trained_one_at_a_time(gp_handle):
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    tok = NatGradAdam(0.1, 0.0025, gamma_com=1.0)
    models = _sized_models()
    twins = copy.deepcopy(models)
    plain = copy.deepcopy(models[1])
    res = optimize_many(models, method=tok, maxiter=2)
    single = [tw.optimize(method=tok, maxiter=2) for tw in twins]
    assert all(r.success for r in res), [r.message for r in res]
    _assert_trained_alike(models, twins, 2)
    for m, r, s in zip(models, res, single):
        P = m.num_sources
        assert r.natgrad == s.natgrad == {"halvings": [0] * (2 * P), "shortest_gamma": [0.1] * P + [1.0] * P}
    plain.optimize(method=NatGradAdam(0.1, 0.0025), maxiter=2)      # (the components' own length made a difference)
    assert np.abs(plain.q_mu_com[0].value - models[1].q_mu_com[0].value).max() > 1e-4


# ---- 3. halving, against the models trained one at a time -----------------------------------------------------------------------
def test_halving_matches_the_models_trained_one_at_a_time(gp_handle):
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    tok = NatGradAdam(1.0, 1e-6, halvings=4)
    models = [pdgp_from_problem(nga.halving_problem(nv)) for nv, _, _ in nga.HALVING_TABLE]
    models.insert(1, pdgp_from_problem(ng.shape_problem(0)))
    want = [j for _, _, j in nga.HALVING_TABLE]
    want.insert(1, 0)
    twins = copy.deepcopy(models)
    res = optimize_many(models, method=tok, maxiter=1)
    single = [tw.optimize(method=tok, maxiter=1) for tw in twins]
    assert all(r.success for r in res), [r.message for r in res]
    _assert_trained_alike(models, twins, 1)
    for r, s, j in zip(res, single, want):
        assert r.natgrad == s.natgrad == {"halvings": [j, 0], "shortest_gamma": [2.0 ** -j, 1.0]}
    # a second call starts its counters from zero and from the full length
    again = optimize_many([models[1]], method=tok, maxiter=1)
    assert again[0].success and again[0].natgrad["halvings"][1] == 0 and again[0].natgrad["shortest_gamma"][1] == 1.0


# ---- 4. a halving and an exhausted model between two ordinary ones ------------------------------------------------------------------
def test_an_exhausted_model_is_refused_alone(gp_handle):
    """noise 6e-6 needs two halvings from gamma = 1 and noise 1e-6 four, with three allowed.  A numerical refusal through the
    model's refusal word: nothing here faults the device."""
    from gpitch_amd import _lib
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    tok = NatGradAdam(1.0, 0.01, halvings=3)
    a = [pdgp_from_problem(p) for p in (ng.shape_problem(0), nga.halving_problem(6e-6), nga.halving_problem(1e-6),
                                        ng.shape_problem(1))]
    b = copy.deepcopy([a[0], a[3]])
    halving_twin = copy.deepcopy(a[1])
    before = _state(a[2])
    res = optimize_many(a, method=tok, maxiter=1)
    ref = optimize_many(b, method=tok, maxiter=1)
    assert not res[2].success and isinstance(res[2].error, _lib.NotPositiveDefiniteError)
    msg = str(res[2].error)
    assert "NatGradAdam" in msg and "model 2" in msg and "activation GP 0" in msg and "gamma = 0.125" in msg, msg
    assert "halvings = 3" in msg and "too long" in msg and "more halvings" in msg and res[2].message in msg
    _assert_same_state(_state(a[2]), before)
    assert res[2].natgrad == {"halvings": [0, 0], "shortest_gamma": [1.0, 1.0]}
    for r, q, m, n in zip([res[0], res[3]], ref, [a[0], a[3]], b):
        assert r.success and q.success
        np.testing.assert_array_equal(r.x, q.x)
        np.testing.assert_array_equal(r.jac, q.jac)
        assert r.fun == q.fun and r.natgrad == q.natgrad
        _assert_same_state(_state(m), _state(n))
        G = 2 * m.num_sources
        assert r.natgrad == {"halvings": [0] * G, "shortest_gamma": [1.0] * G}
    assert res[1].success and res[1].natgrad == {"halvings": [2, 0], "shortest_gamma": [0.25, 1.0]}
    # (its q against the same model trained alone; the other Params are compared in the test above, at a learning rate that
    # does not take an inducing input of 0.01 to 0.01 - 0.01, where a relative bar has nothing to hold on to)
    halving_twin.optimize(method=tok, maxiter=1)
    for p, q in zip(_qkeys(a[1]), _qkeys(halving_twin)):
        assert _rule(p.value, q.value)
    again = optimize_many([a[2]], method=NatGradAdam(1.0, 0.01, halvings=4), maxiter=1)
    assert again[0].success and again[0].natgrad == {"halvings": [4, 0], "shortest_gamma": [2.0 ** -4, 1.0]}
    assert a[2]._adam_t == 1


# ---- 5. halving GPs at the tile edges, an ordinary model beside them ---------------------------------------------------------------
def test_halving_at_the_tile_edges_beside_an_ordinary_model(gp_handle):
    """The form kernel's loop at M = 33 / 65 and 128 / 127 with j = 1, 3, 2, 3, the last two in the last round the budget allows.
    The margins of the deciding eigenvalues are checked on the host from a single-model twin's device gradient; the twin's own
    step is held against adaptive_step of that gradient, and the batch against the twin."""
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    from helpers import model_grad_dict
    tok = NatGradAdam(1.0, 1e-6, halvings=3)
    probs = [nga.sized_halving_problem(*row[:5]) for row in nga.SIZED_HALVING_TABLE]
    want = [row[5] for row in nga.SIZED_HALVING_TABLE]
    probs.insert(2, ng.shape_problem(1))                   # the ordinary model: 50 / 64, P = 3, between them
    want.insert(2, None)
    models = [pdgp_from_problem(p) for p in probs]
    twins = copy.deepcopy(models)
    alone = copy.deepcopy([models[2]])
    for prob, j, probe in zip(probs, want, copy.deepcopy(models)):
        if j is None:
            continue
        probe._pack()
        probe._elbo(True)
        grads = model_grad_dict(probe)
        refused, accepted = nga.deciding_eigenvalues(prob["q_sqrt_act"][0], grads["q_sqrt_act0"], j)
        print("M = %d / %d, noise %g: smallest eigenvalue of B %.3f at 2^-%d, %.3f at 2^-%d (device gradient)"
              % (prob["q_mu_act"][0].size, prob["q_mu_com"][0].size, prob["noise_var"], refused, j - 1, accepted, j))
        assert refused <= -nga.EDGE_MARGIN and accepted >= nga.EDGE_MARGIN
        assert nga.deciding_eigenvalues(prob["q_sqrt_com"][0], grads["q_sqrt_com0"], 0)[1] >= nga.EDGE_MARGIN
        stepped, js = nga.step_problem_adaptive(prob, grads, 1.0, None, 3)
        assert js == [j, 0]
        probe.optimize(method=tok, maxiter=1)
        got = dict(prob, q_mu_act=[q.value for q in probe.q_mu_act], q_mu_com=[q.value for q in probe.q_mu_com],
                   q_sqrt_act=[q.value for q in probe.q_sqrt_act], q_sqrt_com=[q.value for q in probe.q_sqrt_com])
        assert ng.q_distance(got, stepped) <= 1e-8
    res = optimize_many(models, method=tok, maxiter=1)
    single = [tw.optimize(method=tok, maxiter=1) for tw in twins]
    ref = optimize_many(alone, method=tok, maxiter=1)
    assert all(r.success for r in res), [r.message for r in res]
    _assert_trained_alike(models, twins, 1)
    for r, s, j in zip(res, single, want):
        assert r.natgrad == s.natgrad
        if j is not None:
            assert r.natgrad == {"halvings": [j, 0], "shortest_gamma": [2.0 ** -j, 1.0]}
    # the ordinary model: as in a call without the halving ones, bit for bit
    assert res[2].natgrad == ref[0].natgrad == {"halvings": [0] * 6, "shortest_gamma": [1.0] * 6}
    _assert_same_state(_state(models[2]), _state(alone[0]))
    np.testing.assert_array_equal(res[2].x, ref[0].x)
    assert res[2].fun == ref[0].fun


# ---- 6. the entry's own checks ---------------------------------------------------------------------------------------------------
def test_the_entry_checks_its_arguments(gp_handle):
    import ctypes as C
    from gpitch_amd import _lib
    from gpitch_amd.pdgp_batch import PdgpBatch, _predict_plan, draw_indices
    m = pdgp_from_problem(ng.shape_problem(0))
    batch = PdgpBatch([m])
    h = batch._handle
    batch._pack()
    nbytes = h.lib.gp_pdgpb_natgrad_adaptive_workspace_bytes(batch._plan)
    assert nbytes > h.lib.gp_pdgpb_natgrad_workspace_bytes(batch._plan) and nbytes % 256 == 0
    ws = h.workspace(nbytes + 256)
    idx = h.torch.as_tensor(batch._indices([draw_indices(m, 1)])).to(h.device)
    lr = h.torch.as_tensor(np.array([0.01])).to(h.device)
    before = batch._params.cpu().numpy().copy()

    def call(gammas=(0.5, 0.5), halvings=2, ptr=ws.data_ptr(), size=nbytes, plan=None, flags=None, steps=1):
        fl = None if flags is None else (C.c_int32 * len(flags))(*flags)
        gm = None if gammas is None else (C.c_double * len(gammas))(*gammas)
        return h.lib.gp_pdgpb_natgrad_adaptive(plan or batch._plan, batch._free.data_ptr(), batch._params.data_ptr(),
                                               batch._tcode.data_ptr(), batch._adam_m.data_ptr(), batch._adam_v.data_ptr(),
                                               batch._x.data_ptr(), batch._y.data_ptr(), idx.data_ptr(), steps, lr.data_ptr(), 0.9,
                                               0.999, 1e-8, gm, halvings, fl, ptr, size)
    for bad in ((0.0, 0.5), (0.5, 1.0000001), (float("nan"), 0.5), None):
        assert call(gammas=bad) == _lib.GP_ERR_BAD_ARG
    assert call(halvings=-1) == _lib.GP_ERR_BAD_ARG and call(halvings=11) == _lib.GP_ERR_BAD_ARG
    assert call(ptr=None) == _lib.GP_ERR_BAD_ARG
    assert call(size=nbytes - 1) == _lib.GP_ERR_WORKSPACE
    assert call(ptr=ws.data_ptr() + 8) == _lib.GP_ERR_BAD_ARG
    with _predict_plan(h, [m]) as pred:
        assert h.lib.gp_pdgpb_natgrad_adaptive_workspace_bytes(pred) == 0
        assert call(plan=pred) == _lib.GP_ERR_BAD_ARG
    hv, sg = (C.c_int64 * 2)(), (C.c_double * 2)()
    assert h.lib.gp_pdgpb_natgrad_counts(batch._plan, hv, sg, 0) == _lib.GP_ERR_WORKSPACE     # no call has been taken yet
    h.sync()
    assert np.array_equal(batch._params.cpu().numpy(), before) and not batch.not_pd().any()
    assert call(steps=0) == _lib.GP_OK
    assert call(flags=[0, 1], halvings=10) == _lib.GP_OK
    assert h.lib.gp_pdgpb_natgrad_counts(batch._plan, hv, None, 0) == _lib.GP_ERR_BAD_ARG
    assert h.lib.gp_pdgpb_natgrad_counts(batch._plan, hv, sg, 1) == _lib.GP_OK
    assert list(hv) == [0, 0] and list(sg) == [float("inf"), 0.5]      # (GP 0 was not flagged: no step since the reset)
    out = (C.c_int32 * 1)()
    assert h.lib.gp_pdgpb_natgrad_refused(batch._plan, out, 1) == _lib.GP_OK and out[0] == 0
    assert not batch.not_pd().any()
    assert not np.array_equal(batch._params.cpu().numpy(), before)
