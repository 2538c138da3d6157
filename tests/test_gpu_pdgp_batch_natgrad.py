"""optimize_many / PdgpBatch.optimize with a NatGradAdam token on the device (csrc/pdgp_batch.hip pdgpb_ng_form_kernel and
pdgpb_ng_apply_kernel through gp_pdgpb_natgrad) against the numpy restatement of tests/natgrad_ref.py, against the same models
trained one at a time by Pdgp.optimize, and against the Adam path of the batch.

Full batch (minibatch_size = N) unless stated, so an iteration is deterministic.  The batch takes at most 1024 frames per
model and step, so the one problem with N = 2990 runs on a minibatch of 256: its twin (a deep copy, the same generator
state) draws the same frames for the gradient that drives the restatement.  Bars: the project's 1e-8 rule
(|a - b| <= 1e-8 max(|b|, 1e-3)) on variational Params, 1e-9 relative on the others after a few iterations (the bar of
tests/test_gpu_pdgp_batch.py's comparison after 3 steps), equality where two runs of the same kernels are compared."""
import copy

import numpy as np
import pytest

import natgrad_ref as ng
import pdgp_sample_ref as psr
from helpers import pdgp_from_problem

pytestmark = pytest.mark.gpu

Q_NAMES = ("q_mu_act", "q_mu_com", "q_sqrt_act", "q_sqrt_com")


def _fix_all_but_q(m):
    m.likelihood.variance.fixed = True
    m.za.fixed = True
    m.zc.fixed = True
    for k in list(m.kern_act) + list(m.kern_com):
        for p in k.theta_params():
            p.fixed = True


def _q_params(m, r):
    """(q_mu, q_sqrt) of row r of [g_0..g_{P-1}, f_0..f_{P-1}]"""
    P = m.num_sources
    return (m.q_mu_act[r], m.q_sqrt_act[r]) if r < P else (m.q_mu_com[r - P], m.q_sqrt_com[r - P])


def _fix_q(m, rows):
    for r in rows:
        for p in _q_params(m, r):
            p.fixed = True


def _qkeys(m):
    return [p for lst in (m.q_mu_act, m.q_mu_com, m.q_sqrt_act, m.q_sqrt_com) for p in lst]


def _hkeys(m):
    ps = [m.likelihood.variance]
    for k in list(m.kern_act) + list(m.kern_com):
        ps += k.theta_params()
    return ps + list(m.za) + list(m.zc)


def _model_q(m):
    return dict(q_mu_act=[q.value for q in m.q_mu_act], q_mu_com=[q.value for q in m.q_mu_com],
                q_sqrt_act=[q.value for q in m.q_sqrt_act], q_sqrt_com=[q.value for q in m.q_sqrt_com])


def _rule(a, b):
    return np.abs(a - b).max() <= 1e-8 * max(np.abs(b).max(), 1e-3)


def _assert_q(m, want, tag):
    """every variational Param against `want` by the 1e-8 rule; the stored strict upper triangle bit for bit"""
    got = _model_q(m)
    for k in Q_NAMES:
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.shape == b.shape
            assert _rule(a, b), (tag, k, i, np.abs(a - b).max())
            if k.startswith("q_sqrt"):
                iu = np.triu_indices(a.shape[0], 1)
                assert np.array_equal(a[:, :, 0][iu], b[:, :, 0][iu]), (tag, k, i)


def _with_upper_junk(prob):
    """the stored strict upper triangle of q_sqrt carries no gradient and matrix_band_part ignores it: fill it"""
    out = dict(prob)
    for k in ("q_sqrt_act", "q_sqrt_com"):
        out[k] = []
        for a in prob[k]:
            a = a.copy()
            a[:, :, 0][np.triu_indices(a.shape[0], 1)] = 0.37
            out[k].append(a)
    return out


def _batch_grads(models):
    """the batch's own device gradient of the variational Params at the models' present state, on the minibatch each
    model's next iteration draws (the models are consumed: hand over twins): one dict per model, keyed as
    natgrad_ref.variational_names"""
    from gpitch_amd.pdgp_batch import PdgpBatch, draw_indices, model_segments
    batch = PdgpBatch(models)
    batch._pack()
    _, grad = batch._evaluate([draw_indices(m, 1) for m in models])
    assert not batch.not_pd().any()
    out = []
    for k, m in enumerate(models):
        segs, _ = model_segments(m, batch._range[k][0])
        at = {id(p): off for off, p in segs}
        d = {}
        for r, (nm, ns) in enumerate(ng.variational_names(m.num_sources)):
            mu, sq = _q_params(m, r)
            M = mu.size
            d[nm] = grad[at[id(mu)]:at[id(mu)] + M].reshape(M, 1).copy()
            d[ns] = grad[at[id(sq)]:at[id(sq)] + M * M].reshape(M, M, 1).copy()
        out.append(d)
    return out


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


# ---- 1. one step against the restatement ---------------------------------------------------------------------------------------
# Tile edges of the kernels as written.  pdgpb_ng_form_kernel forms B over 16 x 16 sub-tiles of the lower triangle, dealt to
# four wavefronts in turn, with a k loop in steps of 4 from the sub-tile's first row; pdgpb_ng_apply_kernel takes blocks of 32
# rows made of 16 x 16 sub-tiles.  The issue's problems give M = 12 / 10 and 5 / 6 (below one sub-tile, a k loop that ends
# inside a group of 4), 16 / 17 (a whole sub-tile; one row past it), 33 (one row past a 32-row block), 50 (a last block of
# 18 rows), 64 / 65, 127 / 128 (the size limit and one row short of it: 36 sub-tiles, nine per wavefront) and 66 latent GPs in one
# model.  Added: 32 / 48 (exactly one block; a last block whose second sub-tile row is empty) and 97 / 112 (one row past six
# sub-tiles, 25 sub-tiles: an uneven deal; seven sub-tiles, a half-empty last block).
def _step_problems():
    return [(psr.shape_problem(0)[0], None), (psr.shape_problem(1)[0], None), (ng.shape_problem("extra"), None),
            (ng.shape_problem("many"), None), (psr.problem(128, 127, 1, 2, 2990, seed=160), 256),
            (psr.problem(16, 17, 1, 2, 512, seed=161), None), (psr.problem(32, 48, 1, 2, 256, seed=162), None),
            (psr.problem(97, 112, 1, 2, 512, seed=163), None)]


_start = {}


def _step_models(probs):
    out = []
    for prob, mb in probs:
        m = pdgp_from_problem(prob, minibatch_size=mb)
        _fix_all_but_q(m)
        out.append(m)
    return out


def _start_state():
    """(problems with a filled upper triangle, the batch's gradient of twins at that state), once"""
    if not _start:
        probs = [(_with_upper_junk(p), mb) for p, mb in _step_problems()]
        _start["probs"] = probs
        _start["grads"] = _batch_grads(_step_models(probs))
    return _start["probs"], _start["grads"]


@pytest.mark.parametrize("gamma", (0.1, 1.0))
def test_one_step_follows_the_restatement(gp_handle, gamma):
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    probs, grads = _start_state()
    models = _step_models(probs)
    res = optimize_many(models, method=NatGradAdam(gamma), maxiter=1)
    for k, (m, (prob, _), g) in enumerate(zip(models, probs, grads)):
        assert res[k].success, (k, res[k].message)
        _assert_q(m, ng.step_problem(prob, g, gamma), (k, gamma))
        moved = max(np.abs(a - b).max() for key in Q_NAMES for a, b in zip(_model_q(m)[key], prob[key]))
        assert moved > 1e-4, k                              # (a step was taken)
        assert m._adam_t == 1


# ---- 2. the same models trained one at a time ----------------------------------------------------------------------------------
def _act(t, ls=0.02, v=3.5):
    return {"type": t, "variance": v, "lengthscales": ls, "energy": [], "frequency": []}


def _mixed_minibatched():
    """a randint-branch model (64 of 700 frames) with z and the kernels free, a permutation-branch model (400 of 600, z
    fixed), and a P = 2 model (100 of 500, z fixed, kernels free) whose first component GP has q_mu and q_sqrt both fixed.

    z of the P = 2 model is fixed because its Adam dynamics amplify the rounding difference between the batch's and the
    single-model path's gradient kernels, whatever the optimiser token: with z free, AdamOptimizer(0.0025) alone — no
    natural-gradient step — leaves the two paths 1.7e-9 apart after 3 iterations and 4.5e-7 after 5 (worst entry of z,
    relative), growing about 10-fold per iteration; NatGradAdam(0.1, 0.0025) 8e-10 and 2.2e-9.  tests/test_gpu_pdgp_batch.py
    describes the same growth for its ragged three-pitch model and also compares it with z fixed.  The P = 1 model keeps z
    free (measured there: 7e-13 after 3 iterations, 5e-11 after 5)."""
    from gpitch_amd.synth import make_problem
    out = []
    p = make_problem(700, 20, 1, num_partials=2, seed=41)
    p["kern_act"][0] = _act("matern32")
    out.append(pdgp_from_problem(p, minibatch_size=64))
    p = make_problem(600, 24, 1, num_partials=4, seed=22)
    p["kern_act"][0] = _act("matern32")
    m = pdgp_from_problem(p, minibatch_size=400)
    m.za.fixed = True
    m.zc.fixed = True
    out.append(m)
    p = make_problem(500, 18, 2, num_partials=3, seed=43)
    p["kern_act"] = [_act("matern32") for _ in range(2)]
    m = pdgp_from_problem(p, minibatch_size=100)
    m.za.fixed = True
    m.zc.fixed = True
    _fix_q(m, [2])
    out.append(m)
    return out


def _assert_trained_alike(models, twins, t):
    for k, (m, tw) in enumerate(zip(models, twins)):
        for a, b in zip(_qkeys(m), _qkeys(tw)):
            assert _rule(a.value, b.value), (k, np.abs(a.value - b.value).max())
        for a, b in zip(_hkeys(m), _hkeys(tw)):
            np.testing.assert_allclose(a.value, b.value, rtol=1e-9, atol=0)
        assert str(m.x.rng.get_state()) == str(tw.x.rng.get_state())
        assert str(m.y.rng.get_state()) == str(tw.y.rng.get_state())
        assert m._adam_t == tw._adam_t == t


def test_matches_the_models_trained_one_at_a_time(gp_handle):
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    tok = NatGradAdam(0.1, 0.0025)
    models = _mixed_minibatched()
    twins = copy.deepcopy(models)
    start = [p.value.copy() for p in _q_params(models[2], 2)]
    res = optimize_many(models, method=tok, maxiter=3)
    for tw in twins:
        tw.optimize(method=tok, maxiter=3)
    assert all(r.success for r in res)
    _assert_trained_alike(models, twins, 3)
    # a second call, resuming from the moments left in the models
    res = optimize_many(models, method=tok, maxiter=2)
    single = [tw.optimize(method=tok, maxiter=2) for tw in twins]
    assert all(r.success for r in res)
    _assert_trained_alike(models, twins, 5)
    for r, s in zip(res, single):
        assert r.x.shape == s.x.shape and abs(r.fun - s.fun) <= 1e-8 * abs(s.fun)
    for p, v in zip(_q_params(models[2], 2), start):       # the skipped GP's q has not been touched
        np.testing.assert_array_equal(p.value, v)
    assert np.abs(models[0].za[0].value - twins[0].za[0].value).max() <= 1e-9 and models[0]._adam_state() is not None


# ---- 3. Adam beside the step ---------------------------------------------------------------------------------------------------
def test_adam_moves_everything_else_exactly_as_on_its_own(gp_handle):
    from gpitch_amd.pdgp_batch import model_segments, optimize_many
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    args = (0.01, 0.8, 0.99, 1e-7)
    models = _mixed_minibatched()
    twins = copy.deepcopy(models)
    optimize_many(models, method=NatGradAdam(0.1, *args), maxiter=1)
    optimize_many(twins, method=AdamOptimizer(*args), maxiter=1)
    for m, tw in zip(models, twins):
        for a, b in zip(_hkeys(m), _hkeys(tw)):
            np.testing.assert_array_equal(a.value, b.value)
        stepped = {id(p) for r, f in enumerate(m._natgrad_gps(NatGradAdam())) if f for p in _q_params(m, r)}
        order = [p for _, p in model_segments(m)[0]]
        seen = 0
        for p, (mm, mv), (tm, tv) in zip(order, m._adam_state(), tw._adam_state()):
            if id(p) in stepped:
                assert not np.any(mm) and not np.any(mv)      # exactly 0: Adam saw a zero gradient there
                seen += 1
            else:
                np.testing.assert_array_equal(mm, tm)
                np.testing.assert_array_equal(mv, tv)
        assert seen == len(stepped) > 0
        moved = max(np.abs(a.value - b.value).max() for a, b in zip(_qkeys(m), _qkeys(tw)))
        assert moved > 1e-6                                   # (and the step is not Adam's)


def test_with_every_q_fixed_it_is_the_adam_path_bit_for_bit(gp_handle):
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    models = _mixed_minibatched()
    for m in models:
        _fix_q(m, range(2 * m.num_sources))
    twins = copy.deepcopy(models)
    ra = optimize_many(models, method=NatGradAdam(0.3, 0.01), maxiter=5)
    rb = optimize_many(twins, method=AdamOptimizer(0.01), maxiter=5)
    for m, tw, a, b in zip(models, twins, ra, rb):
        _assert_same_state(_state(m), _state(tw))
        assert m._adam_t == 5 and a.fun == b.fun
        np.testing.assert_array_equal(a.x, b.x)
        np.testing.assert_array_equal(a.jac, b.jac)


# ---- 4. known answer -----------------------------------------------------------------------------------------------------------
def test_one_step_of_length_one_lands_on_the_optimal_component_posterior(gp_handle):
    """natgrad_ref.conjugate_problem(1) and (2) in one batch.  With everything but ONE component GP's q(u) fixed the data
    term is linear in that GP's expectation parameters, and one step of length 1 is the maximiser; two free component GPs
    of one model are coupled by the product term of the residual, so P = 2 frees its second component GP only, as
    tests/test_gpu_natgrad.py does.  The gradient ratio is printed, not asserted: the batch's gradient kernels round
    differently from the path natgrad_ref.CONJ_GRAD_BAR was derived for.
    Measured on MI355X: see DESIGN.md 3j."""
    from gpitch_amd.pdgp_batch import PdgpBatch, optimize_many
    from gpitch_amd.train import AdamOptimizer, NatGradAdam

    def build():
        out = []
        for P in (1, 2):
            m = pdgp_from_problem(ng.conjugate_problem(P))
            _fix_all_but_q(m)
            _fix_q(m, [r for r in range(2 * P) if r != 2 * P - 1])
            out.append(m)
        return out
    before = [np.linalg.norm(j) for _, j in PdgpBatch(build()).objective_many()]
    models = build()
    tok = NatGradAdam(1.0)
    res = optimize_many(models, method=tok, maxiter=1)
    assert all(r.success for r in res)
    q1 = [_model_q(m) for m in models]
    res2 = optimize_many(models, method=tok, maxiter=1)
    assert all(r.success for r in res2)
    twins = build()
    ra = optimize_many(twins, method=AdamOptimizer(0.01), maxiter=50)
    for k, m in enumerate(models):
        print("P = %d: gradient of the stepped GP after / before the step %.2e" % (k + 1, np.linalg.norm(res[k].jac) / before[k]))
        print("P = %d: ELBO after one natural-gradient step %.9f, after 50 Adam(0.01) iterations %.9f"
              % (k + 1, -res[k].fun, -ra[k].fun))
        q2 = _model_q(m)
        for key in Q_NAMES:
            for a, b in zip(q2[key], q1[k][key]):
                assert _rule(a, b), (k, key, np.abs(a - b).max())
        assert -res[k].fun > -ra[k].fun


# ---- 5. refusal ----------------------------------------------------------------------------------------------------------------
def test_a_step_that_is_too_long_is_refused_for_that_model_alone(gp_handle):
    """natgrad_ref.refusal_problem(): B of the activation GP has a negative eigenvalue at gamma = 1 (shown on the CPU in
    test_natgrad_cpu.py).  A numerical refusal through the model's refusal word: nothing here faults the device."""
    from gpitch_amd import _lib
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    tok = NatGradAdam(ng.REFUSAL_GAMMA, 0.01)
    a = [pdgp_from_problem(p) for p in (ng.shape_problem(0), ng.refusal_problem(), ng.shape_problem(1))]
    b = copy.deepcopy([a[0], a[2]])
    before = _state(a[1])
    res = optimize_many(a, method=tok, maxiter=2)
    ref = optimize_many(b, method=tok, maxiter=2)
    assert not res[1].success and isinstance(res[1].error, _lib.NotPositiveDefiniteError)
    msg = str(res[1].error)
    assert "NatGradAdam" in msg and "model 1" in msg and "activation GP 0" in msg and "gamma = 1" in msg, msg
    assert "too long" in msg and "smaller gamma" in msg and res[1].message in msg
    _assert_same_state(_state(a[1]), before)
    for r, q, m, n in zip([res[0], res[2]], ref, [a[0], a[2]], b):
        assert r.success == q.success
        if r.success:
            np.testing.assert_array_equal(r.x, q.x)
            np.testing.assert_array_equal(r.jac, q.jac)
            assert r.fun == q.fun
        _assert_same_state(_state(m), _state(n))
    assert res[0].success and res[2].success
    again = optimize_many([a[1]], method=NatGradAdam(ng.REFUSAL_SMALL_GAMMA, 0.01), maxiter=2)
    assert again[0].success and np.isfinite(again[0].fun) and a[1]._adam_t == 2
    assert np.abs(a[1].q_mu_act[0].value - before["params"][-4]).max() > 0


def test_a_failed_kuu_is_reported_as_that_not_as_a_refused_step(gp_handle):
    from gpitch_amd import _lib
    from gpitch_amd.param import transforms
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    models = _mixed_minibatched()
    bad = copy.deepcopy(models[0])
    bad.kern_act[0].variance.transform = transforms.Identity()
    bad.kern_act[0].variance = -1.0
    before = _state(bad)
    res = optimize_many([models[0], bad, models[1]], method=NatGradAdam(0.1, 0.01), maxiter=3)
    assert res[0].success and res[2].success
    assert not res[1].success and isinstance(res[1].error, _lib.NotPositiveDefiniteError)
    assert res[1].message.startswith("Cholesky failed") and "NatGradAdam" not in res[1].message
    _assert_same_state(_state(bad), before)


# ---- 6. bit-identical runs -----------------------------------------------------------------------------------------------------
def test_two_identical_runs_are_bit_identical(gp_handle):
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.train import NatGradAdam
    tok = NatGradAdam(0.1, 0.01)
    a = _mixed_minibatched()
    b = copy.deepcopy(a)
    ra = optimize_many(a, method=tok, maxiter=25)
    rb = optimize_many(b, method=tok, maxiter=25)
    for x, y in zip(ra, rb):
        assert x.success and y.success
        np.testing.assert_array_equal(x.x, y.x)
        np.testing.assert_array_equal(x.jac, y.jac)
        assert x.fun == y.fun


# ---- 7. the entry's own checks -------------------------------------------------------------------------------------------------
def test_the_entry_checks_its_arguments(gp_handle):
    """gp_pdgpb_natgrad: a step length outside (0, 1], a null, short or misaligned workspace and a prediction-only plan are
    refused before anything is enqueued: parameters, Kuu words and refusal words stay as they were"""
    import ctypes as C
    from gpitch_amd import _lib
    from gpitch_amd.pdgp_batch import PdgpBatch, _predict_plan, draw_indices
    m = pdgp_from_problem(ng.shape_problem(0))
    batch = PdgpBatch([m])
    h = batch._handle
    batch._pack()
    nbytes = h.lib.gp_pdgpb_natgrad_workspace_bytes(batch._plan)
    assert nbytes >= 8 * sum(M * M + M for M in (12, 10)) and nbytes % 256 == 0
    ws = h.workspace(nbytes + 256)
    idx = h.torch.as_tensor(batch._indices([draw_indices(m, 1)])).to(h.device)
    lr = h.torch.as_tensor(np.array([0.01])).to(h.device)
    before = batch._params.cpu().numpy().copy()

    def call(gamma, ptr=ws.data_ptr(), size=nbytes, plan=None, flags=None, steps=1):
        fl = None if flags is None else (C.c_int32 * len(flags))(*flags)
        return h.lib.gp_pdgpb_natgrad(plan or batch._plan, batch._free.data_ptr(), batch._params.data_ptr(),
                                      batch._tcode.data_ptr(), batch._adam_m.data_ptr(), batch._adam_v.data_ptr(),
                                      batch._x.data_ptr(), batch._y.data_ptr(), idx.data_ptr(), steps, lr.data_ptr(), 0.9, 0.999,
                                      1e-8, gamma, fl, ptr, size)
    for gamma in (0.0, 1.0000001, float("nan")):
        assert call(gamma) == _lib.GP_ERR_BAD_ARG
    assert call(0.5, ptr=None) == _lib.GP_ERR_BAD_ARG
    assert call(0.5, size=nbytes - 1) == _lib.GP_ERR_WORKSPACE
    assert call(0.5, ptr=ws.data_ptr() + 8) == _lib.GP_ERR_BAD_ARG
    with _predict_plan(h, [m]) as pred:
        assert h.lib.gp_pdgpb_natgrad_workspace_bytes(pred) == 0
        assert call(0.5, plan=pred) == _lib.GP_ERR_BAD_ARG
    out = (C.c_int32 * 1)()
    assert h.lib.gp_pdgpb_natgrad_refused(batch._plan, out, 0) == _lib.GP_ERR_WORKSPACE     # no call has been taken yet
    h.sync()
    assert np.array_equal(batch._params.cpu().numpy(), before) and not batch.not_pd().any()
    # no iteration, and an iteration with no latent GP flagged (an Adam step): both taken, no model refused
    assert call(0.5, steps=0) == _lib.GP_OK
    assert call(0.5, flags=[0, 0]) == _lib.GP_OK
    assert h.lib.gp_pdgpb_natgrad_refused(batch._plan, out, 1) == _lib.GP_OK and out[0] == 0
    assert not batch.not_pd().any()
    assert not np.array_equal(batch._params.cpu().numpy(), before)


# ---- 8. afterwards -------------------------------------------------------------------------------------------------------------
def test_trained_model_predicts_like_a_fresh_model(gp_handle):
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.synth import make_problem
    from gpitch_amd.train import NatGradAdam
    p = make_problem(800, 32, 1, num_partials=3, seed=31)
    p["kern_act"][0] = _act("matern32")
    m = pdgp_from_problem(p, minibatch_size=100)
    xt = np.linspace(0., 799. / 16000., 333).reshape(-1, 1)
    before = m.predict_act_n_com(xt)                       # memoised state that must not survive the training
    res = optimize_many([m], method=NatGradAdam(0.2, 0.01), maxiter=4)
    assert res[0].success
    fresh = copy.deepcopy(p)
    fresh["za"] = [m.za[0].value]; fresh["zc"] = [m.zc[0].value]
    fresh["q_mu_act"] = [m.q_mu_act[0].value]; fresh["q_mu_com"] = [m.q_mu_com[0].value]
    fresh["q_sqrt_act"] = [m.q_sqrt_act[0].value]; fresh["q_sqrt_com"] = [m.q_sqrt_com[0].value]
    f = pdgp_from_problem(fresh)
    for kf, km in ((f.kern_act[0], m.kern_act[0]), (f.kern_com[0], m.kern_com[0])):
        for a, b in zip(kf.theta_params(), km.theta_params()):
            a.value = b.value
    f.likelihood.variance = m.likelihood.variance.value
    got, ref = m.predict_act_n_com(xt), f.predict_act_n_com(xt)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a[0], b[0])
    assert not np.array_equal(got[0][0], before[0][0])
