"""Pdgp.optimize(method=NatGradAdam(...)) on the device (csrc/natgrad.hip through gp_pdgp_natgrad_step) against the numpy
restatement of tests/natgrad_ref.py: the three launches alone at every tile boundary, the conjugate known answer, Adam
beside the step, three iterations end to end, the refusal of a step that is too long, and the loop's bookkeeping.
Full batch (minibatch_size = N) unless stated, so an iteration is deterministic.  The bars that are not the project's 1e-8
rule are derived in tests/test_natgrad_cpu.py and written into natgrad_ref.py."""
import numpy as np
import pytest

import natgrad_ref as ng
from helpers import model_grad_dict, oracle_elbo_and_grads

pytestmark = pytest.mark.gpu

Q_NAMES = ("q_mu_act", "q_mu_com", "q_sqrt_act", "q_sqrt_com")


def _model(prob, gp_handle, whiten=True, **kw):
    from gpitch_amd.synth import pdgp_from_problem
    return pdgp_from_problem(prob, whiten=whiten, handle=gp_handle, **kw)


def _fix_all_but_q(m):
    m.likelihood.variance.fixed = True
    m.za.fixed = True
    m.zc.fixed = True
    for k in list(m.kern_act) + list(m.kern_com):
        for p in k.theta_params():
            p.fixed = True


def _fix_q(m, rows):
    """fix q(u) of the latent GPs `rows` of [g_0..g_{P-1}, f_0..f_{P-1}]"""
    P = m.num_sources
    for r in rows:
        mu, sq = (m.q_mu_act[r], m.q_sqrt_act[r]) if r < P else (m.q_mu_com[r - P], m.q_sqrt_com[r - P])
        mu.fixed = True
        sq.fixed = True


def _device_grads(m):
    """the device gradient at the model's present state (what one iteration's evaluation sees at full batch)"""
    m._pack()
    m._elbo(True)
    return model_grad_dict(m)


def _model_q(m):
    return dict(q_mu_act=[q.value for q in m.q_mu_act], q_mu_com=[q.value for q in m.q_mu_com],
                q_sqrt_act=[q.value for q in m.q_sqrt_act], q_sqrt_com=[q.value for q in m.q_sqrt_com])


def _assert_q(m, want, tag):
    """every variational Param against the restatement by the 1e-8 rule; the stored strict upper triangle bit for bit"""
    got = _model_q(m)
    for k in Q_NAMES:
        for i, (a, b) in enumerate(zip(got[k], want[k])):
            assert a.shape == b.shape
            err = np.abs(a - b).max()
            assert err <= 1e-8 * max(np.abs(b).max(), 1e-3), (tag, k, i, err)
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


# ---- the new kernels alone ---------------------------------------------------------------------------------------------------
# Boundaries of the kernels as written: 32 x 32 tiles of four 16 x 16 sub-tiles (12 and 10: below one sub-tile; 33: one row
# past a tile; 50 / 109 / 130: a last tile of 18 / 13 / 2 rows; 64, 512: whole tiles; 528: a last tile of 16 rows, one
# sub-tile row empty); the factorisation's LDS-resident form up to M = 64 (64 and 65 straddle it) and its LDS panel up to
# M = 512 (512 and 528 straddle it); 64 latent GPs per form / apply launch ("many": 66 GPs, two chunks around one factorisation).
_STEP_CASES = [(k, True) for k in ng.STEP_SHAPES + ["extra", "many"]] + [("unwhitened", False)]
_start = {}


def _start_state(key, whiten, gp_handle):
    """(problem, device gradient of a twin model at the same state), once per shape"""
    if key not in _start:
        prob = ng.unwhitened_problem() if key == "unwhitened" else ng.shape_problem(key)
        prob = _with_upper_junk(prob)
        twin = _model(prob, gp_handle, whiten)
        _fix_all_but_q(twin)
        _start[key] = (prob, _device_grads(twin))
    return _start[key]


@pytest.mark.parametrize("gamma", (0.1, 1.0))
@pytest.mark.parametrize("key,whiten", _STEP_CASES)
def test_one_step_follows_the_restatement(gp_handle, key, whiten, gamma):
    from gpitch_amd.train import NatGradAdam
    prob, grads = _start_state(key, whiten, gp_handle)
    want = ng.step_problem(prob, grads, gamma)
    m = _model(prob, gp_handle, whiten)
    _fix_all_but_q(m)
    m.optimize(method=NatGradAdam(gamma), maxiter=1)
    _assert_q(m, want, (key, gamma))
    moved = max(np.abs(a - b).max() for k in Q_NAMES for a, b in zip(_model_q(m)[k], prob[k]))
    assert moved > 1e-4                                     # (a step was taken)


def test_the_entry_checks_its_arguments(gp_handle):
    """gp_pdgp_natgrad_step: a step length outside (0, 1], a short or misaligned workspace and a GP-sharded plan are refused
    before anything is enqueued; no latent GP flagged is a step of nothing"""
    import ctypes as C
    from gpitch_amd import _lib
    prob = ng.shape_problem(0)
    m = _model(prob, gp_handle)
    grads = _device_grads(m)
    h = m._handle
    nbytes = h.lib.gp_pdgp_natgrad_workspace_bytes(m._plan)
    Ms = [12, 10]
    assert nbytes >= 8 * sum(2 * M * M + M for M in Ms)
    ws = h.workspace(nbytes)
    before = m._params.cpu().numpy().copy()

    def call(gamma, flags=None, ptr=None, size=None, plan=None):
        fl = None if flags is None else (C.c_int32 * len(flags))(*flags)
        return h.lib.gp_pdgp_natgrad_step(plan or m._plan, m._params.data_ptr(), m._free.data_ptr(), m._grad.data_ptr(), gamma, fl,
                                          ws.data_ptr() if ptr is None else ptr, ws.numel() if size is None else size)
    for gamma in (0.0, -0.5, 1.5, float("nan")):
        assert call(gamma) == _lib.GP_ERR_BAD_ARG
    assert call(0.5, size=nbytes // 2) == _lib.GP_ERR_WORKSPACE
    assert call(0.5, ptr=ws.data_ptr() + 8) == _lib.GP_ERR_BAD_ARG
    assert call(0.5, flags=[0, 0]) == _lib.GP_OK
    h.sync()
    assert np.array_equal(m._params.cpu().numpy(), before)
    sub = _model(prob, gp_handle, shard=("gp", 0, 2))
    sub._compile()
    assert call(0.5, plan=sub._plan) == _lib.GP_ERR_BAD_ARG
    # one GP flagged: only that one moves, and as the restatement says
    assert call(0.5, flags=[0, 1]) == _lib.GP_OK
    m._unpack()
    want = ng.step_problem(prob, grads, 0.5, rows=[1])
    _assert_q(m, want, "one flag")
    assert np.array_equal(m.q_mu_act[0].value, prob["q_mu_act"][0])


# ---- conjugate known answer --------------------------------------------------------------------------------------------------
def _com_grad_norm(grads, i):
    return np.sqrt(np.sum(grads["q_mu_com%d" % i] ** 2) + np.sum(np.tril(grads["q_sqrt_com%d" % i][:, :, 0]) ** 2))


@pytest.mark.parametrize("P", (1, 2))
def test_one_step_of_length_one_lands_on_the_optimal_component_posterior(gp_handle, P):
    """With everything but one component GP's q(u) fixed the data term is linear in that GP's expectation parameters: one step
    of length 1 is the maximiser.  P = 2 fixes three of the four latent GPs, which are then skipped.
    Measured on MI355X: see the figures printed below and DESIGN.md 3i."""
    import gpitch_amd
    from gpitch_amd.train import NatGradAdam
    prob = ng.conjugate_problem(P)
    i = P - 1
    fixed_rows = [r for r in range(2 * P) if r != P + i]

    def build():
        m = _model(prob, gp_handle)
        _fix_all_but_q(m)
        _fix_q(m, fixed_rows)
        return m
    before = _device_grads(build())
    m = build()
    m.optimize(method=NatGradAdam(1.0), maxiter=1)
    after = model_grad_dict(m)                               # optimize() ends with an evaluation at the final state
    ratio = _com_grad_norm(after, i) / _com_grad_norm(before, i)
    print("P = %d: gradient of the stepped GP after / before the step %.2e (bar %.1e)" % (P, ratio, ng.CONJ_GRAD_BAR))
    q1 = _model_q(m)
    elbo_ng = m.compute_log_likelihood()
    m.optimize(method=NatGradAdam(1.0), maxiter=1)
    q2 = _model_q(m)
    for k in Q_NAMES:
        for a, b in zip(q2[k], q1[k]):
            assert np.abs(a - b).max() <= 1e-8 * max(np.abs(b).max(), 1e-3), k
    for r in fixed_rows:                                     # fixed GPs were skipped
        k_mu, k_sq, j = ("q_mu_act", "q_sqrt_act", r) if r < P else ("q_mu_com", "q_sqrt_com", r - P)
        assert np.array_equal(q1[k_mu][j], prob[k_mu][j]) and np.array_equal(q1[k_sq][j], prob[k_sq][j])
    twin = build()
    twin.optimize(method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=50)
    elbo_adam = twin.compute_log_likelihood()
    print("P = %d: ELBO after one natural-gradient step %.9f, after 50 Adam(0.01) iterations %.9f" % (P, elbo_ng, elbo_adam))
    assert elbo_ng >= elbo_adam - 1e-9 * abs(elbo_ng)
    assert ratio <= ng.CONJ_GRAD_BAR, ratio


# ---- Adam beside it ----------------------------------------------------------------------------------------------------------
def _variational_mask(m):
    mask = np.zeros(m._nparams, dtype=bool)
    Ms = list(m.num_inducing_a) + list(m.num_inducing_c)
    for (o_th, o_z, o_mu, o_sq), M in zip(m._layout, Ms):
        mask[o_mu:o_mu + M] = True
        mask[o_sq:o_sq + M * M] = True
    return mask


def test_adam_moves_everything_else_exactly_as_on_its_own(gp_handle):
    import gpitch_amd
    from gpitch_amd.train import NatGradAdam
    prob = ng.shape_problem(1)
    twin = _model(prob, gp_handle)
    grads = _device_grads(twin)
    twin.optimize(method=gpitch_amd.train.AdamOptimizer(0.01, 0.8, 0.99, 1e-7), maxiter=1)
    m = _model(prob, gp_handle)
    m.optimize(method=NatGradAdam(0.1, 0.01, 0.8, 0.99, 1e-7), maxiter=1)
    var = _variational_mask(m)
    assert 0 < (~var).sum() < var.size
    for name in ("_params", "_free", "_adam_m", "_adam_v"):
        a, b = getattr(m, name).cpu().numpy(), getattr(twin, name).cpu().numpy()
        assert np.array_equal(a[~var], b[~var]), name
    assert np.abs(m._adam_m.cpu().numpy()[~var]).max() > 0   # (Adam did move them)
    assert not np.any(m._adam_m.cpu().numpy()[var]) and not np.any(m._adam_v.cpu().numpy()[var])
    _assert_q(m, ng.step_problem(prob, grads, 0.1), "adam beside")


# ---- three iterations end to end ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gamma", ng.THREE_ITER_GAMMAS)
@pytest.mark.parametrize("k", ng.THREE_ITER_SHAPES)
def test_three_iterations_against_the_oracle_driven_restatement(gp_handle, k, gamma):
    from gpitch_amd.train import NatGradAdam
    prob = ng.shape_problem(k)
    want = ng.iterate(prob, gamma, 3, lambda p: oracle_elbo_and_grads(p)[1])
    m = _model(prob, gp_handle)
    _fix_all_but_q(m)
    m.optimize(method=NatGradAdam(gamma), maxiter=3)
    got = dict(prob, **_model_q(m))
    d = ng.q_distance(got, want)
    print("shape %d, gamma = %g: q after three iterations differs from the restatement by %.2e (bar %.1e)"
          % (k, gamma, d, ng.three_iter_bar(k, gamma)))
    assert d <= ng.three_iter_bar(k, gamma)


# ---- refusal -----------------------------------------------------------------------------------------------------------------
def test_a_step_that_is_too_long_is_refused_and_changes_nothing(gp_handle):
    """natgrad_ref.refusal_problem(): B of the activation GP has a negative eigenvalue at gamma = 1 (shown on the CPU in
    test_natgrad_cpu.py).  A numerical refusal through the handle's status word: nothing here faults the device."""
    from gpitch_amd import _lib
    from gpitch_amd.train import NatGradAdam
    prob = ng.refusal_problem()
    m = _model(prob, gp_handle)
    m._pack()
    state = lambda: [getattr(m, n).cpu().numpy().copy() for n in ("_params", "_free", "_adam_m", "_adam_v")]
    before = state()
    with pytest.raises(_lib.NotPositiveDefiniteError) as ei:
        m.optimize(method=NatGradAdam(ng.REFUSAL_GAMMA, 0.01), maxiter=2)
    msg = str(ei.value)
    assert "too long" in msg and "activation GP 0" in msg and "gamma = 1" in msg, msg
    for a, b in zip(state(), before):
        assert np.array_equal(a, b)
    for k in Q_NAMES:                                        # ... and neither did the host Params
        assert all(np.array_equal(a, b) for a, b in zip(_model_q(m)[k], prob[k]))
    res = m.optimize(method=NatGradAdam(ng.REFUSAL_SMALL_GAMMA, 0.01), maxiter=2)
    assert np.isfinite(res.fun)
    assert np.abs(m.q_mu_act[0].value - prob["q_mu_act"][0]).max() > 0
    assert np.abs(state()[2]).max() > 0                      # Adam ran beside it


# ---- bookkeeping -------------------------------------------------------------------------------------------------------------
def test_two_identical_runs_agree_bit_for_bit(gp_handle):
    from gpitch_amd.train import NatGradAdam
    prob = ng.shape_problem(2)
    runs = []
    for _ in range(2):
        m = _model(prob, gp_handle)
        m.optimize(method=NatGradAdam(0.1, 0.01), maxiter=3)
        runs.append([getattr(m, n).cpu().numpy() for n in ("_params", "_free", "_adam_m", "_adam_v")])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


class _RecordingRng(object):
    """the generator of MinibatchData, recording the index sets it hands out"""

    def __init__(self):
        self.rng = np.random.RandomState(0)
        self.drawn = []

    def randint(self, N, size):
        idx = self.rng.randint(N, size=size)
        self.drawn.append(idx.copy())
        return idx


def test_minibatches_are_drawn_as_in_the_adam_branch(gp_handle):
    import gpitch_amd
    from gpitch_amd.synth import make_problem
    from gpitch_amd.train import NatGradAdam
    prob = make_problem(3000, 24, 1, num_partials=2, seed=3)
    drawn = []
    for method in (NatGradAdam(0.1, 0.0025), gpitch_amd.train.AdamOptimizer(0.0025)):
        m = _model(prob, gp_handle, minibatch_size=100)
        m.za.fixed = True
        m.zc.fixed = True
        rec = _RecordingRng()
        m.x.rng = rec
        m.y.rng = rec
        res = m.optimize(method=method, maxiter=5)
        assert np.isfinite(res.fun) and m._adam_t == 5
        drawn.append(rec.drawn)
    assert len(drawn[0]) == len(drawn[1]) == 6               # five iterations and the returned `fun` / `jac`
    for a, b in zip(*drawn):
        assert a.shape == (100,) and np.array_equal(a, b)


def test_predictions_after_training_are_refactorised_and_the_callback_runs(gp_handle):
    from gpitch_amd.train import NatGradAdam
    prob = ng.shape_problem(0)
    m = _model(prob, gp_handle)
    xs = prob["x"][::3].copy()
    mean0, var0 = m.predict_act(xs)
    calls = []
    res = m.optimize(method=NatGradAdam(0.5, 0.01), maxiter=4, callback=lambda xf: calls.append(xf.copy()))
    assert len(calls) == 4 and all(c.shape == res.x.shape for c in calls)
    assert np.array_equal(calls[-1], res.x) and not np.array_equal(calls[0], calls[1])
    assert res.success and np.isfinite(res.fun) and res.jac.shape == res.x.shape
    mean1, var1 = m.predict_act(xs)
    assert np.abs(mean1[0] - mean0[0]).max() > 1e-6 and np.abs(var1[0] - var0[0]).max() > 1e-6


def test_float32_strips_take_the_same_step(gp_handle):
    """float_type = float32 changes the strips the gradient is computed from, not this step (float64 throughout): one
    iteration against the float64 twin within tests/test_gpu_f32.py's bounds for trained parameters (hyper-parameters 2e-4
    relative, q 1e-2 of the largest entry)"""
    from gpitch_amd.synth import make_problem
    from gpitch_amd.train import NatGradAdam
    prob = make_problem(4096, 128, 2, num_partials=3, seed=2)
    out = []
    for ft in (np.float32, np.float64):
        m = _model(prob, gp_handle, float_type=ft)
        m.za.fixed = True
        m.zc.fixed = True
        m.optimize(method=NatGradAdam(0.1, 0.0025), maxiter=1)
        out.append((m._params.cpu().numpy(), _variational_mask(m), _model_q(m)))
    (p32, var, q32), (p64, _, q64) = out
    assert np.abs(p32[~var] - p64[~var]).max() <= 2e-4 * np.abs(p64[~var]).max()
    assert np.all(np.abs(p32[~var] - p64[~var]) <= 2e-4 * np.maximum(np.abs(p64[~var]), 1e-3))
    for k in Q_NAMES:
        for a, b in zip(q32[k], q64[k]):
            assert np.abs(a - b).max() <= 1e-2 * np.abs(b).max(), k
