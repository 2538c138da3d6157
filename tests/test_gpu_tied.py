"""Tied Params of optimize_many / PdgpBatch on the device (csrc/pdgp_batch.hip pdgpb_tie_kernel, gp_pdgpb_set_ties) against
the host restatement of tests/tied_ref.py, and their exact properties: members bit-identical, runs bit-identical, models
outside a tie untouched, a tied set stopping together."""
import copy
import ctypes as C

import numpy as np
import pytest

from tied_ref import hkeys, qkeys, segment_model, segments, train_tied

pytestmark = pytest.mark.gpu


def _adam(lr=0.01):
    import gpitch_amd
    return gpitch_amd.train.AdamOptimizer(lr)


def _copy_with_groups(models, tied):
    """deep copies of the models and of groups of their Params, the groups following the copies"""
    return copy.deepcopy((list(models), [list(g) for g in tied]))


def _assert_restated(models, ref):
    """the bars of test_optimize_many_matches_single_model_training for two three-step Adam trajectories: q blocks within
    1e-9 absolute, every other Param within 1e-9 relative, generator states identical"""
    for k, (m, t) in enumerate(zip(models, ref)):
        for a, b in zip(qkeys(m), qkeys(t)):
            np.testing.assert_allclose(a.value, b.value, rtol=0, atol=1e-9, err_msg="model %d" % k)
        for a, b in zip(hkeys(m), hkeys(t)):
            np.testing.assert_allclose(a.value, b.value, rtol=1e-9, atol=0, err_msg="model %d" % k)
        assert m._adam_t == t._adam_t
        assert str(m.x.rng.get_state()) == str(t.x.rng.get_state())
        assert str(m.y.rng.get_state()) == str(t.y.rng.get_state())


def _moments(m):
    """id(Param) -> (m, v) as the model's next optimize() continues from them"""
    return {id(p): mv for p, mv in zip(m._param_order(), m._adam_state())}


def _assert_members_identical(models, tied):
    mom = {}
    for m in models:
        mom.update(_moments(m))
    for g in tied:
        for p in g[1:]:
            assert p.value.tobytes() == g[0].value.tobytes()
            for a, b in zip(mom[id(p)], mom[id(g[0])]):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes()


def _assert_same_bits(ra, rb, ma, mb):
    for x, y in zip(ra, rb):
        assert x.success and y.success
        np.testing.assert_array_equal(x.x, y.x)
        np.testing.assert_array_equal(x.jac, y.jac)
        assert x.fun == y.fun
    for m, n in zip(ma, mb):
        for p, q in zip(hkeys(m) + qkeys(m), hkeys(n) + qkeys(n)):
            np.testing.assert_array_equal(p.value, q.value)


@pytest.fixture(scope="module")
def three_steps(gp_handle):
    """the three segments before training, after 3 tied Adam iterations, and after the restatement's 3"""
    from gpitch_amd import optimize_many, tie_groups
    start = segments(3)
    models, tied = _copy_with_groups(start, tie_groups(start))
    res = optimize_many(models, method=_adam(), maxiter=3, tied=tied)
    ref = train_tied(start, tie_groups(start), _adam(), 3)
    return dict(start=start, models=models, tied=tied, res=res, ref=ref)


def test_three_tied_adam_steps_match_the_restatement(three_steps):
    s = three_steps
    assert all(r.success for r in s["res"])
    _assert_restated(s["models"], s["ref"])
    # the ties did something: the shared noise variance is not what the first segment learns alone
    from gpitch_amd import optimize_many
    alone = copy.deepcopy(s["start"])
    optimize_many(alone, method=_adam(), maxiter=3)
    assert alone[0].likelihood.variance.value[0] != s["models"][0].likelihood.variance.value[0]
    assert alone[0].likelihood.variance.value[0] != alone[1].likelihood.variance.value[0]


def test_members_and_runs_are_bit_identical(three_steps):
    """the same run continued to 25 iterations (from the values and moments the first 3 left in the models)"""
    from gpitch_amd import optimize_many, tie_groups
    s = three_steps
    _assert_members_identical(s["models"], s["tied"])
    a, ta = _copy_with_groups(s["models"], s["tied"])
    ra = optimize_many(a, method=_adam(), maxiter=22, tied=ta)
    assert all(m._adam_t == 25 for m in a)
    _assert_members_identical(a, ta)
    assert not np.array_equal(a[0].kern_com[1].lengthscales.value, s["models"][0].kern_com[1].lengthscales.value)
    # a second run from fresh copies: 3 + 22 again
    b, tb = _copy_with_groups(s["start"], tie_groups(s["start"]))
    optimize_many(b, method=_adam(), maxiter=3, tied=tb)
    rb = optimize_many(b, method=_adam(), maxiter=22, tied=tb)
    _assert_same_bits(ra, rb, a, b)
    # no group, and groups of one member only, are the call without `tied`
    runs = []
    for tied in (None, [], lambda ms: [[m.likelihood.variance] for m in ms] + [[ms[1].kern_act[0].lengthscales]]):
        ms = copy.deepcopy(s["start"])
        runs.append((optimize_many(ms, method=_adam(), maxiter=5, tied=tied(ms) if callable(tied) else tied), ms))
    _assert_same_bits(runs[0][0], runs[1][0], runs[0][1], runs[1][1])
    _assert_same_bits(runs[0][0], runs[2][0], runs[0][1], runs[2][1])


def test_group_and_grid_edges_in_one_batch(gp_handle):
    """three tied segments, an untied model, a P = 3 model whose activation lengthscales are one parameter, and two M = 64
    models tied with their inducing inputs: more groups than one workgroup of pdgpb_tie_kernel takes (256).

    The step length is 1e-4 here.  Adam's first steps move every free entry by about the learning rate whatever its
    gradient, and the 64 inducing inputs lie 0.625 ms apart: at 0.01 s a step is 16 spacings, and two inputs 32 spacings
    apart that move towards each other meet to rounding.  Kuu is then singular up to its jitter of 1e-6, and a condition
    number of 1e6 per step carries the rounding of two correct trajectories past any bar (at 0.01: one z entry of 64 off
    by 3.1e-9 relative, 3e-12 s).  At 1e-4 three steps move an input by less than half a spacing: no two meet, and the
    bars of the z-fixed comparison apply as they are."""
    from gpitch_amd import check_tied, optimize_many, tie_groups
    tok = _adam(1e-4)
    seg = segments(3)
    lone = segment_model(74)
    inner = segment_model(75, P=3)
    pair = segments(2, first=76, M=64, zfixed=False)
    models = seg + [lone, inner] + pair
    tied = tie_groups(seg) + [[k.lengthscales for k in inner.kern_act]] + tie_groups(pair, inducing=True)
    groups = check_tied(models, tied)
    assert len(groups) == 16 + 1 + 16 + 4 * 64 and len(groups) > 256
    assert sorted(len(g) for g in groups)[::len(groups) - 1] == [2, 3]
    ref = train_tied(models, tied, tok, 3)
    solo = copy.deepcopy(lone)
    res = optimize_many(models, method=tok, maxiter=3, tied=tied)
    assert all(r.success for r in res)
    _assert_restated(models, ref)
    _assert_members_identical(models, tied)
    rs = optimize_many([solo], method=tok, maxiter=3)
    _assert_same_bits([res[3]], rs, [lone], [solo])


def test_natgrad_steps_precede_the_tie(three_steps):
    """one iteration: q(u) as the untied call's with the same token, the tied Params as the Adam-only tied run's"""
    import gpitch_amd
    from gpitch_amd import optimize_many, tie_groups
    s = three_steps
    adam, ta = _copy_with_groups(s["start"], tie_groups(s["start"]))
    assert all(r.success for r in optimize_many(adam, method=_adam(), maxiter=1, tied=ta))
    for tok in (gpitch_amd.train.NatGradAdam(0.1, 0.01),
                gpitch_amd.train.NatGradAdam(0.5, 0.01, gamma_com=1.0, halvings=3)):
        untied = copy.deepcopy(s["start"])
        assert all(r.success for r in optimize_many(untied, method=tok, maxiter=1))
        got, tg = _copy_with_groups(s["start"], tie_groups(s["start"]))
        assert all(r.success for r in optimize_many(got, method=tok, maxiter=1, tied=tg))
        for m, u, a in zip(got, untied, adam):
            for p, q in zip(qkeys(m), qkeys(u)):
                np.testing.assert_array_equal(p.value, q.value)
            for p, q in zip(hkeys(m), hkeys(a)):
                np.testing.assert_array_equal(p.value, q.value)
        assert got[0].likelihood.variance.value[0] != untied[0].likelihood.variance.value[0]
        _assert_members_identical(got, tg)


def _with_failing_member():
    from gpitch_amd.param import transforms
    h = segments(4)
    bad = copy.deepcopy(h[0])
    bad.kern_act[0].variance.transform = transforms.Identity()
    bad.kern_act[0].variance = -1.0
    models = [h[0], bad, h[1], h[2], h[3]]
    return models, [[h[0].likelihood.variance, bad.likelihood.variance, h[1].likelihood.variance]]


def test_a_tied_set_stops_together(gp_handle):
    """the noise variances of a model whose Kuu is not positive definite (activation variance -1: the handled status of
    test_failed_cholesky_freezes_one_model_...) and of two healthy models are one parameter; two more models are untied"""
    from gpitch_amd import _lib, optimize_many
    from gpitch_amd.pdgp_batch import PdgpBatch, draw_indices
    models, tied = _with_failing_member()
    outside = copy.deepcopy(models[3:])
    fresh, tied_fresh = _copy_with_groups(models, tied)
    before = [[p.value.copy() for p in hkeys(m) + qkeys(m)] for m in models[:3]]
    rng_before = [(str(m.x.rng.get_state()), str(m.y.rng.get_state())) for m in models[:3]]
    res = optimize_many(models, method=_adam(), maxiter=30, tied=tied)
    ref = optimize_many(outside, method=_adam(), maxiter=30)
    for k in range(3):
        assert not res[k].success and isinstance(res[k].error, _lib.NotPositiveDefiniteError)
        m = models[k]
        assert m._adam_t == 0 and m._adam_state() is None
        assert (str(m.x.rng.get_state()), str(m.y.rng.get_state())) == rng_before[k]
        for p, v in zip(hkeys(m) + qkeys(m), before[k]):
            np.testing.assert_array_equal(p.value, v)
    assert res[1].message.startswith("Cholesky failed: latent GP row 0")
    for k in (0, 2):
        assert "tied" in res[k].message and "model 1" in res[k].message and res[1].message in res[k].message
    _assert_same_bits(res[3:], ref, models[3:], outside)
    # the words behind it, after two iterations through the step entry: the Kuu status names the failing model alone, the
    # frozen words the whole set with 1 + its index
    batch = PdgpBatch(fresh, tied=tied_fresh)
    h = batch._handle
    batch._pack()
    batch._load_moments()
    idx = h.torch.as_tensor(batch._indices([draw_indices(m, 2) for m in fresh])).to(h.device)
    lr = h.torch.full((2 * len(fresh),), 0.01, dtype=h.torch.float64, device=h.device)
    noise = batch._params.cpu().numpy()[[r[0] for r in batch._range]]
    h.check(h.lib.gp_pdgpb_adam(batch._plan, batch._free.data_ptr(), batch._params.data_ptr(), batch._tcode.data_ptr(),
                                batch._adam_m.data_ptr(), batch._adam_v.data_ptr(), batch._x.data_ptr(),
                                batch._y.data_ptr(), idx.data_ptr(), 2, lr.data_ptr(), 0.9, 0.999, 1e-8))
    assert [int(v != 0) for v in batch.not_pd(clear=False)] == [0, 1, 0, 0, 0]
    assert list(batch.ties_frozen(clear=False)) == [2, 2, 2, 0, 0]
    after = batch._params.cpu().numpy()[[r[0] for r in batch._range]]
    assert np.array_equal(after[:3], noise[:3]) and np.all(after[3:] != noise[3:]) and np.all(np.isfinite(after))
    assert list(batch.ties_frozen(clear=True)) == [2, 2, 2, 0, 0] and not batch.ties_frozen().any()


def test_set_ties_checks_its_arguments(gp_handle):
    from gpitch_amd import _lib, tie_groups
    from gpitch_amd.pdgp_batch import PdgpBatch
    models = segments(2)
    batch = PdgpBatch(models)
    h, lib, plan = batch._handle, batch._handle.lib, batch._plan
    off = {id(p): o for segs in batch._segs for o, p in segs}
    noise = [off[id(m.likelihood.variance)] for m in models]
    ls = [off[id(m.kern_act[1].lengthscales)] for m in models]
    need = lib.gp_pdgpb_ties_workspace_bytes(2, 4, 2)
    ws = h.workspace(need)

    def call(start, members, ptr=None, nbytes=None):
        gs = (C.c_int32 * len(start))(*start)
        mem = (C.c_int64 * len(members))(*members)
        st = lib.gp_pdgpb_set_ties(plan, len(start) - 1, gs, mem, ws.data_ptr() if ptr is None else ptr,
                                   ws.numel() if nbytes is None else nbytes)
        return st, (lib.gp_last_error(h.h) or b"").decode()

    qsq = off[id(models[1].q_sqrt_com[0])]
    for start, members, kw, status, text in (
            ([0, 2, 4], noise + [ls[0], batch.num_params], {}, _lib.GP_ERR_BAD_ARG, "outside the parameter vector"),
            ([0, 2, 4], noise + [ls[0], -1], {}, _lib.GP_ERR_BAD_ARG, "outside the parameter vector"),
            ([0, 2, 4], noise + [ls[0], qsq + 7], {}, _lib.GP_ERR_BAD_ARG, "q_mu / q_sqrt block of latent GP 6"),
            ([0, 2, 4], noise + [ls[0], off[id(models[0].q_mu_act[0])]], {}, _lib.GP_ERR_BAD_ARG, "q_mu / q_sqrt block of latent GP 0"),
            ([0, 2, 4], noise + [ls[0], noise[1]], {}, _lib.GP_ERR_BAD_ARG, "named twice"),
            ([0, 3, 2], noise + ls, {}, _lib.GP_ERR_BAD_ARG, "does not ascend at group 1"),
            ([0, 2, 4], noise + ls, {"nbytes": need - 1}, _lib.GP_ERR_WORKSPACE, "workspace too small"),
            ([0, 2, 4], noise + ls, {"ptr": ws.data_ptr() + 8}, _lib.GP_ERR_WORKSPACE, "256-byte aligned")):
        st, msg = call(start, members, **kw)
        assert st == status and text in msg, (start, members, st, msg)
    # nothing was set: the plan trains as an untied one
    twins = copy.deepcopy(models)
    ra = batch.optimize(_adam(), 2)
    rb = PdgpBatch(twins).optimize(_adam(), 2)
    _assert_same_bits(ra, rb, models, twins)
    # a good call through the same entry ties the two; clearing (ngroups = 0) gives the untied plan back, bit for bit
    models = segments(2)
    batch = PdgpBatch(models)
    batch.set_tied(tie_groups(models))
    assert batch.optimize(_adam(), 2)[0].success
    assert models[0].likelihood.variance.value.tobytes() == models[1].likelihood.variance.value.tobytes()
    twins = copy.deepcopy(models)
    batch.set_tied(None)
    ra = batch.optimize(_adam(), 3)
    rb = PdgpBatch(twins).optimize(_adam(), 3)
    _assert_same_bits(ra, rb, models, twins)
    assert models[0].likelihood.variance.value.tobytes() != models[1].likelihood.variance.value.tobytes()
