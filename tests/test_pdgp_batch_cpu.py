"""Host-side parts of gpitch_amd.pdgp_batch (no device): the scope refusals, the minibatch index streams and the
free-state layout."""
import copy

import numpy as np
import pytest

from helpers import pdgp_from_problem


def _model(**kw):
    from gpitch_amd.synth import make_problem
    return pdgp_from_problem(make_problem(600, 16, 2, num_partials=3, seed=3), **kw)


def _tok():
    import gpitch_amd
    return gpitch_amd.train.AdamOptimizer(0.01)


def test_accepts_the_scope():
    from gpitch_amd.pdgp_batch import check_batchable
    ms = [_model(), _model(minibatch_size=100)]
    assert check_batchable(ms, _tok()) == ms


@pytest.mark.parametrize("what", ["whiten", "float32", "pair", "shard", "lbfgs", "callback", "M", "minibatch",
                                  "kernel_m12sm", "kernel_prod", "duplicate", "empty", "not_a_model"])
def test_refusals_name_the_single_model_path(what):
    import gpitch_amd
    from gpitch_amd.pdgp_batch import check_batchable, optimize_many
    from gpitch_amd.synth import make_problem
    method, callback, models = _tok(), None, None
    err = NotImplementedError
    if what == "whiten":
        models = [_model(whiten=False)]
    elif what == "float32":
        models = [_model(float_type=np.float32)]
    elif what == "pair":
        models = [_model(float_type=(np.float64, np.float32))]
    elif what == "shard":
        models = [_model(shard=(0, 2))]
    elif what == "lbfgs":
        models, method = [_model()], "L-BFGS-B"
    elif what == "callback":
        models, callback = [_model()], (lambda x: None)
    elif what == "M":
        models, err = [pdgp_from_problem(make_problem(600, 129, 1, num_partials=2))], ValueError
    elif what == "minibatch":
        models, err = [pdgp_from_problem(make_problem(2000, 16, 1, num_partials=2), minibatch_size=1025)], ValueError
    elif what == "kernel_m12sm":
        p = make_problem(600, 16, 1, num_partials=2)
        p["kern_com"][0]["type"] = "matern12sm"
        models = [pdgp_from_problem(p)]
    elif what == "kernel_prod":
        p = make_problem(600, 16, 1, num_partials=2)
        p["kern_com"][0]["type"] = "mercer_matern52sm"
        models = [pdgp_from_problem(p)]
    elif what == "duplicate":
        m = _model()
        models, err = [m, m], ValueError
    elif what == "empty":
        models, err = [], ValueError
    else:
        models, err = [_model(), object()], ValueError
    with pytest.raises(err) as e:
        check_batchable(models, method, callback)
    if what not in ("duplicate", "empty", "not_a_model"):
        assert "Pdgp.optimize" in str(e.value)
    with pytest.raises(err):           # refused by the public entry before any device work (no GPU here)
        optimize_many(models, method=method, maxiter=3, callback=callback)


@pytest.mark.parametrize("mb", [100, 400])
def test_block_drawn_indices_equal_per_step_draws(mb):
    """N = 600: mb = 100 draws with replacement (one block for all steps), mb = 400 permutation prefixes (step by step);
    both equal Pdgp._batch's per-step MinibatchData draws, sorted, and leave the same generator states"""
    from gpitch_amd.pdgp_batch import draw_indices
    a = _model(minibatch_size=mb)
    b = copy.deepcopy(a)
    got = draw_indices(a, 7)
    ref = []
    for _ in range(7):
        idx = b.x.next_indices()
        b.y.rng.set_state(b.x.rng.get_state())
        ref.append(np.sort(idx, kind="stable"))
    np.testing.assert_array_equal(got, np.stack(ref))
    for ga, gb in ((a.x.rng, b.x.rng), (a.y.rng, b.y.rng)):
        sa, sb = ga.get_state(), gb.get_state()
        assert sa[0] == sb[0] and sa[2:] == sb[2:]
        np.testing.assert_array_equal(sa[1], sb[1])


def test_full_batch_models_draw_nothing():
    from gpitch_amd.pdgp_batch import draw_indices
    a = _model()
    s0 = a.x.rng.get_state()[1].copy()
    np.testing.assert_array_equal(draw_indices(a, 3), np.tile(np.arange(600), (3, 1)))
    np.testing.assert_array_equal(a.x.rng.get_state()[1], s0)


def test_free_state_layout_is_the_models_gpflow_order():
    """the batch vector's free entries of each model, in the order free_index lists them, are the Params of
    param.sorted_params (GPflow's free-state order of Pdgp._objective) with `.fixed` ones left out"""
    from gpitch_amd.param import sorted_params
    from gpitch_amd.pdgp_batch import free_index, model_segments
    a, b = _model(), _model(minibatch_size=100)
    b.za.fixed = True
    b.kern_com[1].frequency[0].fixed = True
    segs_a, na = model_segments(a, 0)
    segs_b, nb = model_segments(b, na)
    for m, segs in ((a, segs_a), (b, segs_b)):
        at = {o: p for o, p in segs}
        want = [(id(p), j) for p in sorted_params(m) if not p.fixed for j in range(p.size)]
        got = []
        starts = sorted(at)
        for e in free_index(m, segs):
            o = max(s for s in starts if s <= e)
            got.append((id(at[o]), e - o))
        assert got == want
    # block lengths: noise + per latent GP theta (2 + 2m) + z + q_mu + q_sqrt
    P, M, mp = 2, 16, 3
    assert na == 1 + P * (2 + 2 * M + M * M) + P * (2 + 2 * mp + 2 * M + M * M)
    assert segs_b[0][0] == na


def test_adam_moments_handed_over_by_position_survive_a_copy():
    """moments installed on a model that has no plan yet are kept by Param position, so a deep copy keeps them"""
    a = _model()
    state = [(np.full(p.size, 0.5 + i), np.full(p.size, 2.0 + i)) for i, p in enumerate(a._param_order())]
    a._set_adam_state(state)
    b = copy.deepcopy(a)
    got = b._adam_state()
    assert len(got) == len(state)
    for (gm, gv), (sm, sv) in zip(got, state):
        np.testing.assert_array_equal(gm, sm)
        np.testing.assert_array_equal(gv, sv)
    from gpitch_amd.pdgp_batch import model_segments
    assert [p for _, p in model_segments(a)[0]] == a._param_order()
