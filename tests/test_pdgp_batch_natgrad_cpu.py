"""Host-side parts of optimize_many / PdgpBatch.optimize with a NatGradAdam token (no device): the scope check beside
check_batchable and the new ABI entries."""
import numpy as np
import pytest

from helpers import pdgp_from_problem


def _model(**kw):
    from gpitch_amd.synth import make_problem
    return pdgp_from_problem(make_problem(600, 16, 2, num_partials=3, seed=3), **kw)


def test_accepts_the_scope_and_returns_each_models_flags():
    from gpitch_amd.pdgp_batch import check_batchable_natgrad
    from gpitch_amd.train import NatGradAdam
    tok = NatGradAdam(0.5, 0.01)
    ms = [_model(), _model(minibatch_size=100), _model()]
    for q in (ms[1].q_mu_com[0], ms[1].q_sqrt_com[0]):        # both of a pair fixed: skipped, not refused
        q.fixed = True
    for q in list(ms[2].q_mu_act) + list(ms[2].q_sqrt_act) + list(ms[2].q_mu_com) + list(ms[2].q_sqrt_com):
        q.fixed = True
    models, flags = check_batchable_natgrad(ms, tok)
    assert models == ms
    assert flags == [m._natgrad_gps(tok) for m in ms] == [[1, 1, 1, 1], [1, 1, 0, 1], [0, 0, 0, 0]]


@pytest.mark.parametrize("what", ["pair", "gamma", "callback", "whiten", "shard", "M", "adam_token"])
def test_refusals_come_before_any_device_work(what):
    from gpitch_amd.pdgp_batch import check_batchable_natgrad, optimize_many
    from gpitch_amd.synth import make_problem
    from gpitch_amd.train import AdamOptimizer, NatGradAdam
    method, callback, err, says = NatGradAdam(0.5, 0.01), None, NotImplementedError, "Pdgp.optimize"
    models = [_model(), _model()]
    if what == "pair":
        models[1].q_mu_com[1].fixed = True
        err, says = ValueError, "model 1: "
    elif what == "gamma":
        method.gamma = 1.5                                    # a token changed after it was made
        err, says = ValueError, "model 0: "
    elif what == "callback":
        callback = lambda x: None
    elif what == "whiten":
        models[1] = _model(whiten=False)
    elif what == "shard":
        models[1] = _model(shard=(0, 2))
    elif what == "M":
        models[1] = pdgp_from_problem(make_problem(600, 129, 1, num_partials=2))
        err = ValueError
    else:
        method, says = AdamOptimizer(0.01), "NatGradAdam"
    with pytest.raises(err) as e:
        check_batchable_natgrad(models, method, callback)
    assert says in str(e.value), str(e.value)
    if what == "pair":
        assert "component GP 1" in str(e.value) and "q_mu fixed" in str(e.value)
    if what == "gamma":
        assert "gamma" in str(e.value) and "1.5" in str(e.value)
    if what == "adam_token":
        return                                                # (optimize_many takes that token: the Adam path)
    with pytest.raises(err):                                  # the public entry refuses it as well (no GPU here)
        optimize_many(models, method=method, maxiter=3, callback=callback)
    assert all(m._plan is None for m in models)


def test_check_batchable_still_refuses_the_token():
    from gpitch_amd.pdgp_batch import check_batchable
    from gpitch_amd.train import NatGradAdam
    with pytest.raises(NotImplementedError):
        check_batchable([_model()], method=NatGradAdam())


def test_the_refusal_message_names_model_gp_pivot_and_gamma():
    from gpitch_amd.pdgp_batch import _describe_refused
    msg = _describe_refused(1, 1 + 128 * 0 + 7, 1, 1.0)
    assert "NatGradAdam" in msg and "model 1" in msg and "activation GP 0" in msg and "pivot 7" in msg
    assert "gamma = 1" in msg and "smaller gamma" in msg
    msg = _describe_refused(4, 1 + 128 * 5 + 127, 3, 0.25)
    assert "model 4" in msg and "component GP 2" in msg and "pivot 127" in msg and "gamma = 0.25" in msg


def test_the_new_entries_are_exported():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    assert lib.gp_pdgpb_natgrad_workspace_bytes(None) == 0
    out = (np.ctypeslib.ctypes.c_int32 * 1)()
    assert lib.gp_pdgpb_natgrad_refused(None, out, 0) == _lib.GP_ERR_BAD_ARG
    assert lib.gp_pdgpb_natgrad(None, None, None, None, None, None, None, None, None, 0, None, 0.9, 0.999, 1e-8, 0.5, None,
                                None, 0) == _lib.GP_ERR_BAD_ARG
