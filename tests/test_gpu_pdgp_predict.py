"""Many Pdgp models predicted together (gpitch_amd.predict_many, csrc/pdgp_batch.hip pdgpb_pred_*) against the oracle,
against each model's own predict_act_n_com, and on the real-audio notebook model at the oracle's end state."""
import copy
import os

import numpy as np
import pytest

from test_gpu_demo_anchor import _notebook_model
from test_gpu_pdgp_batch import _act, _build, _mixed_problems

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ("mean_a", "var_a", "mean_c", "var_c", "mean_src")


def _ragged_inputs(probs):
    """per model: 1, 63, 64, 65 frames, a length unrelated to its data, and none; inside the data's range, off its grid"""
    out = []
    for p, n in zip(probs, (1, 63, 64, 65, 777, 0)):
        x = p["x"].reshape(-1)
        out.append(np.linspace(x[0] + 0.37 * (x[1] - x[0]), x[-1], n).reshape(-1, 1))
    return out


def _rel(got, ref):
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300)) if ref.size else 0.0


def _params(m):
    from gpitch_amd.pdgp_batch import model_segments
    return [p.value.copy() for _, p in model_segments(m)[0]]


def test_matches_the_oracle(gp_handle):
    """six mixed models (P 1 / 3, M 8..128 with 109 and values not divisible by 16, m 1 / 5 / 32, all six kernel types,
    all three nonlinearities), each at its own ragged inputs: every array within 1e-8 max(|ref|, 1e-3)"""
    import gpitch_amd
    from oracle import gpflow05 as orc
    probs = _mixed_problems()
    models = [_build(p, nl, zf) for p, nl, zf in probs]
    xs = _ragged_inputs([p for p, _, _ in probs])
    preds = gpitch_amd.predict_many(models, xs)
    for k, ((p, nl, _), xt, pred) in enumerate(zip(probs, xs, preds)):
        P = p["P"]
        assert all(len(a) == P for a in pred)
        if xt.size == 0:
            assert all(a.shape == (0, 1) for arrs in pred for a in arrs)
            continue
        ref = orc.pdgp_predict_act_n_com(xt, p["za"], p["zc"], p["kern_act"], p["kern_com"], p["q_mu_act"],
                                         p["q_sqrt_act"], p["q_mu_com"], p["q_sqrt_com"], nlin_code=nl)
        for name, got, r in zip(NAMES, pred, ref):
            for i in range(P):
                assert got[i].shape == (xt.shape[0], 1)
                err = np.max(np.abs(got[i] - r[i]))
                assert err <= 1e-8 * max(np.abs(r[i]).max(), 1e-3), (k, name, i, err)


def test_matches_each_models_own_prediction_and_changes_no_model(gp_handle):
    """predict_many against predict_act_n_com on deep copies, max|diff| / max|ref| per array: means and variances within
    5e-11 (measured 2.0e-11 at worst), source means within 5e-10 (measured 1.1e-10: the gaussfun source of the RBF
    model, where exp(-2 (mean_a - pi)^2) turns mean_a's 1.4e-11 into about 12 times that).  Two calls are
    bit-identical; no model's Params, generators, Adam count, engine plan or prediction memo is touched."""
    import gpitch_amd
    probs = _mixed_problems()
    models = [_build(p, nl, zf, minibatch_size=mb) for (p, nl, zf), mb in zip(probs, (None, 100, None, 64, 50, 1000))]
    twins = copy.deepcopy(models)
    xs = _ragged_inputs([p for p, _, _ in probs])
    before = [(_params(m), str(m.x.rng.get_state()), str(m.y.rng.get_state()), m._adam_t) for m in models]
    a = gpitch_amd.predict_many(models, xs)
    b = gpitch_amd.predict_many(models, [x.reshape(-1) for x in xs])
    errs = {}
    for k, (m, t, xt) in enumerate(zip(models, twins, xs)):
        ref = t.predict_act_n_com(xt)
        for name, ga, gb, r in zip(NAMES, a[k], b[k], ref):
            for i in range(m.num_sources):
                np.testing.assert_array_equal(ga[i], gb[i])
                errs[(k, name, i)] = _rel(ga[i], r[i])
        ps, xr, yr, at = before[k]
        for v, w in zip(_params(m), ps):
            np.testing.assert_array_equal(v, w)
        assert str(m.x.rng.get_state()) == xr and str(m.y.rng.get_state()) == yr and m._adam_t == at
        assert m._plan is None and getattr(m, "_pred_memo", None) is None
    for key in sorted(errs):
        print("model %d %-8s source %d: max|diff| / max|ref| = %.3g" % (key + (errs[key],)))
    for (k, name, i), e in errs.items():
        assert e <= (5e-10 if name == "mean_src" else 5e-11), (k, name, i, e)


def test_a_model_with_a_plan_keeps_its_plan_and_memo(gp_handle):
    import gpitch_amd
    probs = _mixed_problems()[:3]
    models = [_build(p, nl, zf) for p, nl, zf in probs]
    xs = _ragged_inputs([p for p, _, _ in probs])[:3]
    own = models[1].predict_act_n_com(xs[1])
    plan, memo = models[1]._plan, models[1]._pred_memo
    assert plan is not None and memo is not None
    got = gpitch_amd.predict_many(models, xs)
    assert models[1]._plan is plan and models[1]._pred_memo is memo
    for g, r in zip(got[1], own):
        assert _rel(g[0], r[0]) <= 1e-10


def test_real_audio_model_in_a_batch_of_twelve(gp_handle):
    """the notebook model at the oracle's end state (test_gpu_demo_anchor.py), predicted at x[::3] among 11 perturbed
    copies: within 1e-8 max|ref| of the golden arrays and bit-identical to the same model predicted alone"""
    import gpitch_amd
    a = np.load(os.path.join(HERE, "golden", "demo_real_audio_anchor.npz"))
    m, x, u, f0 = _notebook_model(gp_handle)
    m.kern_act[0].lengthscales = a["final.act.lengthscales"]
    m.kern_act[0].variance = a["final.act.variance"]
    kc = m.kern_com[0]
    kc.lengthscales = a["final.com.lengthscales"]
    kc.variance = a["final.com.variance"]
    for i in range(5):
        kc.energy[i].value = a["final.com.energy%d" % i]
        kc.frequency[i].value = a["final.com.frequency%d" % i]
    m.likelihood.variance = a["final.noise"]
    m.q_mu_act[0].value = a["final.q_mu_act"]
    m.q_mu_com[0].value = a["final.q_mu_com"]
    m.q_sqrt_act[0].value = a["final.q_sqrt_act"]
    m.q_sqrt_com[0].value = a["final.q_sqrt_com"]
    rs = np.random.RandomState(7)
    others = []
    for j in range(11):
        o = copy.deepcopy(m, {id(gp_handle): gp_handle})         # the copies share the session's handle
        o.q_mu_act[0].value = o.q_mu_act[0].value + 0.05 * rs.randn(*o.q_mu_act[0].value.shape)
        o.q_mu_com[0].value = o.q_mu_com[0].value * (1.0 + 0.1 * j)
        o.kern_com[0].lengthscales = o.kern_com[0].lengthscales.value * (1.0 + 0.02 * j)
        others.append(o)
    models = others[:5] + [m] + others[5:]
    xt = x[::3].copy()
    xs = [x[::(2 + j % 3)].copy() for j in range(5)] + [xt] + [x[j:j + 4000].copy() for j in range(6)]
    got = gpitch_amd.predict_many(models, xs)[5]
    alone = gpitch_amd.predict_many([m], [xt])[0]
    for name, g, s in zip(NAMES, got, alone):
        ref = a[name]
        err = np.max(np.abs(g[0] - ref)) / np.max(np.abs(ref))
        print("%-8s max deviation / max |oracle| = %.2e" % (name, err))
        assert err <= 1e-8, (name, err)
        np.testing.assert_array_equal(g[0], s[0])


def test_chunked_call_equals_the_unchunked_one(gp_handle, monkeypatch):
    import gpitch_amd
    from gpitch_amd import pdgp_batch
    probs = _mixed_problems()
    models = [_build(p, nl, zf) for p, nl, zf in probs]
    xs = _ragged_inputs([p for p, _, _ in probs])
    whole = gpitch_amd.predict_many(models, xs)
    monkeypatch.setattr(pdgp_batch, "MAX_PREDICT_FRAMES", 300)
    n_chunks = len(pdgp_batch.predict_chunks([m.num_sources for m in models], [x.shape[0] for x in xs], 300))
    assert n_chunks > 5
    parts = gpitch_amd.predict_many(models, xs)
    for w, p in zip(whole, parts):
        for ga, gb in zip(w, p):
            for u, v in zip(ga, gb):
                np.testing.assert_array_equal(u, v)


def test_after_optimize_many(gp_handle):
    """the workflow this serves: train a list with optimize_many, predict it with predict_many"""
    import gpitch_amd
    from gpitch_amd.synth import make_problem
    models = []
    for s, nl in ((51, 0), (52, 1), (53, 2)):
        p = make_problem(900, 24, 1 + (s == 52), num_partials=3, seed=s)
        p["kern_act"] = [_act("matern32") for _ in range(p["P"])]
        models.append(_build(p, nl, s != 53, minibatch_size=128))
    res = gpitch_amd.optimize_many(models, method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=40)
    assert all(r.success for r in res)
    xt = np.linspace(0., 899. / 16000., 1001).reshape(-1, 1)
    got = gpitch_amd.predict_many(models, xt)
    for m, g in zip(models, got):
        ref = m.predict_act_n_com(xt)
        for name, a, r in zip(NAMES, g, ref):
            for i in range(m.num_sources):
                assert _rel(a[i], r[i]) <= 1e-10, (name, i, _rel(a[i], r[i]))


def test_a_failed_factorisation_names_the_model(gp_handle):
    import gpitch_amd
    from gpitch_amd import _lib
    from gpitch_amd.param import transforms
    from gpitch_amd.synth import make_problem
    ms = []
    for s in (61, 62, 63):
        p = make_problem(700, 20, 1, num_partials=2, seed=s)
        p["kern_act"][0] = _act("matern32")
        ms.append(_build(p, 0, True))
    ms[1].kern_act[0].variance.transform = transforms.Identity()
    ms[1].kern_act[0].variance = -1.0
    with pytest.raises(_lib.NotPositiveDefiniteError) as e:
        gpitch_amd.predict_many(ms, np.linspace(0., 0.04, 100))
    assert "model 1" in str(e.value) and "latent GP row 0" in str(e.value)
    # the others alone still predict
    got = gpitch_amd.predict_many([ms[0], ms[2]], np.linspace(0., 0.04, 100))
    assert all(np.all(np.isfinite(a[0])) for g in got for a in g)
