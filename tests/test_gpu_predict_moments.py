"""Posterior of each source, of the mixture, and the held-out density (csrc/lik.hip mpd_moments_kernel, csrc/pdgp_batch.hip
pdgpb_pred_moments_kernel) against the CPU oracle composed here: oracle.gpflow05.pdgp_predict_act_n_com for (fmean, fvar),
hermgauss1d for E1, E2 (and V from its nodes), mpd_variational_expectations for the expected log density."""
import copy
import os

import numpy as np
import pytest

from test_gpu_demo_anchor import _notebook_model
from test_gpu_pdgp_batch import _build, _mixed_problems

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
FRAMES = (1, 63, 64, 65, 777, 0)
NOISE = 0.37
ULP = 2.0 ** -52


def _ref_moments(Fmu, Fvar, P, nlin, noise, Y=None):
    """the oracle composition on N x 2P moments: (smean, svar) lists of P (N, 1), ymean, yvar (N, 1), logp (N, 1) or None"""
    from oracle import gpflow05 as orc
    nl = orc.nlinfun(nlin)
    gh_x, gh_w = np.polynomial.hermite.hermgauss(20)
    w = (gh_w / np.sqrt(np.pi)).reshape(-1, 1)
    sm, sv = [], []
    for i in range(P):
        mg, vg = Fmu[:, i:i + 1], Fvar[:, i:i + 1]
        mf, vf = Fmu[:, P + i:P + i + 1], Fvar[:, P + i:P + i + 1]
        E1, E2 = orc.hermgauss1d(mg, vg, 20, nl)
        ev = nl(gh_x.reshape(1, -1) * np.sqrt(2. * vg) + mg)
        V = np.matmul((ev - E1) ** 2, w)
        sm.append(E1 * mf)
        sv.append(V * mf ** 2 + E2 * vf)
    ym, yv = sm[0].copy(), sv[0].copy()
    for a, b in zip(sm[1:], sv[1:]):
        ym, yv = ym + a, yv + b
    lp = None if Y is None else orc.mpd_variational_expectations(Fmu, Fvar, Y.reshape(-1, 1), noise, P, nlin)
    return sm, sv, ym, yv + noise, lp


def _bar(ref):
    """the project's prediction bar"""
    return 1e-8 * max(float(np.max(np.abs(ref))), 1e-3) if ref.size else 0.0


def _close(got, ref, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if ref.size:
        err = float(np.max(np.abs(got - ref)))
        print("%s: max|diff| = %.3g (bar %.3g)" % (what, err, _bar(ref)))
        assert err <= _bar(ref), (what, err, _bar(ref))


def _operator(h, Fmu, Fvar, Y, P, nlin, noise=NOISE, want_logp=True):
    """gp_mpd_predict_moments on host arrays through the raw C-ABI"""
    N = Fmu.shape[0]
    dmu, dvar = h.to_device(Fmu), h.to_device(Fvar)
    dy = h.to_device(Y.reshape(-1)) if want_logp else None
    nv = h.to_device(np.array([noise]))
    sm, sv, ym, yv, lp = h.empty(P, N), h.empty(P, N), h.empty(N), h.empty(N), (h.empty(N) if want_logp else None)
    h.check(h.lib.gp_mpd_predict_moments(h.h, dmu.data_ptr(), dvar.data_ptr(), dy.data_ptr() if want_logp else None, N, P,
                                         nlin, nv.data_ptr(), sm.data_ptr(), sv.data_ptr(), ym.data_ptr(), yv.data_ptr(),
                                         lp.data_ptr() if want_logp else None))
    h.sync()
    out = [t.cpu().numpy() for t in (sm, sv, ym, yv)] + [lp.cpu().numpy() if want_logp else None]
    assert np.all(out[1] >= 0.) and np.all(out[3] >= noise)          # exact, on every case of this file
    return out


def _check_against_ref(got, ref, P, tag):
    sm, sv, ym, yv, lp = got
    rsm, rsv, rym, ryv, rlp = ref
    for i in range(P):
        _close(sm[i].reshape(-1, 1), rsm[i], "%s smean[%d]" % (tag, i))
        _close(sv[i].reshape(-1, 1), rsv[i], "%s svar[%d]" % (tag, i))
    _close(ym.reshape(-1, 1), rym, tag + " ymean")
    _close(yv.reshape(-1, 1), ryv, tag + " yvar")
    if rlp is not None:
        # the bar test_gpu_ops.py::test_mpd_varexp_matches_oracle holds gp_mpd_varexp to (same arithmetic, same order)
        np.testing.assert_allclose(lp.reshape(-1, 1), rlp, rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("nlin", [0, 1, 2])
@pytest.mark.parametrize("P", [1, 3])
def test_operator_entry_matches_the_oracle(gp_handle, nlin, P):
    for N in FRAMES:
        rng = np.random.RandomState(1000 * P + 10 * nlin + N % 7)
        Fmu = rng.randn(N, 2 * P) * 2.0 + 1.0
        Fvar = rng.rand(N, 2 * P) * 3.0 + 1e-8
        Y = rng.randn(N, 1)
        got = _operator(gp_handle, Fmu, Fvar, Y, P, nlin)
        if N == 0:
            assert all(a.size == 0 for a in got)
            continue
        _check_against_ref(got, _ref_moments(Fmu, Fvar, P, nlin, NOISE, Y), P, "nlin %d P %d N %d" % (nlin, P, N))


def test_likelihood_methods_are_the_operator_entry(gp_handle):
    """MpdLik.predict_mean_and_var / predict_sources / expected_log_density: thin calls, column layout of
    variational_expectations; checked against the oracle composition and against variational_expectations itself"""
    import gpitch_amd
    P, N = 3, 333
    rng = np.random.RandomState(5)
    Fmu, Fvar, Y = rng.randn(N, 2 * P) + 2.0, rng.rand(N, 2 * P) + 1e-6, rng.randn(N, 1)
    lik = gpitch_amd.likelihoods.MpdLik(gpitch_amd.softplus_tf, P)
    lik.variance = NOISE
    rsm, rsv, rym, ryv, rlp = _ref_moments(Fmu, Fvar, P, 1, NOISE, Y)
    ms, vs = lik.predict_sources(Fmu, Fvar)
    my, vy = lik.predict_mean_and_var(Fmu, Fvar)
    lp = lik.expected_log_density(Fmu, Fvar, Y)
    assert len(ms) == len(vs) == P
    for i in range(P):
        _close(ms[i], rsm[i], "lik smean[%d]" % i)
        _close(vs[i], rsv[i], "lik svar[%d]" % i)
    _close(my, rym, "lik ymean")
    _close(vy, ryv, "lik yvar")
    np.testing.assert_allclose(lp, rlp, rtol=1e-11, atol=1e-11)
    np.testing.assert_allclose(lp, lik.variational_expectations(Fmu, Fvar, Y), rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("nlin", [0, 1, 2])
def test_degenerate_activation(gp_handle, nlin):
    """v_g = 0: every node sits at m_g, so smean = nlin(m_g) m_f and svar = nlin(m_g)^2 v_f up to rounding.  The bound,
    in ulps of the reference: E1 is 20 fused steps, each rounding by at most half an ulp of a partial sum that never
    exceeds E1 (10 ulp); the rounded weights sum to 1 within 3 ulp; the product with m_f adds half an ulp; exp / log of the
    device and of numpy are a few ulp apart, the logistic's division and the reference's own product add theirs: 24 ulp
    for the mean.  E2 squares the value first (one more ulp, and the reference's square doubles its share): 32 ulp for
    the variance; V is of the order of (10 ulp)^2 and vanishes beside it.  On top of that comes the conditioning of the
    nonlinearity itself, which is not the kernel's: both sides round the argument t of exp(t) twice, in different
    association (-2 d d), up to 2 ulp apart, and exp turns a relative difference r of t into |t| r; the softplus at
    negative x is exp(x) to first order.  So each frame is allowed 4 |t| ulp more (twice that for the square), with
    t = 2 (m_g - pi), m_g, 2 (m_g - pi)^2 for the three nonlinearities.  v_g = 1e-12 joins for the exact signs
    (svar >= 0, yvar >= noise: asserted in _operator for every case of this file)."""
    from oracle import gpflow05 as orc
    P, N = 3, 257
    rng = np.random.RandomState(40 + nlin)
    Fmu = rng.randn(N, 2 * P) * 2.0 + 1.5
    Fvar = rng.rand(N, 2 * P) * 3.0 + 1e-8
    Fvar[:, :P] = 0.0
    sm, sv, ym, yv, _ = _operator(gp_handle, Fmu, Fvar, None, P, nlin, want_logp=False)
    nl = orc.nlinfun(nlin)
    for i in range(P):
        mg = Fmu[:, i]
        s = nl(mg)
        t = np.abs([2. * (mg - np.pi), mg, 2. * (mg - np.pi) ** 2][nlin])
        rm, rv = s * Fmu[:, P + i], s * s * Fvar[:, P + i]
        em, ev = np.abs(sm[i] - rm) / (ULP * np.abs(rm)), np.abs(sv[i] - rv) / (ULP * np.abs(rv))
        print("nlin %d source %d: worst mean %.1f ulp, worst variance %.1f ulp; worst beyond the conditioning term %.1f / %.1f"
              % (nlin, i, em.max(), ev.max(), (em - 4 * t).max(), (ev - 8 * t).max()))
        assert np.all(em <= 24 + 4 * t), (i, float(np.max(em - 4 * t)))
        assert np.all(ev <= 32 + 8 * t), (i, float(np.max(ev - 8 * t)))
    Fvar[:, :P] = 1e-12
    Fvar[::2, P:] = 0.0                    # and sources without any variance of their own
    _operator(gp_handle, Fmu, Fvar, None, P, nlin, want_logp=False)
    got = _operator(gp_handle, Fmu, Fvar, None, P, nlin, noise=1e-300, want_logp=False)
    assert np.all(got[3] >= 1e-300)


def _ragged_inputs(probs):
    """per model: 1, 63, 64, 65 frames, a length unrelated to its data, and none; inside the data's range, off its grid"""
    out = []
    for p, n in zip(probs, FRAMES):
        x = p["x"].reshape(-1)
        out.append(np.linspace(x[0] + 0.37 * (x[1] - x[0]), x[-1], n).reshape(-1, 1))
    return out


def _targets(xs, seed=9):
    rs = np.random.RandomState(seed)
    return [0.3 * rs.randn(x.shape[0], 1) for x in xs]


def _oracle_model_moments(p, nl, xt, yt):
    from oracle import gpflow05 as orc
    ma, va, mc, vc, _ = orc.pdgp_predict_act_n_com(xt, p["za"], p["zc"], p["kern_act"], p["kern_com"], p["q_mu_act"],
                                                   p["q_sqrt_act"], p["q_mu_com"], p["q_sqrt_com"], nlin_code=nl)
    Fmu, Fvar = np.concatenate(ma + mc, 1), np.concatenate(va + vc, 1)
    return _ref_moments(Fmu, Fvar, p["P"], nl, float(np.asarray(p["noise_var"]).reshape(-1)[0]), yt)


def test_model_level_against_the_oracle_and_the_operator(gp_handle):
    """the six mixed models of test_gpu_pdgp_predict.py through Pdgp.predict_sources / predict_y / predict_mixture /
    expected_log_density: (a) against the oracle composition, at the project's prediction bar 1e-8 max(|ref|, 1e-3);
    (b) against the operator entry applied to the model's own predict_act_n_com output, which isolates the new kernel
    from the conditionals: same kernel code on the same conditionals, held to 1e-13 max|ref| (a few hundred ulp)."""
    probs = _mixed_problems()
    xs = _ragged_inputs([p for p, _, _ in probs])
    ys = _targets(xs)
    for k, ((p, nl, zf), xt, yt) in enumerate(zip(probs, xs, ys)):
        m = _build(p, nl, zf)
        P = p["P"]
        ms, vs = m.predict_sources(xt)
        my, vy = m.predict_y(xt)
        mm, vm = m.predict_mixture(xt)
        lp = m.expected_log_density(xt, yt)
        n = xt.shape[0]
        assert len(ms) == len(vs) == P and all(a.shape == (n, 1) for a in ms + vs + [my, vy, mm, vm, lp])
        if n == 0:
            continue
        noise = float(m.likelihood.variance.value[0])
        assert all(np.all(v >= 0.) for v in vs) and np.all(vm >= 0.) and np.all(vy >= noise)
        np.testing.assert_array_equal(mm, my)
        np.testing.assert_array_equal(vy, vm + noise)
        rsm, rsv, rym, ryv, rlp = _oracle_model_moments(p, nl, xt, yt)
        for i in range(P):
            _close(ms[i], rsm[i], "model %d mean_s[%d]" % (k, i))
            _close(vs[i], rsv[i], "model %d var_s[%d]" % (k, i))
        _close(my, rym, "model %d mean_y" % k)
        _close(vy, ryv, "model %d var_y" % k)
        err = float(np.max(np.abs(lp - rlp)))
        print("model %d logp: max|diff| = %.3g (bar %.3g)" % (k, err, _bar(rlp)))
        assert err <= _bar(rlp), (k, err)
        # (b) the operator entry on the model's own conditionals
        ma, va, mc, vc, _ = m.predict_act_n_com(xt)
        Fmu, Fvar = np.concatenate(ma + mc, 1), np.concatenate(va + vc, 1)
        osm, osv, oym, oyv, olp = _operator(gp_handle, Fmu, Fvar, yt, P, nl, noise=noise)
        for got, ref, name in [(ms[i], osm[i], "mean_s") for i in range(P)] + [(vs[i], osv[i], "var_s") for i in range(P)] + \
                              [(my, oym, "mean_y"), (vy, oyv, "var_y"), (lp, olp, "logp")]:
            e = float(np.max(np.abs(got.reshape(-1) - ref.reshape(-1))))
            assert e <= 1e-13 * float(np.max(np.abs(ref))), (k, name, e)


def _at_golden_end_state(m, a):
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


def test_tie_to_the_elbo_on_the_real_audio_model(gp_handle):
    """full batch, whitened: sum_n E_q[log p(y_n | g, f)] at the training data minus the 2P whitened KL terms
    (conditionals.gauss_kl) is the ELBO: compute_log_likelihood() within the project's ELBO bar, 1e-9 relative, on the
    real-audio notebook model at the golden end state"""
    import gpitch_amd
    from gpitch_amd.conditionals import gauss_kl
    a = np.load(os.path.join(HERE, "golden", "demo_real_audio_anchor.npz"))
    nb, x, u, f0 = _notebook_model(gp_handle)
    y = nb.y._array.copy()
    m = gpitch_amd.pdgp.Pdgp(x=x.copy(), y=y, z=[[nb.za[0].value.copy()], [nb.zc[0].value.copy()]],
                             kern=[[nb.kern_act[0]], [nb.kern_com[0]]], minibatch_size=None, handle=gp_handle)
    _at_golden_end_state(m, a)
    assert m.whiten and m.minibatch_size == x.shape[0]
    lp = m.expected_log_density(x, y)
    kl = gauss_kl(m.q_mu_act[0].value, m.q_sqrt_act[0].value) + gauss_kl(m.q_mu_com[0].value, m.q_sqrt_com[0].value)
    elbo = m.compute_log_likelihood()
    got = float(np.sum(lp)) - float(kl)
    print("sum logp %.10f  KL %.10f  difference %.10f  ELBO %.10f" % (float(np.sum(lp)), float(kl), got, elbo))
    assert abs(got - elbo) <= 1e-9 * abs(elbo), (got, elbo)


def _flat(res):
    out = []
    for r in res:
        for name in sorted(r):
            v = r[name]
            out += [(name, a) for a in v] if isinstance(v, list) else [(name, v)]
    return out


def _same_bits(a, b):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb)
    for (na, u), (nb, v) in zip(fa, fb):
        assert na == nb
        np.testing.assert_array_equal(u, v)


def test_batch_matches_each_models_own_methods_and_the_oracle(gp_handle):
    """predict_sources_many over the six mixed models at ragged inputs (one of them empty): against the oracle composition
    and against each model's own Pdgp methods (deep copies), both at the prediction bar; two calls bit-identical;
    ynews=None drops logp and changes nothing else bit for bit"""
    import gpitch_amd
    probs = _mixed_problems()
    models = [_build(p, nl, zf) for p, nl, zf in probs]
    twins = copy.deepcopy(models)
    xs = _ragged_inputs([p for p, _, _ in probs])
    ys = _targets(xs)
    a = gpitch_amd.predict_sources_many(models, xs, ys)
    b = gpitch_amd.predict_sources_many(models, [x.reshape(-1) for x in xs], [y.reshape(-1) for y in ys])
    c = gpitch_amd.predict_sources_many(models, xs)
    _same_bits(a, b)
    assert all(sorted(r) == ["mean_s", "mean_y", "var_s", "var_y"] for r in c)
    _same_bits([{k: v for k, v in r.items() if k != "logp"} for r in a], c)
    for k, ((p, nl, _), t, xt, yt, r) in enumerate(zip(probs, twins, xs, ys, a)):
        P, n = p["P"], xt.shape[0]
        assert sorted(r) == ["logp", "mean_s", "mean_y", "var_s", "var_y"]
        assert len(r["mean_s"]) == len(r["var_s"]) == P
        assert all(v.shape == (n, 1) for v in r["mean_s"] + r["var_s"] + [r["mean_y"], r["var_y"], r["logp"]])
        if n == 0:
            continue
        noise = float(t.likelihood.variance.value[0])
        assert all(np.all(v >= 0.) for v in r["var_s"]) and np.all(r["var_y"] >= noise)
        rsm, rsv, rym, ryv, rlp = _oracle_model_moments(p, nl, xt, yt)
        oms, ovs = t.predict_sources(xt)
        omy, ovy = t.predict_y(xt)
        olp = t.expected_log_density(xt, yt)
        for i in range(P):
            _close(r["mean_s"][i], rsm[i], "batch model %d mean_s[%d] vs oracle" % (k, i))
            _close(r["var_s"][i], rsv[i], "batch model %d var_s[%d] vs oracle" % (k, i))
            _close(r["mean_s"][i], oms[i], "batch model %d mean_s[%d] vs own" % (k, i))
            _close(r["var_s"][i], ovs[i], "batch model %d var_s[%d] vs own" % (k, i))
        for name, ref, own in (("mean_y", rym, omy), ("var_y", ryv, ovy), ("logp", rlp, olp)):
            _close(r[name], ref, "batch model %d %s vs oracle" % (k, name))
            _close(r[name], own, "batch model %d %s vs own" % (k, name))


def test_batch_alone_versus_among_twelve_and_split_versus_unsplit(gp_handle, monkeypatch):
    """a model's results do not depend on its neighbours in the batch nor on how its frames are split between launches"""
    import gpitch_amd
    from gpitch_amd import pdgp_batch
    probs = _mixed_problems()
    models = [_build(p, nl, zf) for p, nl, zf in probs]
    xs = [np.linspace(p["x"][0, 0], p["x"][-1, 0], n).reshape(-1, 1) for (p, _, _), n in zip(probs, (130, 65, 200, 1, 97, 64))]
    ys = _targets(xs, seed=11)
    rs = np.random.RandomState(3)
    others = []
    for j in range(6):
        o = copy.deepcopy(models[j])
        o.q_mu_com[0].value = o.q_mu_com[0].value * (1.0 + 0.1 * (j + 1))
        o.q_mu_act[0].value = o.q_mu_act[0].value + 0.05 * rs.randn(*o.q_mu_act[0].value.shape)
        others.append(o)
    twelve = [v for pair in zip(others, models) for v in pair]
    x12 = [v for pair in zip(xs[::-1], xs) for v in pair]
    y12 = [v for pair in zip(ys[::-1], ys) for v in pair]
    whole = gpitch_amd.predict_sources_many(twelve, x12, y12)
    for k in range(6):
        alone = gpitch_amd.predict_sources_many([models[k]], [xs[k]], [ys[k]])
        _same_bits([whole[2 * k + 1]], alone)
    monkeypatch.setattr(pdgp_batch, "MAX_PREDICT_FRAMES", 300)
    n_chunks = len(pdgp_batch.predict_chunks([m.num_sources for m in twelve], [x.shape[0] for x in x12], 300))
    assert n_chunks > 5
    parts = gpitch_amd.predict_sources_many(twelve, x12, y12)
    _same_bits(whole, parts)


def _state(m):
    from gpitch_amd.pdgp_batch import model_segments
    ad = m._adam_state()
    return ([p.value.copy() for _, p in model_segments(m)[0]], [bool(p.fixed) for _, p in model_segments(m)[0]],
            str(m.x.rng.get_state()), str(m.y.rng.get_state()), m._adam_t,
            None if ad is None else [(a.copy(), b.copy()) for a, b in ad])


def _assert_state(m, s):
    t = _state(m)
    for v, w in zip(t[0], s[0]):
        np.testing.assert_array_equal(v, w)
    assert t[1] == s[1] and t[2] == s[2] and t[3] == s[3] and t[4] == s[4]
    if s[5] is None:          # never trained: no moments, or (once an engine plan exists) all-zero ones
        assert t[5] is None or all(not a.any() and not b.any() for a, b in t[5])
    else:
        for (a, b), (c, d) in zip(t[5], s[5]):
            np.testing.assert_array_equal(a, c)
            np.testing.assert_array_equal(b, d)


def test_no_side_effects(gp_handle):
    """after the new calls predict_many and predict_act_n_com return bit for bit what they returned before, and Params,
    `.fixed` flags, generators, Adam count and moments are untouched; predict_sources_many builds no engine plan and
    leaves plan and prediction memo of a model that has them alone"""
    import gpitch_amd
    probs = _mixed_problems()[:4]
    models = [_build(p, nl, zf, minibatch_size=mb) for (p, nl, zf), mb in zip(probs, (None, 100, None, 64))]
    xs = _ragged_inputs([p for p, _, _ in probs])[:4]
    ys = _targets(xs)
    gpitch_amd.optimize_many(models[2:], method=gpitch_amd.train.AdamOptimizer(0.005), maxiter=3)   # Adam moments exist
    before_many = gpitch_amd.predict_many(models, xs)
    own_before = models[1].predict_act_n_com(xs[1])
    plan, memo = models[1]._plan, models[1]._pred_memo
    states = [_state(m) for m in models]
    gpitch_amd.predict_sources_many(models, xs, ys)
    assert models[1]._plan is plan and models[1]._pred_memo is memo
    assert all(m._plan is None and getattr(m, "_pred_memo", None) is None for m in (models[0], models[2], models[3]))
    for m, s in zip(models, states):
        _assert_state(m, s)
    for m, xt, yt in zip(models, xs, ys):
        m.predict_sources(xt)
        m.predict_y(xt)
        m.predict_mixture(xt)
        m.expected_log_density(xt, yt)
    assert models[1]._pred_memo is memo
    for m, s in zip(models, states):
        _assert_state(m, s)
    after_many = gpitch_amd.predict_many(models, xs)
    for u, v in zip(before_many, after_many):
        for ga, gb in zip(u, v):
            for p, q in zip(ga, gb):
                np.testing.assert_array_equal(p, q)
    models[1]._pred_memo = None                       # recompute, not the memo
    own_after = models[1].predict_act_n_com(xs[1])
    for ga, gb in zip(own_before, own_after):
        for p, q in zip(ga, gb):
            np.testing.assert_array_equal(p, q)
