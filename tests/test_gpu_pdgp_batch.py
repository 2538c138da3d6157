"""Many independent Pdgp models per launch sequence (gpitch_amd.pdgp_batch, csrc/pdgp_batch.hip) against torch-CPU
autograd through the oracle and against each model's own single-model path."""
import copy
import os

import numpy as np
import pytest

from helpers import oracle_elbo_and_grads, pdgp_from_problem

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _ragged(prob, Ma, Mc, seed):
    """give latent GP i of the problem Ma[i] / Mc[i] inducing points (uniform over the data) and matching q"""
    from gpitch_amd.synth import uniform_inducing
    rq = np.random.RandomState(seed)
    for i in range(prob["P"]):
        for zk, mk, sk, M in (("za", "q_mu_act", "q_sqrt_act", Ma[i]), ("zc", "q_mu_com", "q_sqrt_com", Mc[i])):
            prob[zk][i] = uniform_inducing(prob["x"], M)
            prob[mk][i] = 0.3 * rq.randn(M, 1)
            prob[sk][i] = np.tril(np.eye(M) + 0.05 * rq.randn(M, M))[:, :, None].copy()
    return prob


def _m32sm(m, f0):
    return {"type": "matern32sm", "variance": 1.0, "lengthscales": 0.1, "energy": [0.2 / m] * m,
            "frequency": [(k + 1) * f0 for k in range(m)]}


def _mercer(m, f0):
    return {"type": "mercer_matern12sm", "variance": 1.0, "lengthscales": 0.1, "energy": [1. / m] * m,
            "frequency": [(k + 1) * f0 for k in range(m)]}


def _act(t, ls=0.02, v=3.5):
    return {"type": t, "variance": v, "lengthscales": ls, "energy": [], "frequency": []}


def _mixed_problems():
    """six models: P in {1, 3}; M from 8 to 128 (109 included), ragged inside a model; m from 1 to 32; both reference
    kernel pairs plus RBF / Matern52; all three nonlinearities; z fixed in some, trained in others.  Activation
    lengthscales of 20 ms keep Kuu well conditioned (test_gpu_partials.py)."""
    from gpitch_amd.synth import make_problem
    out = []
    p = make_problem(400, 109, 1, num_partials=5, seed=11)                       # the demo pair, M = 109 / 64
    p = _ragged(p, [109], [64], 1)
    p["kern_act"][0] = _act("matern32")
    out.append((p, 0, True))
    p = make_problem(600, 8, 3, num_partials=1, seed=12)                          # per-note pair, ragged M, m = 1, 7, 32
    p = _ragged(p, [8, 32, 128], [16, 109, 40], 2)
    p["kern_act"] = [_act("matern12") for _ in range(3)]
    p["kern_com"] = [_m32sm(m, 220. * (i + 1)) for i, m in enumerate((1, 7, 32))]
    for k in p["kern_com"]:
        k["lengthscales"] = 0.01      # 109 trained inducing points in 600 frames: l = 0.1 s gives cond(Kuu) ~ 1e12
    out.append((p, 1, False))
    p = make_problem(300, 16, 1, num_partials=2, seed=13)                         # stationary RBF / Matern52
    p["kern_act"][0] = _act("rbf")
    p["kern_com"][0] = _act("matern52", ls=0.01, v=1.0)
    out.append((p, 2, True))
    p = make_problem(512, 24, 1, num_partials=32, seed=14)                        # Mercer m = 32, z trained
    p["kern_act"][0] = _act("matern32")
    out.append((p, 0, False))
    p = make_problem(256, 12, 3, num_partials=3, seed=15)                         # P = 3, z trained
    p["kern_act"] = [_act("matern32") for _ in range(3)]
    out.append((p, 1, False))
    p = make_problem(1024, 128, 1, num_partials=16, seed=16)                      # M = 128, B = 1024
    p["kern_act"][0] = _act("matern12")
    p["kern_com"][0] = _m32sm(16, 330.)
    out.append((p, 2, True))
    return out


def _build(prob, nlin, zfixed, minibatch_size=None):
    import gpitch_amd
    fn = [gpitch_amd.logistic_tf, gpitch_amd.softplus_tf, gpitch_amd.gaussfun_tf][nlin]
    m = pdgp_from_problem(prob, nlinfun=fn, minibatch_size=minibatch_size)
    if zfixed:
        m.za.fixed = True
        m.zc.fixed = True
    return m


def _batch_grad_dict(batch, k):
    """the batch's constrained gradient of model k, keyed as oracle_elbo_and_grads"""
    g = batch._grad.cpu().numpy()
    m = batch.models[k]
    P = m.num_sources
    base = batch._range[k][0]
    out = {"noise": g[base:base + 1].copy()}
    off = base + 1
    for r in range(2 * P):
        act = r < P
        i = r if act else r - P
        name = ("act%d" if act else "com%d") % i
        kern = (m.kern_act if act else m.kern_com)[i]
        mp = int(kern.num_partials)
        M = (m.num_inducing_a if act else m.num_inducing_c)[i]
        out[name + ".variance"] = g[off:off + 1].copy()
        out[name + ".lengthscales"] = g[off + 1:off + 2].copy()
        for j in range(mp):
            out["%s.energy%d" % (name, j)] = g[off + 2 + j:off + 3 + j].copy()
            out["%s.frequency%d" % (name, j)] = g[off + 2 + mp + j:off + 3 + mp + j].copy()
        off += 2 + 2 * mp
        out[("za%d" if act else "zc%d") % i] = g[off:off + M].reshape(-1, 1).copy()
        out[("q_mu_act%d" if act else "q_mu_com%d") % i] = g[off + M:off + 2 * M].reshape(-1, 1).copy()
        out[("q_sqrt_act%d" if act else "q_sqrt_com%d") % i] = g[off + 2 * M:off + 2 * M + M * M].reshape(M, M, 1).copy()
        off += 2 * M + M * M
    return out


def _block_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def test_objective_matches_autograd_through_the_oracle(gp_handle):
    """every model of a mixed full-batch batch: ELBO within 1e-9 relative, every gradient block within 2e-7"""
    from gpitch_amd.pdgp_batch import PdgpBatch
    probs = _mixed_problems()
    models = [_build(p, nl, zf) for p, nl, zf in probs]
    batch = PdgpBatch(models)
    res = batch.objective_many()
    for k, (p, nl, zf) in enumerate(probs):
        e_ref, g_ref = oracle_elbo_and_grads(p, nlin_code=nl)
        assert abs(-res[k][0] - e_ref) <= 1e-9 * abs(e_ref), (k, -res[k][0], e_ref)
        got = _batch_grad_dict(batch, k)
        for name, gr in g_ref.items():
            if gr is None:
                continue
            if zf and name[:2] in ("za", "zc"):
                continue
            if name.endswith(".variance") and p["kern_" + ("act" if name.startswith("act") else "com")][
                    int(name.split(".")[0][3:])]["type"] == "matern32sm":
                continue          # Matern32sm has no global variance (a fixed unit slot)
            # the activation lengthscale of the M = 128, B = 1024 model sums 128 x 1152 kernel-derivative terms: measured
            # 3.5e-7; as test_gpu_wave_shapes.py's largest cases, that block alone gets 1e-6
            bound = 1e-6 if (k == 5 and name == "act0.lengthscales") else 2e-7
            assert _block_err(got[name], gr) <= bound, (k, name, _block_err(got[name], gr))


def _models_minibatched():
    """the mixed batch with minibatches (randint and permutation branches) plus the real-audio notebook model"""
    import gpitch_amd
    from gpitch_amd.kernels import Matern32
    from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
    from gpitch_amd.synth import make_problem
    d = np.load(os.path.join(HERE, "golden", "init_liv_real_audio.npz"))
    y = np.asarray(d["y"], dtype=np.float64).reshape(-1, 1)
    fs = int(d["fs"])
    x = np.linspace(0., (y.size - 1.) / fs, y.size).reshape(-1, 1)
    f0 = gpitch_amd.find_ideal_f0([str(d["fname"])])
    z, u = gpitch_amd.init_liv(x=x, y=y, win_size=31, thres=0.033, dec=9)
    kcom = MercerMatern12sm(input_dim=1, energy=np.ones(5), frequency=f0 * np.arange(1, 6))
    real = gpitch_amd.pdgp.Pdgp(x=x.copy(), y=y.copy(), z=z, kern=[[Matern32(1, lengthscales=1.0, variance=1.0)], [kcom]],
                                minibatch_size=100)
    real.za.fixed = True
    real.zc.fixed = True
    out = [real]
    p = make_problem(2000, 40, 3, num_partials=3, seed=21)
    p = _ragged(p, [40, 20, 33], [64, 16, 9], 3)
    p["kern_act"] = [_act("matern12") for _ in range(3)]
    p["kern_com"] = [_m32sm(m, 200. * (i + 1)) for i, m in enumerate((2, 5, 9))]
    for k in p["kern_com"]:
        k["lengthscales"] = 0.01      # up to 64 trained inducing points in 125 ms: keeps Kuu well conditioned
    out.append(_build(p, 1, False, minibatch_size=150))
    ragged = p
    p = make_problem(600, 24, 1, num_partials=4, seed=22)
    p["kern_act"][0] = _act("matern32")
    out.append(_build(p, 2, True, minibatch_size=400))          # minibatch / N >= 0.5: permutation draws
    out.append(_build(ragged, 1, True, minibatch_size=150))     # the ragged model again, z fixed
    return out


def _qkeys(m):
    return [p for lst in (m.q_mu_act, m.q_mu_com, m.q_sqrt_act, m.q_sqrt_com) for p in lst]


def _hkeys(m):
    ps = [m.likelihood.variance]
    for k in list(m.kern_act) + list(m.kern_com):
        ps += k.theta_params()
    return ps + list(m.za) + list(m.zc)


def _free_blocks(m, vec):
    """a free-state vector of model m split into one block per non-fixed Param (GPflow's free-state order)"""
    from gpitch_amd.param import sorted_params
    from gpitch_amd.pdgp_batch import model_segments
    owned = {id(p) for _, p in model_segments(m)[0]}
    out, o = [], 0
    for p in sorted_params(m):
        if p.fixed or id(p) not in owned:
            continue
        out.append(vec[o:o + p.size])
        o += p.size
    assert o == vec.size
    return out


def _assert_same_objective(m, got, twin):
    """(-ELBO, -free gradient) against the twin's Pdgp._objective: 1e-9 relative and 2e-7 per Param block"""
    f, g = twin._objective(twin.get_free_state())
    assert abs(got[0] - f) <= 1e-9 * abs(f), (got[0], f)
    assert got[1].shape == g.shape
    for j, (a, b) in enumerate(zip(_free_blocks(m, got[1]), _free_blocks(twin, g))):
        assert _block_err(a, b) <= 2e-7, (j, _block_err(a, b))


def test_objective_many_matches_each_models_own_objective(gp_handle):
    from gpitch_amd.pdgp_batch import PdgpBatch
    models = _models_minibatched()
    twins = copy.deepcopy(models)
    res = PdgpBatch(models).objective_many()
    for k, t in enumerate(twins):
        _assert_same_objective(models[k], res[k], t)
        assert str(models[k].x.rng.get_state()) == str(t.x.rng.get_state())


def test_fixed_flags_changed_between_calls_on_one_batch(gp_handle):
    """the free-state layout and the gradients the backward pass skips follow `.fixed` at every call"""
    from gpitch_amd.pdgp_batch import PdgpBatch
    models = _models_minibatched()[1:3]
    twins = copy.deepcopy(models)
    batch = PdgpBatch(models)
    batch.objective_many()
    for t in twins:
        t._objective(t.get_free_state())
    for m in models + twins:
        m.za.fixed = True                        # z of the activations leaves the free state
        m.kern_com[0].fixed = True               # every hyper-parameter of one component GP as well
    res = batch.objective_many()
    for m, r, t in zip(models, res, twins):
        _assert_same_objective(m, r, t)


def test_optimize_many_matches_single_model_training(gp_handle):
    """3 steps: q blocks within 1e-9 absolute, hyper-parameters within 1e-9 relative.  200 steps: identical generator
    states; the free state within 1e-6 relative and the returned fun within 1e-8 relative for the real-audio model,
    the permutation-branch model and the ragged three-pitch model with z fixed.  Measured: 1.0e-14, 7e-17 and 2e-18.

    The same ragged model with z trained (model 1) gets 1e-4 / 2e-3, measured 5.8e-5 / 7.4e-4.  Its two
    trajectories agree to 1e-16 after 5 steps, and the difference then grows about 15-fold per step until it
    saturates.  At lr = 2.5e-4 the same growth starts later: 1e-14 after 20 steps, 9e-6 after 200.  With z fixed the
    same model stays at rounding level.  So the inducing inputs' Adam dynamics amplify the rounding of the summation
    order; no per-step disagreement is involved.  The objective and gradient of that model match the single-model
    path per Param block within 1e-9 / 2e-7 (test_objective_many_matches_each_models_own_objective)."""
    import gpitch_amd
    from gpitch_amd.pdgp_batch import optimize_many
    tok = gpitch_amd.train.AdamOptimizer(0.0025)
    models = _models_minibatched()
    twins = copy.deepcopy(models)
    optimize_many(models, method=tok, maxiter=3)
    for m, t in zip(models, twins):
        t.optimize(method=tok, maxiter=3)
        for a, b in zip(_qkeys(m), _qkeys(t)):
            np.testing.assert_allclose(a.value, b.value, rtol=0, atol=1e-9)
        for a, b in zip(_hkeys(m), _hkeys(t)):
            np.testing.assert_allclose(a.value, b.value, rtol=1e-9, atol=0)
        assert m._adam_t == t._adam_t == 3
    # 197 more on both sides: 200 in all, the batch resuming from the moments it left in the models
    res = optimize_many(models, method=tok, maxiter=197)
    for k, (m, t) in enumerate(zip(models, twins)):
        r = t.optimize(method=tok, maxiter=197)
        assert str(m.x.rng.get_state()) == str(t.x.rng.get_state())
        assert str(m.y.rng.get_state()) == str(t.y.rng.get_state())
        err = np.max(np.abs(res[k].x - r.x)) / np.max(np.abs(r.x))
        print("model %d: free-state relative difference after 200 steps %.3g, fun %.3g" %
              (k, err, abs(res[k].fun - r.fun) / abs(r.fun)))
        bx, bf = (1e-4, 2e-3) if k == 1 else (1e-6, 1e-8)
        assert err <= bx, (k, err)
        assert abs(res[k].fun - r.fun) <= bf * abs(r.fun), (k, res[k].fun, r.fun)


def test_trained_model_predicts_like_a_fresh_model(gp_handle):
    import gpitch_amd
    from gpitch_amd.pdgp_batch import optimize_many
    from gpitch_amd.synth import make_problem
    p = make_problem(800, 32, 1, num_partials=3, seed=31)
    p["kern_act"][0] = _act("matern32")
    m = _build(p, 0, False, minibatch_size=100)
    xt = np.linspace(0., 799. / 16000., 333).reshape(-1, 1)
    before = m.predict_act_n_com(xt)                       # memoised state that must not survive the training
    optimize_many([m], method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=20)
    fresh = copy.deepcopy(p)
    fresh["za"] = [m.za[0].value]; fresh["zc"] = [m.zc[0].value]
    fresh["q_mu_act"] = [m.q_mu_act[0].value]; fresh["q_mu_com"] = [m.q_mu_com[0].value]
    fresh["q_sqrt_act"] = [m.q_sqrt_act[0].value]; fresh["q_sqrt_com"] = [m.q_sqrt_com[0].value]
    f = _build(fresh, 0, False)
    for kf, km in ((f.kern_act[0], m.kern_act[0]), (f.kern_com[0], m.kern_com[0])):
        for a, b in zip(kf.theta_params(), km.theta_params()):
            a.value = b.value
    f.likelihood.variance = m.likelihood.variance.value
    got, ref = m.predict_act_n_com(xt), f.predict_act_n_com(xt)
    for a, b in zip(got, ref):
        np.testing.assert_array_equal(a[0], b[0])
    assert not np.array_equal(got[0][0], before[0][0])


def _fresh_small():
    from gpitch_amd.synth import make_problem
    out = []
    for s, nl in ((41, 0), (42, 1), (43, 2)):
        p = make_problem(700, 20, 1, num_partials=2, seed=s)
        p["kern_act"][0] = _act("matern32")
        out.append(_build(p, nl, s != 42, minibatch_size=64))
    return out


def test_failed_cholesky_freezes_one_model_and_the_others_match_a_batch_without_it(gp_handle):
    import gpitch_amd
    from gpitch_amd import _lib
    from gpitch_amd.param import transforms
    from gpitch_amd.pdgp_batch import optimize_many
    tok = gpitch_amd.train.AdamOptimizer(0.01)
    a = _fresh_small()
    b = copy.deepcopy(a)
    bad = copy.deepcopy(a[0])
    bad.kern_act[0].variance.transform = transforms.Identity()
    bad.kern_act[0].variance = -1.0
    before = [p.value.copy() for p in _hkeys(bad) + _qkeys(bad)]
    rng_before = str(bad.x.rng.get_state())
    res = optimize_many([a[0], bad, a[1], a[2]], method=tok, maxiter=30)
    ref = optimize_many(b, method=tok, maxiter=30)
    assert not res[1].success and isinstance(res[1].error, _lib.NotPositiveDefiniteError)
    assert bad._adam_t == 0 and str(bad.x.rng.get_state()) == rng_before
    for p, v in zip(_hkeys(bad) + _qkeys(bad), before):
        np.testing.assert_array_equal(p.value, v)
    for r, q, m, n in zip([res[0], res[2], res[3]], ref, [a[0], a[1], a[2]], b):
        assert r.success
        np.testing.assert_array_equal(r.x, q.x)
        assert r.fun == q.fun
        for p1, p2 in zip(_hkeys(m) + _qkeys(m), _hkeys(n) + _qkeys(n)):
            np.testing.assert_array_equal(p1.value, p2.value)


def test_two_identical_runs_are_bit_identical(gp_handle):
    import gpitch_amd
    from gpitch_amd.pdgp_batch import optimize_many
    tok = gpitch_amd.train.AdamOptimizer(0.01)
    a = _fresh_small()
    b = copy.deepcopy(a)
    ra = optimize_many(a, method=tok, maxiter=25)
    rb = optimize_many(b, method=tok, maxiter=25)
    for x, y in zip(ra, rb):
        np.testing.assert_array_equal(x.x, y.x)
        np.testing.assert_array_equal(x.jac, y.jac)
        assert x.fun == y.fun


def test_per_note_flow_end_to_end(gp_handle):
    """init_kernel_training -> one P = 1 model per note -> optimize_many -> init_kernel_with_trained_models -> a
    multi-pitch Pdgp that evaluates"""
    import gpitch_amd
    from gpitch_amd.init_models import init_kernel_training, init_kernel_with_trained_models
    from gpitch_amd.pdgp import Pdgp
    from gpitch_amd.synth import per_fun, uniform_inducing
    fs, N = 16000, 3000
    x = np.linspace(0., (N - 1.) / fs, N).reshape(-1, 1)
    midis = [60, 64, 67]
    names = ["note_M%d.wav" % mi for mi in midis]
    ys = []
    for mi in midis:
        f0 = 2. ** ((mi - 69.) / 12.) * 440.
        y = per_fun(x, 4, f0) * np.exp(-((x - 0.09) / 0.05) ** 2) + 1e-3 * np.random.RandomState(mi).randn(N, 1)
        ys.append(y / np.max(np.abs(y)))
    kern, _ = init_kernel_training([y.reshape(-1) for y in ys], names, fs, maxh=4)
    z = uniform_inducing(x, 40)
    models = []
    for i in range(len(midis)):
        kern[0][i].lengthscales = 0.02
        m = Pdgp(x, ys[i], [[z.copy()], [z.copy()]], [[kern[0][i]], [kern[1][i]]], minibatch_size=100)
        m.za.fixed = True
        m.zc.fixed = True
        models.append(m)
    res = gpitch_amd.optimize_many(models, method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=50)
    assert all(r.success and np.isfinite(r.fun) for r in res)
    kact, kcom = init_kernel_with_trained_models(models)
    big = Pdgp(x, np.sum(ys, axis=0), [[z.copy()] * 3, [z.copy()] * 3], [kact, kcom], minibatch_size=200)
    assert np.isfinite(big.compute_log_likelihood())
    np.testing.assert_array_equal(kcom[1].frequency[0].value, models[1].kern_com[0].frequency[0].value)
