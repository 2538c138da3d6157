"""GPU parity of the Pdgp ELBO path (forward, gradient, prediction, Adam) against the oracle."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import (pdgp_from_problem, oracle_elbo, oracle_elbo_and_grads, model_grad_dict)  # noqa: E402

# float64 tolerance of north_star: ELBO and posterior means within 1e-4 relative; we hold 1e-9.
ELBO_RTOL = 1e-9


@pytest.mark.parametrize("N,M,P,m", [(64, 8, 1, 2), (500, 33, 2, 3), (4096, 64, 1, 5), (3000, 109, 3, 4)])
def test_elbo_forward_matches_oracle(gp_handle, N, M, P, m):
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=m, seed=N % 7)
    model = pdgp_from_problem(prob, handle=gp_handle)
    got = model.compute_log_likelihood()
    ref = float(oracle_elbo(prob))
    assert abs(got - ref) <= ELBO_RTOL * abs(ref), (got, ref)


def test_prior_elbo_identity_K1(gp_handle):
    """at q_mu=0, q_sqrt=I (whitened) KL=0, fmean=0, fvar=Kdiag, so the ELBO has a closed
    form independent of M, Z and lengthscales."""
    from gpitch_amd.synth import make_problem
    from oracle import gpflow05 as orc
    prob = make_problem(1024, 32, 2, num_partials=3, seed=1, trivial_q=True)
    model = pdgp_from_problem(prob, handle=gp_handle)
    got = model.compute_log_likelihood()
    N, s2 = prob["N"], prob["noise_var"]
    tot = np.sum(prob["y"] ** 2)
    for i in range(prob["P"]):
        vg = prob["kern_act"][i]["variance"]
        vf = prob["kern_com"][i]["variance"] * sum(prob["kern_com"][i]["energy"])
        _, E2 = orc.hermgauss1d(np.zeros((1, 1)), np.full((1, 1), vg), 20, orc.logistic)
        tot += N * vf * E2[0, 0]
    ref = -0.5 * tot / s2 - 0.5 * N * (np.log(2 * np.pi) + np.log(s2))
    assert abs(got - ref) <= 1e-10 * abs(ref)


# (4200, 12, 1, 16): many partials and frames -> the spectral-mixture hyper-gradient contraction runs as two partial groups
@pytest.mark.parametrize("N,M,P,m", [(300, 16, 1, 2), (700, 40, 2, 3), (4200, 12, 1, 16)])
def test_elbo_gradient_matches_autograd(gp_handle, N, M, P, m):
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=m, seed=3)
    model = pdgp_from_problem(prob, handle=gp_handle)
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob)
    assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f)
    got_g = model_grad_dict(model)
    for name, rg in ref_g.items():
        gg = got_g[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]   # band_part: no gradient reaches the upper triangle
            assert np.all(np.triu(gg[:, :, 0], 1) == 0)
        scale = max(np.abs(rg).max(), 1e-12)
        np.testing.assert_allclose(gg.reshape(rg.shape), rg, rtol=0, atol=2e-7 * scale, err_msg=name)


def test_predict_matches_oracle(gp_handle):
    from gpitch_amd.synth import make_problem
    from oracle import gpflow05 as orc
    prob = make_problem(2000, 50, 2, num_partials=3, seed=5)
    model = pdgp_from_problem(prob, handle=gp_handle)
    xt = prob["x"][::3].copy()
    ma, va, mc, vc, ms = model.predict_act_n_com(xt)
    r = orc.pdgp_predict_act_n_com(xt, prob["za"], prob["zc"], prob["kern_act"], prob["kern_com"], prob["q_mu_act"],
                                   prob["q_sqrt_act"], prob["q_mu_com"], prob["q_sqrt_com"])
    for got, ref in zip((ma, va, mc, vc, ms), r):
        for i in range(prob["P"]):
            np.testing.assert_allclose(got[i], ref[i], rtol=0, atol=1e-8 * max(np.abs(ref[i]).max(), 1e-3))
    ma2, va2 = model.predict_act(xt)
    np.testing.assert_array_equal(ma2[1], ma[1])


def test_adam_steps_match_oracle_trajectory(gp_handle):
    """three full-batch Adam steps on the free state reproduce the oracle's (autograd + TF-1.2 Adam)."""
    import gpitch_amd
    from gpitch_amd.synth import make_problem
    from oracle import gpflow05 as orc
    prob = make_problem(400, 12, 1, num_partials=2, seed=2)
    model = pdgp_from_problem(prob, handle=gp_handle)
    model.za.fixed = True
    model.zc.fixed = True
    model.optimize(method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=3)
    # oracle trajectory over the same free-state coordinates
    import copy
    p = copy.deepcopy(prob)
    names_pos = ["noise", "act0.variance", "act0.lengthscales", "com0.variance", "com0.lengthscales",
                 "com0.energy0", "com0.energy1", "com0.frequency0", "com0.frequency1"]
    def get(p, name):
        if name == "noise": return np.array([p["noise_var"]])
        k, f = name.split(".")
        d = (p["kern_act"] if k.startswith("act") else p["kern_com"])[0]
        if f.startswith("energy"): return np.array([d["energy"][int(f[6:])]])
        if f.startswith("frequency"): return np.array([d["frequency"][int(f[9:])]])
        return np.array([d[f]])
    def put(p, name, v):
        v = float(v[0])
        if name == "noise": p["noise_var"] = v; return
        k, f = name.split(".")
        d = (p["kern_act"] if k.startswith("act") else p["kern_com"])[0]
        if f.startswith("energy"): d["energy"][int(f[6:])] = v
        elif f.startswith("frequency"): d["frequency"][int(f[9:])] = v
        else: d[f] = v
    ident = ["q_mu_act0", "q_mu_com0", "q_sqrt_act0", "q_sqrt_com0"]
    state = {n: orc.positive_backward(get(p, n)) for n in names_pos}
    for n in ident:
        state[n] = p[n[:-1]][0].copy()
    mom = {n: (np.zeros_like(v), np.zeros_like(v)) for n, v in state.items()}
    for t in range(1, 4):
        _, g = oracle_elbo_and_grads(p)
        for n in state:
            gc = g[n]
            if n in names_pos:
                gf = -gc.reshape(state[n].shape) / (1. + np.exp(-state[n]))
            else:
                gf = -gc
                if n.startswith("q_sqrt"):
                    gf = np.tril(gf[:, :, 0])[:, :, None]
            x, m_, v_ = orc.adam_step(state[n], gf, mom[n][0], mom[n][1], t, 0.01)
            state[n], mom[n] = x, (m_, v_)
        for n in names_pos:
            put(p, n, orc.positive_forward(state[n]))
        for n in ident:
            p[n[:-1]][0] = state[n]
    np.testing.assert_allclose(model.q_mu_act[0].value, p["q_mu_act"][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(model.q_sqrt_com[0].value, p["q_sqrt_com"][0], rtol=0, atol=1e-9)
    np.testing.assert_allclose(model.likelihood.variance.value, [p["noise_var"]], rtol=1e-9)
    np.testing.assert_allclose(model.kern_com[0].frequency[1].value, [p["kern_com"][0]["frequency"][1]], rtol=1e-10)
    np.testing.assert_allclose(model.kern_act[0].lengthscales.value, [p["kern_act"][0]["lengthscales"]], rtol=1e-9)


@pytest.mark.parametrize("name", ["pdgp_small_logistic", "pdgp_small_softplus", "pdgp_small_gauss"])
def test_hip_path_matches_committed_golden(gp_handle, name):
    """HIP ELBO / conditionals against the 50-digit golden vectors (tests/golden/*.npz): 1e-9 relative."""
    import gpitch_amd
    from gpitch_amd.pdgp import Pdgp
    from gpitch_amd.conditionals import conditional
    from test_oracle_golden import load_pdgp
    from helpers import kernels_from_problem
    prob, d = load_pdgp(name)
    nl = [gpitch_amd.logistic_tf, gpitch_amd.softplus_tf, gpitch_amd.gaussfun_tf][prob["nlin"]]
    kern = kernels_from_problem(prob)
    m = Pdgp(prob["x"], prob["y"], [prob["za"], prob["zc"]], kern, whiten=True, nlinfun=nl, handle=gp_handle)
    P = prob["P"]
    for i in range(P):
        m.q_mu_act[i].value = prob["q_mu_act"][i]; m.q_mu_com[i].value = prob["q_mu_com"][i]
        m.q_sqrt_act[i].value = prob["q_sqrt_act"][i]; m.q_sqrt_com[i].value = prob["q_sqrt_com"][i]
    m.likelihood.variance = prob["noise_var"]
    got = m.compute_log_likelihood()
    ref = float(d["elbo_white"])
    assert abs(got - ref) <= 1e-9 * abs(ref)
    assert abs(m.build_prior_kl() - float(d["kl_white"])) <= 1e-9 * abs(float(d["kl_white"]))
    ma, va, mc, vc, _ = m.predict_act_n_com(prob["x"])
    for i in range(P):
        np.testing.assert_allclose(ma[i][:, 0], d["fmean_white"][:, i], rtol=0, atol=1e-9 * np.abs(d["fmean_white"]).max())
        np.testing.assert_allclose(vc[i][:, 0], d["fvar_white"][:, P + i], rtol=0, atol=1e-9 * np.abs(d["fvar_white"]).max())
        # unwhitened conditional through the operator API
        fm, fv = conditional(prob["x"], prob["zc"][i], kern[1][i], prob["q_mu_com"][i], q_sqrt=prob["q_sqrt_com"][i], whiten=False)
        np.testing.assert_allclose(fm[:, 0], d["fmean_unwhite"][:, P + i], rtol=0, atol=1e-9 * np.abs(d["fmean_unwhite"]).max())
        np.testing.assert_allclose(fv[:, 0], d["fvar_unwhite"][:, P + i], rtol=0, atol=1e-9 * np.abs(d["fvar_unwhite"]).max())
    # unwhitened model: ELBO and prior KL (pdgp.py:122-129) against the golden values
    mu = Pdgp(prob["x"], prob["y"], [prob["za"], prob["zc"]], kernels_from_problem(prob), whiten=False, nlinfun=nl,
              handle=gp_handle)
    for i in range(P):
        mu.q_mu_act[i].value = prob["q_mu_act"][i]; mu.q_mu_com[i].value = prob["q_mu_com"][i]
        mu.q_sqrt_act[i].value = prob["q_sqrt_act"][i]; mu.q_sqrt_com[i].value = prob["q_sqrt_com"][i]
    mu.likelihood.variance = prob["noise_var"]
    gu = mu.compute_log_likelihood()
    assert abs(gu - float(d["elbo_unwhite"])) <= 1e-9 * abs(float(d["elbo_unwhite"]))
    assert abs(mu.build_prior_kl() - float(d["kl_unwhite"])) <= 1e-9 * abs(float(d["kl_unwhite"]))


def test_gradient_with_fixed_params_skips_work_but_stays_exact(gp_handle):
    """`.fixed = True` on inducing inputs / a whole kernel removes those entries from the gradient (zeros)
    and must leave every other entry unchanged."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(600, 24, 2, num_partials=3, seed=4)
    model = pdgp_from_problem(prob, handle=gp_handle)
    model.za.fixed = True
    model.zc.fixed = True
    model.kern_act[1].fixed = True          # one latent GP needs no kernel gradient at all
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob)
    assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f)
    got = model_grad_dict(model)
    for name, rg in ref_g.items():
        gg = got[name]
        if name.startswith("z") or name.startswith("act1."):
            assert np.all(gg == 0), name
            continue
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
        scale = max(np.abs(rg).max(), 1e-12)
        np.testing.assert_allclose(gg.reshape(rg.shape), rg, rtol=0, atol=2e-7 * scale, err_msg=name)


@pytest.mark.parametrize("N,M,P,m", [(1500, 40, 2, 3)])
def test_unwhitened_elbo_matches_oracle(gp_handle, N, M, P, m):
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=m, seed=9)
    model = pdgp_from_problem(prob, whiten=False, handle=gp_handle)
    got = model.compute_log_likelihood()
    ref = float(oracle_elbo(prob, whiten=False))
    # cond(Kuu) ~ 1e9 here (Matern32, l=1, 40 points in 94 ms): both sides carry ~cond*eps in the K^-1 terms
    assert abs(got - ref) <= 1e-6 * abs(ref), (got, ref)


@pytest.mark.parametrize("N,M,P,m,fixed", [(2000, 10, 1, 2, False), (2400, 12, 2, 3, False), (2400, 12, 2, 3, True)])
def test_unwhitened_gradient_matches_autograd(gp_handle, N, M, P, m, fixed):
    """whiten=False (pdgp.py:123-129, conditional(..., whiten=False)): gradient w.r.t. every parameter against torch
    autograd through the oracle.  Kuu^-1 enters q_mu / q_sqrt directly here, so the comparison carries
    cond(Kuu)*eps (cond ~ 1e7 for these sizes) on both sides."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=m, seed=4)
    model = pdgp_from_problem(prob, whiten=False, handle=gp_handle)
    if fixed:   # m.za.fixed / m.zc.fixed as in demo-modgp.py:40-41 (kernel chain still needed for theta)
        model.za.fixed = True
        model.zc.fixed = True
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob, whiten=False)
    assert abs(f - ref_f) <= 1e-7 * abs(ref_f)
    got_g = model_grad_dict(model)
    worst = 0.0
    for name, rg in ref_g.items():
        gg = got_g[name]
        if fixed and name.startswith("z"):
            assert np.all(gg == 0)
            continue
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
            assert np.all(np.triu(gg[:, :, 0], 1) == 0)
        scale = max(np.abs(rg).max(), 1e-12)
        err = np.abs(gg.reshape(rg.shape) - rg).max() / scale
        worst = max(worst, err)
        assert err <= 1e-7, (name, err)
    print("unwhitened gradient worst scaled error", worst)


@pytest.mark.parametrize("whiten", [True, False])
def test_legacy_matern12sm_gradient_matches_autograd(gp_handle, whiten):
    """component kernel = the broadcast-form Matern12sm (matern12_spectral_mixture.py:38-56) instead of the Mercer
    form: ELBO and every gradient (variance, lengthscale, energies, frequencies, z, q) against autograd"""
    from gpitch_amd.synth import make_problem
    prob = make_problem(600, 14, 2, num_partials=3, seed=8)
    for d in prob["kern_com"]:
        d["type"] = "matern12sm"
    model = pdgp_from_problem(prob, whiten=whiten, handle=gp_handle)
    for kk in model.kern_com:                    # the reference fixes these by default (:34,64-67); free them here so
        kk.vars_n_freqs_fixed(False, False)      # that the engine's full gradient vector is compared
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob, whiten=whiten)
    assert abs(f - ref_f) <= 1e-8 * abs(ref_f)
    got_g = model_grad_dict(model)
    for name, rg in ref_g.items():
        gg = got_g[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
        scale = max(np.abs(rg).max(), 1e-12)
        err = np.abs(gg.reshape(rg.shape) - rg).max() / scale
        assert err <= 1e-6, (name, err)


@pytest.mark.parametrize("ktype", ["matern32sm", "mercer_matern52sm"])
@pytest.mark.parametrize("whiten", [True, False])
def test_older_component_kernels_gradient_matches_autograd(gp_handle, ktype, whiten):
    """component kernel = Matern32sm (kernels.py:204-258, init_models.py:84) or the
    Matern52 * MercerCosMix product (init_models.py:183-198): ELBO and every gradient against autograd"""
    from gpitch_amd.synth import make_problem
    prob = make_problem(640, 12, 2, num_partials=3, seed=12)
    for d in prob["kern_com"]:
        d["type"] = ktype
        if ktype == "matern32sm":
            d["variance"] = 1.0                       # no global variance in this kernel
            d["energy"] = [0.2 * e for e in d["energy"]]   # variance_k ~ Logistic(0, 0.25)
            d["lengthscales"] = 0.02     # envelope decays inside the 40 ms window: keeps Kuu well conditioned
        else:
            d["variance"] = 0.25
            d["lengthscales"] = 0.25
    model = pdgp_from_problem(prob, whiten=whiten, handle=gp_handle)
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob, whiten=whiten)
    assert abs(f - ref_f) <= 1e-8 * abs(ref_f)
    got_g = model_grad_dict(model)
    for name, rg in ref_g.items():
        gg = got_g[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
        scale = max(np.abs(rg).max(), 1e-12)
        err = np.abs(gg.reshape(rg.shape) - rg).max() / scale
        assert err <= 1e-6, (name, err)
    # and the model trains through the Logistic transforms: a few Adam steps raise the full-batch ELBO
    import gpitch_amd
    before = model.compute_log_likelihood()
    model.optimize(method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=15)
    after = model.compute_log_likelihood()
    assert np.isfinite(after) and after > before
    for kk in model.kern_com:
        if ktype == "matern32sm":
            assert 0. < kk.lengthscales.value[0] < 2.
            assert all(0. < v.value[0] < 0.25 for v in kk.variance)


def test_minibatch_elbo_scaling_and_pairing(gp_handle):
    """minibatch_size < N: GPflow's MinibatchData draws WITH replacement when mb/N < 0.5 (x and y generators are
    seeded identically, pdgp.py:76-77) and the ELBO is rescaled by N/mb (pdgp.py:168-169)."""
    from gpitch_amd.synth import make_problem
    from oracle import gpflow05 as orc
    prob = make_problem(3000, 30, 2, num_partials=3, seed=6)
    mb = 100
    model = pdgp_from_problem(prob, minibatch_size=mb, handle=gp_handle)
    got = model.compute_log_likelihood()
    idx = orc.minibatch_indices(np.random.RandomState(0), 3000, mb)      # first draw of the same seeded generator
    ref = orc.pdgp_elbo(prob["x"][idx], prob["y"][idx], prob["za"], prob["zc"], prob["kern_act"], prob["kern_com"],
                        prob["q_mu_act"], prob["q_sqrt_act"], prob["q_mu_com"], prob["q_sqrt_com"], prob["noise_var"],
                        num_data=3000)
    assert abs(got - float(ref)) <= ELBO_RTOL * abs(float(ref))
    got2 = model.compute_log_likelihood()                                  # a fresh minibatch every call
    assert got2 != got


def test_ragged_inducing_counts_and_single_frame(gp_handle):
    """M differs per source and per role (pdgp.py:93-94); N = 1 frame; M = 1 inducing point."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(257, 20, 2, num_partials=2, seed=8)
    prob["za"][1] = prob["za"][1][:7].copy(); prob["q_mu_act"][1] = prob["q_mu_act"][1][:7].copy()
    prob["q_sqrt_act"][1] = prob["q_sqrt_act"][1][:7, :7].copy()
    prob["zc"][0] = prob["zc"][0][:1].copy(); prob["q_mu_com"][0] = prob["q_mu_com"][0][:1].copy()
    prob["q_sqrt_com"][0] = prob["q_sqrt_com"][0][:1, :1].copy()
    model = pdgp_from_problem(prob, handle=gp_handle)
    got = model.compute_log_likelihood()
    ref = float(oracle_elbo(prob))
    assert abs(got - ref) <= ELBO_RTOL * abs(ref)
    one = dict(prob); one["x"] = prob["x"][:1].copy(); one["y"] = prob["y"][:1].copy(); one["N"] = 1
    m1 = pdgp_from_problem(one, handle=gp_handle)
    g1 = m1.compute_log_likelihood()
    r1 = float(oracle_elbo(one))
    assert abs(g1 - r1) <= ELBO_RTOL * abs(r1)


@pytest.mark.gpu
@pytest.mark.parametrize("P,world,whiten", [(3, 2, True), (5, 3, True), (2, 2, False)])
def test_pitch_sharded_two_stage_matches_unsharded(gp_handle, P, world, whiten):
    """One model spread over `world` ranks (gp_pdgp_elbo_begin -> sum of the 3n+1 exchange vectors ->
    gp_pdgp_elbo_end), the ranks emulated in this process: every rank must report the whole model's ELBO and
    its slice of the unsharded gradient (the pair sum C of likelihoods.py:56-65 becomes A^2 - D)."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(900, 24, P, num_partials=3, seed=11)
    full = pdgp_from_problem(prob, whiten=whiten, handle=gp_handle)
    full._pack()
    e_full = full._elbo(whiten)
    g_full = model_grad_dict(full) if whiten else None
    kl_full = float(full._elbo_dev[1].item())
    shards = [pdgp_from_problem(prob, whiten=whiten, handle=gp_handle, shard=(r, world)) for r in range(world)]
    for s in shards:
        s._pack()
    parts = [s._elbo_begin(whiten).clone() for s in shards]
    total = sum(parts)
    seen = set()
    for s in shards:
        s._xchg[:total.numel()].copy_(total)
        e = s._elbo_end(whiten)
        assert abs(e - e_full) <= 1e-10 * abs(e_full)
        assert abs(float(s._elbo_dev[1].item()) - kl_full) <= 1e-10 * max(1.0, abs(kl_full))
        if whiten:
            gs = model_grad_dict(s)
            for k, v in gs.items():
                ref = g_full[k]
                assert np.allclose(v, ref, rtol=1e-8, atol=1e-9 * max(1.0, np.abs(ref).max())), k
                seen.add(k)
    if whiten:
        assert seen == set(g_full.keys())
    # predictions: each rank fills its own rows (the sum over ranks assembles the list)
    xs = prob["x"][::7]
    ref = full.predict_act_n_com(xs)
    for s in shards:
        object.__setattr__(s, "_pred_allow_local", True)      # emulated ranks in one process: no process group to sum over
    got = [s._predict(xs, True) for s in shards]
    fm = sum(g[0] for g in got)
    src = sum(g[2] for g in got)
    for i in range(P):
        assert np.allclose(fm[i].reshape(-1, 1), ref[0][i], rtol=1e-10, atol=1e-12)
        assert np.allclose(fm[P + i].reshape(-1, 1), ref[2][i], rtol=1e-10, atol=1e-12)
        assert np.allclose(src[i].reshape(-1, 1), ref[4][i], rtol=1e-10, atol=1e-12)


@pytest.mark.gpu
def test_sharded_predict_needs_its_process_group(gp_handle):
    """A sharded model's predictions are a sum over ranks; without an initialised group of that size the result would be the
    local rows with zeros elsewhere — refused instead of returned."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(512, 16, 2, num_partials=2, seed=3)
    m = pdgp_from_problem(prob, handle=gp_handle, shard=(0, 2))
    with pytest.raises(RuntimeError, match="sharded over 2 ranks"):
        m._predict(prob["x"][::5], True)


def test_pitch_sharded_end_requires_matching_begin(gp_handle):
    from gpitch_amd.synth import make_problem
    prob = make_problem(200, 8, 2, num_partials=2, seed=3)
    s = pdgp_from_problem(prob, handle=gp_handle, shard=(0, 2))
    s._pack()
    s._batch_keep = s._batch()
    s._last_batch = s._batch_keep[:2]
    with pytest.raises(Exception):
        s._elbo_end(True)


def test_predictions_reuse_factorisation_and_memoise(gp_handle):
    """predict_windowed (pdgp.py:17-44) calls predict_act and predict_com per window: here the pair is one engine
    evaluation and later windows reuse Kuu's factorisation (gp_pdgp_predict_reuse) until a Param changes."""
    import ctypes as C
    from gpitch_amd.synth import make_problem
    from gpitch_amd.pdgp import predict_windowed
    prob = make_problem(1200, 20, 2, num_partials=3, seed=2)
    m = pdgp_from_problem(prob, handle=gp_handle)
    x = prob["x"]
    ref = pdgp_from_problem(prob, handle=gp_handle)          # fresh model: every call factorises
    full = ref.predict_act_n_com(x)
    out = predict_windowed(m, x, ws=300)
    for j in range(2):
        np.testing.assert_allclose(out[0][j], full[0][j], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(out[1][j], full[1][j], rtol=1e-11, atol=1e-14)
        np.testing.assert_allclose(out[2][j], full[2][j], rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(out[3][j], full[3][j], rtol=1e-11, atol=1e-14)
    # a parameter change invalidates both the memo and the factorisation
    m.kern_act[0].lengthscales = 0.7
    ref.kern_act[0].lengthscales = 0.7
    a1 = m.predict_act(x[:300])
    a2 = ref.predict_act(x[:300])
    np.testing.assert_allclose(a1[0][0], a2[0][0], rtol=1e-12, atol=1e-14)
    assert not np.allclose(a1[0][0], out[0][0][:300])
    # reuse without a preceding factorisation is refused by the library
    fresh = pdgp_from_problem(prob, handle=gp_handle)
    fresh._pack()
    h = fresh._handle
    xs = h.to_device(x[:10].reshape(-1))
    fm, fv = h.empty(4, 10), h.empty(4, 10)
    with pytest.raises(Exception):
        h.check(h.lib.gp_pdgp_predict_reuse(fresh._plan, fresh._params.data_ptr(), xs.data_ptr(), 10, fm.data_ptr(),
                                            fv.data_ptr(), None))


def test_prediction_at_no_inputs_records_no_factorisation(gp_handle):
    """predict_act at an empty xnew factors nothing, so the next prediction of the fresh model must not ask the engine
    to reuse a factorisation: it returns what it returns on a model that never saw the empty call"""
    from gpitch_amd.synth import make_problem
    prob = make_problem(1200, 20, 2, num_partials=3, seed=2)
    m, alone = pdgp_from_problem(prob, handle=gp_handle), pdgp_from_problem(prob, handle=gp_handle)
    x = prob["x"][:300]
    empty = m.predict_act(x[:0])
    assert [a.shape for a in empty[0] + empty[1]] == [(0, 1)] * 4
    for got, want in zip(m.predict_act(x), alone.predict_act(x)):
        for a, b in zip(got, want):
            np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("N", [900, 4200])
def test_blocked_kuu_factorisation_with_partial_last_panel(gp_handle, N):
    """M > 256 switches the Kuu batch to the panel-blocked Cholesky + inverse (engine.hip: cond_batch_factorize);
    M = 300 leaves a 44-column last panel.  N = 900: every panel through the batched GEMMs; N = 4200 (a long batch,
    the Kuf builds fill the device): whole-matrix factor in one resident launch, then the blocked inverse.  ELBO and
    gradients against the oracle (cond(Kuu) ~ 1e9 here, so the comparison carries cond * eps on both sides)."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, 300, 1, num_partials=3, seed=6)
    model = pdgp_from_problem(prob, handle=gp_handle)
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob)
    assert abs(f - ref_f) <= 1e-7 * abs(ref_f), (f, ref_f)
    got_g = model_grad_dict(model)
    for name, rg in ref_g.items():
        gg = got_g[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
            assert np.all(np.triu(gg[:, :, 0], 1) == 0)
        scale = max(np.abs(rg).max(), 1e-12)
        err = np.abs(gg.reshape(rg.shape) - rg).max() / scale
        assert err <= 2e-4, (name, err)
    # the factor itself: L L^T reproduces Kuu + jitter I, W L = I (through the one-shot operator path, M = 300 single
    # workgroup) vs the blocked batch path above is covered by the ELBO; here the prediction path at M = 300
    xs = prob["x"][::9]
    ma, va, mc, vc, ms = model.predict_act_n_com(xs)
    from oracle import gpflow05 as orc
    rm, rv = orc.conditional(xs, prob["za"][0], prob["kern_act"][0], prob["q_mu_act"][0], prob["q_sqrt_act"][0], whiten=True)
    np.testing.assert_allclose(ma[0], rm, rtol=0, atol=1e-6 * np.abs(rm).max())


def test_headline_M512_blocked_factorisation_gradient_vs_autograd(gp_handle):
    """M = 512 (the bench shape's inducing count: four 128-column panels, resident factor + blocked inverse, 4 x 4
    tile grids in every strip product) at P = 1 and a batch the oracle differentiates in seconds: the ELBO and every
    gradient entry against torch autograd through the oracle.  cond(Kuu) ~ 1e9, so both sides carry cond * eps."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(8192, 512, 1, num_partials=5, seed=21)
    model = pdgp_from_problem(prob, handle=gp_handle)
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob)
    assert abs(f - ref_f) <= 1e-8 * abs(ref_f), (f, ref_f)
    got_g = model_grad_dict(model)
    worst = {}
    for name, rg in ref_g.items():
        gg = got_g[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
            assert np.all(np.triu(gg[:, :, 0], 1) == 0)
        scale = max(np.abs(rg).max(), 1e-12)
        worst[name] = np.abs(gg.reshape(rg.shape) - rg).max() / scale
    bad = {k: v for k, v in worst.items() if v > 2e-5}
    assert not bad, bad


# The cases beyond the first two walk other orders of the backward schedule at the smallest forking batch (N = 4096, M = 64):
#   mixed: float64 activations, float32 components (the benchmark's `mixed` line); zc: trainable component inducing inputs, a
#   family contracted GP by GP; two_act: Matern-3/2 and Matern-1/2 activations, three families, the schedule without the
#   two-family split.
# Not here: float32 strips (P = 2) and whiten=False (P = 1).  Their bits agree at every level, their kuf_bar launch counts
# do not: no family of theirs takes a route of its own, so levels 0 and 1 form Kuf_bar in ONE launch over the whole batch
# and level 2, which issues it family by family, in two.
OVERLAP_CASES = [
    pytest.param(4096, 48, 2, None, id="4096-48-2"),
    pytest.param(4200, 300, 1, None, id="4200-300-1"),
    pytest.param(4096, 64, 2, "mixed", id="4096-64-2-mixed"),
    pytest.param(4096, 64, 2, "zc", id="4096-64-2-zc"),
    pytest.param(4096, 64, 2, "two_act", id="4096-64-2-two_act"),
]


@pytest.mark.parametrize("N,M,P,case", OVERLAP_CASES)
def test_overlap_levels_give_identical_results(gp_handle, N, M, P, case):
    """gp_pdgp_set_overlap changes only the schedule (helper-stream fork / join points); the ELBO and every gradient
    entry must come out bit for bit the same at every level (batches of >= 4096 frames are the ones that fork;
    M = 300 takes the resident-factor + blocked-inverse route, chosen by N and M alone), and so must the number of
    launches charged to the kuf_bar, nt_gemm and hyper timers: the level moves launches between streams, it neither
    adds nor drops one."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=3, seed=13)
    kw = {}
    if case == "mixed":
        kw = dict(float_type=(np.float64, np.float32))
    elif case == "two_act":
        prob["kern_act"][0]["type"], prob["kern_act"][1]["type"] = "matern32", "matern12"
    h = gp_handle
    ref = ref_counts = None
    for level in (0, 1, 2, 1, 0):
        m = pdgp_from_problem(prob, handle=h, **kw)
        m.za.fixed = True
        m.zc.fixed = (case != "zc")
        m._pack()
        h.check(h.lib.gp_pdgp_set_overlap(m._plan, level))
        vals = []
        for _ in range(2):                      # the second evaluation (a fresh frame permutation, identically seeded in
            f = m._elbo(True)                   # every model) reuses descriptors and streams
            vals.append((f, m._grad.cpu().numpy().copy()))
        h.check(h.lib.gp_timers_enable(h.h, 1))
        h.check(h.lib.gp_timers_reset(h.h))
        try:
            m._elbo(True)
            h.sync()
            counts = {k: h.timers()[k][1] for k in ("kuf_bar", "nt_gemm", "hyper")}
        finally:
            h.check(h.lib.gp_timers_enable(h.h, 0))
        print("%s level %d: ELBO %r launches %r" % (case, level, vals[0][0], counts))
        if ref is None:
            ref, ref_counts = vals, counts
        else:
            for a, b in zip(vals, ref):
                assert a[0] == b[0], level
                assert np.array_equal(a[1], b[1]), level
            assert counts == ref_counts, (level, counts, ref_counts)
    with pytest.raises(Exception):
        h.check(h.lib.gp_pdgp_set_overlap(m._plan, 3))


def test_adam_stops_at_a_failed_cholesky_and_leaves_the_state_alone(gp_handle):
    """GPflow / TF raise InvalidArgumentError at the step whose tf.cholesky fails.  The sync-free Adam loop polls a
    device flag instead: gp_adam_step freezes free state, parameters and moments while it is set, and the loop raises
    at the next poll that has seen it (well before maxiter)."""
    import gpitch_amd
    from gpitch_amd import _lib
    from gpitch_amd.param import transforms
    from gpitch_amd.synth import make_problem
    prob = make_problem(4096, 32, 1, num_partials=2, seed=4)
    model = pdgp_from_problem(prob, handle=gp_handle)
    model.kern_act[0].variance.transform = transforms.Identity()
    model.kern_act[0].variance = -1.0             # Kuu = -K: the first pivot is negative
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    before = model._free.cpu().numpy().copy()
    calls = []
    with pytest.raises(_lib.NotPositiveDefiniteError):
        model.optimize(method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=400, callback=lambda x: calls.append(1))
    assert len(calls) < 400                      # stopped inside the loop, not at its end
    np.testing.assert_array_equal(model._free.cpu().numpy(), before)     # no update from the garbage gradients
    assert np.all(model._adam_m.cpu().numpy() == 0)
    # the handle is usable again afterwards
    model.kern_act[0].variance = 1.0
    assert np.isfinite(model.compute_log_likelihood())


@pytest.mark.parametrize("ls,ktype", [(0.1, None), (0.002, None), (5.0, None), (0.05, "mercer_matern52sm")])
def test_separable_envelope_paths_match_autograd(gp_handle, ls, ktype):
    """The Kuf build and the Kuf-side contraction factorise the envelope for entries a lengthscale away from the band
    (cov.hip / bwd.hip "separable envelope"); inside it, and whenever a tile straddles it, they run entry by entry.
    ls = 0.1: both in one strip (the bench's case); 0.002: nearly everything separable, factors underflowing to 0 far
    out; 5.0: nothing separable.  The same problem with its data rows shuffled puts the whole signal into every tile,
    i.e. runs the entry-by-entry path alone: the two must agree far below the parity bar, and both with autograd
    through the oracle (inducing inputs fixed: the matrix-core contraction)."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(16384, 64, 1, num_partials=3, seed=5)
    prob["kern_com"][0]["lengthscales"] = ls
    if ktype:                                 # the Matern-5/2 envelope of the product kernel (init_models.py:183-198)
        prob["kern_com"][0]["type"] = ktype
        prob["kern_com"][0]["variance"] = 0.25

    def run(pr):
        model = pdgp_from_problem(pr, handle=gp_handle)
        model.za.fixed = True
        model.zc.fixed = True
        model._pack()
        return model._elbo(True), model_grad_dict(model)
    f, got_g = run(prob)
    shuf = dict(prob)
    perm = np.random.RandomState(0).permutation(prob["N"])
    shuf["x"], shuf["y"] = prob["x"][perm], prob["y"][perm]
    f2, got_g2 = run(shuf)
    assert abs(f - f2) <= 1e-11 * abs(f), (f, f2)
    for name, g1 in got_g.items():
        if name.startswith("z"):
            continue
        scale = max(np.abs(g1).max(), 1e-12)
        np.testing.assert_allclose(got_g2[name], g1, rtol=0, atol=1e-9 * scale, err_msg="separable vs entry-by-entry: " + name)
    ref_f, ref_g = oracle_elbo_and_grads(prob)
    assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f), (f, ref_f)
    # at l = 0.002 the scaled inputs reach 500 and the reference's expanded square (a^2 - 2ab + b^2) loses 1e-5 of the
    # lengthscale gradient to cancellation — autograd through the oracle moves by that much when the rows are shuffled
    tol = (2e-7 if not ktype else 1e-6) if ls >= 0.05 else 1e-4
    for name, rg in ref_g.items():
        if name.startswith("za") or name.startswith("zc"):
            continue
        gg = got_g[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
        scale = max(np.abs(rg).max(), 1e-12)
        np.testing.assert_allclose(gg.reshape(rg.shape), rg, rtol=0, atol=tol * scale, err_msg=name)


@pytest.mark.parametrize("ktype,ls", [("matern32", 1.0), ("matern12", 0.3), ("matern52", 0.05), ("rbf", 0.02)])
def test_fused_kuf_bar_contraction_matches_autograd(gp_handle, ktype, ls):
    """Stationary activation kernels with fixed inducing inputs, float64 strips and whole 128-tiles (M = 128, N = 4096: the
    bench's situation in small) take the form of the Kuf_bar product that contracts its tile with dK/d(variance,
    lengthscale) in the epilogue and stores nothing (gemm_strip.hip role 5).  Every gradient entry against torch autograd
    through the oracle, for the four stationary types; the overlap levels (which pick different launch orders around it)
    must still agree bit for bit."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(4096, 128, 2, num_partials=3, seed=7)
    for d in prob["kern_act"]:
        d["type"] = ktype
        d["lengthscales"] = ls
    ref_f, ref_g = oracle_elbo_and_grads(prob)
    first = None
    for level in (2, 0, 1):
        model = pdgp_from_problem(prob, handle=gp_handle)
        model.za.fixed = True
        model.zc.fixed = True
        model._pack()
        gp_handle.check(gp_handle.lib.gp_pdgp_set_overlap(model._plan, level))
        f = model._elbo(True)
        g = model._grad.cpu().numpy().copy()
        if first is None:
            first = (f, g)
            assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f), (f, ref_f)
            got_g = model_grad_dict(model)
            worst = 0.0
            for name, rg in ref_g.items():
                if name.startswith("z"):
                    continue
                gg = got_g[name]
                if name.startswith("q_sqrt"):
                    rg = np.tril(rg[:, :, 0])[:, :, None]
                scale = max(np.abs(rg).max(), 1e-12)
                err = np.abs(gg.reshape(rg.shape) - rg).max() / scale
                worst = max(worst, err)
                assert err <= 1e-6, (name, err)
            print("fused Kuf_bar contraction (%s): worst gradient block deviation %.2e" % (ktype, worst))
        else:
            assert f == first[0] and np.array_equal(g, first[1]), level


@pytest.mark.parametrize("P,world,whiten", [(3, 2, True), (5, 3, True), (4, 8, True), (2, 3, False)])
def test_gp_sharded_two_stage_matches_unsharded(gp_handle, P, world, whiten):
    """SURVEY section 8e option 2: ONE model with its 2P latent GPs dealt over `world` ranks (gp_pdgp_cond_begin -> all-gather of
    (fmean, fvar) per GP + the KL scalar -> gp_pdgp_cond_end), the ranks emulated in this process (world = 3 with 2P = 10 / 4:
    ranks with one GP fewer pad their block; world = 8 with P = 4: one GP per rank, an activation GP and its component GP on
    different ranks).  Every rank must report the whole model's ELBO and its own slice of the unsharded gradient."""
    import torch
    from gpitch_amd.synth import make_problem
    prob = make_problem(900, 24, P, num_partials=3, seed=13)
    full = pdgp_from_problem(prob, whiten=whiten, handle=gp_handle)
    full._pack()
    e_full = full._elbo(whiten)
    g_full = model_grad_dict(full) if whiten else None
    kl_full = float(full._elbo_dev[1].item())
    shards = [pdgp_from_problem(prob, whiten=whiten, handle=gp_handle, shard=("gp", r, world)) for r in range(world)]
    for s in shards:
        s._pack()
    assert sorted(g for s in shards for g in s._gp_shard) == list(range(2 * P))
    gathered = torch.cat([s._gp_begin(whiten).clone() for s in shards])
    seen = set()
    for s in shards:
        e = s._gp_end(whiten, gathered)
        assert abs(e - e_full) <= 1e-10 * abs(e_full), (e, e_full)
        assert abs(float(s._elbo_dev[1].item()) - kl_full) <= 1e-10 * max(1.0, abs(kl_full))
        if whiten:
            g = s._grad.cpu().numpy()
            assert np.allclose(g[0:1], g_full["noise"], rtol=1e-8, atol=1e-9 * max(1.0, abs(g_full["noise"][0])))
            for l, gi in enumerate(s._gp_shard):
                act = gi < P
                i = gi if act else gi - P
                name = ("act%d" if act else "com%d") % i
                kern = (s.kern_act if act else s.kern_com)[i]
                o_th, o_z, o_mu, o_sq = s._layout[l]
                M, mp = (s.num_inducing_a if act else s.num_inducing_c)[i], int(kern.num_partials)
                got = {name + ".variance": g[o_th:o_th + 1], name + ".lengthscales": g[o_th + 1:o_th + 2],
                       ("za%d" if act else "zc%d") % i: g[o_z:o_z + M].reshape(-1, 1),
                       ("q_mu_act%d" if act else "q_mu_com%d") % i: g[o_mu:o_mu + M].reshape(-1, 1),
                       ("q_sqrt_act%d" if act else "q_sqrt_com%d") % i: g[o_sq:o_sq + M * M].reshape(M, M, 1)}
                for j in range(mp):
                    got["%s.energy%d" % (name, j)] = g[o_th + 2 + j:o_th + 3 + j]
                    got["%s.frequency%d" % (name, j)] = g[o_th + 2 + mp + j:o_th + 3 + mp + j]
                for k, v in got.items():
                    ref = g_full[k]
                    assert np.allclose(v, ref, rtol=1e-8, atol=1e-9 * max(1.0, np.abs(ref).max())), (k, gi)
                    seen.add(k)
    if whiten:
        assert seen | {"noise"} == set(g_full.keys())
    # predictions: each rank fills its own rows; the sum over ranks (the all-reduce of _predict) assembles them
    xs = prob["x"][::7]
    ref = full.predict_act_n_com(xs)
    for s in shards:
        object.__setattr__(s, "_pred_allow_local", True)      # emulated ranks in one process: no process group to sum over
    fm = sum(s._predict(xs, True)[0] for s in shards)
    for i in range(P):
        assert np.allclose(fm[i].reshape(-1, 1), ref[0][i], rtol=1e-10, atol=1e-12)
        assert np.allclose(fm[P + i].reshape(-1, 1), ref[2][i], rtol=1e-10, atol=1e-12)
    src = shards[0].nlinfun(fm[:P]) * fm[P:]
    for i in range(P):
        assert np.allclose(src[i].reshape(-1, 1), ref[4][i], rtol=1e-10, atol=1e-12)


def test_gp_sharded_adam_steps_follow_the_unsharded_model(gp_handle):
    """three Adam steps of a 2-rank GP-sharded model (ranks emulated, the exchange done by hand) against the unsharded
    model's: each rank updates only its own slice, the replicated noise variance stays in step"""
    import ctypes as C
    import torch
    import gpitch_amd
    from gpitch_amd.synth import make_problem
    prob = make_problem(700, 20, 2, num_partials=3, seed=5)
    full = pdgp_from_problem(prob, handle=gp_handle)
    full.za.fixed = True
    full.zc.fixed = True
    full.optimize(method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=3)
    shards = [pdgp_from_problem(prob, handle=gp_handle, shard=("gp", r, 2)) for r in range(2)]
    opt = gpitch_amd.train.AdamOptimizer(0.01)
    for s in shards:
        s.za.fixed = True
        s.zc.fixed = True
        s._pack()
    for it in range(3):
        gathered = torch.cat([s._gp_begin(True).clone() for s in shards])
        for s in shards:
            h = s._handle
            s._gp_end(True, gathered, sync=False)
            s._adam_t += 1
            h.check(h.lib.gp_adam_step(h.h, s._free.data_ptr(), s._params.data_ptr(), s._grad.data_ptr(),
                                       s._tcode.data_ptr(), s._adam_m.data_ptr(), s._adam_v.data_ptr(), s._nparams,
                                       s._adam_t, opt.learning_rate, opt.beta1, opt.beta2, opt.epsilon))
    for s in shards:
        s._unpack()
        assert abs(s.likelihood.variance.value[0] - full.likelihood.variance.value[0]) <= 1e-12
        for gi in s._gp_shard:
            act, i = (True, gi) if gi < 2 else (False, gi - 2)
            for a, b in zip((s.kern_act if act else s.kern_com)[i].theta_params(),
                            (full.kern_act if act else full.kern_com)[i].theta_params()):
                np.testing.assert_allclose(a.value, b.value, rtol=1e-10)
            np.testing.assert_allclose((s.q_mu_act if act else s.q_mu_com)[i].value,
                                       (full.q_mu_act if act else full.q_mu_com)[i].value, rtol=0, atol=1e-11)
            np.testing.assert_allclose((s.q_sqrt_act if act else s.q_sqrt_com)[i].value,
                                       (full.q_sqrt_act if act else full.q_sqrt_com)[i].value, rtol=0, atol=1e-11)


def test_cluster_factorisation_with_two_inducing_set_sizes(gp_handle):
    """activation GPs on 192 inducing points, component GPs on 128 (both whole 32-row tiles, N >= 4096: the Kuu batch of four
    matrices of two sizes takes the workgroup-cluster factorisation, workgroups per matrix by the larger size): ELBO and
    gradient against the oracle"""
    from gpitch_amd.synth import make_problem, uniform_inducing
    N, P, m = 4608, 2, 3
    prob = make_problem(N, 192, P, num_partials=m, seed=5)
    rq = np.random.RandomState(11)
    Mc = 128
    prob["zc"] = [uniform_inducing(prob["x"], Mc) for _ in range(P)]
    prob["q_mu_com"] = [0.3 * rq.randn(Mc, 1) for _ in range(P)]
    prob["q_sqrt_com"] = [np.tril(np.eye(Mc) + 0.05 * rq.randn(Mc, Mc))[:, :, None] for _ in range(P)]
    model = pdgp_from_problem(prob, handle=gp_handle)
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob)
    assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f), (f, ref_f)
    got_g = model_grad_dict(model)
    for name, rg in ref_g.items():
        gg = got_g[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
        scale = max(np.abs(rg).max(), 1e-12)
        np.testing.assert_allclose(gg.reshape(rg.shape), rg, rtol=0, atol=2e-7 * scale, err_msg=name)
