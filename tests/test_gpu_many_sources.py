"""The likelihood kernels beyond sixteen sources and at their source-count limits.  mpd_lik_kernel, mpd_moments_kernel
(csrc/lik.hip), mpd_moments_frame (csrc/gh_quad.h) and pdgpb_pred_moments_kernel (csrc/pdgp_batch.hip) deal the sources
of a frame to sixteen lanes, lane l taking sources l, l + 16, ...; every other test of the suite stops at P = 12, where
no lane makes a second trip.  Here: the operators at every lane-wrap position and at the largest accepted counts (128
for the likelihood, 96 for the moments), the ragged last frame block and the second trip of finish_sum_kernel, the
gradient pass through a model, both sharded forms past their chunk sizes, a batch that mixes wide and narrow models, and
the refusals one source above the limits.  References: oracle.gpflow05 (float64 numpy, torch autograd through it)."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest

from helpers import model_grad_dict, oracle_elbo_and_grads, pdgp_from_problem
from test_gpu_pdgp_batch import _assert_same_objective, _batch_grad_dict, _block_err, _build
from test_gpu_predict_moments import (_check_against_ref, _close, _operator, _oracle_model_moments, _ref_moments, _same_bits,
                                      _targets)
from test_oracle_many_sources import LANES, NOISE, many_source_inputs

pytestmark = pytest.mark.gpu

LIK_MAX_P = 128     # launch_mpd_lik: 16 frames x 3 P doubles of LDS staging <= 48 KiB
MOM_MAX_P = 96      # launch_mpd_moments, gp_pdgpb_predict_moments: 16 frames x 4 P doubles <= 48 KiB
LIK_REFUSAL = "too many sources for the likelihood kernel's LDS staging"
MOM_REFUSAL = "too many sources for the moments kernel's LDS staging"


# ---- 1, 2: the operators ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _operator_case(P, N, nlin):
    """inputs and oracle values of one operator case, computed once and never written to"""
    from oracle import gpflow05 as orc
    Fmu, Fvar, Y = many_source_inputs(P, N, nlin)
    ve = orc.mpd_variational_expectations(Fmu, Fvar, Y, NOISE, P, nlin)
    mom = _ref_moments(Fmu, Fvar, P, nlin, NOISE, Y) if P <= MOM_MAX_P else None
    for a in (Fmu, Fvar, Y, ve):
        a.setflags(write=False)
    return Fmu, Fvar, Y, ve, mom


def _varexp(h, Fmu, Fvar, Y, P, nlin):
    """gp_mpd_varexp on host arrays through the raw C-ABI: per_frame (N,) and the sum it returns to the host"""
    N = Fmu.shape[0]
    dmu, dvar, dy, nv = h.to_device(Fmu), h.to_device(Fvar), h.to_device(Y.reshape(-1)), h.to_device(np.array([NOISE]))
    pf = h.empty(N)
    s = C.c_double()
    h.check(h.lib.gp_mpd_varexp(h.h, dmu.data_ptr(), dvar.data_ptr(), dy.data_ptr(), N, P, nlin, nv.data_ptr(),
                                pf.data_ptr(), C.byref(s)))
    h.sync()
    return pf.cpu().numpy(), s.value


def _check_varexp(pf, s, ve, tag):
    """the bar of test_gpu_ops.py::test_mpd_varexp_matches_oracle"""
    err = float(np.max(np.abs(pf - ve[:, 0]) / np.abs(ve[:, 0])))
    print("%s: per_frame max relative difference %.3g, sum %.3g (bar 1e-11)" % (tag, err, abs(s - ve.sum()) / abs(ve.sum())))
    np.testing.assert_allclose(pf, ve[:, 0], rtol=1e-11, atol=1e-11)
    assert abs(s - ve.sum()) <= 1e-11 * abs(ve.sum()), (tag, s, ve.sum())


_WRAP_CASES = ([(P, 0, 49) for P in (16, 31, 32, MOM_MAX_P, LIK_MAX_P)]
               + [(P, nlin, 49) for P in (17, 33) for nlin in (0, 1, 2)]
               + [(17, 0, N) for N in (1, 15, 16, 17)])


@pytest.mark.parametrize("P,nlin,N", _WRAP_CASES)
def test_operators_at_every_lane_wrap_position(gp_handle, P, nlin, N):
    """gp_mpd_varexp (per_frame and the host sum) against orc.mpd_variational_expectations, and for P <= 96 all five
    outputs of gp_mpd_predict_moments against the oracle composition at that file's bars, with logp equal to per_frame bit
    for bit (the two kernels do the same arithmetic in the same order).  P = 16 | 17 and 32 | 33 sit either side of a
    lane's second and third trip; 96 and 128 are the largest counts the moments and the likelihood kernel accept (the
    moments kernel refuses 128: the likelihood operator alone).  N = 49 is three blocks of 16 frames and one ragged frame;
    N = 1, 15, 16, 17 at P = 17 are the ragged last block on its own.

    Tolerance: the operator's bar, rtol = atol = 1e-11 per frame and 1e-11 relative on the sum, was set at P <= 12; the
    kernel's running prefix and the oracle's explicit pair sum differ in association over P^2 terms.  The float64 oracle
    against the 50-digit mpmath composition on these very inputs (test_oracle_many_sources.oracle_vs_mpmath, N = 49,
    logistic), largest relative error of a frame / relative error of the sum:
        P = 96:  3.96e-15 / 2.85e-16        P = 128:  4.72e-15 / 5.82e-17
    (P = 16 .. 33, all three nonlinearities, N = 1 .. 49: at most 1.7e-15 / 2.9e-16).  Both are far below 2.5e-12, a
    quarter of the bar (two float64 evaluations in different order may each be that far from the exact value, with a
    factor two of margin), so the 1e-11 bar stands at every P here; test_oracle_many_sources.py asserts that budget."""
    Fmu, Fvar, Y, ve, mom = _operator_case(P, N, nlin)
    assert P <= LANES or np.all(Fmu[:, LANES:P] != Fmu[:, :P - LANES])     # many_source_inputs asserts all four moments
    tag = "P %d nlin %d N %d" % (P, nlin, N)
    pf, s = _varexp(gp_handle, Fmu, Fvar, Y, P, nlin)
    _check_varexp(pf, s, ve, tag)
    if mom is None:
        assert P == LIK_MAX_P
        return
    got = _operator(gp_handle, Fmu, Fvar, Y, P, nlin, noise=NOISE)
    _check_against_ref(got, mom, P, tag)
    np.testing.assert_array_equal(got[4], pf)


def test_varexp_past_256_frame_blocks_with_a_single_frame_in_the_last(gp_handle):
    """N = 4113: 258 blocks of 16 frames, so finish_sum_kernel's `c += 256` loop makes a second trip, and the last block
    holds one frame"""
    P, N = 3, 4113
    Fmu, Fvar, Y, ve, _ = _operator_case(P, N, 0)
    pf, s = _varexp(gp_handle, Fmu, Fvar, Y, P, 0)
    _check_varexp(pf, s, ve, "P 3 N 4113")


# ---- 3, 4: the gradient pass and the sharded forms, through a model ----------------------------------------------------
def _problem(N, M, P, seed, **kw):
    """make_problem with an activation lengthscale of 2 ms: the 40 to 48 frames here span 3 ms, and the default of 1 s
    would leave cond(Kuu) of the activation GPs to the jitter (2e7; 5e2 with this one)"""
    from gpitch_amd.synth import make_problem
    p = make_problem(N, M, P, num_partials=2, seed=seed, **kw)
    for k in p["kern_act"]:
        k["lengthscales"] = 0.002
    return p


def _assert_block(got, ref, name):
    """a gradient block as test_gpu_pdgp.py::test_elbo_gradient_matches_autograd holds it: 2e-7 of the block's largest
    reference value, q_sqrt masked to its lower triangle"""
    if name.startswith("q_sqrt"):
        ref = np.tril(ref[:, :, 0])[:, :, None]
        assert np.all(np.triu(got[:, :, 0], 1) == 0), name
    scale = max(np.abs(ref).max(), 1e-12)
    np.testing.assert_allclose(got.reshape(ref.shape), ref, rtol=0, atol=2e-7 * scale, err_msg=name)


@pytest.mark.parametrize("P,nlin", [(17, 0), (33, 1)])
def test_gradient_pass_beyond_sixteen_sources_matches_autograd(gp_handle, P, nlin):
    """mpd_lik_kernel's gradient pass keeps the quadrature of a lane's first source and recomputes every later one
    (source l + 16, l + 32) with its derivatives: ELBO within 1e-9 and every gradient block within 2e-7 of autograd through
    the oracle; the noise gradient (it sums every source of every frame) and the q_mu blocks of sources 16 and above, where
    a quadrature taken from the wrong source lands first, are asserted by name"""
    import gpitch_amd
    prob = _problem(48, 6, P, seed=7)
    fn = [gpitch_amd.logistic_tf, gpitch_amd.softplus_tf, gpitch_amd.gaussfun_tf][nlin]
    model = pdgp_from_problem(prob, nlinfun=fn, handle=gp_handle)
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob, nlin_code=nlin)
    assert abs(f - ref_f) <= 1e-9 * abs(ref_f), (f, ref_f)
    got_g = model_grad_dict(model)
    assert set(ref_g) <= set(got_g) and all(v is not None for v in ref_g.values())
    for name in ["noise"] + ["q_mu_%s%d" % (g, i) for i in range(LANES, P) for g in ("act", "com")]:
        _assert_block(got_g[name], ref_g[name], name)
    for name, rg in ref_g.items():
        _assert_block(got_g[name], rg, name)


def _assert_shard_block(v, ref, what):
    """the bar of the two sharded tests of test_gpu_pdgp.py"""
    assert np.allclose(v, ref, rtol=1e-8, atol=1e-9 * max(1.0, np.abs(ref).max())), what


def test_pitch_sharded_with_more_than_sixteen_sources_per_rank(gp_handle):
    """P = 35 over two emulated ranks, 18 and 17 sources each: the psum pass (this rank's A, B, D) and the gsum pass
    (C = A^2 - D and the gradient) of mpd_lik_kernel both send lanes round again.  The assertions and bars of
    test_gpu_pdgp.py::test_pitch_sharded_two_stage_matches_unsharded."""
    P, world = 35, 2
    prob = _problem(48, 6, P, seed=11)
    full = pdgp_from_problem(prob, handle=gp_handle)
    full._pack()
    e_full = full._elbo(True)
    g_full = model_grad_dict(full)
    kl_full = float(full._elbo_dev[1].item())
    shards = [pdgp_from_problem(prob, handle=gp_handle, shard=(r, world)) for r in range(world)]
    assert sorted(len(s._local) for s in shards) == [17, 18]
    for s in shards:
        s._pack()
    total = sum(s._elbo_begin(True).clone() for s in shards)
    seen = set()
    for s in shards:
        s._xchg[:total.numel()].copy_(total)
        e = s._elbo_end(True)
        assert abs(e - e_full) <= 1e-10 * abs(e_full), (e, e_full)
        assert abs(float(s._elbo_dev[1].item()) - kl_full) <= 1e-10 * max(1.0, abs(kl_full))
        for k, v in model_grad_dict(s).items():
            _assert_shard_block(v, g_full[k], k)
            seen.add(k)
    assert seen == set(g_full.keys())


def test_gp_sharded_rank_with_more_than_64_latent_gps(gp_handle):
    """One rank holding 66 latent GPs (P = 33, a world of one): the gradient rows of the whole model reach the plan through
    RowGather launches of 64 rows, so rows 64 and 65 (the component GPs of sources 31 and 32) come from the second
    launch.  The assertions and bars of test_gpu_pdgp.py::test_gp_sharded_two_stage_matches_unsharded; the blocks of
    rows 64 and above are asserted by name."""
    P = 33
    prob = _problem(40, 4, P, seed=13)
    full = pdgp_from_problem(prob, handle=gp_handle)
    full._pack()
    e_full = full._elbo(True)
    g_full = model_grad_dict(full)
    kl_full = float(full._elbo_dev[1].item())
    s = pdgp_from_problem(prob, handle=gp_handle, shard=("gp", 0, 1))
    s._pack()
    assert list(s._gp_shard) == list(range(2 * P)) and len(s._gp_shard) > 64
    gathered = s._gp_begin(True).clone()
    e = s._gp_end(True, gathered)
    assert abs(e - e_full) <= 1e-10 * abs(e_full), (e, e_full)
    assert abs(float(s._elbo_dev[1].item()) - kl_full) <= 1e-10 * max(1.0, abs(kl_full))
    g = s._grad.cpu().numpy()
    _assert_shard_block(g[0:1], g_full["noise"], "noise")
    rows, seen = {}, {"noise"}
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
        rows[l] = got
        for k, v in got.items():
            _assert_shard_block(v, g_full[k], (k, gi))
            seen.add(k)
    assert seen == set(g_full.keys())
    for l in range(64, 2 * P):
        i = l - P
        for k in ("q_mu_com%d" % i, "q_sqrt_com%d" % i, "zc%d" % i, "com%d.lengthscales" % i, "com%d.energy1" % i):
            assert np.abs(g_full[k]).max() > 0
            _assert_shard_block(rows[l][k], g_full[k], (k, l))


# ---- 5: batched models -----------------------------------------------------------------------------------------------
def _batch_problems():
    """P = 17, 1, 33, the narrow model between the two wide ones; 48, 24 and 40 frames (full batch, so three minibatch
    sizes), 6, 4 and 8 inducing points; a nonlinearity each; z trained"""
    return [(_problem(48, 6, 17, seed=21), 0), (_problem(24, 4, 1, seed=22), 1), (_problem(40, 8, 33, seed=23), 2)]


def test_batch_objective_with_wide_and_narrow_models(gp_handle):
    """pdgpb_lik_kernel's loops over P at P = 17, 1 and 33 in one launch: objective_many against autograd through the
    oracle, ELBO within 1e-9 and every gradient block within 2e-7 (test_objective_matches_autograd_through_the_oracle), and
    against each model's own objective (mpd_lik_kernel) at the bars of
    test_objective_many_matches_each_models_own_objective"""
    from gpitch_amd.pdgp_batch import PdgpBatch
    probs = _batch_problems()
    models = [_build(p, nl, False) for p, nl in probs]
    twins = copy.deepcopy(models)
    assert len(set(m.minibatch_size for m in models)) == 3
    batch = PdgpBatch(models)
    res = batch.objective_many()
    for k, (p, nl) in enumerate(probs):
        e_ref, g_ref = oracle_elbo_and_grads(p, nlin_code=nl)
        assert abs(-res[k][0] - e_ref) <= 1e-9 * abs(e_ref), (k, -res[k][0], e_ref)
        got = _batch_grad_dict(batch, k)
        assert set(g_ref) <= set(got) and all(v is not None for v in g_ref.values())
        for name, gr in g_ref.items():
            assert _block_err(got[name], gr) <= 2e-7, (k, name, _block_err(got[name], gr))
        _assert_same_objective(models[k], res[k], twins[k])


def test_batch_moments_with_wide_and_narrow_models(gp_handle):
    """one predict_sources_many call over the P = 17, 1 and 33 models at 65, 1 and 64 frames off the training grid (the LDS
    stride of pdgpb_pred_moments_kernel is the widest model's 4 x 33): against the oracle composition and each model's own
    methods at the bars of test_batch_matches_each_models_own_methods_and_the_oracle; the P = 1 model's single frame does
    not change, bit for bit, when it is predicted alone"""
    import gpitch_amd
    probs = _batch_problems()
    models = [_build(p, nl, False) for p, nl in probs]
    twins = copy.deepcopy(models)
    xs = []
    for (p, _), n in zip(probs, (65, 1, 64)):
        x = p["x"].reshape(-1)
        xs.append(np.linspace(x[0] + 0.37 * (x[1] - x[0]), x[-1] - 0.21 * (x[1] - x[0]), n).reshape(-1, 1))
        assert not np.intersect1d(xs[-1], x).size
    ys = _targets(xs, seed=13)
    res = gpitch_amd.predict_sources_many(models, xs, ys)
    for k, ((p, nl), t, xt, yt, r) in enumerate(zip(probs, twins, xs, ys, res)):
        P, n = p["P"], xt.shape[0]
        assert sorted(r) == ["logp", "mean_s", "mean_y", "var_s", "var_y"]
        assert len(r["mean_s"]) == len(r["var_s"]) == P
        assert all(v.shape == (n, 1) for v in r["mean_s"] + r["var_s"] + [r["mean_y"], r["var_y"], r["logp"]])
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
    alone = gpitch_amd.predict_sources_many([models[1]], [xs[1]], [ys[1]])
    _same_bits([res[1]], alone)


# ---- 6: one source above the limits ----------------------------------------------------------------------------------
def _refused(h, st, message):
    from gpitch_amd import _lib
    assert st == _lib.GP_ERR_UNSUPPORTED, st
    assert message in h.lib.gp_last_error(h.h).decode()


def test_operators_refuse_one_source_above_their_limits(gp_handle):
    """gp_mpd_varexp at P = 129 and gp_mpd_predict_moments at P = 97 return GP_ERR_UNSUPPORTED with their message (an error
    return before any launch); MpdLik raises the library's exception with it"""
    import gpitch_amd
    from gpitch_amd import _lib
    h = gp_handle
    N = 4
    nv = h.to_device(np.array([NOISE]))
    for P, moments, message in ((LIK_MAX_P + 1, False, LIK_REFUSAL), (MOM_MAX_P + 1, True, MOM_REFUSAL)):
        Fmu, Fvar, Y = many_source_inputs(P, N, 0)
        dmu, dvar, dy = h.to_device(Fmu), h.to_device(Fvar), h.to_device(Y.reshape(-1))
        lik = gpitch_amd.likelihoods.MpdLik(gpitch_amd.logistic_tf, P)
        lik.variance = NOISE
        if moments:
            sm, sv, ym, yv, lp = h.empty(P, N), h.empty(P, N), h.empty(N), h.empty(N), h.empty(N)
            st = h.lib.gp_mpd_predict_moments(h.h, dmu.data_ptr(), dvar.data_ptr(), dy.data_ptr(), N, P, 0, nv.data_ptr(),
                                              sm.data_ptr(), sv.data_ptr(), ym.data_ptr(), yv.data_ptr(), lp.data_ptr())
            _refused(h, st, message)
            with pytest.raises(_lib.GpitchError, match=message) as e:
                lik.predict_mean_and_var(Fmu, Fvar)
        else:
            pf = h.empty(N)
            s = C.c_double()
            st = h.lib.gp_mpd_varexp(h.h, dmu.data_ptr(), dvar.data_ptr(), dy.data_ptr(), N, P, 0, nv.data_ptr(),
                                     pf.data_ptr(), C.byref(s))
            _refused(h, st, message)
            with pytest.raises(_lib.GpitchError, match=message) as e:
                lik.variational_expectations(Fmu, Fvar, Y)
        assert e.value.status == _lib.GP_ERR_UNSUPPORTED
        h.sync()


def test_batched_moments_refuse_97_sources_and_the_plain_prediction_goes_on(gp_handle):
    """a prediction-only batch plan with a P = 97 model: gp_pdgpb_predict_moments returns GP_ERR_UNSUPPORTED (its LDS
    staging is 4 P wide); gp_pdgpb_predict, which stages nothing per source, matches the model's own prediction at the
    bars of test_gpu_pdgp_predict.py (5e-11 of the largest value for means and variances, 5e-10 for the source means)"""
    import gpitch_amd
    from gpitch_amd import _lib
    P = MOM_MAX_P + 1
    prob = _problem(16, 4, P, seed=31, base_midi=21)
    m = _build(prob, 0, True)
    twin = copy.deepcopy(m)
    x = prob["x"].reshape(-1)
    xt = np.linspace(x[0] + 0.37 * (x[1] - x[0]), x[-1], 16).reshape(-1, 1)
    with pytest.raises(_lib.GpitchError, match="gp_pdgpb_predict_moments: " + MOM_REFUSAL) as e:
        gpitch_amd.predict_sources_many([m], [xt])
    assert e.value.status == _lib.GP_ERR_UNSUPPORTED
    got = gpitch_amd.predict_many([m], [xt])[0]
    ref = twin.predict_act_n_com(xt)
    for name, ga, r in zip(("mean_a", "var_a", "mean_c", "var_c", "mean_src"), got, ref):
        assert len(ga) == len(r) == P
        for i in range(P):
            err = float(np.max(np.abs(ga[i] - r[i])) / max(np.max(np.abs(r[i])), 1e-300))
            assert err <= (5e-10 if name == "mean_src" else 5e-11), (name, i, err)
