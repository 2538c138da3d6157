"""Joint posterior draws of many Pdgp models in one call (gpitch_amd.sample_sources_many, csrc/pdgp_batch.hip through
gp_pdgpb_sample over the state-space core of csrc/sample.hip) against the numpy restatement on the same eps
(tests/pdgp_sample_ref.py), the batch's own predictions, the oracle's full-covariance conditionals, and itself.  Tolerance
against the restatement: the project's rule, 1e-8 max(|ref|, 1e-3); the inputs are conditioned for it
(test_pdgp_sample_many_cpu.py::test_gpu_inputs_are_well_conditioned)."""
import ctypes as C

import numpy as np
import pytest

import pdgp_sample_many_cases as cs
import pdgp_sample_ref as ref
from oracle import gpflow05 as orc

pytestmark = pytest.mark.gpu


def _model(prob, nlin=0):
    import gpitch_amd
    from gpitch_amd.synth import pdgp_from_problem
    return pdgp_from_problem(prob, nlinfun=[gpitch_amd.logistic_tf, gpitch_amd.softplus_tf, gpitch_amd.gaussfun_tf][nlin])


def _close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, bar = cs.rule(got, want)
    print("%s: max|diff| %.3e, bar %.3e" % (what, err, bar))
    assert err <= bar, (what, err, bar)


@pytest.fixture(scope="module")
def zoo(gp_handle):
    """models A-F (pdgp_sample_many_cases) built once: name -> (model, prob, frames, nlin)"""
    out = {}
    for name in cs.NAMES:
        prob, xs, nlin, _ = cs.case(name)
        out[name] = (_model(prob, nlin), prob, xs, nlin)
    return out


def _lists(zoo, names):
    return [zoo[n][0] for n in names], [zoo[n][2] for n in names]


@pytest.mark.parametrize("S", [5, 33])
def test_against_the_restatement(zoo, S):
    """A-F in one call plus a seventh model without frames"""
    from gpitch_amd import sample_sources_many
    models, xs = _lists(zoo, cs.NAMES)
    pa = cs.case("A")[0]
    models, xs = models + [_model(pa)], xs + [np.zeros(0)]
    eps = [cs.eps(n, S) for n in cs.NAMES] + [ref.random_eps(pa, 0, S, 9)]
    got = sample_sources_many(models, xs, num_samples=S, eps=eps, return_latents=True)
    assert all(a.shape == (1, S, 0) for a in got[6])
    for name, (src, g, f) in zip(cs.NAMES, got):
        _, prob, x, nlin = zoo[name]
        want = ref.sample_sources(prob, x, cs.eps(name, S), True, nlin)
        for what, a, b in zip(("src", "g", "f"), (src, g, f), want):
            _close(a, b, "%s S = %d %s" % (name, S, what))
        assert np.abs(src - orc.nlinfun(nlin)(g) * f).max() <= 1e-12 * np.abs(src).max()
    only_src = sample_sources_many(models, xs, num_samples=S, eps=eps)
    for a, b in zip(only_src, got):
        np.testing.assert_array_equal(a, b[0])


def test_zero_eps_is_the_batch_prediction(zoo):
    from gpitch_amd import predict_many, sample_sources_many
    models, xs = _lists(zoo, cs.NAMES)
    eps = [ref.zero_eps(zoo[n][1], zoo[n][2].shape[0], 2) for n in cs.NAMES]
    got = sample_sources_many(models, xs, num_samples=2, eps=eps, return_latents=True)
    pred = predict_many(models, xs)
    for name, (src, g, f), (ma, _, mc, _, ms) in zip(cs.NAMES, got, pred):
        for i in range(src.shape[0]):
            for s in range(2):
                _close(g[i, s], ma[i].ravel(), "%s eps = 0 against fmean of g_%d" % (name, i))
                _close(f[i, s], mc[i].ravel(), "%s eps = 0 against fmean of f_%d" % (name, i))
                _close(src[i, s], ms[i].ravel(), "%s eps = 0 against mean_source %d" % (name, i))


def test_identity_eps_of_two_models(zoo):
    """one draw per eps coordinate of each model plus a zero draw; the shorter model's extra draws are zeros"""
    from gpitch_amd import sample_sources_many
    p0 = ref.problem(12, 10, 1, 2, 204, seed=1)
    x0 = ref.frames(p0, 40, 2)
    _, p1, x1, _ = zoo["E"]
    probs, xs = [p0, p1], [x0, x1]
    ident = [ref.identity_eps(p, x.shape[0]) for p, x in zip(probs, xs)]
    own = [e[0][0].shape[0] for e in ident]
    S = max(own)
    assert own == [349, 263]
    eps = [tuple([np.concatenate([a, np.zeros((S - a.shape[0],) + a.shape[1:])]) for a in part] for part in e) for e in ident]
    got = sample_sources_many([_model(p0), zoo["E"][0]], xs, num_samples=S, eps=eps, return_latents=True)
    for k, (prob, x, (src, g, f)) in enumerate(zip(probs, xs, got)):
        co = ref.coordinates(prob, x.shape[0])
        lat = np.concatenate([g, f])
        if own[k] < S:                                                                # the padding draws are the zero draw
            assert np.abs(lat[:, own[k]:] - lat[:, own[k] - 1:own[k]]).max() == 0.0
        T, _ = ref.linear_parts(lat[:, :own[k]], co)
        at = 0
        for r, ((cov, kd), (kern, _, _, _)) in enumerate(zip(ref.full_covs(prob, x), ref.latent_gps(prob))):
            mine = T[r][:, at:at + co[r]]
            other = np.delete(T[r], np.s_[at:at + co[r]], axis=1)
            assert np.abs(other).max() == 0.0                                         # another GP's eps: exactly nothing
            err = np.abs(mine.dot(mine.T) - cov).max() / kd
            print("model %d latent GP %d (%s): T T^T against conditional(full_cov=True) %.3e Kdiag, bar %.0e"
                  % (k, r, kern["type"], err, ref.cov_bar(kern)))
            assert err <= ref.cov_bar(kern)
            at += co[r]


def _equal(a, b):
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_bit_for_bit(zoo, monkeypatch):
    from gpitch_amd import pdgp_batch, sample_sources_many
    names = ["A", "B", "C"]
    models, xs = _lists(zoo, names)
    e21 = [cs.eps(n, 21) for n in names]
    e5 = [tuple([a[:5].copy() for a in part] for part in e) for e in e21]
    a = sample_sources_many(models, xs, num_samples=21, eps=e21, return_latents=True)
    b = sample_sources_many(models, xs, num_samples=21, eps=e21, return_latents=True)
    c = sample_sources_many(models, xs, num_samples=5, eps=e5, return_latents=True)
    for k in range(3):
        _equal(a[k], b[k])
        _equal([u[:, :5] for u in a[k]], c[k])
    alone = sample_sources_many(models[1:2], xs[1:2], num_samples=21, eps=e21[1:2], return_latents=True)
    swapped = sample_sources_many([models[2], models[1]], [xs[2], xs[1]], num_samples=21, eps=[e21[2], e21[1]], return_latents=True)
    _equal(a[1], alone[0])
    _equal(a[1], swapped[1])
    _equal(a[2], swapped[0])
    # a budget of 1.12 MB: [A, B] share a group in chunks of 16 draws, C goes alone in chunks of 16
    e33 = [cs.eps(n, 33) for n in names]
    whole = sample_sources_many(models, xs, num_samples=33, eps=e33, return_latents=True)
    seeded = sample_sources_many(models, xs, num_samples=33, seed=[7, 8, 9], return_latents=True)
    per_draw = pdgp_batch.sample_bytes_per_draw(models, [x.reshape(-1) for x in xs])     # what the call itself weighs
    assert per_draw == [3528, 60456, 132080]
    monkeypatch.setattr(pdgp_batch, "MAX_SAMPLE_BYTES", 16 * 70000)
    split = pdgp_batch.sample_split(per_draw, [2 * m.num_sources for m in models], 33, pdgp_batch.MAX_SAMPLE_BYTES)
    assert [(k0, k1, len(ch)) for k0, k1, ch in split] == [(0, 2, 3), (2, 3, 3)]
    groups, run_group = [], pdgp_batch._sample_group

    def counted(h, ms, gx, first, chunks, *rest):
        groups.append((first, len(ms), [sc for _, sc in chunks]))
        return run_group(h, ms, gx, first, chunks, *rest)

    monkeypatch.setattr(pdgp_batch, "_sample_group", counted)
    cut = sample_sources_many(models, xs, num_samples=33, eps=e33, return_latents=True)
    cut_seeded = sample_sources_many(models, xs, num_samples=33, seed=[7, 8, 9], return_latents=True)
    assert groups == [(0, 2, [16, 16, 1]), (2, 1, [16, 16, 1])] * 2                       # both calls really were split
    for k in range(3):
        _equal(whole[k], cut[k])
        _equal(seeded[k], cut_seeded[k])


def test_seeds(zoo):
    from gpitch_amd import sample_sources_many
    models, xs = _lists(zoo, ["A", "E", "B"])
    a = sample_sources_many(models, xs, num_samples=20, seed=5)
    b = sample_sources_many(models, xs, num_samples=20, seed=5)
    c = sample_sources_many(models, xs, num_samples=20, seed=[5, 6, 7])
    d = sample_sources_many(models, xs, num_samples=20, seed=11)
    for k in range(3):
        np.testing.assert_array_equal(a[k], b[k])
        np.testing.assert_array_equal(a[k], c[k])                     # an int s stands for [s + k]
        assert np.all(np.isfinite(a[k])) and np.abs(a[k] - d[k]).max() > 1e-3
        one = sample_sources_many(models[k:k + 1], xs[k:k + 1], num_samples=20, seed=5 + k)
        np.testing.assert_array_equal(a[k], one[0])                   # model k alone with its seed: its slice of the list call
    assert np.abs(a[0][:, 16:] - a[0][:, :4]).max() > 1e-3            # the second block of draws is not the first again


def test_seeded_sample_means_stay_within_six_standard_errors():
    from gpitch_amd import predict_sources_many, sample_sources_many
    prob, xs, S = ref.mean_bound_problem()
    models = [_model(prob), _model(prob)]
    got = sample_sources_many(models, xs, num_samples=S, seed=[3, 4])
    mom = predict_sources_many(models, xs)
    assert np.abs(got[0] - got[1]).max() > 1e-3
    for k in range(2):
        assert got[k].shape == (2, S, 64) and np.all(np.isfinite(got[k]))
        for i in range(2):
            dev = np.abs(got[k][i].mean(axis=0) - mom[k]["mean_s"][i].ravel()) / np.sqrt(mom[k]["var_s"][i].ravel() / S)
            print("model %d source %d: largest deviation of the sample mean %.2f standard errors" % (k, i, dev.max()))
            assert np.all(dev <= 6.0)


def test_state_follows_the_parameters():
    from gpitch_amd import optimize_many, sample_sources_many
    from gpitch_amd.train import AdamOptimizer
    probs = [ref.problem(12, 10, 1, 2, 204, seed=1), ref.problem(14, 9, 2, 3, 300, seed=31, act_ls=0.05, com_ls=0.02)]
    models = [_model(p) for p in probs]
    xs = [ref.frames(probs[0], 40, 2), ref.frames(probs[1], 23, 41)]
    before = sample_sources_many(models, xs, num_samples=3, seed=1)
    res = optimize_many(models, AdamOptimizer(0.01), maxiter=2)
    assert all(r.success for r in res)
    now = [ref.model_problem(m) for m in models]
    eps = [ref.random_eps(p, x.shape[0], 4, 90 + k) for k, (p, x) in enumerate(zip(now, xs))]
    got = sample_sources_many(models, xs, num_samples=4, eps=eps, return_latents=True)
    for k in range(2):
        want = ref.sample_sources(now[k], xs[k], eps[k])
        for what, a, b in zip(("src", "g", "f"), got[k], want):
            _close(a, b, "model %d after two Adam steps, %s" % (k, what))
    after = sample_sources_many(models, xs, num_samples=3, seed=1)
    assert all(np.abs(a - b).max() > 0.0 for a, b in zip(before, after))


def test_abi(zoo):
    from gpitch_amd import _lib, flatvec, pdgp_batch, sample_sources_many
    from gpitch_amd.sgpr_ss import merged_order
    h = _lib.default_handle()
    lib, t = h.lib, h.torch
    names = ["A", "E"]
    models, xs = _lists(zoo, names)
    models, xs = models + [_model(cs.case("A")[0])], xs + [np.zeros(0)]      # and a model without frames
    S = 3
    eps = [cs.eps(n, S) for n in names] + [ref.random_eps(cs.case("A")[0], 0, S, 9)]
    want = sample_sources_many(models, xs, num_samples=S, eps=eps, return_latents=True)
    P = [m.num_sources for m in models]
    gps = [g for m in models for g in flatvec.latent_gps(m)]
    comps = [c for k, m in enumerate(models) for c in pdgp_batch._sample_comps(m, k)]
    lay = pdgp_batch.sample_layout(P, [x.size for x in xs], [g[1].size for g in gps], comps)
    order = np.ascontiguousarray(np.concatenate([merged_order(xs[k], z.value.reshape(-1))
                                                 for k, m in enumerate(models) for _, z, _, _ in flatvec.latent_gps(m)]))
    flat = [h.to_device(np.concatenate([a.reshape(-1) for e in eps for a in e[j]])) for j in range(3)]
    segs, _, base = pdgp_batch._segments(models)
    params = h.to_device(flatvec.pack([sp for sm in segs for sp in sm], base)[0])
    xd = h.to_device(np.concatenate([x.reshape(-1) for x in xs]))
    off = (C.c_int64 * 4)(*[int(v) for v in lay["x_off"]])
    nlat, nsrc = S * int(lay["latents"][-1]), S * int(lay["sources"][-1])
    lat, src = h.empty(nlat), h.empty(nsrc)

    def call(plan, ws, nbytes, order=order, ex=flat[0].data_ptr(), lat_ptr=lat.data_ptr(), src_ptr=src.data_ptr(), S=S):
        return lib.gp_pdgpb_sample(plan, params.data_ptr(), xd.data_ptr(), off, order.ctypes.data, S, ex, flat[1].data_ptr(),
                                   flat[2].data_ptr(), lat_ptr, src_ptr, ws.data_ptr(), nbytes)

    with pdgp_batch._predict_plan(h, models) as plan:
        nbytes = lib.gp_pdgpb_sample_workspace_bytes(plan, off, S)
        assert nbytes > lib.gp_pdgpb_predict_workspace_bytes(plan) and lib.gp_pdgpb_sample_workspace_bytes(plan, off, 0) == 0
        ws = h.workspace(nbytes)
        assert call(plan, ws, nbytes) == _lib.GP_ERR_BAD_ARG                     # never prepared
        h.check(lib.gp_pdgpb_predict_prepare(plan, params.data_ptr(), ws.data_ptr(), nbytes))
        # refusals: nothing is enqueued by any of them
        assert call(plan, ws, nbytes - 256) == _lib.GP_ERR_WORKSPACE
        assert call(plan, ws, nbytes, ex=None) == _lib.GP_ERR_BAD_ARG
        assert call(plan, ws, nbytes, lat_ptr=None) == _lib.GP_ERR_BAD_ARG
        assert call(plan, ws, nbytes, S=0) == _lib.GP_ERR_BAD_ARG
        for bad_at, bad_value in ((3, order[4]), (int(lay["order"][2]) + 1, int(lay["order"][3] - lay["order"][2])), (0, -1)):
            bad = order.copy()
            bad[bad_at] = bad_value
            assert call(plan, ws, nbytes, order=bad) == _lib.GP_ERR_BAD_ARG
            assert "permutation" in lib.gp_last_error(h.h).decode()
        # a workspace of exactly the reported size
        assert call(plan, ws, nbytes) == _lib.GP_OK
        h.sync()
        got_lat, got_src = lat.cpu().numpy(), src.cpu().numpy()
        lat.zero_()
        assert call(plan, ws, nbytes, src_ptr=None) == _lib.GP_OK                # sources may be NULL
        h.sync()
        np.testing.assert_array_equal(lat.cpu().numpy(), got_lat)
        bad = (C.c_int32 * 3)()
        h.check(lib.gp_pdgpb_not_pd(plan, bad, 1))
        assert list(bad) == [0, 0, 0]
        train = pdgp_batch.PdgpBatch(models[:2])
        assert call(train._plan, ws, nbytes) == _lib.GP_ERR_BAD_ARG              # a training plan
    for k in range(3):
        n = xs[k].size
        l = got_lat[S * lay["latents"][k]:S * lay["latents"][k + 1]].reshape(2 * P[k], S, n)
        s = got_src[S * lay["sources"][k]:S * lay["sources"][k + 1]].reshape(P[k], S, n)
        np.testing.assert_array_equal(s, want[k][0])
        np.testing.assert_array_equal(l[:P[k]], want[k][1])
        np.testing.assert_array_equal(l[P[k]:], want[k][2])
