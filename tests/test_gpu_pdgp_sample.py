"""Joint posterior draws of every Pdgp source on the GPU (Pdgp.sample_sources, csrc/sample.hip through gp_pdgp_sample)
against the numpy restatement on the same eps (tests/pdgp_sample_ref.py), the oracle's full-covariance conditionals, the
model's own predictions, and itself.  Tolerance against the restatement: the project's rule, absolute 1e-8 max(|ref|, 1e-3);
the inputs are conditioned for it (test_pdgp_sample_cpu.py::test_gpu_shapes_are_well_conditioned)."""
import ctypes as C

import numpy as np
import pytest

import pdgp_sample_ref as ref
from oracle import gpflow05 as orc

pytestmark = pytest.mark.gpu


def _model(prob, handle, nlin=0, whiten=True, float_type=None):
    import gpitch_amd
    from gpitch_amd.synth import pdgp_from_problem
    fn = [gpitch_amd.logistic_tf, gpitch_amd.softplus_tf, gpitch_amd.gaussfun_tf][nlin]
    return pdgp_from_problem(prob, whiten=whiten, nlinfun=fn, handle=handle, float_type=float_type)


def _close(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = np.abs(got - want).max()
    bar = 1e-8 * max(np.abs(want).max(), 1e-3)
    print("%s: max|diff| %.3e, bar %.3e" % (what, err, bar))
    assert err <= bar, (what, err, bar)


def _against_restatement(m, prob, xs, eps, whiten=True, nlin=0, tag=""):
    S = eps[0][0].shape[0]
    got = m.sample_sources(xs, num_samples=S, eps=eps, return_latents=True)
    want = ref.sample_sources(prob, xs, eps, whiten, nlin)
    for name, a, b in zip(("src", "g", "f"), got, want):
        _close(a, b, "%s %s" % (tag, name))
    return got


def test_identity_eps_at_the_smallest_shape(gp_handle):
    """P = 1, Matern32 activation (M = 12), MercerMatern12sm component of 2 partials (M = 10), 40 shuffled frames, three of
    them on inducing inputs; one draw per eps coordinate (128 + 220) plus one eps = 0 draw"""
    prob = ref.problem(12, 10, 1, 2, 204, seed=1)
    xs = ref.frames(prob, 40, 2)
    co = ref.coordinates(prob, 40)
    assert co == [128, 220]
    eps = ref.identity_eps(prob, 40)
    m = _model(prob, gp_handle)
    src, g, f = m.sample_sources(xs, num_samples=349, eps=eps, return_latents=True)
    lat = np.concatenate([g, f])
    T, mean = ref.linear_parts(lat, co)
    Tref, _ = ref.linear_parts(ref.sample_latents(prob, xs, eps), co)
    at = 0
    for r, ((cov, kd), (kern, _, _, _)) in enumerate(zip(ref.full_covs(prob, xs), ref.latent_gps(prob))):
        _close(T[r], Tref[r], "T of latent GP %d" % r)
        own = T[r][:, at:at + co[r]]
        other = np.delete(T[r], np.s_[at:at + co[r]], axis=1)
        assert np.abs(other).max() == 0.0                             # the other GP's eps: exactly nothing
        err = np.abs(own.dot(own.T) - cov).max() / kd
        print("latent GP %d (%s): T T^T against conditional(full_cov=True) %.3e Kdiag, bar %.0e" %
              (r, kern["type"], err, ref.cov_bar(kern)))
        assert err <= ref.cov_bar(kern)
        at += co[r]
    ma, _ = m.predict_act(xs)
    mc, _ = m.predict_com(xs)
    ms = m.predict_act_n_com(xs)[4]
    _close(mean[0], ma[0].ravel(), "eps = 0 against predict_act")
    _close(mean[1], mc[0].ravel(), "eps = 0 against predict_com")
    _close(src[0, -1], ms[0].ravel(), "eps = 0 against mean_source")


@pytest.mark.parametrize("k", range(len(ref.SHAPES)))
def test_seeded_eps_against_the_restatement_at_every_tile_shape(gp_handle, k):
    """(M_a, M_c, P, n, S, m, nlin): unequal M inside a model, M not a multiple of 16, every tile width of the sparse
    predictor (M <= 256, <= 512, beyond), n below and above one tile, S below and above 16, every partial padding"""
    prob, xs, S, nlin = ref.shape_problem(k)
    m = _model(prob, gp_handle, nlin)
    eps = ref.random_eps(prob, xs.shape[0], S, 50 + k)
    src, g, f = _against_restatement(m, prob, xs, eps, True, nlin, "shape %d" % k)
    assert np.abs(src - orc.nlinfun(nlin)(g) * f).max() <= 1e-12 * np.abs(src).max()


def test_every_supported_kernel_in_both_roles(gp_handle):
    for k, com in enumerate(("matern12sm", "mercer_matern12sm", "matern12", "matern32")):
        prob = ref.problem(14, 9, 2, 3, 300, seed=30 + k, com=com, act_ls=0.05, com_ls=0.02)
        prob["kern_act"][1] = ref._plain("matern12", 2.0, 0.05)
        xs = ref.frames(prob, 23, 40 + k)
        _against_restatement(_model(prob, gp_handle), prob, xs, ref.random_eps(prob, 23, 4, 60 + k), tag=com)


def test_unsupported_kernels_raise_before_device_work(gp_handle):
    bad = [ref._plain("matern52", 1.0, 0.01), ref._plain("rbf", 1.0, 0.01),
           {"type": "matern32sm", "variance": 1.0, "lengthscales": 0.01, "energy": [0.1, 0.1], "frequency": [100., 200.]},
           {"type": "mercer_matern52sm", "variance": 0.5, "lengthscales": 0.01, "energy": [1.], "frequency": [100.]}]
    for kern in bad:
        for role in ("kern_act", "kern_com"):
            prob = ref.problem(8, 8, 1, 2, 128, seed=3)
            prob[role][0] = kern
            m = _model(prob, gp_handle)
            with pytest.raises(NotImplementedError) as ei:
                m.sample_sources(ref.frames(prob, 5, 4))
            assert ("activation GP 0" if role == "kern_act" else "component GP 0") in str(ei.value)
            assert m._plan is None


def test_bit_for_bit(gp_handle):
    prob, xs, _, nlin = ref.shape_problem(1)
    m = _model(prob, gp_handle, nlin)
    n = xs.shape[0]
    e21 = ref.random_eps(prob, n, 21, 70)
    e5 = tuple([a[:5].copy() for a in e] for e in e21)
    a = m.sample_sources(xs, num_samples=21, eps=e21, return_latents=True)
    b = m.sample_sources(xs, num_samples=21, eps=e21, return_latents=True)
    c = m.sample_sources(xs, num_samples=5, eps=e5, return_latents=True)
    for u, v, w in zip(a, b, c):
        np.testing.assert_array_equal(u, v)
        np.testing.assert_array_equal(u[:, :5], w)
    np.testing.assert_array_equal(m.sample_sources(xs, num_samples=21, eps=e21), a[0])


def test_an_unwhitened_model(gp_handle):
    """the well-conditioned shape (cond(Kuu) <= 2e4) against the restatement, and against the whitened model that holds the
    same q(u): q_mu' = L^-1 q_mu, q_sqrt' = L^-1 tril(q_sqrt)"""
    from scipy.linalg import solve_triangular
    prob, xs, S, nlin = ref.unwhitened_problem()
    eps = ref.random_eps(prob, xs.shape[0], S, 80)
    got = _against_restatement(_model(prob, gp_handle, nlin, whiten=False), prob, xs, eps, False, nlin, "unwhitened")
    wp = dict(prob)
    for role, zname in (("act", "za"), ("com", "zc")):
        wp["q_mu_" + role], wp["q_sqrt_" + role] = [], []
        for i in range(prob["P"]):
            Z = prob[zname][i]
            L = np.linalg.cholesky(orc.K(prob["kern_" + role][i], Z) + ref.JITTER * np.eye(Z.shape[0]))
            wp["q_mu_" + role].append(solve_triangular(L, prob["q_mu_" + role][i], lower=True))
            wp["q_sqrt_" + role].append(solve_triangular(L, np.tril(prob["q_sqrt_" + role][i][:, :, 0]), lower=True)[:, :, None])
    white = _model(wp, gp_handle, nlin).sample_sources(xs, num_samples=S, eps=eps, return_latents=True)
    for name, a, b in zip(("src", "g", "f"), got, white):
        _close(a, b, "unwhitened against its whitened equivalent, %s" % name)


def test_state_follows_the_parameters(gp_handle):
    """after two Adam steps (every Param moved, Z included) and after assigning a Param the draws match the restatement at
    the new values: the factorisation is not reused across a change"""
    import gpitch_amd
    prob = ref.problem(12, 10, 1, 2, 204, seed=90)
    xs = ref.frames(prob, 37, 91)
    eps = ref.random_eps(prob, 37, 5, 92)
    m = _model(prob, gp_handle)
    _against_restatement(m, prob, xs, eps, tag="before")
    m.optimize(method=gpitch_amd.train.AdamOptimizer(0.01), maxiter=2)
    now = ref.model_problem(m)
    assert np.abs(now["q_mu_act"][0] - prob["q_mu_act"][0]).max() > 0
    _against_restatement(m, now, xs, eps, tag="after optimize")
    _against_restatement(m, now, xs, eps, tag="again (factorisation reused)")
    m.q_mu_com[0].value = m.q_mu_com[0].value + 0.25
    m.kern_act[0].lengthscales = 0.7
    _against_restatement(m, ref.model_problem(m), xs, eps, tag="after assigning Params")


def test_float32_model_matches_its_float64_twin(gp_handle):
    prob, xs, S, nlin = ref.shape_problem(1)
    eps = ref.random_eps(prob, xs.shape[0], S, 95)
    a = _model(prob, gp_handle, nlin).sample_sources(xs, num_samples=S, eps=eps, return_latents=True)
    b = _model(prob, gp_handle, nlin, float_type=np.float32).sample_sources(xs, num_samples=S, eps=eps, return_latents=True)
    for name, u, v in zip(("src", "g", "f"), a, b):
        _close(v, u, "float32 model against float64, %s" % name)


def test_seeded_draws(gp_handle, monkeypatch):
    """same seed: identical; another seed: different; chunked generation: the first chunk is the unchunked call of that many
    draws.  S = 2048, n = 64: the per-frame sample mean of every source within 6 sqrt(svar / S) of predict_sources' mean at
    every frame (the bound holds for the restatement alone: test_pdgp_sample_cpu.py)"""
    from gpitch_amd import sgpr_ss
    prob, xs, S = ref.mean_bound_problem()
    m = _model(prob, gp_handle)
    a = m.sample_sources(xs, num_samples=S, seed=3)
    b = m.sample_sources(xs, num_samples=S, seed=3)
    c = m.sample_sources(xs, num_samples=S, seed=4)
    np.testing.assert_array_equal(a, b)
    assert a.shape == (2, S, 64) and np.all(np.isfinite(a)) and np.abs(a - c).max() > 1e-3
    mean, var = m.predict_sources(xs)
    for i in range(2):
        dev = np.abs(a[i].mean(axis=0) - mean[i].ravel()) / np.sqrt(var[i].ravel() / S)
        print("source %d: largest deviation of the sample mean %.2f standard errors" % (i, dev.max()))
        assert np.all(dev <= 6.0)
    per_draw = sum(c_ * (64 + M) + 2 * M for c_, M in zip(m._sample_components(), (12, 12, 10, 10)))
    monkeypatch.setattr(sgpr_ss, "SAMPLE_EPS_BYTES", 8 * per_draw * 7)
    d = m.sample_sources(xs, num_samples=20, seed=3)                  # chunks of 7, 7 and 6 draws
    np.testing.assert_array_equal(d[:, :7], m.sample_sources(xs, num_samples=7, seed=3))
    assert np.all(np.isfinite(d)) and np.abs(d[:, 7:14] - d[:, :7]).max() > 1e-3


def test_arguments(gp_handle):
    from gpitch_amd import _lib
    prob = ref.problem(12, 10, 1, 2, 204, seed=1)
    xs = ref.frames(prob, 9, 2)
    m = _model(prob, gp_handle)
    eps = ref.random_eps(prob, 9, 3, 1)
    with pytest.raises(ValueError):
        m.sample_sources(np.zeros((9, 2)))
    with pytest.raises(ValueError):
        m.sample_sources(xs, num_samples=0)
    with pytest.raises(ValueError):
        m.sample_sources(xs, num_samples=2, eps=eps)                  # eps of 3 draws
    bad = tuple([a.copy() for a in e] for e in eps)
    bad[1][1] = bad[1][1][:, :, :9]
    with pytest.raises(ValueError):
        m.sample_sources(xs, num_samples=3, eps=bad)
    out = m.sample_sources(np.zeros(0), num_samples=3, return_latents=True)
    assert all(a.shape == (1, 3, 0) for a in out)
    assert m.sample_eps_shapes(9, 3) == ref.eps_shapes(prob, 9, 3)
    good = m.sample_sources(xs, num_samples=3, eps=eps)               # compiles and packs the plan
    # direct ABI calls: nothing is enqueued for a null pointer, a bad order, a short workspace
    h, lib = m._handle, m._handle.lib
    order = np.ascontiguousarray(np.concatenate([_lib_order(xs, z) for z in (prob["za"][0], prob["zc"][0])]))
    flat = [h.to_device(np.concatenate([a.reshape(-1) for a in e])) for e in eps]
    xd = h.to_device(xs.ravel())
    lat, src = h.empty(2 * 3 * 9), h.empty(3 * 9)
    ws = h.workspace(lib.gp_pdgp_sample_workspace_bytes(2, 12, 6, 9, 3))

    def call(entry=lib.gp_pdgp_sample_reuse, order=order, ex=flat[0].data_ptr(), lat_ptr=lat.data_ptr(), nbytes=None, n=9, S=3):
        return entry(m._plan, m._params.data_ptr(), xd.data_ptr(), n, order.ctypes.data, S, ex, flat[1].data_ptr(),
                     flat[2].data_ptr(), lat_ptr, src.data_ptr(), ws.data_ptr(), ws.numel() if nbytes is None else nbytes)

    assert call() == _lib.GP_OK
    h.sync()
    np.testing.assert_array_equal(src.cpu().numpy().reshape(1, 3, 9), good)
    assert call(ex=None) == _lib.GP_ERR_BAD_ARG
    assert call(lat_ptr=None) == _lib.GP_ERR_BAD_ARG
    assert call(n=0) == _lib.GP_ERR_BAD_ARG and call(S=0) == _lib.GP_ERR_BAD_ARG
    assert call(nbytes=1024) == _lib.GP_ERR_BAD_ARG
    dup = order.copy()
    dup[3] = dup[4]
    assert call(order=dup) == _lib.GP_ERR_BAD_ARG
    far = order.copy()
    far[-1] = 9 + 10                                                  # one past the second GP's n + M points
    assert call(order=far) == _lib.GP_ERR_BAD_ARG
    assert b"permutation" in lib.gp_last_error(h.h)
    assert call(entry=lib.gp_pdgp_sample) == _lib.GP_OK
    h.sync()
    np.testing.assert_array_equal(src.cpu().numpy().reshape(1, 3, 9), good)


def _lib_order(xs, z):
    from gpitch_amd import merged_order
    return merged_order(xs, z)
