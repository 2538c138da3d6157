"""The exactness contract of gpitch_amd.checkpoint on the device: train, save, load, train ends bit-identical
to a twin that made the two optimize() calls back to back (contract 1), a loaded model predicts and samples what the live
model it was saved from does (contract 3), and SGPRSS.optimize resumes between calls (contract 4).  Every comparison is
np.array_equal: both paths run the same _pack() on the same float64 bits with the same moments, step count and index
stream, so a difference means that something is missing from the state."""
import copy
import gc
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_A, ITERS_A = 1024, 12


# ---- models -------------------------------------------------------------------------------------------------------------------
def _pdgp(handle, minibatch=64, whiten=True, float_type=None, com="mercer", N=N_A, Ma=16, Mc=24, seed=0, fix_zc=False):
    """P = 2: Matern32 activations on Ma inducing points, component kernels `com` on Mc; one lengthscale and za fixed"""
    from gpitch_amd.kernels import Matern32, Matern32sm, Matern52, MercerCosMix
    from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
    from gpitch_amd.pdgp import Pdgp
    from gpitch_amd.synth import make_problem, midi2freq, uniform_inducing
    prob = make_problem(N, 8, 2, num_partials=3, seed=seed)
    x, y = prob["x"], prob["y"]
    f0 = [midi2freq(60.), midi2freq(61.)]
    kact = [Matern32(1, variance=3.5, lengthscales=0.02) for _ in range(2)]
    freqs = [np.array([(k + 1) * f for k in range(3)]) for f in f0]
    if com == "mercer":
        kcom = [MercerMatern12sm(1, energy=np.ones(3) / 3., frequency=fr, variance=1.0, lengthscales=0.004) for fr in freqs]
    else:
        prod = Matern52(1, variance=1.0, lengthscales=0.01) * MercerCosMix(1, energy=np.ones(3) / 3., frequency=freqs[1],
                                                                           variance=0.2, features_as_params=True)
        prod.kern_list[0].variance.fixed = True
        prod.kern_list[1].variance.fixed = True
        kcom = [Matern32sm(1, 3, lengthscales=0.01, variances=0.1 * np.ones(3), frequencies=freqs[0]), prod]
    z = [[uniform_inducing(x, Ma) for _ in range(2)], [uniform_inducing(x, Mc) for _ in range(2)]]
    m = Pdgp(x, y, z, [kact, kcom], whiten=whiten, minibatch_size=minibatch, handle=handle, float_type=float_type)
    m.likelihood.variance = 0.1
    m.za.fixed = True
    m.kern_act[0].lengthscales.fixed = True
    if fix_zc:
        m.zc.fixed = True
    return m


def _draws(holder, n=5):
    h = copy.deepcopy(holder)
    return [h.next_indices() for _ in range(n)]


def _same(a, b, tag):
    """bit-identical, through lists, tuples and dicts"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), tag
        for k in a:
            _same(a[k], b[k], (tag, k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), tag
        for i, (p, q) in enumerate(zip(a, b)):
            _same(p, q, (tag, i))
    elif a is None:
        assert b is None, tag
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype, (tag, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (tag, float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()))


def _same_results(ra, rb, tag):
    assert ra.success and rb.success, (tag, ra.message, rb.message)
    assert ra.fun == rb.fun, (tag, ra.fun, rb.fun)
    _same(ra.jac, rb.jac, (tag, "jac"))
    _same(ra.x, rb.x, (tag, "x"))
    assert ra.get("natgrad") == rb.get("natgrad"), (tag, ra.get("natgrad"), rb.get("natgrad"))


def _same_model(A, B, tag):
    """contract 1 on the models: every Param, _adam_state(), _adam_t, the generators' states and next draws"""
    from gpitch_amd import param
    pa, pb = param.sorted_params(A), param.sorted_params(B)
    assert len(pa) == len(pb)
    for i, (p, q) in enumerate(zip(pa, pb)):
        assert p.fixed == q.fixed and type(p.transform) is type(q.transform), (tag, i)
        _same(p._array, q._array, (tag, "param", i))
    assert A._adam_t == B._adam_t, (tag, A._adam_t, B._adam_t)
    _same(A._adam_state(), B._adam_state(), (tag, "adam"))
    for name in ("x", "y"):
        sa, sb = getattr(A, name).rng.get_state(), getattr(B, name).rng.get_state()
        assert sa[0] == sb[0] and sa[2:] == sb[2:], (tag, name)
        _same(sa[1], sb[1], (tag, name, "key"))
        _same(_draws(getattr(A, name)), _draws(getattr(B, name)), (tag, name, "draws"))


def _two_calls(build, method, iters, path, handle):
    """twin A: optimize, optimize.  B: optimize, save, dropped, load, optimize.  Returns (A, B, results of A, results of B)."""
    import gpitch_amd
    A, B = build(), build()
    ra = [A.optimize(method=method(), maxiter=iters), A.optimize(method=method(), maxiter=iters)]
    rb = [B.optimize(method=method(), maxiter=iters)]
    gpitch_amd.save(path, B, data=True)
    del B
    gc.collect()
    B = gpitch_amd.load(path, handle=handle)
    assert B._plan is None
    rb.append(B.optimize(method=method(), maxiter=iters))
    return A, B, ra, rb


def _assert_contract_1(A, B, ra, rb, tag):
    _same_results(ra[0], rb[0], (tag, "first call"))       # (the same code on the same inputs: a difference here is the device's)
    _same_results(ra[1], rb[1], (tag, "second call"))
    _same_model(A, B, tag)
    assert np.all(np.isfinite(ra[1].x)) and not np.array_equal(ra[0].x, ra[1].x), tag      # (the second call trained)


def _adam():
    from gpitch_amd.train import AdamOptimizer
    return AdamOptimizer(0.01)


def _natgrad():
    from gpitch_amd.train import NatGradAdam
    return NatGradAdam(0.1, 0.01)


def _natgrad_adaptive():
    from gpitch_amd.train import NatGradAdam
    return NatGradAdam(0.2, 0.01, gamma_com=1.0, halvings=2)


# ---- (a) Pdgp + Adam, the three minibatch branches ---------------------------------------------------------------------------------
_case_a_memo = {}


def _case_a(handle, factory, minibatch):
    if minibatch not in _case_a_memo:
        path = str(factory.mktemp("ckpt_a") / ("pdgp_%d.npz" % minibatch))
        A, B, ra, rb = _two_calls(lambda: _pdgp(handle, minibatch), _adam, ITERS_A, path, handle)
        _case_a_memo[minibatch] = dict(A=A, B=B, ra=ra, rb=rb, path=path)
    return _case_a_memo[minibatch]


@pytest.mark.parametrize("minibatch", (64, 768, N_A))       # with replacement; permutation prefix; no draw
def test_pdgp_adam_resumes_bit_for_bit(gp_handle, tmp_path_factory, minibatch):
    c = _case_a(gp_handle, tmp_path_factory, minibatch)
    assert c["A"]._adam_t == 2 * ITERS_A
    _assert_contract_1(c["A"], c["B"], c["ra"], c["rb"], ("adam", minibatch))


# ---- (b) natural-gradient tokens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("token", ("natgrad", "adaptive"))
def test_pdgp_natgrad_resumes_bit_for_bit(gp_handle, tmp_path, token):
    method = _natgrad if token == "natgrad" else _natgrad_adaptive
    A, B, ra, rb = _two_calls(lambda: _pdgp(gp_handle, 64), method, ITERS_A, str(tmp_path / "m.npz"), gp_handle)
    _assert_contract_1(A, B, ra, rb, token)
    if token == "adaptive":
        assert "natgrad" in ra[1] and "natgrad" in rb[1]


# ---- (c) other kernels, precisions and routes ----------------------------------------------------------------------------------------
_CASES_C = {"unwhitened": dict(whiten=False), "float32": dict(float_type=np.float32),
            "float64-float32": dict(float_type=(np.float64, np.float32)), "logistic-and-product": dict(com="other"),
            "inducing-fixed": dict(fix_zc=True)}       # the last: the MercerMatern12sm Q route takes fixed inducing inputs


@pytest.mark.parametrize("case", sorted(_CASES_C))
def test_pdgp_other_kernels_and_precisions(gp_handle, tmp_path, case):
    A, B, ra, rb = _two_calls(lambda: _pdgp(gp_handle, 64, **_CASES_C[case]), _adam, 6, str(tmp_path / "m.npz"), gp_handle)
    _assert_contract_1(A, B, ra, rb, case)
    assert B._bits == A._bits and B.whiten == A.whiten


# ---- (d) optimize_many ----------------------------------------------------------------------------------------------------------------
_case_d_memo = {}


def _many(handle):
    return [_pdgp(handle, 32, N=512, Ma=M, Mc=M, seed=3 + k) for k, M in enumerate((8, 16, 24))]


def _case_d(handle, factory, token, tied):
    import gpitch_amd
    key = (token, tied)
    if key not in _case_d_memo:
        method = _adam if token == "adam" else _natgrad
        groups = (lambda ms: gpitch_amd.tie_groups(ms)) if tied else (lambda ms: None)
        path = str(factory.mktemp("ckpt_d") / "many.npz")
        A, B = _many(handle), _many(handle)
        ra = [gpitch_amd.optimize_many(A, method(), maxiter=10, tied=groups(A)) for _ in range(2)]
        rb = [gpitch_amd.optimize_many(B, method(), maxiter=10, tied=groups(B))]
        gpitch_amd.save(path, B)                      # one file holds the list
        del B
        gc.collect()
        B = gpitch_amd.load(path, handle=handle)
        rb.append(gpitch_amd.optimize_many(B, method(), maxiter=10, tied=groups(B)))     # ties rebuilt on the loaded models
        _case_d_memo[key] = dict(A=A, B=B, ra=ra, rb=rb)
    return _case_d_memo[key]


@pytest.mark.parametrize("tied", (False, True))
@pytest.mark.parametrize("token", ("adam", "natgrad"))
def test_optimize_many_resumes_bit_for_bit(gp_handle, tmp_path_factory, token, tied):
    c = _case_d(gp_handle, tmp_path_factory, token, tied)
    assert isinstance(c["B"], list) and len(c["B"]) == 3
    for k in range(3):
        _assert_contract_1(c["A"][k], c["B"][k], [r[k] for r in c["ra"]], [r[k] for r in c["rb"]], (token, tied, k))
    if tied:
        assert c["B"][0].likelihood.variance.value[0] == c["B"][2].likelihood.variance.value[0]


# ---- (e) predict and sample after load -------------------------------------------------------------------------------------------------
def _pdgp_outputs(m, xnew, ynew):
    return dict(act_n_com=m.predict_act_n_com(xnew), sources=m.predict_sources(xnew), y=m.predict_y(xnew),
                logp=m.expected_log_density(xnew, ynew), draws=m.sample_sources(xnew, 4, seed=3))


def test_pdgp_predicts_and_samples_after_load(gp_handle, tmp_path_factory, tmp_path):
    import gpitch_amd
    live = _case_a(gp_handle, tmp_path_factory, 64)["A"]
    path = str(tmp_path / "trained.npz")
    gpitch_amd.save(path, live)
    loaded = gpitch_amd.load(path, handle=gp_handle)
    assert loaded._plan is None
    xnew, ynew = live.x.value[::3], live.y.value[::3]
    _same(_pdgp_outputs(live, xnew, ynew), _pdgp_outputs(loaded, xnew, ynew), "pdgp outputs")


def test_many_predict_and_sample_after_load(gp_handle, tmp_path_factory, tmp_path):
    import gpitch_amd
    live = _case_d(gp_handle, tmp_path_factory, "adam", False)["A"]
    path = str(tmp_path / "trained.npz")
    gpitch_amd.save(path, live)
    loaded = gpitch_amd.load(path, handle=gp_handle)
    xnews = [m.x.value[::3] for m in live]
    ynews = [m.y.value[::3] for m in live]
    _same(gpitch_amd.predict_sources_many(live, xnews, ynews), gpitch_amd.predict_sources_many(loaded, xnews, ynews), "moments")
    _same(gpitch_amd.sample_sources_many(live, xnews, 4, seed=3), gpitch_amd.sample_sources_many(loaded, xnews, 4, seed=3), "draws")


# ---- (f) SGPRSS ---------------------------------------------------------------------------------------------------------------------
def _sgpr(handle, N=512, M=32):
    from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
    from gpitch_amd.sgpr_ss import SGPRSS
    from gpitch_amd.synth import midi2freq, per_fun, uniform_inducing
    rng = np.random.RandomState(4)
    X = np.linspace(0., (N - 1.) / 16000., N).reshape(-1, 1)
    f0 = [midi2freq(60. + 4 * p) for p in range(3)]
    Y = sum(per_fun(X, 2, f) for f in f0) / 3. + 0.05 * rng.randn(N, 1)
    ks = [MercerMatern12sm(1, energy=np.array([0.6, 0.4]), frequency=np.array([f, 2 * f]), variance=0.3, lengthscales=0.02)
          for f in f0]
    m = SGPRSS(X, Y, np.sum(ks), uniform_inducing(X, M), handle=handle)
    m.likelihood.variance = 0.05
    return m


def _sgpr_outputs(m, Xnew):
    return dict(bound=m.compute_log_likelihood(), f=m.predict_f(Xnew), s=m.predict_s(Xnew), sparse=m.predict_s_sparse(Xnew),
                draws=m.sample_s_sparse(Xnew, 4, seed=3))


def test_sgprss_after_load_and_between_two_optimize_calls(gp_handle, tmp_path):
    import gpitch_amd
    from gpitch_amd import param
    path = str(tmp_path / "s.npz")
    A, B = _sgpr(gp_handle), _sgpr(gp_handle)
    ra = [A.optimize(maxiter=5)]
    rb = [B.optimize(maxiter=5)]
    gpitch_amd.save(path, B)
    loaded = gpitch_amd.load(path, handle=gp_handle)
    assert loaded._plan is None
    Xnew = B.X.value[::3]
    _same(_sgpr_outputs(B, Xnew), _sgpr_outputs(loaded, Xnew), "sgprss outputs")         # contract 3: live against loaded
    del B
    ra.append(A.optimize(maxiter=5))                                                       # contract 4
    rb.append(loaded.optimize(maxiter=5))
    assert ra[0].nit >= 1 and np.isfinite(ra[1].fun)
    for k in range(2):
        assert ra[k].fun == rb[k].fun, (k, ra[k].fun, rb[k].fun)
        _same(ra[k].x, rb[k].x, ("x", k))
        _same(ra[k].jac, rb[k].jac, ("jac", k))
        assert ra[k].nit == rb[k].nit and ra[k].nfev == rb[k].nfev
    for i, (p, q) in enumerate(zip(param.sorted_params(A), param.sorted_params(loaded))):
        _same(p._array, q._array, ("param", i))
        assert p.fixed == q.fixed


# ---- (g) load_state_dict into a model built by hand ----------------------------------------------------------------------------------
def test_load_state_dict_into_a_float32_model(gp_handle, tmp_path_factory):
    from gpitch_amd import param
    src = _case_a(gp_handle, tmp_path_factory, N_A)["A"]          # minibatch = N: the ELBO draws nothing
    target = _pdgp(gp_handle, N_A, float_type=np.float32)
    target.load_state_dict(src.state_dict())
    by_hand = _pdgp(gp_handle, N_A, float_type=np.float32)
    for p, q in zip(param.sorted_params(src), param.sorted_params(by_hand)):
        q.value = p.value
        q.fixed = p.fixed
    assert target._bits == 32 and target._plan is None
    got, want = target.compute_log_likelihood(), by_hand.compute_log_likelihood()
    assert np.isfinite(want) and got == want, (got, want)
    assert want != src.compute_log_likelihood()                  # (float32 strips: not the float64 model's value)


# ---- (h) another process ----------------------------------------------------------------------------------------------------------------
def test_another_process_continues_the_file(gp_handle, tmp_path_factory, tmp_path):
    import gpitch_amd
    c = _case_a(gp_handle, tmp_path_factory, 64)
    out = str(tmp_path / "continued.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_checkpoint_child.py"), c["path"], out, str(ITERS_A)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    B = gpitch_amd.load(out, handle=gp_handle)
    _same_model(c["A"], B, "child")
    with np.load(out + ".result.npz", allow_pickle=False) as f:
        assert float(f["fun"]) == c["ra"][1].fun
        _same(f["jac"], c["ra"][1].jac, "child jac")
        _same(f["x"], c["ra"][1].x, "child x")
