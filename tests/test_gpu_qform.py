"""The Q route (a whitened MercerMatern12sm family with fixed inducing inputs forms G = Q Kuf, Q = W^T (Lq Lq^T - I) W,
instead of A = W Kuf, Lq^T A and the Kuf_bar product) against the Cholesky route in the same process, against autograd through
the oracle, for determinism across runs and overlap levels, for the fallbacks, and for the guard on Kuu's conditioning.
Every model has MercerMatern12sm components and a Matern-3/2 activation family, as the transcription model does."""
import numpy as np
import pytest

from helpers import pdgp_from_problem, oracle_elbo_and_grads, model_grad_dict

pytestmark = pytest.mark.gpu

ELBO_RTOL = 1e-9            # against the oracle (test_gpu_kuf_scan.py's bars)
ORACLE_TOL = 2e-7           # x block scale, against autograd
Q_VS_CHOL_ELBO = 1e-12      # relative
Q_VS_CHOL = 1e-9            # x block scale: the project's bar for two float64 forms of one gradient block

# M x N x P.  The components are the benchmark's in proportion: 20 partials and a lengthscale of 25 inducing spacings (0.25 ms
# at these sizes), which keeps tr(K) tr(K^-1) at 1.2 M^2 (the benchmark's 1.4).  With 3 partials the mixture decorrelates
# nothing at this spacing and only a lengthscale of 2 spacings is as well conditioned — and then x / l reaches M / 2, the
# rounding of the expanded squared distance (x / l)^2 2e-16 reaches the 1e-12 under the root, and autograd's lengthscale gradient
# is rounding noise at every frame that coincides with an inducing point: com0.lengthscales 3e-6 apart, on either route
# (test_inducing_inputs_on_frames_far_from_the_origin_against_oracle takes such a shape, against finite differences).
SHAPES = {
    "64x256x1": dict(N=256, M=64, P=1),          # one tile, one column group
    "128x512x2": dict(N=512, M=128, P=2),        # two row tiles, two families in one batch
    "192x768x2": dict(N=768, M=192, P=2),        # odd tile count, three column groups
    "64x4096x2": dict(N=4096, M=64, P=2),        # the smallest batch the helper streams take: Q is prepared on one of them
}
LS_COM = 0.00625
# The Matern-3/2 activations get 8 spacings.  Their default (1 s, 4000 spacings here) puts cond(Kuu) at its jitter bound, where
# the likelihood's 1e-16 response to ANY change in another family's fmean / fvar comes back as 2e-9 of the activation
# lengthscale's gradient (first run of this file: act0.lengthscales 1.8e-9 between the two routes of the COMPONENTS): no 1e-9
# comparison of two forms is meaningful there, as test_gpu_kuf_scan.py found for its packed thresholds.
LS_ACT = 0.002


def _problem(N, M, P, ls_com=LS_COM, com_type=None, seed=5):
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=20, seed=seed)
    spacing = (N / float(M)) / 4.0                              # in units of 0.25 ms: the same conditioning at every shape
    for d in prob["kern_act"]:
        d["lengthscales"] = LS_ACT * spacing
    for d in prob["kern_com"]:
        d["lengthscales"] = ls_com * spacing
        if com_type:
            d["type"] = com_type
    return prob


COUNTED = ("cond_A", "cond_LTA", "kuf_bar", "nt_gemm", "hyper")


def _evaluate(prob, h, qform=None, overlap=None, fix_zc=True, count=False, grad=True, **model_kw):
    """(ELBO, gradient vector, gradient by name, launches per timer of COUNTED or None).  qform None: as pdgp.py decides."""
    model = pdgp_from_problem(prob, handle=h, **model_kw)
    model.za.fixed = True
    if fix_zc:
        model.zc.fixed = True
    model._pack()
    if qform is not None:
        h.check(h.lib.gp_pdgp_set_qform(model._plan, int(qform)))
    if overlap is not None:
        h.check(h.lib.gp_pdgp_set_overlap(model._plan, overlap))
    if count:
        h.check(h.lib.gp_timers_enable(h.h, 1))
        h.check(h.lib.gp_timers_reset(h.h))
    try:
        f = model._elbo(grad)
        h.sync()
        launches = tuple(h.timers()[k][1] for k in COUNTED) if count else None
    finally:
        if count:
            h.check(h.lib.gp_timers_enable(h.h, 0))
    return f, model._grad.cpu().numpy().copy(), model_grad_dict(model), launches


@pytest.fixture(scope="module")
def oracle_refs():
    """autograd through the oracle, once per shape (the 4096-frame shape is there for the streams, not for another reference)"""
    return {s: oracle_elbo_and_grads(_problem(**SHAPES[s])) for s in SHAPES if s != "64x4096x2"}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_q_route_against_cholesky_route(gp_handle, shape):
    """pdgp.py allows the route at these lengthscales.  What the launch counts can show: the components' Kuf_bar product is
    gone (the activation family contracts by the scan, so no product is left at all), their G = Q Kuf is one more launch
    charged to cond_A, and the split-K product is still one launch.  cond_LTA cannot tell: one launch covers whichever GPs
    are left to it."""
    prob = _problem(**SHAPES[shape])
    f1, _, g1, n1 = _evaluate(prob, gp_handle, count=True)
    f0, _, g0, n0 = _evaluate(prob, gp_handle, qform=0, count=True)
    c1, c0 = dict(zip(COUNTED, n1)), dict(zip(COUNTED, n0))
    assert c0["kuf_bar"] == 1 and c1["kuf_bar"] == 0, (c1, c0)
    assert c1["cond_A"] == c0["cond_A"] + 1 and c1["cond_LTA"] == c0["cond_LTA"] and c1["nt_gemm"] == c0["nt_gemm"], (c1, c0)
    dev = abs(f1 - f0) / abs(f0)
    print("%s ELBO: Q vs Cholesky %.2e relative" % (shape, dev))
    assert dev <= Q_VS_CHOL_ELBO, (f1, f0)
    worst = 0.0
    for name in g0:
        scale = max(np.abs(g0[name]).max(), 1e-12)
        d = np.abs(g1[name] - g0[name]).max() / scale
        print("%s %s: Q vs Cholesky %.2e" % (shape, name, d))
        worst = max(worst, d)
        assert d <= Q_VS_CHOL, (name, d)
    print("%s gradient blocks: Q vs Cholesky, worst %.2e of a block's scale" % (shape, worst))
    # a step's ELBO is one number: the same route with or without a gradient
    f_nograd, _, _, _ = _evaluate(prob, gp_handle, grad=False)
    assert f_nograd == f1


@pytest.mark.parametrize("shape", sorted(s for s in SHAPES if s != "64x4096x2"))
def test_q_route_against_oracle(gp_handle, oracle_refs, shape):
    ref_f, ref_g = oracle_refs[shape]
    f, _, g, _ = _evaluate(_problem(**SHAPES[shape]), gp_handle)
    assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f), (f, ref_f)
    for name, rg in ref_g.items():
        if name.startswith("za") or name.startswith("zc"):      # fixed inducing inputs: no gradient asked
            continue
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
        scale = max(np.abs(rg).max(), 1e-12)
        np.testing.assert_allclose(g[name].reshape(rg.shape), rg, rtol=0, atol=ORACLE_TOL * scale, err_msg=name)


def test_inducing_inputs_on_frames_far_from_the_origin_against_oracle(gp_handle):
    """M = 256 inducing inputs on every fourth of 1024 frames, a lengthscale of one spacing: x / l reaches 256 and one ulp of its
    square 7e-12, seven times the 1e-12 under the root of r = sqrt((a - b)^2 + 1e-12).  The covariance build, the oracle and
    TensorFlow scale both inputs the same way, so a frame that coincides with an inducing input has a = b to the bit, the expanded
    square is 0 and r is 1e-6.  The matrix-core contractions (bwd.hip) scaled one side by x / l and the other by x * (1 / l):
    an ulp apart at 26 of these 256 pairs, the square then -7e-12 ... 0 instead of 0 — below -1e-12 at six of them, where the
    root is NaN and with it the lengthscale's gradient (found by test_gpu_qfar.py's M = 1024 case, on every route).
    Both routes at the bars of this file: against autograd for every block but that lengthscale.  Autograd differentiates the three
    terms of -2 a b + a a + b b one by one, so at a coincident pair its d r2 / d l is the rounding of three terms of size
    4 a^2 / l, not 0, and d r / d l = that / 2e-6: 2e-5 of the block's scale here, different on every BLAS.  The reference for
    the lengthscale is the central difference of the oracle's ELBO (numpy, four points, Richardson), whose own error the test
    bounds by taking it at two step sizes (measured: 1e-10 apart; the engine 9e-11 from it, autograd 1.8e-5)."""
    import copy
    from helpers import oracle_elbo
    prob = _problem(N=1024, M=256, P=1, ls_com=0.00025)

    def central(rel):
        def F(scale):
            p = copy.deepcopy(prob)
            p["kern_com"][0]["lengthscales"] = prob["kern_com"][0]["lengthscales"] * scale
            return float(oracle_elbo(p))
        d1, d2 = (F(1 + rel) - F(1 - rel)) / (2 * rel), (F(1 + 2 * rel) - F(1 - 2 * rel)) / (4 * rel)
        return (4 * d1 - d2) / 3 / prob["kern_com"][0]["lengthscales"]
    fd, fd_b = central(3e-3), central(1e-3)
    print("d ELBO / d l by central differences: %.10e and %.10e, %.2e apart" % (fd, fd_b, abs(fd - fd_b) / abs(fd)))
    assert abs(fd - fd_b) <= 0.1 * ORACLE_TOL * abs(fd)
    z, x, ls = np.ravel(prob["zc"][0]), np.ravel(prob["x"]), float(prob["kern_com"][0]["lengthscales"])
    on = np.isin(z, x)
    a, b = z[on] / ls, z[on] * (1.0 / ls)
    r2 = ((-2.0 * a) * b + a * a) + b * b
    assert on.all() and (r2 < -1e-12).any()                 # the mixed form has no root here; either form alone gives 0
    ref_f, ref_g = oracle_elbo_and_grads(prob)
    for qform in (None, 0):
        f, v, g, _ = _evaluate(prob, gp_handle, qform=qform)
        assert np.all(np.isfinite(v)), [n for n in g if not np.all(np.isfinite(g[n]))]
        print("qform %s: ELBO %.2e relative to the oracle" % (qform, abs(f - ref_f) / abs(ref_f)))
        worst = {}
        for name, rg in ref_g.items():
            if name.startswith("za") or name.startswith("zc"):
                continue
            if name.startswith("q_sqrt"):
                rg = np.tril(rg[:, :, 0])[:, :, None]
            if name == "com0.lengthscales":
                print("qform %s: %s against autograd %.2e" % (qform, name, abs(float(g[name][0]) - float(rg)) / abs(float(rg))))
                rg = np.array(fd)
            worst[name] = np.abs(g[name].reshape(rg.shape) - rg).max() / max(np.abs(rg).max(), 1e-12)
        top = sorted(worst, key=worst.get)[-3:]
        print("qform %s: gradient blocks against autograd, worst %s" % (qform, ["%s %.2e" % (n, worst[n]) for n in top]))
        assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f), (f, ref_f)
        assert all(d <= ORACLE_TOL for d in worst.values()), {n: d for n, d in worst.items() if not d <= ORACLE_TOL}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_q_route_is_deterministic_and_overlap_independent(gp_handle, shape):
    prob = _problem(**SHAPES[shape])
    f_a, g_a, _, n_a = _evaluate(prob, gp_handle, overlap=2, count=True)
    f_b, g_b, _, _ = _evaluate(prob, gp_handle, overlap=2)
    f_c, g_c, _, n_c = _evaluate(prob, gp_handle, overlap=0, count=True)
    assert dict(zip(COUNTED, n_a))["kuf_bar"] == 0 and n_a == n_c        # the Q route, at either level
    assert f_a == f_b == f_c
    assert np.array_equal(g_a, g_b)
    assert np.array_equal(g_a, g_c)


@pytest.mark.parametrize("case", ["ragged_1000x40x2", "f32", "unwhitened", "unfixed_zc", "mercer_matern52sm"])
def test_fallbacks_keep_the_cholesky_route(gp_handle, case):
    """The engine refuses the route by itself: with the permission forced on, the bits and the launch counts are those of the
    same model with it off."""
    shape, kw, pkw = SHAPES["64x256x1"], {}, {}
    if case == "ragged_1000x40x2":
        shape = dict(N=1000, M=40, P=2)
    elif case == "f32":
        kw = dict(float_type=np.float32)
    elif case == "unwhitened":
        kw = dict(whiten=False)
    elif case == "unfixed_zc":
        kw = dict(fix_zc=False)
    elif case == "mercer_matern52sm":
        pkw = dict(com_type="mercer_matern52sm")
    prob = _problem(**shape, **pkw)
    f1, g1, _, n1 = _evaluate(prob, gp_handle, qform=1, count=True, **kw)
    f0, g0, _, n0 = _evaluate(prob, gp_handle, qform=0, count=True, **kw)
    assert n1 == n0, (case, n1, n0)
    assert f1 == f0 and np.array_equal(g1, g0)


def test_an_ill_conditioned_kuu_is_an_error_not_a_less_accurate_result(gp_handle):
    """A component lengthscale of 1 s over inducing points 0.25 ms apart: tr(K) tr(K^-1) = 64 M^2 against the guard's 4 M^2.  pdgp.py does not allow the route there; forced on through the engine call, the evaluation returns the
    error that names the switch.  Nothing faults — the guard only reads L and W — and the handle works again afterwards."""
    from gpitch_amd import _lib
    prob = _problem(**dict(SHAPES["64x256x1"], ls_com=1.0))
    model = pdgp_from_problem(prob, handle=gp_handle)
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    assert not model._qform_admissible()
    f_ok = model._elbo(True)
    assert np.isfinite(f_ok)
    gp_handle.check(gp_handle.lib.gp_pdgp_set_qform(model._plan, 1))
    with pytest.raises(_lib.GpitchError) as err:
        model._elbo(True)
    assert err.value.status == _lib.GP_ERR_UNSUPPORTED and "qform" in str(err.value)
    gp_handle.check(gp_handle.lib.gp_pdgp_set_qform(model._plan, 0))
    assert model._elbo(True) == f_ok
