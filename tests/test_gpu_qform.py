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
# rounding of the expanded squared distance (x / l)^2 2e-16 reaches the 1e-12 under the root, and engine and oracle disagree
# about r at every frame that coincides with an inducing point: com0.lengthscales 3e-6 apart, on either route.
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
