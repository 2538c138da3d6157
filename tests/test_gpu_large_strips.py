"""Models whose M x N strips reach or pass 2 GiB, against the frame-chunked float64 oracle (tests/helpers.py).

The wave-form strip products (gemm_wave.hip, float64; gemm_wave_f32.hip, float32) address A, B and C through buffer
resources: 32-bit byte offsets, num_records = 2^31 - 1.  An access outside that range does not fault — loads return 0 and
stores are dropped — so a strip of 2^31 bytes or more would give a wrong ELBO, gradient or bound with no error.  Every case
here builds a fresh model and checks its FIRST evaluation (no earlier launch at the same parameters could have left the
right values behind a dropped store), and compares every gradient block whole: the part of a row-major strip past 2^31
bytes is its last inducing rows, i.e. the last rows of za, zc, q_mu and q_sqrt.

Strip sizes (M = 512 throughout; ld = N, a multiple of 256):
  float64, N = 2^19 = 524288           512 x 524288 x 8 B = 2^31 B exactly      (the last 16-byte access ends at 2^31)
  float64, N = 2^19 + 768 = 525056     512 x 525056 x 8 B = 2^31 + 3 MiB        (past it)
  float32, N = 2^20 + 256 = 1048832    512 x 1048832 x 4 B = 2^31 + 512 KiB     (past it)
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from helpers import (model_grad_dict, oracle_elbo_and_grads_chunked, oracle_predict_act_n_com_chunked,  # noqa: E402
                     oracle_sgpr_bound_and_grads_chunked, oracle_sgpr_predict_f_chunked,
                     pdgp_from_problem)

M = 512
N_EDGE = 1 << 19
N_PAST = (1 << 19) + 3 * 256
N_F32 = (1 << 20) + 256
GIB2 = 1 << 31
LIB_CHUNK = 65536            # frames per model of the library's own chunked evaluation (strips of 256 MiB / 128 MiB)

# float64: the bounds of test_gpu_pdgp.py::test_headline_M512_blocked_factorisation_gradient_vs_autograd (M = 512,
# cond(Kuu) ~ 1e9), of test_gpu_sgpr.py::test_sgpr_gradient_matches_autograd / test_sgpr_predictions_match_oracle and of
# test_gpu_fullsize.py::test_cfg2_one_pitch_N32768_M512 (predictions)
ELBO_RTOL, GRAD_RTOL = 1e-8, 2e-5
PRED_RTOL = 1e-7
SG_BOUND_RTOL, SG_GRAD_RTOL, SG_PRED_RTOL = 1e-9, 2e-7, 1e-8
# the SGPRSS kernels' lengthscale entries, relative to themselves: each is a sum over the 2.7e8 Kuf entries whose terms
# cancel (tests/test_oracle_chunked.py: the oracle's own value moves by up to 6e-7 with the order of summation at 5000
# frames).  Measured on MI355X at N = 525056: 7.6e-6 (the other entries within 2e-7 of the largest); unfixed strips: 1e-3.
SG_GRAD_RTOL_LS = 5e-5
# float32 strips against the float64 oracle: the stated bounds of test_gpu_f32.py
F32_ELBO_RTOL = 2e-4
F32_GRAD_RTOL, F32_GRAD_RTOL_ILL, F32_GRAD_RTOL_FREQ = 5e-3, 2e-1, 2.5e-2
# float32, one launch over all frames against the same float32 model evaluated by the library on chunks of LIB_CHUNK frames
# (only the summation order and the float32 rounding of the strips' products differ).  Measured on MI355X: ELBO 2.5e-10,
# worst gradient block 2.8e-5 of its largest entry (q_sqrt_com0); unfixed strips past 2^31 gave a NaN ELBO
F32_SELF_ELBO_RTOL, F32_SELF_GRAD_RTOL = 2e-9, 1e-4


def _strip_bytes(N, elem):
    ld = (N + 1) & ~1 if elem == 8 else (N + 3) & ~3       # (csrc/common.h gp_strip_ld)
    return M * ld * elem


def _problem(N):
    from gpitch_amd.synth import make_problem
    return make_problem(N, M, 1, num_partials=5, seed=40)


_ORACLE = {}


def _oracle(N):
    """the chunked oracle's ELBO and gradient, computed once per frame count (cases b and c share the problem)"""
    if N not in _ORACLE:
        _ORACLE[N] = oracle_elbo_and_grads_chunked(_problem(N))
    return _ORACLE[N]


def _grad_errors(got, ref, skip=()):
    """largest deviation of each gradient block relative to the block's largest reference entry"""
    out = {}
    for name, rg in ref.items():
        if name in skip:
            continue
        gg = got[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
            assert np.all(np.triu(gg[:, :, 0], 1) == 0), name
        out[name] = np.abs(gg.reshape(rg.shape) - rg).max() / max(np.abs(rg).max(), 1e-12)
    return out


def _report(what, f, ref_f, errs):
    worst = max(errs, key=errs.get)
    print("%s: ELBO %.3e relative, worst gradient block %s %.3e" % (what, abs(f - ref_f) / abs(ref_f), worst, errs[worst]))


def _f32_tol(name):
    ill = name.startswith("za") or (name.startswith("act") and name.endswith("lengthscales"))
    return F32_GRAD_RTOL_ILL if ill else F32_GRAD_RTOL_FREQ if ".frequency" in name else F32_GRAD_RTOL


def _library_chunked(prob, handle, float_type=None):
    """the ELBO and gradient of the whole-batch model assembled from models over LIB_CHUNK frames each: every chunk model's
    ELBO carries the whole KL term, so sum_c ELBO_c + (n - 1) KL, and the gradient likewise with the whitened KL's
    gradient (q_mu and q_sqrt blocks only: d/d q_mu = q_mu, d/d Lq = Lq - diag(1 / diag Lq))"""
    from gpitch_amd.pdgp import Pdgp
    from gpitch_amd.synth import kernels_from_problem
    N = prob["N"]
    f_sum, g_sum, n = 0.0, None, 0
    for s in range(0, N, LIB_CHUNK):
        m = Pdgp(prob["x"][s:s + LIB_CHUNK], prob["y"][s:s + LIB_CHUNK], [prob["za"], prob["zc"]],
                 kernels_from_problem(prob), whiten=True, handle=handle, float_type=float_type)
        for i in range(prob["P"]):
            m.q_mu_act[i].value = prob["q_mu_act"][i]
            m.q_mu_com[i].value = prob["q_mu_com"][i]
            m.q_sqrt_act[i].value = prob["q_sqrt_act"][i]
            m.q_sqrt_com[i].value = prob["q_sqrt_com"][i]
        m.likelihood.variance = prob["noise_var"]
        m._pack()
        f_sum += m._elbo(True)
        g = model_grad_dict(m)
        g_sum = g if g_sum is None else {k: g_sum[k] + v for k, v in g.items()}
        kl = m.build_prior_kl()
        n += 1
        del m
    f = f_sum + (n - 1) * kl
    for i in range(prob["P"]):
        for side in ("act", "com"):
            mu, sq = prob["q_mu_%s" % side][i], np.tril(prob["q_sqrt_%s" % side][i][:, :, 0])
            g_sum["q_mu_%s%d" % (side, i)] += (n - 1) * mu
            g_sum["q_sqrt_%s%d" % (side, i)] += (n - 1) * (sq - np.diag(1.0 / np.diag(sq)))[:, :, None]
    return f, g_sum


@pytest.mark.parametrize("N", [N_EDGE, N_PAST])
def test_pdgp_f64_elbo_and_gradient_at_and_past_2GiB(gp_handle, N):
    """cases (a) and (b): float64 Pdgp, P = 1, M = 512 for both latent GPs, full batch.  N = 2^19: every strip is
    512 x 524288 x 8 B = 2^31 B exactly (the boundary itself: the last 16-byte access ends one byte past num_records);
    N = 525056: 2^31 + 3 MiB, past it.  Against the chunked oracle and against the library's own chunk sums."""
    assert _strip_bytes(N, 8) >= GIB2
    prob = _problem(N)
    model = pdgp_from_problem(prob, handle=gp_handle)
    model._pack()
    f = model._elbo(True)
    got = model_grad_dict(model)
    del model
    ref_f, ref_g = _oracle(N)
    errs = _grad_errors(got, ref_g)
    lib_f, lib_g = _library_chunked(prob, gp_handle)
    lib_errs = _grad_errors(got, lib_g)
    _report("N = %d vs oracle" % N, f, ref_f, errs)
    _report("N = %d vs library chunks" % N, f, lib_f, lib_errs)
    assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f), (f, ref_f)
    bad = {k: v for k, v in errs.items() if v > GRAD_RTOL}
    assert not bad, bad
    assert abs(f - lib_f) <= ELBO_RTOL * abs(lib_f), (f, lib_f)
    bad = {k: v for k, v in lib_errs.items() if v > GRAD_RTOL}
    assert not bad, bad


def test_pdgp_f64_fused_stationary_contraction_past_2GiB(gp_handle):
    """case (c): as (b) (512 x 525056 x 8 B = 2^31 + 3 MiB per strip, past 2^31) with the activation GP's inducing inputs
    fixed: its Matern32 Kuf_bar is contracted inside the product (role 5, no strip stored), and the engine sizes the
    partial records by gemm_fused_contraction_records — the record count and the launch taken must agree"""
    assert _strip_bytes(N_PAST, 8) >= GIB2
    prob = _problem(N_PAST)
    model = pdgp_from_problem(prob, handle=gp_handle)
    model.za.fixed = True
    model._pack()
    f = model._elbo(True)
    got = model_grad_dict(model)
    del model
    ref_f, ref_g = _oracle(N_PAST)
    errs = _grad_errors(got, ref_g, skip=("za0",))
    _report("za fixed, N = %d vs oracle" % N_PAST, f, ref_f, errs)
    assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f), (f, ref_f)
    bad = {k: v for k, v in errs.items() if v > GRAD_RTOL}
    assert not bad, bad


def test_pdgp_f64_predictions_one_launch_past_2GiB(gp_handle):
    """case (d): predict_act_n_com at all 525056 frames in one conditional launch (max_predict_batch = N): strips of
    512 x 525056 x 8 B = 2^31 + 3 MiB, past 2^31"""
    from gpitch_amd.pdgp import Pdgp
    from gpitch_amd.synth import kernels_from_problem
    assert _strip_bytes(N_PAST, 8) >= GIB2
    prob = _problem(N_PAST)
    model = Pdgp(prob["x"], prob["y"], [prob["za"], prob["zc"]], kernels_from_problem(prob), whiten=True,
                 handle=gp_handle, max_predict_batch=N_PAST)
    model.q_mu_act[0].value = prob["q_mu_act"][0]
    model.q_mu_com[0].value = prob["q_mu_com"][0]
    model.q_sqrt_act[0].value = prob["q_sqrt_act"][0]
    model.q_sqrt_com[0].value = prob["q_sqrt_com"][0]
    model.likelihood.variance = prob["noise_var"]
    got = model.predict_act_n_com(prob["x"])
    del model
    ref = oracle_predict_act_n_com_chunked(prob, prob["x"])
    for name, got_l, ref_l in zip(("mean_act", "var_act", "mean_com", "var_com", "mean_source"), got, ref):
        assert got_l[0].shape == ref_l[0].shape == (N_PAST, 1), name
        err = np.abs(got_l[0] - ref_l[0]).max()
        assert err <= PRED_RTOL * max(np.abs(ref_l[0]).max(), 1e-3), (name, err)


def _sgpr_problem(N):
    from test_gpu_sgpr import _problem as sg_problem
    return sg_problem(N, M, 2, 41)


def _sgpr_bound_and_grad(m):
    """the bound and its gradient w.r.t. the constrained parameters (test_gpu_sgpr.py: the positive transform undone)"""
    m._compile()
    m._pack()
    ps = m._param_list()
    x0 = np.array([p.transform.backward(p.value)[0] for p in ps])
    f, gfree = m._objective(x0)
    return -f, -gfree * (1. + np.exp(-x0))


def test_sgpr_f64_bound_gradient_and_predict_f_past_2GiB(gp_handle):
    """case (e): SGPRSS float64, two Mercer sources, M = 512, N = 525056: A' and Kuf_bar strips of
    512 x 525056 x 8 B = 2^31 + 3 MiB, past 2^31.  Bound and gradient against checkpointed chunked autograd; predict_f
    at every frame, from a second fresh model"""
    from test_gpu_sgpr import _model as sg_model
    assert _strip_bytes(N_PAST, 8) >= GIB2
    X, Y, Z, kl = _sgpr_problem(N_PAST)
    b, g = _sgpr_bound_and_grad(sg_model(X, Y, Z, kl, 0.5, gp_handle))
    ref_b, ref_g = oracle_sgpr_bound_and_grads_chunked(X, Y, Z, kl, 0.5)
    print("SGPRSS float64: bound %.3e relative, gradient %.3e of its largest entry"
          % (abs(b - ref_b) / abs(ref_b), np.abs(g - ref_g).max() / np.abs(ref_g).max()))
    assert abs(b - ref_b) <= SG_BOUND_RTOL * abs(ref_b), (b, ref_b)
    ls = np.zeros(g.shape, dtype=bool)
    o = 1
    for d in kl:                              # [noise, then per kernel: variance, lengthscales, energies, frequencies]
        ls[o + 1] = True
        o += 2 + len(d["energy"]) + len(d["frequency"])
    np.testing.assert_allclose(g[ls], ref_g[ls], rtol=SG_GRAD_RTOL_LS, atol=0)
    np.testing.assert_allclose(g[~ls], ref_g[~ls], rtol=0, atol=SG_GRAD_RTOL * np.abs(ref_g).max())
    mean, var = sg_model(X, Y, Z, kl, 0.5, gp_handle).predict_f(X)
    rm, rv = oracle_sgpr_predict_f_chunked(X, X, Y, Z, kl, 0.5)
    assert mean.shape == rm.shape == (N_PAST, 1) and var.shape == rv.shape
    np.testing.assert_allclose(mean, rm, rtol=0, atol=SG_PRED_RTOL * np.abs(rm).max())
    np.testing.assert_allclose(var, rv, rtol=0, atol=SG_PRED_RTOL * np.abs(rv).max())


def test_pdgp_f32_elbo_and_gradient_past_2GiB(gp_handle):
    """case (f): float32 strips, P = 1, M = 512, N = 1048832: 512 x 1048832 x 4 B = 2^31 + 512 KiB per strip, past 2^31.
    Against the float64 chunked oracle at test_gpu_f32.py's stated bounds, and — tighter — against the same float32 model
    evaluated by the library on chunks of 65536 frames (strips of 128 MiB)"""
    from test_gpu_f32 import _model as f32_model
    assert _strip_bytes(N_F32, 4) >= GIB2
    prob = _problem(N_F32)
    model = f32_model(prob, gp_handle)
    model._pack()
    f = model._elbo(True)
    got = model_grad_dict(model)
    del model
    lib_f, lib_g = _library_chunked(prob, gp_handle, float_type=np.float32)
    self_elbo = abs(f - lib_f) / abs(lib_f)
    self_grad = _grad_errors(got, lib_g)
    ref_f, ref_g = oracle_elbo_and_grads_chunked(prob)
    _report("float32 vs oracle", f, ref_f, _grad_errors(got, ref_g))
    _report("float32 vs library chunks", f, lib_f, self_grad)
    assert abs(f - ref_f) <= F32_ELBO_RTOL * abs(ref_f), (f, ref_f)
    bad = {k: v for k, v in _grad_errors(got, ref_g).items() if v > _f32_tol(k)}
    assert not bad, bad
    assert self_elbo <= F32_SELF_ELBO_RTOL, (f, lib_f)
    bad = {k: v for k, v in self_grad.items() if v > F32_SELF_GRAD_RTOL}
    assert not bad, bad


def test_sgpr_f32_bound_and_gradient_past_2GiB(gp_handle):
    """case (g): SGPRSS with float32 strips, two Mercer sources, M = 512, N = 1048832: strips of
    512 x 1048832 x 4 B = 2^31 + 512 KiB, past 2^31.  The SGPRSS float32 products provide no float32 copy of the M x M
    operand, so they take the strip forms at every size: this case covers those past 2^31.  Bound and gradient against
    the float64 chunked oracle at test_gpu_f32.py's stated bounds"""
    from test_gpu_sgpr import _model as sg_model
    assert _strip_bytes(N_F32, 4) >= GIB2
    X, Y, Z, kl = _sgpr_problem(N_F32)
    b, g = _sgpr_bound_and_grad(sg_model(X, Y, Z, kl, 0.5, gp_handle, float_type=np.float32))
    ref_b, ref_g = oracle_sgpr_bound_and_grads_chunked(X, Y, Z, kl, 0.5)
    print("SGPRSS float32: bound %.3e relative, gradient %.3e of its largest entry"
          % (abs(b - ref_b) / abs(ref_b), np.abs(g - ref_g).max() / np.abs(ref_g).max()))
    assert abs(b - ref_b) <= F32_ELBO_RTOL * abs(ref_b), (b, ref_b)
    np.testing.assert_allclose(g, ref_g, rtol=0, atol=F32_GRAD_RTOL * np.abs(ref_g).max())
