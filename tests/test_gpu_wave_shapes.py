"""The wave-form strip products (gemm_wave.hip, float64; gemm_wave_f32.hip, float32) at every tile grid they take, against
torch-CPU autograd through the oracle.

A launch takes the wave form only when every GP of the batch has the same M, M % 64 == 0 and N % 256 == 0; the rest of the
suite mostly runs ragged shapes (the gemm_strip.hip / gemm.hip fallbacks).  The branches checked here:
  * triangular roles 1 (A = W Kuf) and 2 (Lq^T A) deal the 64-row tiles [t0, t1) in pairs (t0 + u, t1 - 1 - u); an odd
    count pairs the middle tile with itself (one pass);
  * the early row-block split of A = W Kuf (engine.hip cond_batch_run): tiles [0, 2) ahead of the join, [2, M / 64) after
    it.  It needs the diagonal-block event of the resident blocked factorisation, which the workgroup-cluster factorisation
    (chol_cluster.hip) does not leave: the cluster takes a Kuu batch of G matrices while G * cc_groups(M) <= 128 workgroups
    (cc_groups = 3, 5, 7, 13 at M = 192, 256, 320, 448), so the split cases carry enough pitches to exceed that
    (P = 22, 13, 10, 5);
  * the XCD renumbering, on only when (units * N / 256 * batch) % 8 == 0 — odd N / 256 (768, 2304, 4352) switches it off;
  * role 3 (Kuf_bar, dense: one launch over the batch of 2P GPs, or one per precision), role 5 (Kuf_bar with the fused
    stationary contraction, per kernel family: M a multiple of 128 and inducing inputs fixed);
  * sgpr_ss (one problem per launch) at M > 64, and the unwhitened model.

Tile grids in the docstrings: "tiles T; role r pairs ...; early split yes/no; remap on/off per launch (grid units x
column groups x batch)".  Nothing from the library is imported at module level (the CPU run collects this file).
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# float64 bounds of test_gpu_pdgp.py: ELBO 1e-9 relative, gradient blocks 2e-7 of their largest entry
ELBO_RTOL = 1e-9
GRAD_RTOL = 2e-7
# M = 448 (test_headline_M512_blocked_factorisation_gradient_vs_autograd allows 2e-5 at M = 512) and 13 pitches at M = 256:
# measured 2.6e-7 (act2.lengthscales, M = 448) and 2.4e-7 (com10.lengthscales, M = 256), the same to two digits with the
# wave form switched off — summation order of the Kuf-side contractions against the reference's, not the strip products
GRAD_RTOL_WIDE = 1e-6


def _f32_bounds():
    import test_gpu_f32 as t
    return t


def _grad_errors(got, ref, fixed_z=False):
    """largest deviation of every gradient block relative to its largest reference entry (q_sqrt: lower triangle, and the
    strict upper triangle of the HIP gradient must be exactly zero; fixed inducing inputs: exactly zero)"""
    errs = {}
    for name, rg in ref.items():
        gg = got[name]
        if fixed_z and name.startswith("z"):
            assert np.all(gg == 0), name
            continue
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
            assert np.all(np.triu(gg[:, :, 0], 1) == 0), name
        scale = max(np.abs(rg).max(), 1e-12)
        errs[name] = float(np.abs(gg.reshape(rg.shape) - rg).max() / scale)
    return errs


def _pdgp_case(handle, N, M, P, seed, whiten=True, fixed_z=False, float_type=None):
    """ELBO and every gradient block of the HIP path and of autograd through the oracle"""
    from gpitch_amd.synth import make_problem
    from helpers import model_grad_dict, oracle_elbo_and_grads, pdgp_from_problem
    prob = make_problem(N, M, P, num_partials=3, seed=seed)
    model = pdgp_from_problem(prob, whiten=whiten, handle=handle, float_type=float_type)
    if fixed_z:
        model.za.fixed = True
        model.zc.fixed = True
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob, whiten=whiten)
    errs = _grad_errors(model_grad_dict(model), ref_g, fixed_z)
    rel = abs(f - ref_f) / abs(ref_f)
    worst = max(errs, key=errs.get)
    print("N=%d M=%d P=%d: ELBO %.2e, worst gradient block %s %.2e" % (N, M, P, rel, worst, errs[worst]))
    return f, ref_f, errs


def _check_f64(handle, N, M, P, seed, elbo_rtol=ELBO_RTOL, grad_rtol=GRAD_RTOL, **kw):
    f, ref_f, errs = _pdgp_case(handle, N, M, P, seed, **kw)
    assert abs(f - ref_f) <= elbo_rtol * abs(ref_f), (f, ref_f)
    bad = {k: v for k, v in errs.items() if v > grad_rtol}
    assert not bad, bad


def _check_f32(handle, N, M, P, seed):
    """all-float32 strips against the float64 oracle: the stated bounds of test_gpu_f32.py"""
    t = _f32_bounds()
    f, ref_f, errs = _pdgp_case(handle, N, M, P, seed, float_type=np.float32)
    assert abs(f - ref_f) <= t.ELBO_RTOL * abs(ref_f), (f, ref_f)
    bad = {}
    for name, err in errs.items():
        ill = name.startswith("za") or (name.startswith("act") and name.endswith("lengthscales"))
        if err > (t.GRAD_RTOL_ILL if ill else t.GRAD_RTOL_FREQ if ".frequency" in name else t.GRAD_RTOL):
            bad[name] = err
    assert not bad, bad


# ---- 1. pdgp, float64 ----------------------------------------------------------------------------------------------------

def test_f64_one_self_paired_tile_M64_N768(gp_handle):
    """tiles 1; roles 1, 2 pair (0, 0) — one pass; early split no (N < 4096: no fork); remap off everywhere (roles 1, 2, 3:
    1 x 3 x 2 = 6 blocks); roles 1, 2, 3"""
    _check_f64(gp_handle, 768, 64, 1, seed=1)


def test_f64_three_tiles_M192_N2304(gp_handle):
    """tiles 3; roles 1, 2 pairs (0, 2), (1, 1); early split no (no fork); remap on for roles 1, 2 (2 x 9 x 4 = 72),
    off for role 3 (3 x 9 x 4 = 108); roles 1, 2, 3; Kuu by the cluster factorisation"""
    _check_f64(gp_handle, 2304, 192, 2, seed=2)


def test_f64_three_tiles_forked_cluster_M192_N4352(gp_handle):
    """tiles 3; roles 1, 2 pairs (0, 2), (1, 1); early split no — forked (N >= 4096), but the cluster factorisation (2 x 3
    workgroups) leaves no diagonal-block event; remap off everywhere (roles 1, 2: 2 x 17 x 2 = 68, role 3: 3 x 17 x 2);
    roles 1, 2, 3"""
    _check_f64(gp_handle, 4352, 192, 1, seed=3)


def test_f64_early_split_three_tiles_M192_N4352(gp_handle):
    """tiles 3; early split yes: role 1 tiles [0, 2) pair (0, 1), then [2, 3) tile 2 paired with itself (44 GPs x 3
    workgroups exceed the cluster factorisation: resident factor + blocked inverse with two 128-column panels, the last one
    64 wide); role 2 pairs (0, 2), (1, 1); remap off for both role 1 launches (1 x 17 x 44 = 748), on for role 2
    (2 x 17 x 44), off for role 3 (3 x 17 x 44); roles 1, 2, 3"""
    _check_f64(gp_handle, 4352, 192, 22, seed=4)


def test_f64_early_split_five_tiles_M320_N4352(gp_handle):
    """tiles 5; early split yes (20 GPs x 7 workgroups exceed the cluster): role 1 [0, 2) pair (0, 1), remap off
    (1 x 17 x 20 = 340), then [2, 5) pairs (2, 4), (3, 3), remap on (2 x 17 x 20); role 2 pairs (0, 4), (1, 3), (2, 2),
    remap off (3 x 17 x 20); role 3 remap off (5 x 17 x 20); blocked Kuu with a 64-column last panel; roles 1, 2, 3"""
    _check_f64(gp_handle, 4352, 320, 10, seed=5)


def test_f64_early_split_seven_tiles_M448_N4096(gp_handle):
    """tiles 7; early split yes (10 GPs x 13 workgroups exceed the cluster): role 1 [0, 2) pair (0, 1), then [2, 7) pairs
    (2, 6), (3, 5), (4, 4); role 2 pairs (0, 6), (1, 5), (2, 4), (3, 3); remap on everywhere (role 1: 1 x 16 x 10 and
    3 x 16 x 10, role 2: 4 x 16 x 10, role 3: 7 x 16 x 10); blocked Kuu, four panels, the last 64 wide; roles 1, 2, 3.
    Gradient bound GRAD_RTOL_WIDE (measured 2.6e-7)."""
    _check_f64(gp_handle, 4096, 448, 5, seed=6, grad_rtol=GRAD_RTOL_WIDE)


def test_f64_early_split_even_halves_M256_N4352(gp_handle):
    """tiles 4; early split yes with even halves (26 GPs x 5 workgroups exceed the cluster): role 1 [0, 2) pair (0, 1),
    then [2, 4) pair (2, 3); role 2 pairs (0, 3), (1, 2); remap off for roles 1, 2 (role 1: 1 x 17 x 26 = 442 twice,
    role 2: 2 x 17 x 26), on for role 3 (4 x 17 x 26); roles 1, 2, 3.  Gradient bound GRAD_RTOL_WIDE (measured 2.4e-7)."""
    _check_f64(gp_handle, 4352, 256, 13, seed=7, grad_rtol=GRAD_RTOL_WIDE)


def test_f64_fused_stationary_contraction_six_tiles_M384_N2304(gp_handle):
    """tiles 6; za and zc fixed, Matern-3/2 activations: the activation family's Kuf_bar takes role 5 (the fused stationary
    contraction) over 6 x 9 dense tiles x 2 GPs, remap off (108); the spectral-mixture family role 3, remap off (108); roles
    1, 2 pairs (0, 5), (1, 4), (2, 3), remap off (3 x 9 x 4 = 108); early split no (no fork); roles 1, 2, 3, 5.  (The fused
    form needs M a multiple of 128 — the 128 x 128 strip form is its fallback — so M = 320 would not reach it.)"""
    _check_f64(gp_handle, 2304, 384, 2, seed=8, fixed_z=True)


def test_f64_unwhitened_three_tiles_M192_N4352(gp_handle):
    """whiten=False: role 1 pairs (0, 2), (1, 1), remap on (2 x 17 x 4 = 136); W^T A and Lq^T A go to the generic
    products (role 2 takes the wave form for whitened models only); role 3 remap off (3 x 17 x 4); early split no (cluster
    factorisation); roles 1, 3"""
    _check_f64(gp_handle, 4352, 192, 2, seed=9, whiten=False)


# ---- 2. pdgp, float32 strips and mixed precision -------------------------------------------------------------------------

def test_f32_three_tiles_M192_N2304(gp_handle):
    """float32 strips (gemm_wave_f32.hip): tiles 3; roles 1, 2 pairs (0, 2), (1, 1), remap on (2 x 9 x 4); role 3 remap
    off (3 x 9 x 4); early split no"""
    _check_f32(gp_handle, 2304, 192, 2, seed=2)


def test_f32_early_split_five_tiles_M320_N4352(gp_handle):
    """float32 strips: tiles 5; early split yes (as test_f64_early_split_five_tiles_M320_N4352): role 1 [0, 2) pair (0, 1),
    remap off, then pairs (2, 4), (3, 3), remap on; role 2 pairs (0, 4), (1, 3), (2, 2), remap off; role 3 remap off"""
    _check_f32(gp_handle, 4352, 320, 10, seed=5)


def test_f32_early_split_seven_tiles_M448_N4096(gp_handle):
    """float32 strips: tiles 7; early split yes: role 1 [0, 2) pair (0, 1), then (2, 6), (3, 5), (4, 4); role 2 pairs
    (0, 6) .. (3, 3); remap on everywhere; gwf_convert_kernel's grid capped at 256 blocks (448^2 / 256 = 784 wanted)"""
    _check_f32(gp_handle, 4096, 448, 5, seed=6)


def test_mixed_precision_early_split_five_tiles_M320_N4352(gp_handle):
    """float_type=(float64, float32): the 10 activation GPs on gemm_wave.hip, the 10 component GPs on gemm_wave_f32.hip,
    each launch with batch 10: tiles 5; early split yes in both forms, as in the float64 case (role 1 [0, 2) remap off
    (170), then pairs (2, 4), (3, 3) remap off (340)); role 2 pairs (0, 4), (1, 3), (2, 2), remap off (510); role 3 remap
    off (850); the stated mixed-precision bounds of test_gpu_f32.py"""
    t = _f32_bounds()
    f, ref_f, errs = _pdgp_case(gp_handle, 4352, 320, 10, seed=5, float_type=(np.float64, np.float32))
    assert abs(f - ref_f) <= t.MIXED_ELBO_RTOL * abs(ref_f), (f, ref_f)
    bad = {}
    for name, err in errs.items():
        act = name.startswith(("za", "act")) or "_act" in name
        if err > (t.MIXED_GRAD_RTOL_ACT if act else t.GRAD_RTOL_FREQ if ".frequency" in name else t.MIXED_GRAD_RTOL):
            bad[name] = err
    assert not bad, bad


# ---- 3. sgpr_ss ----------------------------------------------------------------------------------------------------------

def _sgpr_case(handle, N, M, P, reg, float_type=None):
    """the collapsed bound and its gradient w.r.t. every constrained parameter, HIP path and autograd through the oracle"""
    from test_gpu_sgpr import _model, _problem, _torch_bound_and_grads
    X, Y, Z, kl = _problem(N, M, P, N + 1)
    m = _model(X, Y, Z, kl, 0.3, handle, reg=reg, float_type=float_type)
    m._compile(); m._pack()
    ps = m._param_list()
    x0 = np.array([p.transform.backward(p.value)[0] for p in ps])
    f, gfree = m._objective(x0)
    ref_b, ref_g = _torch_bound_and_grads(X, Y, Z, kl, 0.3, reg=reg)
    got = -gfree * (1. + np.exp(-x0))        # undo the positive-transform chain rule: d/d constrained
    rel_b = abs(-f - ref_b) / abs(ref_b)
    rel_g = np.abs(got - ref_g).max() / np.abs(ref_g).max()
    print("sgpr N=%d M=%d P=%d reg=%s: bound %.2e, gradient %.2e" % (N, M, P, reg, rel_b, rel_g))
    return -f, ref_b, got, ref_g, kl


def _check_sgpr_f64(handle, N, M, P, reg):
    b, ref_b, got, ref_g, _ = _sgpr_case(handle, N, M, P, reg)
    assert abs(b - ref_b) <= 1e-9 * abs(ref_b), (b, ref_b)
    np.testing.assert_allclose(got, ref_g, rtol=0, atol=2e-7 * np.abs(ref_g).max())


def test_sgpr_f64_two_tiles_M128_N2304(gp_handle):
    """sgpr_ss, one problem per launch: tiles 2; role 1 pair (0, 1), remap off (1 x 9 x 1); role 3 remap off (2 x 9);
    early split no; roles 1, 3"""
    _check_sgpr_f64(gp_handle, 2304, 128, 2, False)


def test_sgpr_f64_three_tiles_M192_N2304_reg(gp_handle):
    """sgpr_ss (reg=True): tiles 3; role 1 pairs (0, 2), (1, 1), remap off (2 x 9 x 1); role 3 remap off (3 x 9); early
    split no; roles 1, 3"""
    _check_sgpr_f64(gp_handle, 2304, 192, 3, True)


def test_sgpr_f64_five_tiles_M320_N4352(gp_handle):
    """sgpr_ss: tiles 5; role 1 pairs (0, 4), (1, 3), (2, 2), remap off (3 x 17 x 1); role 3 remap off (5 x 17); early
    split no; roles 1, 3"""
    _check_sgpr_f64(gp_handle, 4352, 320, 2, False)


def test_sgpr_f64_seven_tiles_M448_N4096_reg(gp_handle):
    """sgpr_ss (reg=True): tiles 7; role 1 pairs (0, 6), (1, 5), (2, 4), (3, 3), remap on (4 x 16 x 1 = 64); role 3
    remap on (7 x 16 = 112); early split no; roles 1, 3"""
    _check_sgpr_f64(gp_handle, 4096, 448, 1, True)


def test_sgpr_f32_five_tiles_M320_N4352(gp_handle):
    """sgpr_ss with float32 strips (gemm_wave_f32.hip): tiles 5; role 1 pairs (0, 4), (1, 3), (2, 2), remap off; role 3
    remap off; early split no; roles 1, 3.  The stated float32 bounds of test_gpu_f32.py: the bound 2e-4 relative, the
    gradient 5e-3 of its largest entry (2.5e-2 for the spectral-mixture frequencies)."""
    t = _f32_bounds()
    b, ref_b, got, ref_g, kl = _sgpr_case(gp_handle, 4352, 320, 2, False, float_type=np.float32)
    assert abs(b - ref_b) <= t.ELBO_RTOL * abs(ref_b), (b, ref_b)
    freq = [False]                                       # gradient order: noise, then per kernel variance, lengthscale,
    for d in kl:                                         # energies, frequencies (_torch_bound_and_grads)
        freq += [False, False] + [False] * len(d["energy"]) + [True] * len(d["frequency"])
    tol = np.where(freq, t.GRAD_RTOL_FREQ, t.GRAD_RTOL) * np.abs(ref_g).max()
    assert np.all(np.abs(got - ref_g) <= tol), (got, ref_g)


# ---- 4. the fallback forms at the same shapes ----------------------------------------------------------------------------

def test_fallback_strip_forms_at_the_wave_shapes():
    """With the wave form switched off (GPITCH_AMD_SWITCHES=strip_wave=0, read once per process) the float64 cases of this
    file run gemm_strip.hip's 128 x 128 tiles where M is a multiple of 128 (M = 128, 256, 384, the fused role 5 included)
    and gemm.hip's 128 x 128 tiles with a partial last row tile at M = 64, 192, 320 and 448 (the early split in 128-row
    blocks), and must meet the same references.  A child process, as test_fallback_strip_forms_keep_parity (its 13 cases
    take about 45 s)."""
    import subprocess
    env = dict(os.environ, GPITCH_AMD_SWITCHES="strip_wave=0")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-m", "gpu", "-x", "-k", "f64"],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and " passed" in r.stdout, (r.stdout[-1500:], r.stderr[-500:])
