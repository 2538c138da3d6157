"""Spectral-mixture kernels at every partial count m (1 <= m <= 32), and pitches whose kernels carry different m, against
float64 references: the oracle's operators, torch-CPU autograd through the oracle (pdgp, sgpr_ss) and the one-window
engine (window batch).

The device pads m to mpad = 4 ceil(m / 4) and picks its instantiation, and often its algorithm, from mpad, from
NT = ceil(2 mpad / 16) feature tiles (NT = 1: m <= 8, 2: 9-16, 3: 17-24, 4: 25-32) and from whether a launch's kernels
share m.  What each case reaches:
  1. operators (test_operators_*): gp_kernel_build / gp_kernel_diag / gp_kernel_build_f32 of one kernel at (109, 1000):
     launch_mercer<MP> (cov_build_kernel<1, 2, MP, ENV>) for MP = 4 .. 32 and ENV = 0 (mercer_matern12sm) and 2
     (mercer_matern52sm), cov_build_kernel<2, 1, 1, 0> (the broadcast form: matern12sm, matern32sm) at m = 1 .. 32.
  2. pdgp, float64, one m per kernel family (test_pdgp_family_*), inducing inputs fixed so that every family is batched:
     (a) M = 256, N = 4096 (M N >= 2^20, N % 128 == 0): Kuf builds cov_mercer_mfma_kernel<8, 0, ..> (m = 5, staged) and
         cov_mercer_mfma_lean_kernel<12 / 24 / 32, 0, ..>; contractions hyper_sm_rows_lean_kernel<1 / 2 / 3, false>
         (m = 5, 12, 24) and hyper_contract_kernel<32, true, ..> (m = 29);
     (b) M = 72 (not a multiple of 16), N = 2004 (= 4 mod 16): hyper_sm_rows_kernel<1, false, false> (m = 4),
         <2, false, false> (m = 9, 16), hyper_contract_kernel<20 / 24 / 28, true, ..> (m = 17, 24, 26); Kuf by
         launch_mercer<MP> (cov_build_kernel<1, 2, MP, 0>);
     (c) mercer_matern52sm, m = 3, 10, 16, 22, 32: hyper_sm_rows_kernel<1 / 2, true, false>, then
         hyper_contract_kernel<24 / 32, true, ..>; at the shape of (a) also cov_mercer_mfma_kernel<4, 2, ..> and
         cov_mercer_mfma_lean_kernel<12 / 16 / 24 / 32, 2, ..> (the ENV = 2 builds);
     (d) legacy broadcast kernels matern12sm / matern32sm at m = 1 and 32: hyper_m12sm_kernel;
     (e) three pitches, every component at m = 24 (then 32), N = 4096: the two-family schedule (activation family and one
         component family) with hyper_sm_rows_lean_kernel<3, false> (m = 24) or hyper_contract_kernel<32, true, ..>.
  3. pdgp with six pitches, component m = [7, 20, 7, 1, 13, 32] (the m = 7 family has non-adjacent members) and
     activations [matern32, matern12, matern32, rbf, matern52, matern32] (test_pdgp_mixed_*): more than two families,
     so the general side-stream schedule; whitened with z fixed (batched families: lean NT = 1 / 2 / 3 and
     hyper_contract_kernel<32, ..>), z trained (per-GP contractions with inducing-input gradients), unwhitened, inducing
     counts that differ inside a family (m = [9, 20, 9] at M = [48, 64, 80]: the per-GP path, lean form; m = [9, 9] at
     M = [72, 56], N = 2004: the per-GP path, row form), and
     all-float32 / (float64, float32) strips (the G32 variants hyper_sm_rows_lean_kernel<NT, true>).  Predictions of the
     mixed model against the oracle.
  4. sgpr_ss, mixed m per source (test_sgpr_mixed_partials): m = [1, 3, 4, 2] hyper_contract_sum_kernel<4> (the fused
     sum contraction, tail items off), m = [5, 8, 6] one shared feature launch at mpad 8, m = [2, 9, 20, 32] one
     hyper_contract_kernel<MPAD, ..> per kernel; reg False / True, M = 48 and M = 96.
  5. window batch (test_window_batch_mixed_partials): template m = [3, 12, 20] (feature and hyper-sum strides sized by
     max m, one contraction launch per source with its own m, finish with 2 + 2 max m blocks) at (2001, 64) and at
     (4096, 256), where M N = 2^20 switches the contraction geometry to 32-row workgroups; eager, captured, replayed.
  6. m = 0 and m = 33 are refused by Pdgp, SGPRSS and SgprWindowBatch with GpitchError before anything is launched.
Every partial frequency stays below 0.45 fs (f0 <= 220 Hz at fs = 16 kHz, partials q f0) and the energies of a kernel
sum to 1 (0.2 for matern32sm, whose per-partial variances are bounded by 0.25).  Nothing from the library is imported
at module level (the CPU run collects this file).
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ELBO_RTOL = 1e-9
GRAD_RTOL = 2e-7
ALL_M = [1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 21, 24, 25, 28, 29, 32]
SM_TYPES = ["mercer_matern12sm", "mercer_matern52sm", "matern12sm", "matern32sm"]


def _f0(i):
    """fundamental of the i-th kernel: 55 Hz .. 220 Hz"""
    return 55. * 2. ** ((5 * i) % 25 / 12.)


def _sm(ktype, m, f0):
    """a spectral-mixture kernel dict (oracle format) with m partials q f0 and energies summing to 1"""
    w = 1. / np.arange(1., m + 1.)
    e = list(w / w.sum())
    d = {"type": ktype, "variance": 1.0, "lengthscales": 0.1, "energy": e, "frequency": [q * f0 for q in range(1, m + 1)]}
    if ktype == "mercer_matern52sm":
        d["variance"], d["lengthscales"] = 0.5, 0.01
    elif ktype == "matern12sm":
        d["variance"], d["lengthscales"] = 0.9, 0.05
    elif ktype == "matern32sm":
        d["lengthscales"] = 0.02
        d["energy"] = [0.2 * v for v in e]           # variance_k ~ Logistic(0, 0.25); no global variance
    return d


_ACT_LS = {"matern32": 1.0, "matern12": 0.5, "rbf": 0.002, "matern52": 0.01}


def _act(ktype):
    return {"type": ktype, "variance": 3.5, "lengthscales": _ACT_LS[ktype], "energy": [], "frequency": []}


def _problem(N, M, com, act=None, seed=0):
    """make_problem with the component kernels `com` (and activation kernels `act`) edited in per pitch"""
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, len(com), num_partials=3, seed=seed, base_midi=45)
    for p, d in enumerate(com):
        prob["kern_com"][p] = d
    for p, t in enumerate(act or []):
        prob["kern_act"][p] = _act(t)
    return prob


def _set_inducing(prob, role, p, M, seed):
    """pitch p's inducing set of `role` ("act" / "com") replaced by M uniform points with fresh q_mu / q_sqrt"""
    from gpitch_amd.synth import uniform_inducing
    rng = np.random.RandomState(seed)
    prob["za" if role == "act" else "zc"][p] = uniform_inducing(prob["x"], M)
    prob["q_mu_" + role][p] = 0.3 * rng.randn(M, 1)
    prob["q_sqrt_" + role][p] = np.tril(np.eye(M) + 0.05 * rng.randn(M, M))[:, :, None].copy()


def _pdgp_case(handle, prob, whiten=True, fixed_z=False, float_type=None):
    """ELBO and every gradient block of the HIP path against autograd through the oracle"""
    from helpers import model_grad_dict, oracle_elbo_and_grads, pdgp_from_problem
    from test_gpu_wave_shapes import _grad_errors
    model = pdgp_from_problem(prob, whiten=whiten, handle=handle, float_type=float_type)
    for kk in list(model.kern_act) + list(model.kern_com):
        if getattr(kk, "oracle_name", "") == "matern12sm":     # energies / frequencies fixed by default (reference :34)
            kk.vars_n_freqs_fixed(False, False)
    if fixed_z:
        model.za.fixed = True
        model.zc.fixed = True
    model._pack()
    f = model._elbo(True)
    ref_f, ref_g = oracle_elbo_and_grads(prob, whiten=whiten)
    errs = _grad_errors(model_grad_dict(model), ref_g, fixed_z)
    rel = abs(f - ref_f) / abs(ref_f)
    worst = max(errs, key=errs.get)
    print("pdgp N=%d m=%s: ELBO %.2e, worst gradient block %s %.2e"
          % (prob["x"].shape[0], [len(d["frequency"]) for d in prob["kern_com"]], rel, worst, errs[worst]))
    return model, f, ref_f, errs


def _check_f64(handle, prob, elbo_rtol=ELBO_RTOL, grad_rtol=GRAD_RTOL, **kw):
    model, f, ref_f, errs = _pdgp_case(handle, prob, **kw)
    assert abs(f - ref_f) <= elbo_rtol * abs(ref_f), (f, ref_f)
    bad = {k: v for k, v in errs.items() if v > grad_rtol}
    assert not bad, bad
    return model


# ---- 1. operators at every mpad -----------------------------------------------------------------------------------------

def _desc(h, k):
    from test_gpu_ops import _desc as d
    return d(h, k)


@pytest.mark.parametrize("m", ALL_M)
@pytest.mark.parametrize("ktype", SM_TYPES)
def test_operators_at_every_partial_count(gp_handle, ktype, m):
    """gp_kernel_build (K(X1, X2), K(X) and its accumulate form) and gp_kernel_diag against the oracle at the tolerances
    of test_kernel_build_matches_oracle; gp_kernel_build_f32 is the float64 build rounded once (rows padded to 4)"""
    import ctypes as C
    from oracle import gpflow05 as orc
    h = gp_handle
    kern = _sm(ktype, m, _f0(m))
    n1, n2 = 109, 1000
    rng = np.random.RandomState(m)
    x2 = np.sort(rng.rand(n2, 1), 0) * 0.5
    x1 = x2[rng.choice(n2, n1, replace=False)].copy()
    d, th = _desc(h, kern)
    dx1, dx2 = h.to_device(x1), h.to_device(x2)
    out = h.empty(n1, n2)
    h.check(h.lib.gp_kernel_build(h.h, C.byref(d), dx1.data_ptr(), n1, dx2.data_ptr(), n2, out.data_ptr(), n2, 0))
    K64 = out.cpu().numpy()
    np.testing.assert_allclose(K64, orc.K(kern, x1, x2), rtol=1e-11, atol=1e-12)
    outs = h.empty(n1, n1)
    h.check(h.lib.gp_kernel_build(h.h, C.byref(d), dx1.data_ptr(), n1, None, 0, outs.data_ptr(), n1, 0))
    np.testing.assert_allclose(outs.cpu().numpy(), orc.K(kern, x1, None), rtol=1e-11, atol=1e-12)
    h.check(h.lib.gp_kernel_build(h.h, C.byref(d), dx1.data_ptr(), n1, None, 0, outs.data_ptr(), n1, 1))
    np.testing.assert_allclose(outs.cpu().numpy(), 2 * orc.K(kern, x1, None), rtol=1e-11, atol=1e-12)
    kd = h.empty(n2)
    h.check(h.lib.gp_kernel_diag(h.h, C.byref(d), n2, kd.data_ptr(), 0))
    np.testing.assert_allclose(kd.cpu().numpy(), orc.Kdiag(kern, x2), rtol=1e-15)
    ld = (n2 + 3) // 4 * 4
    out32 = h.torch.full((n1, ld), 7.0, dtype=h.torch.float32, device=h.device)
    h.check(h.lib.gp_kernel_build_f32(h.h, C.byref(d), dx1.data_ptr(), n1, dx2.data_ptr(), n2, out32.data_ptr(), ld, 0))
    np.testing.assert_array_equal(out32[:, :n2].cpu().numpy(), K64.astype(np.float32))


# ---- 2. pdgp, float64, one m per family -----------------------------------------------------------------------------------

def test_pdgp_family_lean_forms_and_mfma_builds_M256_N4096(gp_handle):
    """m = 5, 12, 24, 29 (mpad 8, 12, 24, 32): Kuf builds cov_mercer_mfma_kernel<8, 0, ..> and
    cov_mercer_mfma_lean_kernel<12 / 24 / 32, 0, ..>; contractions hyper_sm_rows_lean_kernel<1 / 2 / 3, false> and
    hyper_contract_kernel<32, true, ..> (NT = 4)"""
    com = [_sm("mercer_matern12sm", m, _f0(i)) for i, m in enumerate([5, 12, 24, 29])]
    prob = _problem(4096, 256, com, seed=1)
    # activations at l = 20 ms (cond(Kuu) 1e6): at make_problem's l = 1 s (cond 9e8) act0.lengthscales deviates by
    # 5.3e-6, 9.8e-6 with strip_wave=0, 2.0e-6 with chol_cluster=0, and 0.8e-6 .. 4.5e-6 with every component at m = 5
    # or m = 12 — the ill-conditioned direction moving with the summation order, whatever the partial counts
    for d in prob["kern_act"]:
        d["lengthscales"] = 0.02
    _check_f64(gp_handle, prob, fixed_z=True)


def test_pdgp_family_row_forms_ragged_M72_N2004(gp_handle):
    """M = 72, N = 2004: no lean form; hyper_sm_rows_kernel<1, false, false> (m = 4), <2, false, false> (m = 9, 16),
    hyper_contract_kernel<20 / 24 / 28, true, ..> (m = 17, 24: NT = 3; m = 26: NT = 4); Kuf by
    launch_mercer<4 / 12 / 16 / 20 / 24 / 28>"""
    com = [_sm("mercer_matern12sm", m, _f0(i)) for i, m in enumerate([4, 9, 16, 17, 24, 26])]
    _check_f64(gp_handle, _problem(2004, 72, com, seed=2), fixed_z=True)


@pytest.mark.parametrize("N,M", [(2004, 72), (4096, 256)])
def test_pdgp_family_matern52_envelope(gp_handle, N, M):
    """mercer_matern52sm, m = 3, 10, 16, 22, 32: hyper_sm_rows_kernel<1, true, false> (m = 3), <2, true, false>
    (m = 10, 16), hyper_contract_kernel<24 / 32, true, ..>; at (4096, 256) the ENV = 2 Kuf builds
    cov_mercer_mfma_kernel<4, 2, ..> and cov_mercer_mfma_lean_kernel<12 / 16 / 24 / 32, 2, ..>"""
    com = [_sm("mercer_matern52sm", m, _f0(i)) for i, m in enumerate([3, 10, 16, 22, 32])]
    _check_f64(gp_handle, _problem(N, M, com, seed=3), fixed_z=True)


@pytest.mark.parametrize("ktype", ["matern12sm", "matern32sm"])
def test_pdgp_family_legacy_broadcast_kernels(gp_handle, ktype):
    """two pitches, m = 1 and m = 32 (two families): hyper_m12sm_kernel with 1 and 32 partials, cov_build_kernel's
    broadcast form"""
    com = [_sm(ktype, 1, 110.), _sm(ktype, 32, 220.)]
    _check_f64(gp_handle, _problem(1200, 40, com, seed=4), fixed_z=True)


@pytest.mark.parametrize("m", [24, 32])
def test_pdgp_family_two_family_schedule_N4096(gp_handle, m):
    """three pitches, every component at m (one component family beside the activation family): the forked two-family
    schedule at N = 4096 with hyper_sm_rows_lean_kernel<3, false> (m = 24) or hyper_contract_kernel<32, true, ..>"""
    com = [_sm("mercer_matern12sm", m, _f0(i)) for i in range(3)]
    _check_f64(gp_handle, _problem(4096, 128, com, seed=5 + m), fixed_z=True)


# ---- 3. pdgp, mixed m and mixed activation types ---------------------------------------------------------------------------

MIXED_M = [7, 20, 7, 1, 13, 32]
MIXED_ACT = ["matern32", "matern12", "matern32", "rbf", "matern52", "matern32"]


def _mixed_problem(N=2048, M=64, seed=11):
    com = [_sm("mercer_matern12sm", m, _f0(i)) for i, m in enumerate(MIXED_M)]
    return _problem(N, M, com, act=MIXED_ACT, seed=seed)


def test_pdgp_mixed_whitened_fixed_z(gp_handle):
    """families (matern32 x 3), matern12, rbf, matern52, m = 7 (pitches 0 and 2), 20, 1, 13, 32: hyper_sm_rows_lean_kernel
    <1 / 2 / 3, false>, hyper_contract_kernel<32, true, ..>; fam_slot0 = -1 for the m = 7 and matern32 families (no fused
    stationary contraction there).  Predictions against the oracle as well."""
    from oracle import gpflow05 as orc
    prob = _mixed_problem()
    model = _check_f64(gp_handle, prob, fixed_z=True)
    xt = prob["x"][::5].copy()
    got = model.predict_act_n_com(xt)
    ref = orc.pdgp_predict_act_n_com(xt, prob["za"], prob["zc"], prob["kern_act"], prob["kern_com"], prob["q_mu_act"],
                                     prob["q_sqrt_act"], prob["q_mu_com"], prob["q_sqrt_com"])
    for g, r in zip(got, ref):
        for i in range(prob["P"]):
            np.testing.assert_allclose(g[i], r[i], rtol=0, atol=1e-8 * max(np.abs(r[i]).max(), 1e-3))


def test_pdgp_mixed_whitened_z_trained(gp_handle):
    """inducing inputs trained: every family on the per-GP contractions with inducing-input gradients"""
    _check_f64(gp_handle, _mixed_problem(seed=12))


def test_pdgp_mixed_unwhitened(gp_handle):
    """whiten=False with the mixed families (z trained); the Matern-3/2 activations at l = 10 ms, where Kuu^-1 (which
    the unwhitened model applies) is conditioned well enough for the float64 bounds (cond 2e8 at l = 1 s)"""
    prob = _mixed_problem(N=1600, M=48, seed=13)
    for d in prob["kern_act"]:
        if d["type"] == "matern32":
            d["lengthscales"] = 0.01
    _check_f64(gp_handle, prob, whiten=False)


@pytest.mark.parametrize("N,ms,Ms", [(2048, [9, 20, 9], [48, 64, 80]), (2004, [9, 9], [72, 56])],
                         ids=["lean_N2048", "rows_ragged_N2004"])
def test_pdgp_mixed_inducing_counts_inside_a_family(gp_handle, N, ms, Ms):
    """m = [9, 20, 9] at M = [48, 64, 80] (activations too): the m = 9 family holds two inducing counts, so it takes the
    per-GP path (hyper_sm_rows_lean_kernel<2, false>: M and N multiples of 16); m = 20 alone is batched (lean NT = 3).
    m = [9, 9] at M = [72, 56], N = 2004 (no multiple of 16): the per-GP path with hyper_sm_rows_kernel<2, false, false>,
    its record passed by value"""
    com = [_sm("mercer_matern12sm", m, _f0(i)) for i, m in enumerate(ms)]
    prob = _problem(N, max(Ms), com, act=["matern32", "matern12", "matern32"][:len(ms)], seed=14)
    for p, M in enumerate(Ms):
        _set_inducing(prob, "act", p, M, 100 + p)
        _set_inducing(prob, "com", p, M, 200 + p)
    _check_f64(gp_handle, prob, fixed_z=True)


def test_pdgp_mixed_float32_strips(gp_handle):
    """all-float32 strips: the G32 contraction variants; the stated bounds of test_gpu_f32.py"""
    import test_gpu_f32 as t
    model, f, ref_f, errs = _pdgp_case(gp_handle, _mixed_problem(seed=15), fixed_z=True, float_type=np.float32)
    assert abs(f - ref_f) <= t.ELBO_RTOL * abs(ref_f), (f, ref_f)
    bad = {}
    for name, err in errs.items():
        ill = name.startswith("za") or (name.startswith("act") and name.endswith("lengthscales"))
        if err > (t.GRAD_RTOL_ILL if ill else t.GRAD_RTOL_FREQ if ".frequency" in name else t.GRAD_RTOL):
            bad[name] = err
    assert not bad, bad


def test_pdgp_mixed_precision_activation_f64_component_f32(gp_handle):
    """float_type=(float64, float32): float64 activation families, float32 (G32) component families; the stated
    mixed-precision bounds of test_gpu_f32.py"""
    import test_gpu_f32 as t
    model, f, ref_f, errs = _pdgp_case(gp_handle, _mixed_problem(seed=16), fixed_z=True,
                                       float_type=(np.float64, np.float32))
    assert abs(f - ref_f) <= t.MIXED_ELBO_RTOL * abs(ref_f), (f, ref_f)
    bad = {}
    for name, err in errs.items():
        act = name.startswith(("za", "act")) or "_act" in name
        if err > (t.MIXED_GRAD_RTOL_ACT if act else t.GRAD_RTOL_FREQ if ".frequency" in name else t.MIXED_GRAD_RTOL):
            bad[name] = err
    assert not bad, bad


# ---- 4. sgpr_ss, mixed m per source ----------------------------------------------------------------------------------------

def _sgpr_problem(N, M, ms, seed):
    from test_gpu_sgpr import _problem as sp
    X, Y, Z, kl = sp(N, M, len(ms), seed)
    for p, m in enumerate(ms):
        d = _sm("mercer_matern12sm", m, _f0(p + 1))
        d["variance"], d["lengthscales"] = 1.0 + 0.1 * p, 0.05 + 0.02 * p
        kl[p] = d
    return X, Y, Z, kl


@pytest.mark.parametrize("reg", [False, True])
@pytest.mark.parametrize("ms", [[1, 3, 4, 2], [5, 8, 6], [2, 9, 20, 32]], ids=["sum", "shared_mpad8", "per_kernel"])
def test_sgpr_mixed_partials(gp_handle, ms, reg):
    """bound within 1e-9 and gradient within 2e-7 of its largest entry against autograd; reg=False at (1500, 48),
    reg=True at (2500, 96) (M > 64: the 32 x 32 tile chain)"""
    from test_gpu_sgpr import _model, _torch_bound_and_grads
    N, M = (2500, 96) if reg else (1500, 48)
    X, Y, Z, kl = _sgpr_problem(N, M, ms, N + len(ms))
    m = _model(X, Y, Z, kl, 0.3, gp_handle, reg=reg)
    m._compile(); m._pack()
    ps = m._param_list()
    x0 = np.array([p.transform.backward(p.value)[0] for p in ps])
    f, gfree = m._objective(x0)
    ref_b, ref_g = _torch_bound_and_grads(X, Y, Z, kl, 0.3, reg=reg)
    got = -gfree * (1. + np.exp(-x0))        # undo the positive-transform chain rule: d/d constrained
    print("sgpr m=%s reg=%s: bound %.2e, gradient %.2e" % (ms, reg, abs(-f - ref_b) / abs(ref_b),
                                                         np.abs(got - ref_g).max() / np.abs(ref_g).max()))
    assert abs(-f - ref_b) <= 1e-9 * abs(ref_b), (-f, ref_b)
    np.testing.assert_allclose(got, ref_g, rtol=0, atol=2e-7 * np.abs(ref_g).max())


# ---- 5. window batch, mixed m per source -----------------------------------------------------------------------------------

@pytest.mark.parametrize("N,M,nwin", [(2001, 64, 4), (4096, 256, 3)])
def test_window_batch_mixed_partials(gp_handle, N, M, nwin):
    """template m = [3, 12, 20]: per window against the oracle (1e-9) and the one-window engine (bound 1e-11, gradient
    1e-9), eager, captured and replayed"""
    from oracle import gpflow05 as orc
    from gpitch_amd.windows import SgprWindowBatch
    from test_gpu_sgpr import _model
    from test_gpu_windows_batched import _params_vector, _windows
    ms = [3, 12, 20]
    wins = _windows(nwin, N, M, len(ms))
    for w, (_, _, _, kl) in enumerate(wins):
        for p, m in enumerate(ms):
            d = _sm("mercer_matern12sm", m, _f0(p + w + 1))
            d["variance"], d["lengthscales"] = kl[p]["variance"], kl[p]["lengthscales"]
            kl[p] = d
    tmpl = _model(*wins[0][:3], wins[0][3], 0.3, gp_handle)
    dev = SgprWindowBatch(tmpl, nwin + 1, N, M, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    noises = [0.3 + 0.05 * i for i in range(nwin)]
    pv = np.stack([_params_vector(nz, w[3]) for nz, w in zip(noises, wins)])
    assert pv.shape[1] == dev.nparams
    try:
        for rep in range(3):                                           # eager, captured, replayed
            bound, grad = dev.evaluate(pv)
            for i, w in enumerate(wins):
                ref = orc.sgpr_bound(w[0], w[1], w[2], w[3], noises[i])
                assert abs(bound[i] - ref) <= 1e-9 * abs(ref), (rep, i, bound[i], ref)
                one = _model(w[0], w[1], w[2], w[3], noises[i], gp_handle)
                one._compile(); one._pack()
                g1 = gp_handle.zeros(one._nparams)
                f1 = one._bound(grad=g1)
                assert abs(bound[i] - f1) <= 1e-11 * abs(f1), (rep, i, bound[i], f1)
                g1 = g1.cpu().numpy()
                assert np.abs(grad[i] - g1).max() <= 1e-9 * max(np.abs(g1).max(), 1e-12), (rep, i)
    finally:
        dev.close()


# ---- 6. partial counts out of range ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", [0, 33])
def test_partial_counts_out_of_range_are_refused(gp_handle, m):
    """m = 0 and m = 33 (beside a valid kernel): GpitchError from the plan's creation, nothing launched, the handle
    still usable afterwards"""
    from gpitch_amd import _lib
    from gpitch_amd.windows import SgprWindowBatch
    from helpers import oracle_elbo, pdgp_from_problem
    from test_gpu_sgpr import _model
    bad = {"type": "mercer_matern12sm", "variance": 1.0, "lengthscales": 0.1, "energy": [1. / 33] * m,
           "frequency": [55. * q for q in range(1, m + 1)]}
    prob = _problem(600, 16, [_sm("mercer_matern12sm", 3, 110.), bad], seed=21)
    with pytest.raises(_lib.GpitchError):
        pdgp_from_problem(prob, handle=gp_handle).compute_log_likelihood()
    X, Y, Z, kl = _sgpr_problem(600, 16, [3, 2], 22)
    kl[1] = bad
    with pytest.raises(_lib.GpitchError):
        _model(X, Y, Z, kl, 0.3, gp_handle).build_likelihood()
    tmpl = _model(X, Y, Z, kl, 0.3, gp_handle)
    with pytest.raises(_lib.GpitchError):
        SgprWindowBatch(tmpl, 2, 600, 16, handle=gp_handle)
    gp_handle.sync()
    good = _problem(600, 16, [_sm("mercer_matern12sm", 3, 110.)], seed=23)
    got = pdgp_from_problem(good, handle=gp_handle).compute_log_likelihood()
    ref = float(oracle_elbo(good))
    assert abs(got - ref) <= ELBO_RTOL * abs(ref)
