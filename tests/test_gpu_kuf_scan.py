"""The scan form of the Kuf-side contraction (gpitch_amd/csrc/kuf_scan.hip: a Matern-3/2 / Matern-5/2 family with fixed
inducing inputs over ascending frames, no Kuf_bar product) against the product form in the same process, against autograd
through the oracle, for determinism, for the fallbacks and for a broken promise about the frames' order."""
import numpy as np
import pytest

from helpers import pdgp_from_problem, oracle_elbo_and_grads, model_grad_dict

pytestmark = pytest.mark.gpu

ELBO_RTOL = 1e-9
SCAN_VS_PRODUCT = 1e-9      # x block scale: test_gpu_pdgp.py's bar for "separable against entry-by-entry"
ORACLE_TOL = 2e-7           # x block scale: test_gpu_pdgp.py's bar against autograd


def _problem(N, M, P, ls, seed=11, ktypes=None, z_stretch=False):
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=3, seed=seed)
    for i, d in enumerate(prob["kern_act"]):
        d["lengthscales"] = ls
        if ktypes:
            d["type"] = ktypes[i]
    if z_stretch:
        # every activation threshold inside a 30-frame stretch that straddles a chunk boundary (many thresholds in two chunks,
        # none in the others), one of them equal to a frame, and two outside the frames' range (a far side with no chunk at
        # all).  Evenly spaced at 0.3 lengthscales: cond(Kuu) ~ 1e4.  (Packed at 0.006 lengthscales cond(Kuu) sits at its
        # jitter bound 2e8, W = L^-1 and with it Kuf_bar carry entries ~1e6 times the sums they cancel to, and ANY two
        # roundings of the same sum differ by ~1e-8 of it: no 1e-9 comparison of two forms is meaningful there.)
        x = prob["x"].reshape(-1)
        z = np.linspace(x[700], x[729], M - 2)
        z[np.argmin(np.abs(z - x[715]))] = x[715]
        z = np.concatenate([[x[0] - 3.0 * ls, x[-1] + 2.0 * ls], z])
        prob["za"] = [z.reshape(-1, 1).copy() for _ in range(P)]
    return prob


def _evaluate(prob, h, flag=None, fix_z=True, overlap=None, float_type=None, count=False):
    """(ELBO, gradient vector, gradient by name, launches charged to the (kuf_bar, hyper) timers or None).  The path shows in
    that pair: the scan form charges three launches to `hyper` and no product of the family to `kuf_bar`.  (kuf_bar alone
    cannot tell at ragged shapes, where ONE product launch covers every family: it stays at 1 when the scan takes one of
    them.)"""
    model = pdgp_from_problem(prob, handle=h, float_type=float_type)
    if fix_z:
        model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    if flag is not None:
        h.check(h.lib.gp_pdgp_set_frames_ascending(model._plan, int(flag)))
    if overlap is not None:
        h.check(h.lib.gp_pdgp_set_overlap(model._plan, overlap))
    if count:
        h.check(h.lib.gp_timers_enable(h.h, 1))
        h.check(h.lib.gp_timers_reset(h.h))
    try:
        f = model._elbo(True)
        h.sync()
        launches = (h.timers()["kuf_bar"][1], h.timers()["hyper"][1]) if count else None
    finally:
        if count:
            h.check(h.lib.gp_timers_enable(h.h, 0))
    return f, model._grad.cpu().numpy().copy(), model_grad_dict(model), launches


def _is_act_theta(name):
    return name.startswith("act") and (name.endswith(".variance") or name.endswith(".lengthscales"))


SHAPES = {
    "ragged_1000x40x2": dict(N=1000, M=40, P=2, ls=0.01),                                    # an Lc remainder, M + 1 = 41 rows
    "aligned_4096x128x2": dict(N=4096, M=128, P=2, ls=0.05, ktypes=["matern32", "matern52"]),   # cleared flag: fused wave product
    "stretch_2048x64x1": dict(N=2048, M=64, P=1, ls=1e-4, ktypes=["matern52"], z_stretch=True),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_scan_against_product(gp_handle, shape):
    prob = _problem(**SHAPES[shape])
    f1, _, g1, n1 = _evaluate(prob, gp_handle, count=True)              # pdgp.py sets the flag: the frames are ascending
    f0, _, g0, n0 = _evaluate(prob, gp_handle, flag=0, count=True)
    assert n1[0] <= n0[0] and n1[1] > n0[1], ("the scan path: no Kuf_bar product for the activation family", n1, n0)
    if shape.startswith("aligned"):            # one product launch per family there: those of the two activation families are gone
        assert n1[0] == n0[0] - 2, (n1, n0)
    assert f1 == f0
    for name in g0:
        if _is_act_theta(name):
            scale = max(np.abs(g0[name]).max(), 1e-12)
            dev = np.abs(g1[name] - g0[name]).max() / scale
            print("%s %s: scan vs product %.2e" % (shape, name, dev))
            assert dev <= SCAN_VS_PRODUCT, (name, dev)
        else:
            assert np.array_equal(g1[name], g0[name]), name


@pytest.fixture(scope="module")
def small_ref():
    prob = _problem(**SHAPES["ragged_1000x40x2"])
    return prob, oracle_elbo_and_grads(prob)


def _assert_matches_oracle(f, got, ref_f, ref_g, tol=ORACLE_TOL, with_za=False):
    assert abs(f - ref_f) <= ELBO_RTOL * abs(ref_f), (f, ref_f)
    for name, rg in ref_g.items():
        if name.startswith("zc") or (name.startswith("za") and not with_za):      # fixed inducing inputs: no gradient asked
            continue
        gg = got[name]
        if name.startswith("q_sqrt"):
            rg = np.tril(rg[:, :, 0])[:, :, None]
        scale = max(np.abs(rg).max(), 1e-12)
        np.testing.assert_allclose(gg.reshape(rg.shape), rg, rtol=0, atol=tol * scale, err_msg=name)


def test_scan_against_oracle(gp_handle, small_ref):
    prob, (ref_f, ref_g) = small_ref
    f, _, g, _ = _evaluate(prob, gp_handle)
    _assert_matches_oracle(f, g, ref_f, ref_g)


def test_scan_is_deterministic_and_overlap_independent(gp_handle):
    prob = _problem(**SHAPES["aligned_4096x128x2"])
    f_a, g_a, _, _ = _evaluate(prob, gp_handle, overlap=2)
    f_b, g_b, _, _ = _evaluate(prob, gp_handle, overlap=2)
    f_c, g_c, _, _ = _evaluate(prob, gp_handle, overlap=0)
    assert f_a == f_b == f_c
    assert np.array_equal(g_a, g_b)
    assert np.array_equal(g_a, g_c)


@pytest.mark.parametrize("case", ["unfixed_z", "matern12", "f32", "cleared_flag"])
def test_fallbacks_keep_the_product_path(gp_handle, small_ref, case):
    """Each of these must still form the Kuf_bar product: the launch counts of the kuf_bar and hyper timers are those of
    the same model with the flag cleared (the scan path's differ), so are the bits, and the gradient is the oracle's.  float32 strips cannot
    meet the float64 bar against the oracle; that case takes the bounds test_gpu_f32.py sets for a whitened model with
    float32 strips (5e-3 of a block's scale, 2e-1 for the ill-conditioned activation lengthscales, 2.5e-2 for frequencies)."""
    prob, (ref_f, ref_g) = small_ref
    kw = {}
    if case == "unfixed_z":
        kw = dict(fix_z=False)
    elif case == "matern12":
        prob = _problem(**dict(SHAPES["ragged_1000x40x2"], ktypes=["matern12", "matern12"]))
        ref_f, ref_g = oracle_elbo_and_grads(prob)
    elif case == "f32":
        kw = dict(float_type=np.float32)
    _, _, _, n_scan = _evaluate(_problem(**SHAPES["ragged_1000x40x2"]), gp_handle, count=True)
    f, gvec, g, n = _evaluate(prob, gp_handle, flag=(0 if case == "cleared_flag" else None), count=True, **kw)
    f0, gvec0, _, n0 = _evaluate(prob, gp_handle, flag=0, count=True, **kw)
    assert n == n0, (case, n, n0)
    if case == "cleared_flag":
        assert n != n_scan, (n, n_scan)
    assert f == f0 and np.array_equal(gvec, gvec0)
    if case == "f32":
        assert abs(f - ref_f) <= 2e-4 * abs(ref_f), (f, ref_f)
        for name, rg in ref_g.items():
            if name.startswith("za") or name.startswith("zc"):
                continue
            if name.startswith("q_sqrt"):
                rg = np.tril(rg[:, :, 0])[:, :, None]
            tol = 2e-1 if (name.startswith("act") and name.endswith("lengthscales")) else 2.5e-2 if ".frequency" in name else 5e-3
            scale = max(np.abs(rg).max(), 1e-12)
            assert np.abs(g[name].reshape(rg.shape) - rg).max() <= tol * scale, name
    else:
        _assert_matches_oracle(f, g, ref_f, ref_g, with_za=(case == "unfixed_z"))


def test_a_wrong_promise_is_an_error_not_a_wrong_gradient(gp_handle):
    """The flag set through the engine call on a model whose resident frames were shuffled (pdgp.py's own check would
    clear it): the streaming kernel sees a descending pair among the neighbours it reads anyway and raises the handle's
    device status word; the evaluation returns the error status.  Nothing faults: every index the scan forms stays inside
    its arrays whatever the order of x."""
    from gpitch_amd import _lib
    prob = dict(_problem(**SHAPES["ragged_1000x40x2"]))
    perm = np.random.RandomState(0).permutation(prob["N"])
    prob["x"], prob["y"] = prob["x"][perm], prob["y"][perm]
    model = pdgp_from_problem(prob, handle=gp_handle)
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    f_ok = model._elbo(True)                       # pdgp.py cleared the flag: the product path, no error
    assert np.isfinite(f_ok)
    gp_handle.check(gp_handle.lib.gp_pdgp_set_frames_ascending(model._plan, 1))
    with pytest.raises(_lib.GpitchError) as err:
        model._elbo(True)
    assert err.value.status == _lib.GP_ERR_BAD_ARG and "not ascending" in str(err.value)
    # the status word is cleared with the report: the handle works again
    gp_handle.check(gp_handle.lib.gp_pdgp_set_frames_ascending(model._plan, 0))
    assert model._elbo(True) == f_ok
