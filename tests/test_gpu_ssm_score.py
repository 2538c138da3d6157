"""The score of the exact likelihood on the GPU (SGPRSS.exact_log_likelihood_and_grad / optimize(objective="exact"),
SgprWindowBatch.exact_loglik_grad, windows.fit_windows_exact, csrc/ssm_smooth.hip): every case of tests/ssm_smooth_ref.py against
the numpy restatement (tests/ssm_score_ref.py) under 1e-8 max(|ref_i|, S_i, 1e-3) per entry, the batched and chunked forms bit
for bit against the one-window call, the model layer (columns, fixed Params, a mean function), the exact fits, and the argument
checks of the ABI."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ssm_score_ref as S  # noqa: E402
import ssm_smooth_ref as R  # noqa: E402

IDS = [S.case_id(i) for i in range(len(S.CASES))]
_REF = {}


def _ref(i):
    """the restatement of case i, computed once"""
    if i not in _REF:
        X, Y, _, kl, nz = S.case(i)
        _REF[i] = S.score(X, Y[:, 0], kl, nz)
    return _REF[i]


def _within(got, ref, scale, what):
    ratio = (np.abs(np.asarray(got) - np.asarray(ref)) / S.bar(np.asarray(ref), np.asarray(scale))).max()
    print("    %s: worst |device - restatement| / bar %.3e" % (what, ratio))
    assert ratio <= 1.0, what


@pytest.mark.parametrize("i", range(len(S.CASES)), ids=IDS)
def test_matches_restatement(gp_handle, i):
    X, Y, _, kl, nz = S.case(i)
    m = R.model(X, Y, kl, nz, gp_handle)
    ll, g = m.exact_log_likelihood_and_grad()
    rl, rg, rs, _ = _ref(i)
    assert g.shape == rg.shape == (len(m._param_list()),)
    _within(g, rg, rs, "gradient")
    assert abs(ll - rl) <= 1e-8 * max(abs(rl), 1e-3)
    assert ll == m.exact_log_likelihood()                     # the forward walk's bits, with and without its history
    m._destroy()


# ---- batched ------------------------------------------------------------------------------------------------------------------
def _three_windows():
    """three windows of N = 37 frames on one kernel structure (d = 65, all three families) with their own data and parameters"""
    kl0 = R.kernels(65)
    wins = []
    for w in range(3):
        X, Y, _, _ = R.problem(37, 1, 2, 70 + w)
        kl = [dict(k) for k in kl0]
        for p, k in enumerate(kl):
            k["variance"] = k["variance"] * (1.0 + 0.2 * w)
            k["lengthscales"] = k["lengthscales"] * (1.0 + 0.1 * ((w + p) % 3))
        wins.append((X + 0.01 * w, Y * (1.0 + 0.3 * w), kl, 0.05 + 0.1 * w))
    return wins


def test_batched_windows_are_the_one_window_call(gp_handle):
    from gpitch_amd.windows import SgprWindowBatch
    wins = _three_windows()
    tmpl = R.model(wins[0][0], wins[0][1], wins[0][2], wins[0][3], gp_handle)
    dev = SgprWindowBatch(tmpl, 3, 37, 4, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[0][:4] for w in wins])
    pv = np.stack([S.param_vector(w[3], w[2]) for w in wins])
    ll, g = dev.exact_loglik_grad(pv)
    assert ll.shape == (3,) and g.shape == (3, pv.shape[1])
    for q, w in enumerate(wins):
        one = R.model(w[0], w[1], w[2], w[3], gp_handle)
        l1, g1 = one.exact_log_likelihood_and_grad()
        l2, g2 = one.exact_log_likelihood_and_grad()
        assert l1 == l2 and np.array_equal(g1, g2)            # two calls
        assert ll[q] == l1 and np.array_equal(g[q], g1)       # the window among others
        one._destroy()
    for chunk in (1, 2):
        llc, gc = dev.exact_loglik_grad(pv, chunk=chunk)
        assert np.array_equal(llc, ll) and np.array_equal(gc, g)
    ll0, g0 = dev.exact_loglik_grad(pv, with_grad=False)      # the forward walk alone
    assert g0 is None and np.array_equal(ll0, ll)
    dev.close()
    tmpl._destroy()


# ---- the model layer ----------------------------------------------------------------------------------------------------------
def test_two_output_columns_sum(gp_handle):
    X, Y, _, kl, nz = S.case(IDS.index("d4-N37-mixed-s0.03"))
    Y2 = np.hstack([Y, 0.5 * Y[::-1]])
    m = R.model(X, Y2, kl, nz, gp_handle)
    ll, g = m.exact_log_likelihood_and_grad()
    r0, r1 = S.score(X, Y2[:, 0], kl, nz), S.score(X, Y2[:, 1], kl, nz)
    _within(g, r0[1] + r1[1], r0[2] + r1[2], "two columns")
    assert abs(ll - (r0[0] + r1[0])) <= 1e-8 * abs(r0[0] + r1[0]) and ll == m.exact_log_likelihood()
    m._destroy()


def test_linear_mean_function(gp_handle):
    """the mean function's entries follow the engine's: d / d A = -sum_j gres_j x_j, d / d b = -sum_j gres_j with gres = -uu"""
    from gpitch_amd.mean_functions import Linear
    X, Y, _, kl, nz = S.case(IDS.index("d65-N37-dup-s0.1"))
    A, b = 3.0, -0.4
    m = R.model(X, Y + A * X + b, kl, nz, gp_handle, mean_function=Linear(A, b))
    ll, g = m.exact_log_likelihood_and_grad()
    rl, rg, rs, gres = S.score(X, ((Y + A * X + b) - (A * X + b))[:, 0], kl, nz)
    x = X[:, 0]
    ref = np.concatenate([rg, [-np.dot(gres, x), -gres.sum()]])
    scale = np.concatenate([rs, [np.abs(gres * x).sum(), np.abs(gres).sum()]])
    assert g.shape == ref.shape
    _within(g, ref, scale, "engine and mean-function entries")
    m._destroy()


def _perturbed(i, gp_handle, seed=0, X=None, Y=None):
    """case i's model (MercerMatern12sm: every hyper-parameter trainable) with the frequencies fixed and the others moved off
    their values"""
    Xc, Yc, _, kl, nz = S.case(i)
    m = R.model(Xc if X is None else X, Yc if Y is None else Y, kl, nz, gp_handle)
    rng = np.random.RandomState(seed)
    m.likelihood.variance = nz * 3.0
    for k in m.kern.kern_list:
        for f in k.frequency:
            f.fixed = True
        k.variance = k.variance.value[0] * (0.6 + 0.3 * rng.rand())
        k.lengthscales = k.lengthscales.value[0] * (1.3 + 0.3 * rng.rand())
        for e in k.energy:
            e.assign(e.value[0] * (0.8 + 0.4 * rng.rand()))
    return m


def test_a_fixed_param_gets_no_step(gp_handle):
    i = IDS.index("d4-N37-mixed-s0.03")
    m = _perturbed(i, gp_handle)
    k = m.kern.kern_list[0]
    k.lengthscales.fixed = True
    before = [p.value.copy() for p in m._param_list()]
    m.optimize(objective="exact", maxiter=3)
    after = [p.value.copy() for p in m._param_list()]
    for p, a, b in zip(m._param_list(), before, after):
        if p.fixed:
            assert np.array_equal(a, b)
    assert np.array_equal(k.lengthscales.value, before[2]) and all(np.array_equal(a, b) for a, b in zip(before[5:], after[5:]))
    assert not np.array_equal(before[0], after[0]) and not np.array_equal(before[1], after[1])
    m._destroy()


def test_optimize_exact(gp_handle):
    i = IDS.index("d4-N300-mixed-s0.001")
    m = _perturbed(i, gp_handle)
    start = m.exact_log_likelihood()
    res = m.optimize(objective="exact", maxiter=20)
    end = m.exact_log_likelihood()
    print("    exact log-likelihood %.6f -> %.6f in %d evaluations" % (start, end, res.nfev))
    assert end >= start
    assert abs(res.fun + end) <= 1e-10 * abs(end)
    m.Z = m.X._array[::50] + 1e-5                             # Z plays no part
    assert m.exact_log_likelihood() == end
    m._destroy()


def test_fit_windows_exact_is_each_windows_own_optimize(gp_handle):
    from gpitch_amd.windows import fit_windows_exact
    i = IDS.index("d4-N300-mixed-s0.001")
    wins = []
    for w in range(4):
        X, Y, _, _ = R.problem(300, 1, 2, 90 + w)
        wins.append((X + 0.004 * w, Y * (1.0 + 0.2 * w)))
    res = fit_windows_exact(lambda h: _perturbed(i, h), wins, maxiter=20, batch=4, handle=gp_handle)
    assert len(res) == 4
    for q, (X, Y) in enumerate(wins):
        one = _perturbed(i, gp_handle, X=X, Y=Y)
        r1 = one.optimize(objective="exact", maxiter=20)
        own = np.array([p.value[0] for p in one._param_list()])
        assert res[q]["params"].shape == own.shape
        assert np.all(np.abs(res[q]["params"] - own) <= 1e-8 * np.abs(own))
        assert abs(res[q]["loglik"] + r1.fun) <= 1e-8 * abs(r1.fun) and res[q]["nfev"] == r1.nfev and res[q]["nit"] == r1.nit
        assert res[q]["noise"] == res[q]["params"][0] and res[q]["variances"].shape == (1,)
        one._destroy()


# ---- arguments through the ABI: nothing is enqueued -----------------------------------------------------------------------------
def _plan(h, codes, N):
    from gpitch_amd import _lib
    P = len(codes)
    i32 = C.c_int32 * P
    keep = (i32(*[c for c, _ in codes]), i32(*[m for _, m in codes]))
    cfg = _lib.SgprConfig(P, N, 4, keep[0], keep[1], 1e-6, 0)
    plan = C.c_void_p()
    h.check(h.lib.gp_sgpr_create(h.h, C.byref(cfg), C.byref(plan)))
    return plan, keep


def test_arguments(gp_handle):
    from gpitch_amd import _lib
    h, lib = gp_handle, gp_handle.lib
    i = IDS.index("d4-N37-mixed-s0.03")
    X, Y, _, kl, nz = S.case(i)
    N, d, P = 37, 4, 1
    order = np.ascontiguousarray(np.argsort(X[:, 0], kind="stable").astype(np.int32))
    plan, keep = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 2)], N)
    pv = S.param_vector(nz, kl)
    par, xd, yd = h.to_device(pv), h.to_device(X.reshape(-1)), h.to_device(Y.reshape(-1))
    sentinel = -77.0
    ll, grad, resid = h.zeros(1) + sentinel, h.zeros(pv.size) + sentinel, h.zeros(N) + sentinel
    need = int(lib.gp_ssm_score_workspace_bytes(d, N, P, 1))
    ws = h.workspace(need)

    def call(plan_=plan, ws_bytes=need, **kw):
        a = dict(params=par.data_ptr(), X=xd.data_ptr(), Y=yd.data_ptr(), order=order.ctypes.data, ll=ll.data_ptr(),
                 grad=grad.data_ptr(), resid=resid.data_ptr(), ws=ws.data_ptr())
        a.update(kw)
        st = lib.gp_sgpr_exact_loglik_grad(plan_, a["params"], a["X"], a["Y"], N, a["order"], a["ll"], a["grad"], a["resid"],
                                           a["ws"], ws_bytes)
        msg = lib.gp_last_error(h.h)
        return st, (msg.decode() if msg else "")

    def untouched():
        h.sync()
        return all(bool((t == sentinel).all()) for t in (ll, grad, resid))

    for name in ("params", "X", "Y", "order", "ll", "grad", "ws"):                                   # a null pointer
        st, msg = call(**{name: None})
        assert st == _lib.GP_ERR_BAD_ARG and "null" in msg, name
    st, msg = call(ws_bytes=need - 256)                                                             # a short workspace
    assert st == _lib.GP_ERR_BAD_ARG and "workspace" in msg
    st, msg = call(ws_bytes=int(lib.gp_ssm_smooth_workspace_bytes(d, N, P, 1)))                     # (the smoother's is short)
    assert st == _lib.GP_ERR_BAD_ARG and "workspace" in msg
    bad = order.copy()
    bad[3] = bad[4]                                                                                 # not a permutation
    st, msg = call(order=bad.ctypes.data)
    assert st == _lib.GP_ERR_BAD_ARG and "permutation" in msg
    bad = order.copy()
    bad[5] = N                                                                                      # an entry past the frames
    st, msg = call(order=bad.ctypes.data)
    assert st == _lib.GP_ERR_BAD_ARG and "permutation" in msg
    p129, keep129 = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 32), (_lib.KERN_MERCER_MATERN12SM, 32), (_lib.KERN_MATERN12, 0)], N)
    st, msg = call(plan_=p129)                                                                      # d = 129
    assert st == _lib.GP_ERR_UNSUPPORTED and "128" in msg
    p32, keep32 = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 2), (_lib.KERN_MATERN32, 0)], N)
    st, msg = call(plan_=p32)                                                                       # a Matern32 in the sum
    assert st == _lib.GP_ERR_UNSUPPORTED and "Matern-1/2" in msg
    assert untouched()
    # the measured workspace is accepted; resid_grad may be null
    st, msg = call(resid=None)
    assert st == _lib.GP_OK, msg
    h.sync()
    assert bool((resid == sentinel).all())
    st, msg = call()
    assert st == _lib.GP_OK, msg
    rl, rg, rs, gres = _ref(i)
    _within(grad.cpu().numpy(), rg, rs, "gradient through the ABI")
    assert np.abs(resid.cpu().numpy() - gres).max() <= 1e-8 * max(np.abs(gres).max(), 1e-3)
    for pl in (plan, p129, p32):
        lib.gp_sgpr_destroy(pl)
