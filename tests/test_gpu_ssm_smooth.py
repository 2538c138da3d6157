"""The state-space smoother on the GPU (SGPRSS.predict_s_ssm / exact_log_likelihood, SgprWindowBatch.predict_s_ssm,
fit_windows_batched(predict="ssm"), csrc/ssm_smooth.hip): every case of tests/ssm_smooth_ref.py against the numpy restatement
(1e-8 of the largest magnitude), the device's own predict_s under the measured gap of the reference's 1e-12, the batched and
chunked forms bit for bit against the one-window call, a float32 plan, determinism, and the argument checks of the ABI."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ssm_smooth_ref as R  # noqa: E402

_REF = {}


def _ref(i):
    """the restatement of case i, computed once"""
    if i not in _REF:
        X, Y, Xn, kl, nz = R.case(i)
        _REF[i] = R.smooth(X, Y, Xn, kl, nz)
    return _REF[i]


def _close(got, ref, rel=1e-8, floor=1e-3):
    err, bar = np.abs(np.asarray(got) - np.asarray(ref)).max(), rel * max(np.abs(ref).max(), floor)
    print("    largest difference %.3e (bar %.3e)" % (err, bar))
    assert err <= bar


def _stack(lst):
    return np.array([a[:, 0] for a in lst])


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=[R.case_id(i) for i in range(len(R.CASES))])
def test_matches_restatement(gp_handle, i):
    X, Y, Xn, kl, nz = R.case(i)
    m = R.model(X, Y, kl, nz, gp_handle)
    sm, sv = m.predict_s_ssm(Xn)
    ll = m.exact_log_likelihood()
    rm, rv, rl = _ref(i)
    assert len(sm) == len(sv) == len(kl) and sm[0].shape == sv[0].shape == (Xn.shape[0], 1)
    _close(_stack(sm), rm)
    _close(_stack(sv), rv)
    _close([ll], [rl])
    m._destroy()


def test_against_the_devices_predict_s(gp_handle):
    """N = 300, P = 3: predict_s factorises the N x N matrix of the reference's kernels (1e-12 under the root) and starts its
    variance from the sum kernel's Kdiag; the bars are ten times the gap measured on the CPU between the restatement and
    the oracle's kernels at this shape (ssm_smooth_ref.ORACLE_GAP)"""
    i = [R.case_id(k) for k in range(len(R.CASES))].index("d60-N300-same-s0.01")
    X, Y, Xn, kl, nz = R.case(i)
    gm, gv, _ = R.ORACLE_GAP[R.case_id(i)]
    m = R.model(X, Y, kl, nz, gp_handle)
    sm, sv = m.predict_s_ssm(Xn)
    em, ev = m.predict_s(Xn)
    shift = sum(R.kdiag(k) for k in kl)
    dm = max(np.abs(sm[p] - em[p]).max() for p in range(3))
    dv = max(np.abs(sv[p] + (shift - R.kdiag(kl[p])) - ev[p]).max() for p in range(3))
    print("    predict_s against predict_s_ssm: mean %.3e (bar %.1e), variance %.3e (bar %.1e)" % (dm, 10 * gm, dv, 10 * gv))
    assert dm <= 10 * gm and dv <= 10 * gv
    m._destroy()


# ---- batched ------------------------------------------------------------------------------------------------------------------
def _params_vector(noise, kl):
    v = [noise]
    for d in kl:
        v += [d["variance"], d["lengthscales"]] + list(d["energy"]) + list(d["frequency"])
    return np.array(v)


def _three_windows():
    """three windows of N = 37 frames on one kernel structure (d = 63, all three families) with their own data and parameters"""
    kl0 = R.kernels(63)
    wins = []
    for w in range(3):
        X, Y, _, _ = R.problem(37, 1, 2, 70 + w)
        kl = [dict(k) for k in kl0]
        for p, k in enumerate(kl):
            k["variance"] = k["variance"] * (1.0 + 0.2 * w)
            k["lengthscales"] = k["lengthscales"] * (1.0 + 0.1 * ((w + p) % 3))
        wins.append((X + 0.01 * w, Y * (1.0 + 0.3 * w), kl, 0.05 + 0.1 * w))
    return wins


@pytest.mark.parametrize("xnew", ["frames", "mixed"])
def test_batched_windows_are_the_one_window_call(gp_handle, monkeypatch, xnew):
    from gpitch_amd import sgpr_ss
    from gpitch_amd.windows import SgprWindowBatch
    wins = _three_windows()
    tmpl = R.model(wins[0][0], wins[0][1], wins[0][2], wins[0][3], gp_handle)
    dev = SgprWindowBatch(tmpl, 3, 37, 4, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[0][:4] for w in wins])
    pv = np.stack([_params_vector(w[3], w[2]) for w in wins])
    xnews = None if xnew == "frames" else [R.new_frames(w[0], 7 + q) for q, w in enumerate(wins)]
    sm, sv, ll = dev.predict_s_ssm(pv, xnews, return_loglik=True)
    ones = []
    for q, w in enumerate(wins):
        one = R.model(w[0], w[1], w[2], w[3], gp_handle)
        ms, vs = one.predict_s_ssm(w[0] if xnews is None else xnews[q])
        ones.append((_stack(ms), _stack(vs), one.exact_log_likelihood()))
        one._destroy()
        assert np.array_equal(sm[q], ones[q][0]) and np.array_equal(sv[q], ones[q][1])
        if xnews is None:                             # the same steps as the forward walk alone: the same bits
            assert ll[q] == ones[q][2]
        else:                                         # unobserved steps split the transitions: rounding only
            assert abs(ll[q] - ones[q][2]) <= 1e-12 * abs(ones[q][2])
    # a chunk budget of one window per library call changes no bit
    per = int(gp_handle.lib.gp_ssm_smooth_workspace_bytes(63, 37 + 50, 4, 1))
    monkeypatch.setattr(sgpr_ss, "MAX_SSM_BYTES", per)
    sm1, sv1 = dev.predict_s_ssm(pv, xnews)
    assert np.array_equal(sm1, sm) and np.array_equal(sv1, sv)
    # a window alone in its launch
    sm2, sv2 = dev.predict_s_ssm(pv, xnews, chunk=2)
    assert np.array_equal(sm2, sm) and np.array_equal(sv2, sv)
    dev.close()
    tmpl._destroy()


def test_two_calls_are_bit_identical_and_float32_plans_give_the_same_bits(gp_handle):
    i = [R.case_id(k) for k in range(len(R.CASES))].index("d65-N300-mixed-s0.1")
    X, Y, Xn, kl, nz = R.case(i)
    m = R.model(X, Y, kl, nz, gp_handle)
    a, b = m.predict_s_ssm(Xn), m.predict_s_ssm(Xn)
    m32 = R.model(X, Y, kl, nz, gp_handle, float_type=np.float32)
    c = m32.predict_s_ssm(Xn)
    for q in range(2):
        assert np.array_equal(_stack(a[q]), _stack(b[q])) and np.array_equal(_stack(a[q]), _stack(c[q]))
    assert m.exact_log_likelihood() == m.exact_log_likelihood() == m32.exact_log_likelihood()
    m._destroy()
    m32._destroy()


def test_two_output_columns_and_mean_function(gp_handle):
    from gpitch_amd.mean_functions import Constant
    X, Y, Xn, kl, nz = R.case(2)
    Y2 = np.hstack([Y, 0.5 * Y[::-1]])
    m = R.model(X, Y2 + 0.7, kl, nz, gp_handle, mean_function=Constant(0.7))
    sm, sv = m.predict_s_ssm(Xn)
    r0, r1 = R.smooth(X, Y2[:, 0], Xn, kl, nz), R.smooth(X, Y2[:, 1], Xn, kl, nz)
    assert sm[0].shape == sv[0].shape == (Xn.shape[0], 2) and np.array_equal(sv[0][:, 0], sv[0][:, 1])
    _close(sm[0][:, 0], r0[0][0])
    _close(sm[0][:, 1], r1[0][0])
    _close(sv[0][:, 0], r0[1][0])
    _close([m.exact_log_likelihood()], [r0[2] + r1[2]])
    m._destroy()


def _fit_windows(N, M):
    wins = []
    for w in range(4):
        X, Y, Z, _ = R.problem(N, M, 2, 90 + w)
        wins.append((X + 0.004 * w, Y, Z + 0.004 * w + 0.3 / R.FS))
    return wins


def test_fit_windows_batched_ssm(gp_handle):
    from gpitch_amd.windows import fit_windows_batched, merge_sources
    N, M = 128, 16
    kl = R.kernels(4) + [R._mix("mercer_matern12sm", 1, 1, 0.006)]
    wins = _fit_windows(N, M)

    def make(handle):
        return R.model(wins[0][0], wins[0][1], kl, 1.0, handle, Z=wins[0][2])

    res = fit_windows_batched(make, wins, maxiter=2, batch=4, predict="ssm")
    for i, w in enumerate(wins):
        one = make(gp_handle)
        for prm, v in zip(one._param_list(), res[i]["params"]):
            prm.value = np.array([v])
        one.X, one.Y, one.Z = w
        ms, vs = one.predict_s_ssm(w[0])
        for k in range(2):
            assert res[i]["smean"][k].shape == (N, 1)
            assert np.array_equal(res[i]["smean"][k], ms[k]) and np.array_equal(res[i]["svar"][k], vs[k])
        one._destroy()
    # merge_sources overlap-adds windows of an odd number of frames (window_overlap: half = (ws - 1) / 2), so it takes the
    # "smean" / "svar" of the same fit at N = 129
    N = 129
    wins = _fit_windows(N, M)
    res = fit_windows_batched(make, wins, maxiter=1, batch=4, predict="ssm")
    merged = merge_sources(res, N, (len(wins) + 1) * (N // 2) + 1)
    assert len(merged) == 2 and all(m.shape == (321, 1) and np.isfinite(m).all() and np.isfinite(v).all() for m, v in merged)


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
    from gpitch_amd.sgpr_ss import ssm_timeline
    h, lib = gp_handle, gp_handle.lib
    X, Y, Xn, kl, nz = R.case(2)                      # d = 4, N = 37, 50 new frames
    N, n, d, P = 37, 50, 4, 1
    order, ostep, steps = ssm_timeline(X, Xn)
    plan, keep = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 2)], N)
    par = h.to_device(_params_vector(nz, kl))
    xd, yd, xs = h.to_device(X.reshape(-1)), h.to_device(Y.reshape(-1)), h.to_device(Xn.reshape(-1))
    sentinel = -77.0
    mean, var, ll = h.zeros(P, n) + sentinel, h.zeros(P, n) + sentinel, h.zeros(1) + sentinel
    need = int(lib.gp_ssm_smooth_workspace_bytes(d, steps, P, 1))
    ws = h.workspace(need)

    def call(plan_=plan, ws_bytes=need, **kw):
        a = dict(params=par.data_ptr(), X=xd.data_ptr(), Y=yd.data_ptr(), Xnew=xs.data_ptr(), order=order.ctypes.data,
                 ostep=ostep.ctypes.data, mean=mean.data_ptr(), var=var.data_ptr(), ll=ll.data_ptr(), ws=ws.data_ptr())
        a.update(kw)
        st = lib.gp_sgpr_predict_source_ssm(plan_, a["params"], a["X"], a["Y"], N, a["Xnew"], n, a["order"], a["ostep"], steps,
                                            a["mean"], a["var"], a["ll"], a["ws"], ws_bytes)
        msg = lib.gp_last_error(h.h)
        return st, (msg.decode() if msg else "")

    def untouched():
        h.sync()
        return bool((mean == sentinel).all()) and bool((var == sentinel).all()) and bool((ll == sentinel).all())

    for name in ("params", "X", "Y", "Xnew", "order", "ostep", "mean", "var", "ll", "ws"):        # a null pointer
        st, msg = call(**{name: None})
        assert st == _lib.GP_ERR_BAD_ARG and "null" in msg, name
    st, msg = call(ws_bytes=need - 256)                                                             # a short workspace
    assert st == _lib.GP_ERR_BAD_ARG and "workspace" in msg and "steps" in msg
    bad = order.copy()
    bad[3] = bad[4]                                                                                 # not a permutation
    st, msg = call(order=bad.ctypes.data)
    assert st == _lib.GP_ERR_BAD_ARG and "permutation" in msg
    bad = order.copy()
    bad[bad < N] = np.roll(bad[bad < N], 1)                                                         # (a permutation still: fine)
    bad[np.flatnonzero(bad < N)[0]] = N + n
    st, msg = call(order=bad.ctypes.data)
    assert st == _lib.GP_ERR_BAD_ARG and "permutation" in msg
    for v in (-1, steps):                                                                           # out_step out of range
        bad = ostep.copy()
        bad[7] = v
        st, msg = call(ostep=bad.ctypes.data)
        assert st == _lib.GP_ERR_BAD_ARG and "out_step" in msg
    assert untouched()
    p130, keep130 = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 32), (_lib.KERN_MERCER_MATERN12SM, 32), (_lib.KERN_MATERN12SM, 1)], N)
    st, msg = call(plan_=p130)                                                                      # d = 130
    assert st == _lib.GP_ERR_UNSUPPORTED and "d" in msg and "128" in msg
    p32, keep32 = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 2), (_lib.KERN_MATERN32, 0)], N)
    st, msg = call(plan_=p32)                                                                       # a Matern32 in the sum
    assert st == _lib.GP_ERR_UNSUPPORTED and "Matern-1/2" in msg
    p33, keep33 = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 2)], N)
    assert untouched()
    # the measured workspace is accepted, and is the smallest that is: one 256-byte unit less was refused above
    st, msg = call()
    assert st == _lib.GP_OK, msg
    rm, rv, rl = _ref(2)
    _close(mean.cpu().numpy(), rm)
    _close(var.cpu().numpy(), rv)
    for pl in (plan, p130, p32, p33):
        lib.gp_sgpr_destroy(pl)
    # the dry run (host only): whole 256-byte units; 0 outside 1 <= P <= d <= 128, steps >= 1
    for dd, ss, pp, cc in ((1, 1, 1, 1), (4, 87, 1, 1), (63, 87, 4, 3), (128, 350, 2, 1)):
        assert int(lib.gp_ssm_smooth_workspace_bytes(dd, ss, pp, cc)) % 256 == 0
    assert lib.gp_ssm_smooth_workspace_bytes(129, 10, 1, 1) == 0 and lib.gp_ssm_smooth_workspace_bytes(4, 0, 1, 1) == 0
