"""The simulation smoother on the GPU (SGPRSS.sample_s_ssm, SgprWindowBatch.sample_s_ssm, csrc/ssm_smooth.hip): every case of
tests/ssm_smooth_ref.py against the numpy restatement of the map on explicit normals (1e-8 of the largest magnitude), zero
normals against the device's own predict_s_ssm, the linear part's A A^T against the dense joint posterior covariance, the
bit-identities (calls, S, batches, chunks, seeds), two output columns and the argument checks of the ABI."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import ssm_sample_ref as SR  # noqa: E402
import ssm_smooth_ref as R  # noqa: E402

IDS = [R.case_id(i) for i in range(len(R.CASES))]


def _close(got, ref, rel=1e-8, floor=1e-3):
    err, bar = np.abs(np.asarray(got) - np.asarray(ref)).max(), rel * max(np.abs(ref).max(), floor)
    print("    largest difference %.3e (bar %.3e)" % (err, bar))
    assert err <= bar


def _stack(lst):
    """[P] of (S, n, 1) -> (P, S, n)"""
    return np.array([a[:, :, 0] for a in lst])


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_matches_restatement(gp_handle, i):
    X, Y, Xn, kl, nz = R.case(i)
    gn = SR.gains(X, Xn, kl, nz)
    ex, ey = SR.random_eps(gn, 3, 300 + i)
    m = R.model(X, Y, kl, nz, gp_handle)
    got = m.sample_s_ssm(Xn, 3, eps=(ex, ey))
    assert len(got) == len(kl) and got[0].shape == (3, Xn.shape[0], 1)
    _close(_stack(got), SR.draw(gn, Y, ex, ey))
    m._destroy()


@pytest.mark.parametrize("name", ["d1-N37-mixed", "d60-N300-same", "d65-N300-mixed", "d128-N37-mixed", "d65-N37-dup"])
def test_zero_normals_give_predict_s_ssm_mean(gp_handle, name):
    X, Y, Xn, kl, nz = R.case(SR.case_index(name))
    m = R.model(X, Y, kl, nz, gp_handle)
    from gpitch_amd import ssm_sample_eps_shapes, ssm_timeline
    shx, shy = ssm_sample_eps_shapes(m.kern, ssm_timeline(X, Xn)[2], X.shape[0], 1)
    got = m.sample_s_ssm(Xn, 1, eps=(np.zeros(shx), np.zeros(shy)))
    mean = m.predict_s_ssm(Xn)[0]
    _close(_stack(got)[:, 0], np.array([a[:, 0] for a in mean]))
    m._destroy()


def test_linear_part_has_the_joint_posterior_covariance(gp_handle):
    """d = 4, N = 2, 47 steps: the 4 * 47 + 2 = 190 unit normals as the draws of ONE call"""
    X, Y, Xn, kl, nz = R.case(SR.case_index("d4-N2-mixed"))
    gn = SR.gains(X, Xn, kl, nz)
    T, d, N = gn["steps"], gn["d"], gn["N"]
    K = T * d + N
    assert K == 190
    E = np.eye(K)
    m = R.model(X, Y, kl, nz, gp_handle)
    unit = _stack(m.sample_s_ssm(Xn, K, eps=(E[:, :T * d].reshape(K, T, d), E[:, T * d:])))
    zero = _stack(m.sample_s_ssm(Xn, 1, eps=(np.zeros((1, T, d)), np.zeros((1, N)))))
    A = np.transpose(unit - zero, (0, 2, 1)).reshape(-1, K)
    _close(A.dot(A.T), SR.dense_joint(X, Y, Xn, kl, nz)[1])
    m._destroy()


def test_calls_draws_and_seeds_are_bit_identical(gp_handle):
    X, Y, Xn, kl, nz = R.case(SR.case_index("d65-N300-mixed"))
    gn = SR.gains(X, Xn, kl, nz)
    ex, ey = SR.random_eps(gn, 3, 11)
    m = R.model(X, Y, kl, nz, gp_handle)
    a, b = _stack(m.sample_s_ssm(Xn, 3, eps=(ex, ey))), _stack(m.sample_s_ssm(Xn, 3, eps=(ex, ey)))
    assert np.array_equal(a, b)
    one = _stack(m.sample_s_ssm(Xn, 1, eps=(ex[2:3], ey[2:3])))            # a draw's bits do not depend on S
    assert np.array_equal(one[:, 0], a[:, 2])
    s1, s2, s3 = (_stack(m.sample_s_ssm(Xn, 2, seed=s)) for s in (5, 5, 6))
    assert np.array_equal(s1, s2) and not np.array_equal(s1, s3) and not np.array_equal(s1[:, 0], s1[:, 1])
    assert np.isfinite(s1).all()
    m._destroy()


def test_two_output_columns(gp_handle):
    X, Y, Xn, kl, nz = R.case(2)
    Y2 = np.hstack([Y, 0.5 * Y[::-1]])
    gn = SR.gains(X, Xn, kl, nz)
    ex, ey = np.stack([SR.random_eps(gn, 2, 21)[0], SR.random_eps(gn, 2, 22)[0]]), np.stack(
        [SR.random_eps(gn, 2, 21)[1], SR.random_eps(gn, 2, 22)[1]])
    m = R.model(X, Y2, kl, nz, gp_handle)
    got = m.sample_s_ssm(Xn, 2, eps=(ex, ey))
    assert len(got) == 1 and got[0].shape == (2, Xn.shape[0], 2)
    for c in range(2):
        _close(got[0][:, :, c], SR.draw(gn, Y2[:, c], ex[c], ey[c])[0])
    seeded = m.sample_s_ssm(Xn, 1, seed=3)[0]
    assert not np.array_equal(seeded[:, :, 0], seeded[:, :, 1])            # independent normals per column
    m._destroy()


# ---- batched ------------------------------------------------------------------------------------------------------------------
def _params_vector(noise, kl):
    v = [noise]
    for d in kl:
        v += [d["variance"], d["lengthscales"]] + list(d["energy"]) + list(d["frequency"])
    return np.array(v)


def _three_windows():
    """three windows of N = 37 frames on one kernel structure (d = 63, all three families) with their own data, parameters and
    50 new frames; the windows' timelines differ in length (79, 71 and 75 steps: more of the second's and third's new frames
    lie on training frames), so each is padded differently inside a batch"""
    kl0 = R.kernels(63)
    wins = []
    for w in range(3):
        X, Y, _, _ = R.problem(37, 1, 2, 70 + w)
        kl = [dict(k) for k in kl0]
        for p, k in enumerate(kl):
            k["variance"] = k["variance"] * (1.0 + 0.2 * w)
            k["lengthscales"] = k["lengthscales"] * (1.0 + 0.1 * ((w + p) % 3))
        X = X + 0.01 * w
        xn = R.new_frames(X, 7 + w)
        fresh = np.flatnonzero(~np.isin(xn, X.reshape(-1)))
        xn[fresh[:[0, 10, 5][w]]] = X[:[0, 10, 5][w], 0]
        wins.append((X, Y * (1.0 + 0.3 * w), kl, 0.05 + 0.1 * w, xn))
    return wins


def test_batched_windows_are_the_one_window_call(gp_handle):
    from gpitch_amd import ssm_timeline
    from gpitch_amd.windows import SgprWindowBatch
    wins = _three_windows()
    steps = [ssm_timeline(w[0], w[4])[2] for w in wins]
    smax, S = max(steps), 2
    assert steps == [79, 71, 75]
    tmpl = R.model(wins[0][0], wins[0][1], wins[0][2], wins[0][3], gp_handle)
    dev = SgprWindowBatch(tmpl, 3, 37, 4, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[0][:4] for w in wins])
    pv = np.stack([_params_vector(w[3], w[2]) for w in wins])
    xnews = [w[4] for w in wins]
    rng = np.random.RandomState(31)
    ex, ey = rng.randn(3, S, smax, 63), rng.randn(3, S, 37)
    got = dev.sample_s_ssm(pv, xnews, S, eps=(ex, ey))
    assert got.shape == (3, 4, S, 50)
    for q, w in enumerate(wins):                       # a window alone, on its own (shorter) timeline
        one = R.model(w[0], w[1], w[2], w[3], gp_handle)
        alone = _stack(one.sample_s_ssm(w[4], S, eps=(ex[q, :, :steps[q]], ey[q])))
        one._destroy()
        assert np.array_equal(got[q], alone)
        gn = SR.gains(w[0], w[4], w[2], w[3])
        _close(got[q], SR.draw(gn, w[1], ex[q, :, :steps[q]], ey[q]))
    for chunk in (1, 2):                               # windows per library call: no bit changes
        assert np.array_equal(dev.sample_s_ssm(pv, xnews, S, eps=(ex, ey), chunk=chunk), got)
    a, b, c = (dev.sample_s_ssm(pv, xnews, S, seed=9, chunk=ch) for ch in (None, None, 1))
    assert np.array_equal(a, b) and np.array_equal(a, c) and not np.array_equal(a[0], got[0])
    own = dev.sample_s_ssm(pv, None, 1, seed=9)        # at the windows' own frames
    assert own.shape == (3, 4, 1, 37) and np.isfinite(own).all()
    with pytest.raises(ValueError, match=r"eps must be \(eps_x, eps_y\) of shapes \[\(3, 2, %d, 63\), \(3, 2, 37\)\]" % smax):
        dev.sample_s_ssm(pv, xnews, S, eps=(ex[:, :, :-1], ey))
    with pytest.raises(ValueError, match="at least one sample"):
        dev.sample_s_ssm(pv, xnews, 0)
    dev.close()
    tmpl._destroy()


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
    N, n, d, P, S = 37, 50, 4, 1, 2
    order, ostep, steps = ssm_timeline(X, Xn)
    gn = SR.gains(X, Xn, kl, nz)
    ex_h, ey_h = SR.random_eps(gn, S, 41)
    plan, keep = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 2)], N)
    par = h.to_device(_params_vector(nz, kl))
    xd, yd, xs = h.to_device(X.reshape(-1)), h.to_device(Y.reshape(-1)), h.to_device(Xn.reshape(-1))
    ex, ey = h.to_device(ex_h), h.to_device(ey_h)
    sentinel = -77.0
    out = h.zeros(P, S, n) + sentinel
    need = int(lib.gp_ssm_sample_workspace_bytes(d, steps, P, S, 1))
    ws = h.workspace(need)

    def call(plan_=plan, ws_bytes=need, S_=S, **kw):
        a = dict(params=par.data_ptr(), X=xd.data_ptr(), Y=yd.data_ptr(), Xnew=xs.data_ptr(), order=order.ctypes.data,
                 ostep=ostep.ctypes.data, ex=ex.data_ptr(), ey=ey.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr())
        a.update(kw)
        st = lib.gp_sgpr_sample_source_ssm(plan_, a["params"], a["X"], a["Y"], N, a["Xnew"], n, a["order"], a["ostep"], steps,
                                           S_, a["ex"], a["ey"], a["out"], a["ws"], ws_bytes)
        msg = lib.gp_last_error(h.h)
        return st, (msg.decode() if msg else "")

    def untouched():
        h.sync()
        return bool((out == sentinel).all())

    for name in ("params", "X", "Y", "Xnew", "order", "ostep", "ex", "ey", "out", "ws"):            # a null pointer
        st, msg = call(**{name: None})
        assert st == _lib.GP_ERR_BAD_ARG and "null" in msg, name
    st, msg = call(S_=0)
    assert st == _lib.GP_ERR_BAD_ARG and "S >= 1" in msg
    st, msg = call(ws_bytes=need - 256)                                                             # a short workspace
    assert st == _lib.GP_ERR_BAD_ARG and "workspace" in msg and "gp_ssm_sample_workspace_bytes" in msg
    bad = order.copy()
    bad[3] = bad[4]                                                                                 # not a permutation
    st, msg = call(order=bad.ctypes.data)
    assert st == _lib.GP_ERR_BAD_ARG and "permutation" in msg
    for v in (-1, steps):                                                                           # out_step out of range
        bad = ostep.copy()
        bad[7] = v
        st, msg = call(ostep=bad.ctypes.data)
        assert st == _lib.GP_ERR_BAD_ARG and "out_step" in msg
    p130, keep130 = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 32), (_lib.KERN_MERCER_MATERN12SM, 32), (_lib.KERN_MATERN12SM, 1)], N)
    st, msg = call(plan_=p130)                                                                      # d = 130
    assert st == _lib.GP_ERR_UNSUPPORTED and "128" in msg
    p32, keep32 = _plan(h, [(_lib.KERN_MERCER_MATERN12SM, 2), (_lib.KERN_MATERN32, 0)], N)
    st, msg = call(plan_=p32)                                                                       # a Matern32 in the sum
    assert st == _lib.GP_ERR_UNSUPPORTED and "Matern-1/2" in msg
    assert untouched()
    # the measured workspace is accepted, and is the smallest that is: one 256-byte unit less was refused above
    st, msg = call()
    assert st == _lib.GP_OK, msg
    _close(out.cpu().numpy(), SR.draw(gn, Y, ex_h, ey_h))
    for pl in (plan, p130, p32):
        lib.gp_sgpr_destroy(pl)
