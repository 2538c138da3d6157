"""The sparse per-source posterior on the GPU (SGPRSS.predict_s_sparse, SgprWindowBatch.predict_s_sparse,
fit_windows_batched(predict="sparse")): one window against the float64 restatement (tests/sparse_source_ref.py) at every
tile shape the fused kernel takes, its identities with predict_f, bit-for-bit repeatability, the batched and ragged forms
against the one-window call, argument checks and a float32 plan."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from sparse_source_ref import problem, sparse_source  # noqa: E402

FS = 16000.


def _kern(d):
    from gpitch_amd import kernels as K
    from gpitch_amd.matern12_spectral_mixture import Matern12sm, MercerMatern12sm
    t = d["type"]
    e, f = np.array(d["energy"]), np.array(d["frequency"])
    if t == "mercer_matern12sm":
        return MercerMatern12sm(1, energy=e, frequency=f, variance=d["variance"], lengthscales=d["lengthscales"])
    if t == "matern12sm":
        return Matern12sm(1, energy=e, frequency=f, variance=d["variance"], lengthscales=d["lengthscales"])
    if t == "matern32sm":
        return K.Matern32sm(1, len(f), lengthscales=d["lengthscales"], variances=e, frequencies=f)
    if t == "mercer_matern52sm":
        k52 = K.Matern52(1, variance=d["variance"] / 0.2, lengthscales=d["lengthscales"])
        kc = K.MercerCosMix(1, energy=e, frequency=f, variance=0.2)
        k52.variance.fixed = True
        kc.variance.fixed = True
        return K.Prod(k52, kc)
    return {"matern32": K.Matern32, "matern12": K.Matern12}[t](1, variance=d["variance"], lengthscales=d["lengthscales"])


def _model(X, Y, Z, kdicts, noise, handle, float_type=None, mean_function=None):
    from gpitch_amd.sgpr_ss import SGPRSS
    kw = {} if mean_function is None else {"mean_function": mean_function}
    m = SGPRSS(X, Y, np.sum([_kern(d) for d in kdicts]), Z, handle=handle, float_type=float_type, **kw)
    m.likelihood.variance = noise
    return m


def _close(got, ref, rel, floor=1e-3):
    np.testing.assert_allclose(got, ref, rtol=0, atol=rel * max(np.abs(ref).max(), floor))


def _check_against_restatement(m, Xs, X, Y, Z, kl, noise, rel=1e-8):
    sm, sv = m.predict_s_sparse(Xs)
    rm, rv = sparse_source(Xs, X, Y, Z, kl, noise)
    assert len(sm) == len(sv) == len(kl)
    for p in range(len(kl)):
        assert sm[p].shape == rm[p].shape and sv[p].shape == rv[p].shape
        _close(sm[p], rm[p], rel)
        _close(sv[p], rv[p], rel)
    return sm, sv


# M below one MFMA tile; M no multiple of 16 / of 64; the 256 / 272 change of factorisation route; M above 256 (32-frame
# tiles); frame-tile tails everywhere
@pytest.mark.parametrize("N,M,P,n", [(200, 12, 1, 37), (1500, 50, 3, 215), (3000, 130, 5, 429), (600, 256, 2, 65),
                                      (700, 272, 2, 100), (1100, 512, 2, 100)])
def test_one_window_matches_restatement(gp_handle, N, M, P, n):
    X, Y, Z, kl = problem(N, M, P, N + M)
    Z = Z + 0.3 / FS
    m = _model(X, Y, Z, kl, 0.2, gp_handle)
    Xs = np.linspace(X.min(), X.max(), n).reshape(-1, 1) + 1e-5
    _check_against_restatement(m, Xs, X, Y, Z, kl, 0.2)
    m._destroy()


def _mixed_kernels():
    e20 = 1. / np.arange(1., 21.)
    return [
        {"type": "mercer_matern12sm", "variance": 1.1, "lengthscales": 0.05, "energy": [1.0], "frequency": [220.]},
        {"type": "mercer_matern12sm", "variance": 0.9, "lengthscales": 0.07, "energy": list(e20 / e20.sum()),
         "frequency": [110. * q for q in range(1, 21)]},
        {"type": "matern12sm", "variance": 0.9, "lengthscales": 0.05, "energy": [0.7, 0.3], "frequency": [277., 554.]},
        {"type": "matern32sm", "variance": 1.0, "lengthscales": 0.02, "energy": [0.12, 0.05, 0.03],
         "frequency": [330., 660., 990.]},
        {"type": "mercer_matern52sm", "variance": 0.5, "lengthscales": 0.01, "energy": [0.5, 0.3, 0.2],
         "frequency": [165., 330., 495.]},
        {"type": "matern32", "variance": 0.4, "lengthscales": 0.03, "energy": [], "frequency": []},
    ]


def test_mixed_kernel_sum_matches_restatement(gp_handle):
    X, Y, Z, _ = problem(900, 70, 2, 4)
    Z = Z + 0.3 / FS
    kl = _mixed_kernels()
    m = _model(X, Y, Z, kl, 0.25, gp_handle)
    kl = [k.oracle_dict() for k in m.kern.kern_list]          # what the model holds, in the oracle's format
    Xs = np.linspace(X.min(), X.max(), 131).reshape(-1, 1) + 1e-5
    _check_against_restatement(m, Xs, X, Y, Z, kl, 0.25)
    m._destroy()


def test_more_new_frames_than_the_plan_holds(gp_handle):
    N = 400
    X, Y, Z, kl = problem(N, 30, 2, 9)
    m = _model(X, Y, Z, kl, 0.2, gp_handle)
    Xs = np.linspace(X.min() - 0.002, X.max() + 0.002, 2 * N + 3).reshape(-1, 1)
    _check_against_restatement(m, Xs, X, Y, Z, kl, 0.2)
    m._destroy()


# ---- identities: two routes to one quantity (1e-9 of the largest magnitude) -------------------------------------------
def test_sources_add_up_to_predict_f(gp_handle):
    X, Y, Z, kl = problem(1500, 50, 3, 7)
    m = _model(X, Y, Z, kl, 0.2, gp_handle)
    Xs = X[::7] + 1e-5
    sm, _ = m.predict_s_sparse(Xs)
    fm, _ = m.predict_f(Xs)
    _close(sum(sm), fm, 1e-9)
    m._destroy()
    X, Y, Z, kl = problem(200, 12, 1, 3)
    m = _model(X, Y, Z, kl, 0.2, gp_handle)
    Xs = X[::2] + 1e-5
    sm, sv = m.predict_s_sparse(Xs)
    fm, fv = m.predict_f(Xs)
    _close(sm[0], fm, 1e-9)
    _close(sv[0], fv, 1e-9)
    m._destroy()


def test_mean_function_stays_out_of_the_sources(gp_handle):
    from gpitch_amd.mean_functions import Constant
    X, Y, Z, kl = problem(500, 20, 2, 11)
    m = _model(X, Y + 0.7, Z, kl, 0.2, gp_handle, mean_function=Constant(0.7))
    Xs = X[::5] + 1e-5
    sm, _ = m.predict_s_sparse(Xs)
    fm, _ = m.predict_f(Xs)
    _close(sum(sm) + 0.7, fm, 1e-9)
    rm, _ = sparse_source(Xs, X, Y, Z, kl, 0.2)
    for p in range(2):
        _close(sm[p], rm[p], 1e-8)
    m._destroy()


def test_two_output_columns(gp_handle):
    X, Y, Z, kl = problem(500, 20, 2, 12)
    Y2 = np.hstack([Y, 0.5 * Y[::-1]])
    m = _model(X, Y2, Z, kl, 0.2, gp_handle)
    Xs = X[::5] + 1e-5
    sm, sv = _check_against_restatement(m, Xs, X, Y2, Z, kl, 0.2)
    for p in range(2):
        assert sm[p].shape == (Xs.shape[0], 2)
        assert np.array_equal(sv[p][:, 0], sv[p][:, 1])
    m._destroy()


# ---- bit for bit ----------------------------------------------------------------------------------------------------
def test_repeatable_and_independent_of_the_other_frames(gp_handle):
    X, Y, Z, kl = problem(1500, 50, 3, 7)
    m = _model(X, Y, Z, kl, 0.2, gp_handle)
    Xs = X[::7] + 1e-5
    a = m.predict_s_sparse(Xs)
    b = m.predict_s_sparse(Xs)
    lo, hi = m.predict_s_sparse(Xs[:101]), m.predict_s_sparse(Xs[101:])
    for p in range(3):
        for q in range(2):
            assert np.array_equal(a[q][p], b[q][p])
            assert np.array_equal(a[q][p], np.vstack([lo[q][p], hi[q][p]]))
    m._destroy()


# ---- batched ----------------------------------------------------------------------------------------------------------
def _params_vector(noise, kl):
    v = [noise]
    for d in kl:
        v += [d["variance"], d["lengthscales"]] + list(d["energy"]) + list(d["frequency"])
    return np.array(v)


def _windows(counts, N, P, seed0):
    out = []
    for w, k in enumerate(counts):
        X, Y, _, kl = problem(N, k, P, seed0 + 17 * w)
        X = X + 0.125 * w
        for p, d in enumerate(kl):
            d["variance"] = 0.8 + 0.15 * ((w + p) % 4)
            d["lengthscales"] = 0.04 + 0.01 * ((2 * w + p) % 5)
        Z = X[np.linspace(0, N - 1, k).round().astype(int)] + 0.3 / FS
        out.append((X, Y * (1.0 + 0.1 * w), Z, kl))
    return out


@pytest.mark.parametrize("N,M,P,n", [(300, 16, 2, None), (2001, 64, 3, None), (500, 130, 3, 77)])
def test_batched_windows_match_one_window(gp_handle, N, M, P, n):
    from gpitch_amd.windows import SgprWindowBatch
    wins = _windows([M] * 5, N, P, seed0=3)
    tmpl = _model(*wins[0][:3], wins[0][3], 0.3, gp_handle)
    dev = SgprWindowBatch(tmpl, 5, N, M, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    noises = [0.2 + 0.05 * i for i in range(5)]
    pv = np.stack([_params_vector(nz, w[3]) for nz, w in zip(noises, wins)])
    xnews = None if n is None else [np.linspace(w[0].min(), w[0].max(), n).reshape(-1, 1) for w in wins]
    sm, sv = dev.predict_s_sparse(pv, xnews)
    assert sm.shape == sv.shape == (5, P, N if n is None else n)
    for i, w in enumerate(wins):
        one = _model(w[0], w[1], w[2], w[3], noises[i], gp_handle)
        ms, vs = one.predict_s_sparse(w[0] if xnews is None else xnews[i])
        for k in range(P):
            _close(sm[i, k], ms[k][:, 0], 1e-10, floor=1e-12)
            _close(sv[i, k], vs[k][:, 0], 1e-10, floor=1e-12)
        one._destroy()
    dev.close()
    tmpl._destroy()


def test_ragged_windows_match_their_own_size(gp_handle):
    """counts [64, 30, 47, 1, 64] on an M = 64 plan with the unused rows of Z set to NaN: each slot is the one-window model on
    Z[:k] (1e-10 of the largest magnitude: what test_gpu_windows_ragged.py holds predictions to), and no NaN comes out"""
    from gpitch_amd.windows import SgprWindowBatch
    counts, N, P = [64, 30, 47, 1, 64], 700, 2
    wins = _windows(counts, N, P, seed0=5)
    tmpl = _model(*wins[0][:3], wins[0][3], 0.3, gp_handle)
    dev = SgprWindowBatch(tmpl, 5, N, 64, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    zpad = np.full((5, 64), np.nan)
    for i, w in enumerate(wins):
        zpad[i, :counts[i]] = w[2].reshape(-1)
    dev.Z.copy_(gp_handle.torch.as_tensor(zpad))
    noises = [0.2 + 0.05 * i for i in range(5)]
    pv = np.stack([_params_vector(nz, w[3]) for nz, w in zip(noises, wins)])
    sm, sv = dev.predict_s_sparse(pv)
    assert np.isfinite(sm).all() and np.isfinite(sv).all()
    for i, w in enumerate(wins):
        one = _model(w[0], w[1], w[2], w[3], noises[i], gp_handle)
        ms, vs = one.predict_s_sparse(w[0])
        for k in range(P):
            _close(sm[i, k], ms[k][:, 0], 1e-10, floor=1e-12)
            _close(sv[i, k], vs[k][:, 0], 1e-10, floor=1e-12)
        one._destroy()
    dev.close()
    tmpl._destroy()


def test_fit_windows_batched_sparse(gp_handle):
    from gpitch_amd.windows import fit_windows_batched, merge_sources
    N, M = 301, 16
    wins = _windows([M] * 6, N, 2, seed0=21)
    data = [(w[0], w[1], w[2]) for w in wins]

    def make(handle):
        return _model(wins[0][0], wins[0][1], wins[0][2], wins[0][3], 1.0, handle)

    res = fit_windows_batched(make, data, maxiter=3, batch=6, predict="sparse")
    ref = fit_windows_batched(make, data, maxiter=3, batch=6, predict=True)
    for i, w in enumerate(wins):
        r = res[i]
        assert np.array_equal(r["mean"], ref[i]["mean"]) and np.array_equal(r["var"], ref[i]["var"])
        one = make(gp_handle)
        for prm, v in zip(one._param_list(), r["params"]):
            prm.value = np.array([v])
        one.X, one.Y, one.Z = w[0], w[1], w[2]
        ms, vs = one.predict_s_sparse(w[0])
        for k in range(2):
            assert r["smean"][k].shape == (N, 1)
            _close(r["smean"][k], ms[k], 1e-9, floor=1e-12)
            _close(r["svar"][k], vs[k], 1e-9, floor=1e-12)
        one._destroy()
    merged = merge_sources(res, N, (len(wins) + 1) * (N // 2) + 1)
    assert len(merged) == 2 and all(np.isfinite(m).all() and np.isfinite(v).all() for m, v in merged)


# ---- arguments: none of these launches anything -------------------------------------------------------------------------
def test_arguments(gp_handle):
    from gpitch_amd import _lib
    from gpitch_amd.sgpr_ss import SGPRSS
    from gpitch_amd.windows import SgprWindowBatch
    h, lib = gp_handle, gp_handle.lib
    X, Y, Z, kl = problem(100, 10, 2, 1)
    m = _model(X, Y, Z, kl, 0.2, h)
    m._compile()
    m._pack()
    xs, out = h.to_device(X.reshape(-1)), h.empty(2, 100)
    good = [m._plan, m._params.data_ptr(), m._Xd.data_ptr(), m._Yd.data_ptr(), 100, m._Zd.data_ptr(), xs.data_ptr(), 100,
            out.data_ptr(), out.data_ptr()]
    for pos in (1, 2, 3, 5, 6, 8, 9):       # null pointers
        a = list(good)
        a[pos] = None
        assert lib.gp_sgpr_predict_source_sparse(*a) == _lib.GP_ERR_BAD_ARG
    a = list(good)
    a[7] = 0                                # n < 1
    assert lib.gp_sgpr_predict_source_sparse(*a) == _lib.GP_ERR_BAD_ARG
    a = list(good)
    a[4] = 101                              # more training frames than the plan was made for
    assert lib.gp_sgpr_predict_source_sparse(*a) == _lib.GP_ERR_BAD_ARG
    dev = SgprWindowBatch(m, 2, 100, 10, handle=h)
    bgood = [dev.plan, dev.params.data_ptr(), dev.X.data_ptr(), dev.Y.data_ptr(), dev.Z.data_ptr(), dev.X.data_ptr(), 100, 2,
             out.data_ptr(), out.data_ptr()]
    for pos, bad in ((5, None), (8, None), (6, 0), (7, 0), (7, 3)):     # null pointers, n < 1, count out of range
        a = list(bgood)
        a[pos] = bad
        assert lib.gp_sgprb_predict_source_sparse(*a) == _lib.GP_ERR_BAD_ARG
    dev.close()
    m._destroy()
    # M above the limit: refused before the workspace is even looked at
    P = 1
    i32 = C.c_int32 * P
    keep = (i32(_lib.KERN_MATERN32), i32(0))
    cfg = _lib.SgprConfig(P, 100, 1040, keep[0], keep[1], 1e-6, 0)
    plan = C.c_void_p()
    h.check(lib.gp_sgpr_create(h.h, C.byref(cfg), C.byref(plan)))
    a = list(good)
    a[0] = plan
    assert lib.gp_sgpr_predict_source_sparse(*a) == _lib.GP_ERR_UNSUPPORTED
    lib.gp_sgpr_destroy(plan)
    sharded = SGPRSS(X, Y, np.sum([_kern(d) for d in kl]), Z, handle=h, shard=(0, 2))
    with pytest.raises(NotImplementedError):
        sharded.predict_s_sparse(X)


# ---- float32 plan -----------------------------------------------------------------------------------------------------
def test_float32_plan(gp_handle):
    """the state (W, WB, c) comes from the float32 forward pass, the fused kernel's arithmetic is float64: held to the bound
    tests/test_gpu_f32.py states for SGPRSS predict_f on a float32 plan, 1e-4 of the largest magnitude (measured here: means
    3.4e-7, variances 4.3e-9)"""
    X, Y, Z, kl = problem(2001, 64, 3, 8)
    Xs = X[::3] + 1e-5
    m64 = _model(X, Y, Z, kl, 0.2, gp_handle)
    m32 = _model(X, Y, Z, kl, 0.2, gp_handle, float_type=np.float32)
    a, b = m64.predict_s_sparse(Xs), m32.predict_s_sparse(Xs)
    for p in range(3):
        for q in range(2):
            dev = np.abs(a[q][p] - b[q][p]).max() / np.abs(a[q][p]).max()
            print("float32 plan: source %d %s relative difference %.3e" % (p, "mean" if q == 0 else "var", dev))
            assert dev <= 1e-4
    m64._destroy()
    m32._destroy()
