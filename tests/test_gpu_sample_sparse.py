"""Joint posterior draws of the SGPRSS sources on the GPU (SGPRSS.sample_s_sparse, SgprWindowBatch.sample_s_sparse,
gp_sgpr_sample_source_sparse, gp_sgprb_sample_source_sparse) against the float64 restatement of the map
(tests/sample_sparse_ref.py): identity eps (the linear part T, T T^T against the closed-form joint covariance, eps = 0
against predict_s_sparse), seeded random eps at every tile shape, a mixed kernel sum, bit-for-bit repeatability, two output
columns, the batched and ragged forms, the device generator, argument checks and a float32 plan.

The rule against the restatement is tests/test_gpu_sparse_source.py's: absolute error <= 1e-8 max(|ref|.max(), 1e-3)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import sample_sparse_ref as ref  # noqa: E402
from sparse_source_ref import problem  # noqa: E402
from test_gpu_sparse_source import _close, _kern, _model, _params_vector, _windows  # noqa: E402

FS = 16000.


def _random_eps(kl, n, M, S, seed):
    rng = np.random.RandomState(seed)
    return [rng.randn(*sh) for sh in ref.eps_shapes(kl, n, M, S)]


def _check(m, Xs, X, Y, Z, kl, noise, eps, rel=1e-8):
    got = m.sample_s_sparse(Xs, num_samples=eps[0].shape[0], eps=eps)
    want = ref.sample_sources(Xs, X, Y, Z, kl, noise, *eps)
    assert len(got) == len(kl)
    for p in range(len(kl)):
        assert got[p].shape == (eps[0].shape[0], np.asarray(Xs).reshape(-1).size, 1)
        err = np.abs(got[p][:, :, 0] - want[p]).max()
        print("source %d: |gpu - restatement| %.3e at |ref| %.3e" % (p, err, np.abs(want[p]).max()))
        _close(got[p][:, :, 0], want[p], rel)
    return got


# ---- 1. identity eps at the smallest shape: the mathematics ---------------------------------------------------------------
def test_identity_eps_pins_the_map(gp_handle):
    X, Y, Z, kl, noise, Xs = ref.smallest_problem(shuffle=True)
    n, M, P = 40, 12, 2
    ex, ez, eu = ref.identity_eps(kl, n, M)
    S = ex.shape[0]
    assert S == (40 + 12) * 8 + 24
    eps1 = [np.concatenate([e, np.zeros((1,) + e.shape[1:])]) for e in (ex, ez, eu)]      # the last draw: eps = 0
    m = _model(X, Y, Z, kl, noise, gp_handle)
    got = np.stack([g[:, :, 0] for g in m.sample_s_sparse(Xs, num_samples=S + 1, eps=eps1)])          # (P, S + 1, n)
    want = ref.sample_sources(Xs, X, Y, Z, kl, noise, *eps1)
    T = (got[:, :S] - got[:, S:]).transpose(0, 2, 1).reshape(P * n, S)
    Tr = (want[:, :S] - want[:, S:]).transpose(0, 2, 1).reshape(P * n, S)
    print("T: |gpu - restatement| %.3e at |T| %.3e" % (np.abs(T - Tr).max(), np.abs(Tr).max()))
    _close(T, Tr, 1e-8)
    cov, kd = ref.joint_cov(Xs, X, Y, Z, kl, noise)
    err = np.abs(T.dot(T.T) - cov).max()
    print("T T^T against the closed form: %.3e at max Kdiag %.3f" % (err, kd))
    assert err <= 1e-5 * kd
    sm, _ = m.predict_s_sparse(Xs)
    for p in range(P):
        _close(got[p, S], sm[p][:, 0], 1e-8)
    m._destroy()


# ---- 2. seeded random eps at every shape the kernels take -------------------------------------------------------------------
# M below one MFMA tile and S below 16; a plain middle; S tail past two 16-draw blocks; partials padded to 8; 32-frame
# tiles; M = 512
@pytest.mark.parametrize("N,M,P,n,S,npart", [(200, 12, 1, 37, 5, 2), (1500, 50, 3, 215, 16, 2), (3000, 130, 5, 429, 33, 2),
                                             (600, 256, 2, 65, 7, 5), (700, 272, 2, 100, 17, 2), (1100, 512, 2, 100, 16, 2)])
def test_random_eps_matches_restatement(gp_handle, N, M, P, n, S, npart):
    X, Y, Z, kl = problem(N, M, P, N + M, npart=npart)
    Z = Z + 0.3 / FS
    m = _model(X, Y, Z, kl, 0.2, gp_handle)
    Xs = np.linspace(X.min(), X.max(), n).reshape(-1, 1) + 1e-5
    _check(m, Xs, X, Y, Z, kl, 0.2, _random_eps(kl, n, M, S, N + S))
    m._destroy()


# ---- 3. a mixed sum -------------------------------------------------------------------------------------------------------
def _mixed_kernels():
    e20 = 1. / np.arange(1., 21.)
    return [
        {"type": "mercer_matern12sm", "variance": 1.1, "lengthscales": 0.05, "energy": [1.0], "frequency": [220.]},
        {"type": "mercer_matern12sm", "variance": 0.9, "lengthscales": 0.07, "energy": list(e20 / e20.sum()),
         "frequency": [110. * q for q in range(1, 21)]},
        {"type": "matern12sm", "variance": 0.9, "lengthscales": 0.05, "energy": [0.7, 0.3], "frequency": [277., 554.]},
        {"type": "matern12", "variance": 0.4, "lengthscales": 0.03, "energy": [], "frequency": []},
    ]


def test_mixed_kernel_sum(gp_handle):
    X, Y, Z, _ = problem(900, 70, 2, 4)
    Z = Z + 0.3 / FS
    kl = _mixed_kernels()
    m = _model(X, Y, Z, kl, 0.25, gp_handle)
    Xs = np.linspace(X.min(), X.max(), 131).reshape(-1, 1) + 1e-5
    assert ref.eps_shapes(kl, 131, 70, 9) == ((9, 47, 131), (9, 47, 70), (9, 2, 70))
    _check(m, Xs, X, Y, Z, kl, 0.25, _random_eps(kl, 131, 70, 9, 3))
    m._destroy()


# ---- 4. bit for bit -----------------------------------------------------------------------------------------------------------
def test_repeatable_and_a_draw_sees_only_its_own_eps(gp_handle):
    X, Y, Z, kl = problem(1500, 50, 3, 7)
    m = _model(X, Y, Z, kl, 0.2, gp_handle)
    Xs = X[::7] + 1e-5
    eps = _random_eps(kl, Xs.shape[0], 50, 21, 5)
    a = m.sample_s_sparse(Xs, num_samples=21, eps=eps)
    b = m.sample_s_sparse(Xs, num_samples=21, eps=eps)
    c = m.sample_s_sparse(Xs, num_samples=5, eps=[e[:5] for e in eps])
    for p in range(3):
        assert np.array_equal(a[p], b[p])
        assert np.array_equal(a[p][:5], c[p])
    m._destroy()


# ---- 5. two output columns ---------------------------------------------------------------------------------------------------
def test_two_output_columns(gp_handle):
    X, Y, Z, kl = problem(500, 20, 2, 12)
    Y2 = np.hstack([Y, 0.5 * Y[::-1]])
    m = _model(X, Y2, Z, kl, 0.2, gp_handle)
    Xs = X[::5] + 1e-5
    n, S = Xs.shape[0], 6
    eps = [np.stack([a, b]) for a, b in zip(_random_eps(kl, n, 20, S, 1), _random_eps(kl, n, 20, S, 2))]
    got = m.sample_s_sparse(Xs, num_samples=S, eps=eps)
    assert len(got) == 2 and all(g.shape == (S, n, 2) for g in got)
    for d in range(2):
        want = ref.sample_sources(Xs, X, Y2[:, d:d + 1], Z, kl, 0.2, *[e[d] for e in eps])
        for p in range(2):
            _close(got[p][:, :, d], want[p], 1e-8)
    with pytest.raises(ValueError):
        m.sample_s_sparse(Xs, num_samples=S, eps=[e[0] for e in eps])          # the D axis is missing
    m._destroy()


# ---- 6. batched -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,M,P", [(300, 16, 2), (2001, 64, 3)])
def test_batched_windows_match_one_window(gp_handle, N, M, P):
    from gpitch_amd.windows import SgprWindowBatch
    S = 4
    wins = _windows([M] * 5, N, P, seed0=3)
    tmpl = _model(*wins[0][:3], wins[0][3], 0.3, gp_handle)
    dev = SgprWindowBatch(tmpl, 5, N, M, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    noises = [0.2 + 0.05 * i for i in range(5)]
    pv = np.stack([_params_vector(nz, w[3]) for nz, w in zip(noises, wins)])
    per = [_random_eps(w[3], N, M, S, 40 + i) for i, w in enumerate(wins)]
    eps = [np.stack([e[q] for e in per]) for q in range(3)]
    got = dev.sample_s_sparse(pv, num_samples=S, eps=eps)
    assert got.shape == (5, P, S, N)
    for i, w in enumerate(wins):
        one = _model(w[0], w[1], w[2], w[3], noises[i], gp_handle)
        want = one.sample_s_sparse(w[0], num_samples=S, eps=per[i])
        for k in range(P):
            _close(got[i, k], want[k][:, :, 0], 1e-8)
        one._destroy()
    dev.close()
    tmpl._destroy()


def test_ragged_windows_match_their_own_size(gp_handle):
    """counts [16, 9, 1, 12] on an M = 16 plan; the rows of eps_z, eps_u and Z past a window's own count are NaN: each slot is
    the one-window model on Z[:k] with eps[..., :k], and no NaN comes out"""
    from gpitch_amd.windows import SgprWindowBatch
    counts, N, P, M, S, n = [16, 9, 1, 12], 300, 2, 16, 4, 77
    wins = _windows(counts, N, P, seed0=5)
    tmpl = _model(*wins[0][:3], wins[0][3], 0.3, gp_handle)
    dev = SgprWindowBatch(tmpl, 4, N, M, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    zpad = np.full((4, M), np.nan)
    for i, w in enumerate(wins):
        zpad[i, :counts[i]] = w[2].reshape(-1)
    dev.Z.copy_(gp_handle.torch.as_tensor(zpad))
    noises = [0.2 + 0.05 * i for i in range(4)]
    pv = np.stack([_params_vector(nz, w[3]) for nz, w in zip(noises, wins)])
    xnews = [np.linspace(w[0].min(), w[0].max(), n).reshape(-1, 1) for w in wins]
    per = [_random_eps(w[3], n, M, S, 60 + i) for i, w in enumerate(wins)]
    for i, k in enumerate(counts):
        per[i][1][:, :, k:] = np.nan
        per[i][2][:, :, k:] = np.nan
    eps = [np.stack([e[q] for e in per]) for q in range(3)]
    got = dev.sample_s_sparse(pv, xnews, num_samples=S, eps=eps)
    assert got.shape == (4, P, S, n) and np.isfinite(got).all()
    for i, w in enumerate(wins):
        k = counts[i]
        one = _model(w[0], w[1], w[2], w[3], noises[i], gp_handle)
        own = [per[i][0], per[i][1][:, :, :k], per[i][2][:, :, :k]]
        want = one.sample_s_sparse(xnews[i], num_samples=S, eps=own)
        rest = ref.sample_sources(xnews[i], w[0], w[1], w[2], w[3], noises[i], *own)
        for q in range(P):
            _close(got[i, q], want[q][:, :, 0], 1e-8)
            _close(got[i, q], rest[q], 1e-8)
        one._destroy()
    dev.close()
    tmpl._destroy()


def _ragged_mixed_windows(counts, N):
    """every window the mixed sum (partials padded to 4, 20 and 4, and a Matern12 with no table) at its own variances and
    lengthscales"""
    wins = []
    for i, (X, Y, Z, _) in enumerate(_windows(counts, N, 2, seed0=5)):
        kl = _mixed_kernels()
        for p, d in enumerate(kl):
            d["variance"] *= 1.0 + 0.1 * ((i + p) % 3)
            d["lengthscales"] *= 1.0 + 0.2 * ((2 * i + p) % 3)
        wins.append((X, Y, Z, kl))
    return wins


def test_ragged_windows_with_a_mixed_kernel_sum(gp_handle):
    """test_ragged_windows_match_their_own_size with counts [16, 9, 1] on an M = 16 plan, n = 70 (a 64-frame tile and a partial
    one), S = 17 (a 16-draw block and one draw) and the mixed sum: the strides of a process record where they all differ: a
    source's component offset inside C = 47, the eps_z row stride M = 16 against the feature-table stride k = 9 or 1, a
    Matern12 source without a table beside sources padded to 20 partials in one launch.  The inputs are conditioned for the 1e-8 rule
    (tests/test_sample_sparse_cpu.py::test_ragged_mixed_gpu_shape_is_well_conditioned: two host routes differ by 1.8e-15)."""
    from gpitch_amd.windows import SgprWindowBatch
    counts, N, P, M, S, n = [16, 9, 1], 300, 4, 16, 17, 70
    wins = _ragged_mixed_windows(counts, N)
    assert ref.eps_shapes(wins[0][3], n, M, S) == ((S, 47, n), (S, 47, M), (S, 2, M))
    tmpl = _model(*wins[0][:3], wins[0][3], 0.3, gp_handle)
    dev = SgprWindowBatch(tmpl, 3, N, M, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    zpad = np.full((3, M), np.nan)
    for i, w in enumerate(wins):
        zpad[i, :counts[i]] = w[2].reshape(-1)
    dev.Z.copy_(gp_handle.torch.as_tensor(zpad))
    noises = [0.2 + 0.05 * i for i in range(3)]
    pv = np.stack([_params_vector(nz, w[3]) for nz, w in zip(noises, wins)])
    xnews = [np.linspace(w[0].min(), w[0].max(), n).reshape(-1, 1) for w in wins]
    per = [_random_eps(w[3], n, M, S, 80 + i) for i, w in enumerate(wins)]
    for i, k in enumerate(counts):
        per[i][1][:, :, k:] = np.nan
        per[i][2][:, :, k:] = np.nan
    eps = [np.stack([e[q] for e in per]) for q in range(3)]
    got = dev.sample_s_sparse(pv, xnews, num_samples=S, eps=eps)
    assert got.shape == (3, P, S, n) and np.isfinite(got).all()
    for i, w in enumerate(wins):
        k = counts[i]
        one = _model(w[0], w[1], w[2], w[3], noises[i], gp_handle)
        own = [per[i][0], per[i][1][:, :, :k], per[i][2][:, :, :k]]
        want = one.sample_s_sparse(xnews[i], num_samples=S, eps=own)
        rest = ref.sample_sources(xnews[i], w[0], w[1], w[2], w[3], noises[i], *own)
        for q in range(P):
            print("slot %d source %d: |batch - one window| %.3e, |batch - restatement| %.3e at |ref| %.3e" % (
                i, q, np.abs(got[i, q] - want[q][:, :, 0]).max(), np.abs(got[i, q] - rest[q]).max(), np.abs(rest[q]).max()))
            _close(got[i, q], want[q][:, :, 0], 1e-8)
            _close(got[i, q], rest[q], 1e-8)
        one._destroy()
    dev.close()
    tmpl._destroy()


# ---- 7. eps=None: the device generator ---------------------------------------------------------------------------------------
def test_seeded_draws_and_their_mean(gp_handle):
    X, Y, Z, kl, noise, Xs = ref.smallest_problem()
    m = _model(X, Y, Z, kl, noise, gp_handle)
    a = m.sample_s_sparse(Xs, num_samples=8, seed=3)
    b = m.sample_s_sparse(Xs, num_samples=8, seed=3)
    c = m.sample_s_sparse(Xs, num_samples=8, seed=4)
    for p in range(2):
        assert a[p].shape == (8, 40, 1) and np.array_equal(a[p], b[p]) and not np.array_equal(a[p], c[p])
    S = 4096
    draws = m.sample_s_sparse(Xs, num_samples=S, seed=0)
    sm, sv = m.predict_s_sparse(Xs)
    for p in range(2):
        dev = np.abs(draws[p][:, :, 0].mean(0) - sm[p][:, 0])
        bound = 6. * np.sqrt(sv[p][:, 0] / S)
        print("source %d: worst |sample mean - posterior mean| / bound = %.3f" % (p, (dev / bound).max()))
        assert np.all(dev <= bound)
    m._destroy()


# ---- 8. arguments ------------------------------------------------------------------------------------------------------------
def _plan(h, codes, M, N=100):
    from gpitch_amd import _lib
    P = len(codes)
    i32 = C.c_int32 * P
    keep = (i32(*[c for c, _ in codes]), i32(*[m for _, m in codes]))
    cfg = _lib.SgprConfig(P, N, M, keep[0], keep[1], 1e-6, 0)
    plan = C.c_void_p()
    h.check(h.lib.gp_sgpr_create(h.h, C.byref(cfg), C.byref(plan)))
    return plan, keep


def test_arguments(gp_handle):
    from gpitch_amd import _lib, merged_order
    from gpitch_amd.sgpr_ss import SGPRSS
    from gpitch_amd.windows import SgprWindowBatch
    h, lib = gp_handle, gp_handle.lib
    N, M, n, S, Cc = 100, 10, 30, 3, 8
    X, Y, Z, kl = problem(N, M, 2, 1)
    Xs = np.linspace(X.min(), X.max(), n).reshape(-1, 1) + 1e-5
    m = _model(X, Y, Z, kl, 0.2, h)
    eps = _random_eps(kl, n, M, S, 9)
    want = ref.sample_sources(Xs, X, Y, Z, kl, 0.2, *eps)

    def still_right():
        got = m.sample_s_sparse(Xs, num_samples=S, eps=eps)
        for p in range(2):
            _close(got[p][:, :, 0], want[p], 1e-8)

    still_right()
    xs, out = h.to_device(Xs.reshape(-1)), h.empty(2, S, n)
    ex, ez, eu = (h.to_device(e) for e in eps)
    order = np.ascontiguousarray(merged_order(Xs, Z))
    nbytes = lib.gp_sgpr_sample_source_workspace_bytes(M, 2, Cc, n, S, 1)
    ws = h.workspace(nbytes)
    good = [m._plan, m._params.data_ptr(), m._Xd.data_ptr(), m._Yd.data_ptr(), N, m._Zd.data_ptr(), xs.data_ptr(), n,
            order.ctypes.data, S, ex.data_ptr(), ez.data_ptr(), eu.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel()]
    assert lib.gp_sgpr_sample_source_sparse(*good) == _lib.GP_OK
    for p in range(2):
        _close(out[p].cpu().numpy(), want[p], 1e-8)
    bad = [(pos, None) for pos in (1, 2, 3, 5, 6, 8, 10, 11, 12, 13, 14)]         # null pointers
    bad += [(7, 0), (9, 0), (4, N + 1), (15, nbytes - 4096 - 256)]                 # n < 1, S < 1, N above max_N, short workspace
    for pos, v in bad:
        a = list(good)
        a[pos] = v
        assert lib.gp_sgpr_sample_source_sparse(*a) == _lib.GP_ERR_BAD_ARG, pos
    still_right()
    for j, v in ((3, int(order[4])), (11, n + M), (0, -1)):                      # a repeated index, n + M, a negative one
        o = order.copy()
        o[j] = v
        a = list(good)
        a[8] = o.ctypes.data
        assert lib.gp_sgpr_sample_source_sparse(*a) == _lib.GP_ERR_BAD_ARG, (j, v)
        still_right()
    # the batched entry: the same checks per slot
    dev = SgprWindowBatch(m, 2, N, M, handle=h)
    dev.load([X, X], [Y, Y], [Z, Z])
    xn = h.to_device(np.stack([Xs.reshape(-1)] * 2))
    pv = np.stack([_params_vector(0.2, kl)] * 2)
    dev.params.copy_(h.to_device(pv))
    e2 = [h.to_device(np.stack([e, e])) for e in eps]
    o2 = np.ascontiguousarray(np.stack([order, order]))
    out2 = h.empty(2, 2, S, n)
    nb2 = lib.gp_sgpr_sample_source_workspace_bytes(M, 2, Cc, n, S, 2)
    ws2 = h.workspace(nb2)
    bgood = [dev.plan, dev.params.data_ptr(), dev.X.data_ptr(), dev.Y.data_ptr(), dev.Z.data_ptr(), xn.data_ptr(), n, 2,
             o2.ctypes.data, S, e2[0].data_ptr(), e2[1].data_ptr(), e2[2].data_ptr(), out2.data_ptr(), ws2.data_ptr(),
             ws2.numel()]
    assert lib.gp_sgprb_sample_source_sparse(*bgood) == _lib.GP_OK
    for w in range(2):
        for p in range(2):
            _close(out2[w, p].cpu().numpy(), want[p], 1e-8)
    bbad = [(pos, None) for pos in (1, 2, 3, 4, 5, 8, 10, 11, 12, 13, 14)]
    bbad += [(6, 0), (7, 0), (7, 3), (9, 0), (15, nb2 - 4096 - 256)]
    for pos, v in bbad:
        a = list(bgood)
        a[pos] = v
        assert lib.gp_sgprb_sample_source_sparse(*a) == _lib.GP_ERR_BAD_ARG, pos
    for j, v in ((3, int(order[4])), (11, n + M), (0, -1)):                      # in the SECOND slot
        o = o2.copy()
        o[1, j] = v
        a = list(bgood)
        a[8] = o.ctypes.data
        assert lib.gp_sgprb_sample_source_sparse(*a) == _lib.GP_ERR_BAD_ARG, (j, v)
    assert lib.gp_sgprb_sample_source_sparse(*bgood) == _lib.GP_OK
    for p in range(2):
        _close(out2[1, p].cpu().numpy(), want[p], 1e-8)
    dev.close()
    # M above the limit, and sums that hold a kernel without a Matern-1/2 envelope: GP_ERR_UNSUPPORTED from the library ...
    plans = [_plan(h, [(_lib.KERN_MATERN12, 0)], 1040)]
    for code, mm in ((_lib.KERN_MATERN32, 0), (_lib.KERN_MATERN52, 0), (_lib.KERN_RBF, 0), (_lib.KERN_MATERN32SM, 2),
                     (_lib.KERN_MERCER_MATERN52SM, 2)):
        plans.append(_plan(h, [(_lib.KERN_MERCER_MATERN12SM, 2), (code, mm)], M))
    for plan, keep in plans:
        a = list(good)
        a[0] = plan
        assert lib.gp_sgpr_sample_source_sparse(*a) == _lib.GP_ERR_UNSUPPORTED
        lib.gp_sgpr_destroy(plan)
    still_right()
    m._destroy()
    # ... and NotImplementedError from the model, naming the kernel, before any device work
    from gpitch_amd import kernels as K
    k52 = K.Matern52(1, variance=2.5, lengthscales=0.01)
    prod = K.Prod(k52, K.MercerCosMix(1, energy=np.array([1.]), frequency=np.array([100.]), variance=0.2))
    for name, k in (("Matern32", K.Matern32(1)), ("Matern52", K.Matern52(1)), ("RBF", K.RBF(1)),
                    ("Matern32sm", K.Matern32sm(1, 3)), ("MercerCosMix", prod)):
        mm = SGPRSS(X, Y, np.sum([_kern(kl[0]), k]), Z, handle=h)
        with pytest.raises(NotImplementedError, match=name):
            mm.sample_s_sparse(Xs)
        assert mm._plan is None
    sharded = SGPRSS(X, Y, np.sum([_kern(d) for d in kl]), Z, handle=h, shard=(0, 2))
    with pytest.raises(NotImplementedError):
        sharded.sample_s_sparse(Xs)


def test_float32_plan(gp_handle):
    """the state (W, WB, c) comes from the float32 forward pass, the sampling kernels' arithmetic is float64: held to the
    bound tests/test_gpu_f32.py states for SGPRSS predict_f on a float32 plan, 1e-4 of the largest magnitude"""
    X, Y, Z, kl = problem(2001, 64, 3, 8)
    Xs = X[::3] + 1e-5
    eps = _random_eps(kl, Xs.shape[0], 64, 8, 11)
    m64 = _model(X, Y, Z, kl, 0.2, gp_handle)
    m32 = _model(X, Y, Z, kl, 0.2, gp_handle, float_type=np.float32)
    a, b = m64.sample_s_sparse(Xs, num_samples=8, eps=eps), m32.sample_s_sparse(Xs, num_samples=8, eps=eps)
    for p in range(3):
        dev = np.abs(a[p] - b[p]).max() / np.abs(a[p]).max()
        print("float32 plan: source %d relative difference %.3e" % (p, dev))
        assert dev <= 1e-4
    m64._destroy()
    m32._destroy()
