"""Kernel learning from training audio on the device: segment Gram, autocorrelation, batched kernel-fit objective and the
fits built on them, each against its own numpy restatement."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture():
    d = np.load(os.path.join(HERE, "golden", "init_liv_real_audio.npz"))
    return d["y"].astype(np.float64).reshape(-1, 1), float(d["fs"]), str(d["fname"])


# ---- numpy restatements ---------------------------------------------------------------------------------------------
def _np_gram(x, starts, L):
    S = np.stack([x[s:s + L] for s in starts])
    return S.T @ S / len(starts)


def _np_kernfit(p, x, y):
    """k, f = sqrt(mean((k - y)^2)), df/dp of the Matern-3/2 x cosine-mixture fit (m = (len(p) - 2) // 2)"""
    p = np.asarray(p, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    m = (p.size - 2) // 2
    r = np.abs(x)
    l, v, fr = p[1], p[2:2 + m], p[2 + m:2 + 2 * m]
    a = np.sqrt(3.) * r / np.abs(l)
    env = (1. + a) * np.exp(-a)
    cs = np.cos(2 * np.pi * np.abs(fr)[:, None] * r[None, :])
    sn = np.sin(2 * np.pi * np.abs(fr)[:, None] * r[None, :])
    S = np.abs(v) @ cs
    k = env * S
    e = k - y
    f = np.sqrt(np.mean(e ** 2))
    c = e / (x.size * f)
    g = np.zeros(p.size)
    g[1] = np.sign(l) * np.sum(c * S * a * a * np.exp(-a) / np.abs(l))
    g[2:2 + m] = np.sign(v) * ((cs * env) @ c)
    g[2 + m:2 + 2 * m] = np.sign(fr) * ((-(sn * env * 2 * np.pi * r) * np.abs(v)[:, None]) @ c)
    return k, f, g


def _host_fit(x, y, p0):
    from gpitch_amd import lbfgsb_batch
    run = lbfgsb_batch.LbfgsbRC(p0, ftol=1e-12, gtol=1e-12)
    while run.step():
        _, f, g = _np_kernfit(run.x, x, y)
        run.give(f, g)
    return run


# ---- 1. segment Gram ------------------------------------------------------------------------------------------------
def _recordings(B, L, K, seed):
    rng = np.random.RandomState(seed)
    xs = [rng.randn(L + 50 + 37 * b) for b in range(B)]
    starts = [rng.randint(0, x.size - L + 1, size=K) for x in xs]
    return xs, starts


@pytest.mark.parametrize("L", [1, 17, 64, 441, 512])
@pytest.mark.parametrize("K", [1, 3, 10000])
@pytest.mark.parametrize("B", [1, 5, 88])
def test_segment_gram_matches_numpy(gp_handle, L, K, B):
    from gpitch_amd import samplecov
    if B == 88 and K == 10000 and L != 441:
        pytest.skip("the B = 88, K = 10000 shape runs at L = 441 (and in the repeat test)")
    xs, starts = _recordings(B, L, K, 1000 * L + K + B)
    got = samplecov.segment_gram(xs, starts, L, gp_handle)
    again = samplecov.segment_gram(xs, starts, L, gp_handle)
    for b in range(B):
        C = got[b]
        assert np.array_equal(C, C.T)
        assert np.array_equal(C, again[b])
        if B == 88 and b % 29:
            continue
        ref = _np_gram(xs[b], starts[b], L)
        assert np.max(np.abs(C - ref)) <= 1e-12 * np.max(np.abs(ref)), (b, np.max(np.abs(C - ref)))


def test_segment_gram_repeats_bit_for_bit_at_a_device_filling_shape(gp_handle):
    from gpitch_amd import samplecov
    rng = np.random.RandomState(7)
    xs = [rng.randn(16000 + 113 * b) for b in range(88)]
    starts = [rng.randint(0, x.size - 441, size=10000) for x in xs]
    first = samplecov.segment_gram(xs, starts, 441, gp_handle)
    for b in (0, 43, 87):
        ref = _np_gram(xs[b], starts[b], 441)
        assert np.max(np.abs(first[b] - ref)) <= 1e-12 * np.max(np.abs(ref))
    for _ in range(24):
        again = samplecov.segment_gram(xs, starts, 441, gp_handle)
        for b in range(88):
            assert np.array_equal(first[b], again[b]), b


def test_segment_gram_argument_checks(gp_handle):
    import ctypes as C
    from gpitch_amd import _lib
    h = gp_handle
    y = h.to_device(np.zeros(1000))
    out = h.empty(10 * 10)
    ws = h.workspace(samplecov_ws(1, 4, 10))
    off = np.zeros(1, np.int64)
    ln = np.array([1000], np.int64)
    st = np.array([0, 10, 500, 990], np.int32)

    def call(K=4, L=10, starts=st, nbytes=None, yy=y):
        return h.lib.gp_segment_gram(h.h, _lib._ptr(yy), 1000, off.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p),
                                     1, starts.ctypes.data_as(C.c_void_p), K, L, _lib._ptr(out), _lib._ptr(ws),
                                     samplecov_ws(1, 4, 10) if nbytes is None else nbytes)
    assert call() == _lib.GP_OK
    h.sync()
    assert call(L=0) == _lib.GP_ERR_BAD_ARG
    assert call(K=0) == _lib.GP_ERR_BAD_ARG
    assert call(yy=None) == _lib.GP_ERR_BAD_ARG
    assert call(nbytes=16) == _lib.GP_ERR_BAD_ARG
    assert b"workspace" in h.lib.gp_last_error(h.h)
    assert call(starts=np.array([0, 10, 500, 991], np.int32)) == _lib.GP_ERR_BAD_ARG
    assert b"outside" in h.lib.gp_last_error(h.h)


def samplecov_ws(B, K, L):
    from gpitch_amd import samplecov
    return samplecov.gram_workspace_bytes(B, K, L)


# ---- 2. get_cov, comatrix, autocorr on the real note ---------------------------------------------------------------
def test_get_cov_and_comatrix_on_the_real_note(gp_handle):
    from gpitch_amd import samplecov
    y, fs, name = _fixture()
    np.random.seed(0)
    cov, kern, samples = samplecov.get_cov(y, 10000, 441, gp_handle)
    np.random.seed(0)
    st = [np.random.randint(0, y.size - 441) for _ in range(10000)]
    ref = sum(np.outer(y[s:s + 441], y[s:s + 441]) for s in st) / 10000.
    rk = ref[0].copy().reshape(-1, 1)
    rk /= np.max(np.abs(rk))
    sc = np.max(np.abs(ref))
    assert cov.shape == (441, 441) and kern.shape == (441, 1)
    assert np.max(np.abs(cov - ref)) <= 1e-12 * sc
    assert np.max(np.abs(kern - rk)) <= 1e-12
    assert len(samples) == 10000 and samples[5].shape == (441, 1) and np.array_equal(samples[5], y[st[5]:st[5] + 441])
    co = samplecov.comatrix(samples, gp_handle)
    assert np.max(np.abs(co - ref)) <= 1e-12 * sc


def test_autocorr_on_the_real_note(gp_handle):
    from gpitch_amd import samplecov
    y, fs, name = _fixture()
    r, samples = samplecov.autocorr(y, 441, gp_handle)
    x = y.reshape(-1)
    N = x.size - 441
    ref = np.array([np.dot(x[:N], x[j:j + N]) for j in range(441)])
    ref /= np.max(np.abs(ref))
    assert r.shape == (441, 1)
    assert np.max(np.abs(r[:, 0] - ref)) <= 1e-12
    assert samples.shape == (441, N) and not samples.flags.writeable
    assert np.array_equal(samples[:, 123], x[123:123 + 441])


# ---- 3. the kernel-fit objective -----------------------------------------------------------------------------------
def _problem(m, n=441, fs=16000., seed=0, negative=False):
    rng = np.random.RandomState(seed)
    x = np.linspace(0, (n - 1.) / fs, n)
    p = np.hstack(([0.3, 0.01 + 0.01 * rng.rand()], 0.2 + rng.rand(m), 200. * (np.arange(m) + 1) + 20 * rng.randn(m)))
    if negative:
        p[[0, 1, 2, 2 + m]] *= -1
    y = _np_kernfit(np.abs(p) * (1 + 0.05 * rng.randn(p.size)), x, np.zeros(n))[0] + 0.01 * rng.randn(n)
    return x, y, p


@pytest.mark.parametrize("negative", [False, True])
def test_kernfit_eval_matches_numpy(gp_handle, negative):
    from gpitch_amd.kernelfit import KernfitBatch
    x, y, p = _problem(5, negative=negative)
    f, gs, ks = KernfitBatch([x], [y], [5], gp_handle)([p], want_k=True)
    k0, f0, g0 = _np_kernfit(p, x, y)
    assert abs(f[0] - f0) <= 1e-12 * f0
    assert np.max(np.abs(ks[0] - k0)) <= 1e-12 * np.max(np.abs(k0))
    assert gs[0][0] == 0.0
    assert np.max(np.abs(gs[0] - g0)) <= 1e-12 * np.max(np.abs(g0))
    # central differences of the device objective
    for i in range(1, p.size):
        hh = 1e-6 * max(abs(p[i]), 1e-3)
        pp, pm = p.copy(), p.copy()
        pp[i] += hh
        pm[i] -= hh
        fd = (KernfitBatch([x], [y], [5], gp_handle)([pp])[0][0] - KernfitBatch([x], [y], [5], gp_handle)([pm])[0][0]) / (2 * hh)
        assert abs(fd - gs[0][i]) <= 1e-6 * max(abs(gs[0][i]), 1e-3 * np.max(np.abs(gs[0]))), (i, fd, gs[0][i])


def test_kernfit_eval_batch_is_bit_identical_to_single(gp_handle):
    from gpitch_amd.kernelfit import KernfitBatch
    probs = [_problem(m, n=n, seed=s, negative=bool(s % 2)) for s, (m, n) in enumerate([(1, 441), (5, 300), (20, 441),
                                                                                           (3, 17), (12, 441)])]
    xs, ys, ps = zip(*probs)
    ms = [(p.size - 2) // 2 for p in ps]
    fb, gb, kb = KernfitBatch(xs, ys, ms, gp_handle)(ps, want_k=True)
    for w in range(len(ps)):
        f1, g1, k1 = KernfitBatch([xs[w]], [ys[w]], [ms[w]], gp_handle)([ps[w]], want_k=True)
        assert fb[w] == f1[0]
        assert np.array_equal(gb[w], g1[0])
        assert np.array_equal(kb[w], k1[0])


# ---- 4. recovery of known parameters ---------------------------------------------------------------------------------
def test_fit_recovers_known_parameters(gp_handle):
    from gpitch_amd import kernelfit
    fs, L = 16000., 441
    x = np.linspace(0., (L - 1.) / fs, L)
    f0 = 261.6
    ptrue = np.hstack(([0., 0.02], [1.0, 0.6, 0.35, 0.2, 0.1], f0 * np.arange(1, 6) * (1 + 0.001 * np.arange(5))))
    y = _np_kernfit(ptrue, x, np.zeros(L))[0]
    p0 = ptrue * (1 + 0.01 * np.array([0, 1, -1, 1, -1, 1, -1, 1, -1, 1, -1, 1]))
    pstar = kernelfit.optimize_kern(x.reshape(-1, 1), y.reshape(-1, 1), p0, gp_handle)
    assert np.max(np.abs(pstar[1:] - ptrue[1:]) / ptrue[1:]) <= 1e-6, pstar - ptrue
    # ftol = 1e-12 is relative to max(|f|, 1): below f = 1 the run stops at the first iteration that gains less than 1e-12,
    # which ulp-level trajectory differences put anywhere between 1e-10 and 1e-7 here (host numpy: 1.4e-10; device: 1.1e-7)
    assert kernelfit.loss_func(pstar, x, y, gp_handle) <= 1e-6


# ---- 5. the real note, three sampling seeds ------------------------------------------------------------------------
def _real_problem(seed, gp_handle):
    from gpitch_amd import samplecov
    from gpitch_amd.methods import find_ideal_f0, init_cparam
    y, fs, name = _fixture()
    np.random.seed(seed)
    cov, kern, _ = samplecov.get_cov(y, 10000, 441, gp_handle)
    if0 = find_ideal_f0([name])[0]
    init_f, init_v = init_cparam(y=y, fs=fs, maxh=20, ideal_f0=if0, scaled=False)[0:2]
    p0 = np.hstack(([0., 1.], init_v, init_f))
    xk = np.linspace(0., 440. / fs, 441).reshape(-1, 1)
    return y, fs, name, kern, xk, p0


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fit_on_the_real_note(gp_handle, seed):
    from scipy.optimize import minimize
    from gpitch_amd import kernelfit
    y, fs, name, kern, xk, p0 = _real_problem(seed, gp_handle)
    params, k_init, k_approx = kernelfit.fit(kern, y, name, 20, fs, gp_handle)
    pstar = np.hstack(([0., params[0]], params[1], params[2]))
    got = _np_kernfit(pstar, xk, kern)[1]
    host = _host_fit(xk, kern, p0)
    # the same minimisation on the numpy restatement: ulp-level differences in f and g steer the two runs apart within
    # one basin (seed 0: 5e-6 relative; the host run alone moves by 2e-5 between two CPUs)
    assert abs(got - host.fun) <= 1e-4 * host.fun, (got, host.fun)
    assert (params[0] > 0.5) == (abs(host.x[1]) > 0.5)
    fd = minimize(lambda p: _np_kernfit(p, xk, kern)[1], p0, method="L-BFGS-B", tol=1e-12)
    # the reference's finite-difference path: the same basin ends within 1 %; on seed 1 the lengthscale stays near its
    # start of 1.0 on both paths on one CPU, while on another the difference quotients carry the FD run into the basin
    # near 0.12 (half the RMSE): the FD path's basin is not a property of the objective
    if (params[0] > 0.5) == (abs(fd.x[1]) > 0.5):
        assert got <= 1.01 * fd.fun, (got, fd.fun)
    assert np.max(np.abs(k_approx[:, 0] - _np_kernfit(pstar, xk, kern)[0])) <= 1e-12
    assert np.max(np.abs(k_init[:, 0] - _np_kernfit(p0, xk, kern)[0])) <= 1e-12 * np.max(np.abs(k_init))


# ---- 6. batching -----------------------------------------------------------------------------------------------------
def test_fit_many_is_bit_identical_to_single_fits(gp_handle):
    from gpitch_amd import kernelfit, samplecov
    y, fs, name = _fixture()
    audios = [y] * 3 + [y[500 * i:] for i in range(1, 4)] + [y[::-1].copy(), y[:20000], y[5000:]] + [y * 0.5] * 3
    kerns = []
    for i, a in enumerate(audios):
        np.random.seed(i)
        kerns.append(samplecov.get_cov(a, 10000, 441, gp_handle)[1])
    many = kernelfit.fit_many(kerns, audios, [name] * 12, 20, fs, gp_handle)
    for w in range(12):
        one = kernelfit.fit(kerns[w], audios[w], name, 20, fs, gp_handle)
        assert one[0][0] == many[w][0][0]
        assert np.array_equal(one[0][1], many[w][0][1]) and np.array_equal(one[0][2], many[w][0][2])
        assert np.array_equal(one[1], many[w][1]) and np.array_equal(one[2], many[w][2])


# ---- 7. end to end ---------------------------------------------------------------------------------------------------
def test_learn_kernels_into_an_sgprss_window(gp_handle):
    import gpitch_amd
    from gpitch_amd import kernelfit
    from gpitch_amd.sgpr_ss import SGPRSS
    from oracle import gpflow05 as orc
    y, fs, name = _fixture()
    np.random.seed(0)
    params, (xkern, skern), covs = kernelfit.learn_kernels([y], [name], fs, handle=gp_handle)
    assert len(covs) == 1 and covs[0].shape == (441, 441) and skern[0].shape == (441, 1) and xkern[0].shape == (441, 1)
    kc = gpitch_amd.init_kern_com(1, params[0], params[1], params[2], len_fixed=False)
    N, M = 1600, 80
    X = np.linspace(0, (N - 1) / fs, N).reshape(-1, 1)
    Y = y[8000:8000 + N].copy()
    Z = X[::N // M][:M].copy()
    m = SGPRSS(X, Y, kc[0], Z, handle=gp_handle)
    m.likelihood.variance = 0.1
    got = m.build_likelihood()
    assert np.isfinite(got)
    kl = [{"type": "mercer_matern12sm", "variance": 1.0, "lengthscales": float(params[0][0]),
           "energy": list(params[1][0]), "frequency": list(params[2][0])}]
    ref = orc.sgpr_bound(X, Y, Z, kl, 0.1)
    assert abs(got - ref) <= 1e-9 * abs(ref), (got, ref)
