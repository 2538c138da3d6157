"""Window-batched SGPRSS with a different inducing-point count per window (gp_sgprb_set_inducing_counts): the drivers
pick every window's Z from its own audio (init_liv, transcription.py:229-238 / separation.py:238-250), so M differs
from window to window.  Each window is carried as the exact M-point problem with an identity pad block: per-window parity
with the oracle and with the one-window engine at the window's own Z, graphs that see new counts, independence from the
neighbouring slots, and the batched fits of init_liv windows against the sequential ones.  Tolerances are those of
test_gpu_windows_batched.py."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import gpflow05 as orc  # noqa: E402

FS = 16000.


def _kdicts(P, w):
    """P kernels of mixed forms: a MercerMatern12sm (feature contraction), a Matern12sm (broadcast form) and, at P = 3,
    a Matern32 (stationary form); hyper-parameters differ per window"""
    out = []
    for p in range(P):
        f0 = 220. * 2 ** (p * 4 / 12.)
        d = {"variance": 0.8 + 0.15 * ((w + p) % 4), "lengthscales": 0.04 + 0.01 * ((2 * w + p) % 5)}
        if p == 0:
            d.update(type="mercer_matern12sm", energy=[0.6, 0.4], frequency=[f0, 2 * f0])
        elif p == 1:
            d.update(type="matern12sm", energy=[0.7, 0.3], frequency=[f0, 2 * f0])
        else:
            d.update(type="matern32", energy=[], frequency=[])
        out.append(d)
    return out


def _model(X, Y, Z, kdicts, noise, handle, reg=False):
    from gpitch_amd.kernels import Matern32
    from gpitch_amd.matern12_spectral_mixture import Matern12sm, MercerMatern12sm
    from gpitch_amd.sgpr_ss import SGPRSS
    ks = []
    for d in kdicts:
        if d["type"] == "mercer_matern12sm":
            ks.append(MercerMatern12sm(1, energy=np.array(d["energy"]), frequency=np.array(d["frequency"]),
                                       variance=d["variance"], lengthscales=d["lengthscales"]))
        elif d["type"] == "matern12sm":
            ks.append(Matern12sm(1, energy=np.array(d["energy"]), frequency=np.array(d["frequency"]),
                                 variance=d["variance"], lengthscales=d["lengthscales"]))
        else:
            ks.append(Matern32(1, variance=d["variance"], lengthscales=d["lengthscales"]))
    m = SGPRSS(X, Y, np.sum(ks), Z, reg=reg, handle=handle)
    m.likelihood.variance = noise
    return m


def _params_vector(noise, kl):
    v = [noise]
    for d in kl:
        v += [d["variance"], d["lengthscales"]] + list(d["energy"]) + list(d["frequency"])
    return np.array(v)


def _ragged_windows(counts, N, P, seed0=0):
    out = []
    for w, k in enumerate(counts):
        rng = np.random.RandomState(seed0 + 17 * w)
        X = np.linspace(0, (N - 1) / FS, N).reshape(-1, 1) + 0.125 * w
        Y = np.zeros((N, 1))
        for p in range(P):
            f0 = 220. * 2 ** (p * 4 / 12.)
            Y += np.sin(2 * np.pi * f0 * X) * np.exp(-((X - X.mean()) / (0.3 * np.ptp(X))) ** 2)
        Y = Y * (1.0 + 0.1 * w) + 0.05 * rng.randn(N, 1)
        Z = X[np.linspace(0, N - 1, k).round().astype(int)] + 0.3 / FS        # k points, off the frame grid
        out.append((X, Y, Z, _kdicts(P, w)))
    return out


def _one_window(w, noise, handle, reg):
    one = _model(w[0], w[1], w[2], w[3], noise, handle, reg=reg)
    one._compile()
    one._pack()
    g1 = handle.zeros(one._nparams)
    f1 = one._bound(grad=g1)
    return f1, g1.cpu().numpy()


@pytest.fixture
def stream_handle(gp_handle):
    """a handle on a stream of its own: the plan records its launch sequence into a graph and replays it"""
    import torch
    from gpitch_amd import _lib
    s = torch.cuda.Stream(device=gp_handle.device)
    with torch.cuda.stream(s):
        h = _lib.Handle(gp_handle.device.index, stream=s)
        yield h
        s.synchronize()
        h.close()


def _counts(dev):
    e, c, r = C.c_int64(), C.c_int64(), C.c_int64()
    dev.h.check(dev.h.lib.gp_sgprb_eval_counts(dev.plan, C.byref(e), C.byref(c), C.byref(r)))
    return e.value, c.value, r.value


COUNTS = [1, 15, 16, 17, 40, 64, 100, 130]


@pytest.mark.parametrize("N,P,reg", [(2001, 2, False), (2001, 3, True), (1500, 2, True), (1500, 3, False)])
def test_ragged_bound_and_gradient_per_window(stream_handle, N, P, reg):
    from gpitch_amd.windows import SgprWindowBatch
    h = stream_handle
    wins = _ragged_windows(COUNTS, N, P)
    tmpl = _model(*wins[-1][:3], wins[-1][3], 0.3, h, reg=reg)
    dev = SgprWindowBatch(tmpl, len(wins), N, 130, handle=h)
    order = [3, 0, 7, 5, 1, 6, 2, 4]                        # the slots do not follow the counts
    ws = [wins[i] for i in order]
    dev.load([w[0] for w in ws], [w[1] for w in ws], [w[2] for w in ws])
    assert dev.counts == [COUNTS[i] for i in order]
    noises = [0.3 + 0.05 * i for i in range(len(ws))]
    pv = np.stack([_params_vector(nz, w[3]) for nz, w in zip(noises, ws)])
    assert pv.shape[1] == dev.nparams
    ones = [_one_window(w, nz, h, reg) for nz, w in zip(noises, ws)]
    for rep in range(3):                                    # eager, captured, replayed
        bound, grad = dev.evaluate(pv)
        for i, w in enumerate(ws):
            ref = orc.sgpr_bound(w[0], w[1], w[2], w[3], noises[i], reg=reg)
            assert abs(bound[i] - ref) <= 1e-9 * abs(ref), (rep, i, bound[i], ref)
            f1, g1 = ones[i]
            assert abs(bound[i] - f1) <= 1e-11 * abs(f1), (rep, i, bound[i], f1)
            assert np.abs(grad[i] - g1).max() <= 1e-9 * max(np.abs(g1).max(), 1e-12), (rep, i)
    assert _counts(dev) == (1, 1, 1)
    dev.close()
    tmpl._destroy()


def test_new_counts_reach_a_replayed_graph(stream_handle):
    from gpitch_amd.windows import SgprWindowBatch
    h = stream_handle
    N, P = 1500, 2
    a = _ragged_windows([130, 40, 64, 17, 100], N, P, seed0=3)
    b = _ragged_windows([16, 130, 1, 100, 64], N, P, seed0=3)        # same frames and data, other Z sizes
    tmpl = _model(*a[0][:3], a[0][3], 0.3, h)
    pv = np.stack([_params_vector(0.3 + 0.02 * i, w[3]) for i, w in enumerate(a)])
    dev = SgprWindowBatch(tmpl, 5, N, 130, handle=h)
    dev.load([w[0] for w in a], [w[1] for w in a], [w[2] for w in a])
    for _ in range(3):
        ba, ga = dev.evaluate(pv)
    dev.load([w[0] for w in b], [w[1] for w in b], [w[2] for w in b])     # same buffers: only the counts tell
    for _ in range(3):                                # new descriptors (eager), recaptured, replayed
        bb, gb = dev.evaluate(pv)
    assert _counts(dev) == (2, 2, 2)
    fresh = SgprWindowBatch(tmpl, 5, N, 130, handle=h)
    fresh.load([w[0] for w in b], [w[1] for w in b], [w[2] for w in b])
    bf, gf = fresh.evaluate(pv)
    np.testing.assert_array_equal(bb, bf)
    np.testing.assert_array_equal(gb, gf)
    assert not np.array_equal(ba, bb)
    for i, w in enumerate(b):
        ref = orc.sgpr_bound(w[0], w[1], w[2], w[3], 0.3 + 0.02 * i)
        assert abs(bb[i] - ref) <= 1e-9 * abs(ref), (i, bb[i], ref)
    dev.close()
    fresh.close()
    tmpl._destroy()


def test_a_window_does_not_depend_on_its_neighbours(stream_handle):
    from gpitch_amd.windows import SgprWindowBatch
    h = stream_handle
    N, P = 2001, 3
    wins = _ragged_windows([40, 130, 1, 64, 17, 100, 16, 15], N, P, seed0=11)
    tmpl = _model(*wins[1][:3], wins[1][3], 0.3, h)
    nz = [0.25 + 0.03 * i for i in range(len(wins))]
    pv = np.stack([_params_vector(n, w[3]) for n, w in zip(nz, wins)])
    l1, l2 = [0, 1, 2, 3, 4, 5], [6, 7, 5, 2, 0, 1]          # window 0 in slot 0, then in slot 4, other neighbours
    out = []
    for load in (l1, l2):
        dev = SgprWindowBatch(tmpl, 6, N, 130, handle=h)
        dev.load([wins[i][0] for i in load], [wins[i][1] for i in load], [wins[i][2] for i in load])
        out.append(dev.evaluate(pv[load]))
        dev.close()
    for i in (0, 1, 2, 5):
        s1, s2 = l1.index(i), l2.index(i)
        assert out[0][0][s1] == out[1][0][s2], i
        np.testing.assert_array_equal(out[0][1][s1], out[1][1][s2])
    tmpl._destroy()


def test_uniform_counts_are_todays_results_bit_for_bit(stream_handle):
    from gpitch_amd.windows import SgprWindowBatch
    h = stream_handle
    N, P, M = 2001, 2, 64
    wins = _ragged_windows([M] * 4, N, P, seed0=5)
    short = _ragged_windows([17, M, 40, 1], N, P, seed0=5)
    tmpl = _model(*wins[0][:3], wins[0][3], 0.3, h)
    pv = np.stack([_params_vector(0.3, w[3]) for w in wins])
    never = SgprWindowBatch(tmpl, 4, N, M, handle=h)
    never.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    b0, g0 = never.evaluate(pv)
    np.testing.assert_array_equal(never.evaluate(pv)[0], b0)        # (captured)
    # every count set to M explicitly
    dev = SgprWindowBatch(tmpl, 4, N, M, handle=h)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    h.check(h.lib.gp_sgprb_set_inducing_counts(dev.plan, (C.c_int32 * 4)(*([M] * 4)), 4))
    b1, g1 = dev.evaluate(pv)
    np.testing.assert_array_equal(b1, b0)
    np.testing.assert_array_equal(g1, g0)
    # ragged, then back to M everywhere
    dev.load([w[0] for w in short], [w[1] for w in short], [w[2] for w in short])
    dev.evaluate(pv)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    for _ in range(2):
        b2, g2 = dev.evaluate(pv)
        np.testing.assert_array_equal(b2, b0)
        np.testing.assert_array_equal(g2, g0)
    # the entry's argument checks
    from gpitch_amd import _lib
    assert h.lib.gp_sgprb_set_inducing_counts(dev.plan, (C.c_int32 * 4)(1, 2, M + 1, 3), 4) == _lib.GP_ERR_BAD_ARG
    assert h.lib.gp_sgprb_set_inducing_counts(dev.plan, (C.c_int32 * 4)(1, 0, 3, 3), 4) == _lib.GP_ERR_BAD_ARG
    assert h.lib.gp_sgprb_set_inducing_counts(dev.plan, (C.c_int32 * 5)(1, 2, 3, 4, 5), 5) == _lib.GP_ERR_BAD_ARG
    with pytest.raises(ValueError):
        dev.load([wins[0][0]], [wins[0][1]], [np.zeros((M + 1, 1))])
    never.close()
    dev.close()
    tmpl._destroy()


@pytest.mark.parametrize("N,P,n_new", [(2001, 2, None), (700, 3, 211)])
def test_ragged_predictions_per_window(gp_handle, N, P, n_new):
    from gpitch_amd.windows import SgprWindowBatch
    wins = _ragged_windows([40, 1, 130, 17, 64], N, P, seed0=7)
    tmpl = _model(*wins[2][:3], wins[2][3], 0.3, gp_handle)
    dev = SgprWindowBatch(tmpl, 5, N, 130, handle=gp_handle)
    dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
    noises = [0.2 + 0.05 * i for i in range(len(wins))]
    pv = np.stack([_params_vector(nz, w[3]) for nz, w in zip(noises, wins)])
    xnews = None
    if n_new is not None:
        xnews = [np.linspace(w[0].min(), w[0].max(), n_new).reshape(-1, 1) for w in wins]
    fm, fv = dev.predict_f(pv, xnews)
    sm, sv = dev.predict_s(pv, xnews, chunk=3)
    for i, w in enumerate(wins):
        xs = w[0] if xnews is None else xnews[i]
        one = _model(w[0], w[1], w[2], w[3], noises[i], gp_handle)
        m1, v1 = one.predict_f(xs)
        np.testing.assert_allclose(fm[i], m1[:, 0], rtol=0, atol=1e-10 * np.abs(m1).max())
        np.testing.assert_allclose(fv[i], v1[:, 0], rtol=0, atol=1e-10 * np.abs(v1).max())
        ms, vs = one.predict_s(xs)
        for k in range(P):
            np.testing.assert_allclose(sm[i, k], ms[k][:, 0], rtol=0, atol=1e-10 * max(np.abs(ms[k]).max(), 1e-12))
            np.testing.assert_allclose(sv[i, k], vs[k][:, 0], rtol=0, atol=1e-10 * np.abs(vs[k]).max())
        one._destroy()
    # the predictions leave the plan usable
    b, _ = dev.evaluate(pv, with_grad=False)
    for i, w in enumerate(wins):
        ref = orc.sgpr_bound(w[0], w[1], w[2], w[3], noises[i])
        assert abs(b[i] - ref) <= 1e-9 * abs(ref)
    dev.close()
    tmpl._destroy()


# ---- the drivers' own input: windowed audio, init_liv inducing inputs -------------------------------------------------
def _audio(nwin, ws=2001, seed=0, noise=0.02):
    """synthetic audio of nwin half-overlapping windows: per_fun notes whose pitch and loudness change per window"""
    from gpitch_amd import synth
    rng = np.random.RandomState(seed)
    hop = (ws - 1) // 2
    n = hop * (nwin + 1) + 1
    x = np.linspace(0, (n - 1) / FS, n).reshape(-1, 1)
    y = np.zeros_like(x)
    for w in range(nwin + 1):
        f0 = 110. * 2 ** (rng.randint(0, 30) / 12.)
        seg = slice(w * hop, min(n, (w + 1) * hop + 1))
        y[seg] += (0.2 + rng.rand()) * synth.per_fun(x[seg], 3, f0)
    y += noise * rng.randn(*y.shape)
    return x, y


def _driver_windows(nwin, dec=3, seed=0, noise=0.02):
    from gpitch_amd import window_overlap
    from gpitch_amd.init_models import init_liv
    x, y = _audio(nwin, seed=seed, noise=noise)
    xs, ys = window_overlap.windowed(x, y, 2001)
    zs = [np.asarray(init_liv(a, b, dec=dec)[0][1][0]) for a, b in zip(xs, ys)]     # the component GP's Z
    return x, y, list(zip(xs, ys, zs))


def _make(data):
    kl = [{"type": "mercer_matern12sm", "variance": 1.0, "lengthscales": 0.05, "energy": [0.6, 0.4],
           "frequency": [220., 440.]},
          {"type": "mercer_matern12sm", "variance": 1.0, "lengthscales": 0.07, "energy": [0.6, 0.4],
           "frequency": [330., 660.]}]

    def make(h):
        return _model(data[0][0], data[0][1], data[0][2], kl, 1.0, h)
    return make


def test_fit_windows_batched_takes_init_liv_windows(gp_handle):
    from gpitch_amd.windows import fit_windows, fit_windows_batched, merge_sources
    x, y, data = _driver_windows(9)
    counts = [w[2].shape[0] for w in data]
    assert len(data) == 9 and len(set(counts)) >= 4 and max(counts) <= 256, counts
    make = _make(data)
    seq = fit_windows(make, data, maxiter=10, num_streams=1)
    bat = fit_windows_batched(make, data, maxiter=10, batch=4, predict=True)
    for i, (a, b) in enumerate(zip(seq, bat)):
        assert "error" not in b and "engine" not in b
        assert b["nfev"] >= 2 and b["nit"] <= 10
        assert abs(a["bound"] - b["bound"]) <= 1e-6 * abs(a["bound"]), (i, counts[i], a["bound"], b["bound"])
        np.testing.assert_allclose(b["variances"], a["variances"], rtol=1e-4)
        assert abs(a["noise"] - b["noise"]) <= 1e-4 * abs(a["noise"])
        assert b["mean"].shape == (2001, 1) and len(b["smean"]) == 2
    assert len({round(b["bound"], 6) for b in bat}) == len(bat)
    src = merge_sources(bat, 2001, x.shape[0])
    assert len(src) == 2
    for m, v in src:
        assert np.all(np.isfinite(m)) and np.all(np.isfinite(v))


def test_a_window_beyond_256_points_goes_to_the_one_window_engine(gp_handle):
    from gpitch_amd.windows import fit_windows, fit_windows_batched
    _, _, data = _driver_windows(3, seed=4)
    _, _, noisy = _driver_windows(1, dec=1, seed=1, noise=0.2)
    big = noisy[0]
    assert big[2].shape[0] > 256
    allw = [data[0], big, data[1], data[2]]
    make = _make(data)
    res = fit_windows_batched(make, allw, maxiter=5, batch=4, predict=True)
    ref = fit_windows(make, [big], maxiter=5, num_streams=1)[0]
    r = res[1]
    assert r["engine"] == "single" and "error" not in r
    assert r["bound"] == ref["bound"] and r["nfev"] == ref["nfev"]
    np.testing.assert_array_equal(r["variances"], ref["variances"])
    assert r["noise"] == ref["noise"]
    assert r["mean"].shape == (2001, 1) and len(r["svar"]) == 2
    for i in (0, 2, 3):
        assert "engine" not in res[i] and np.isfinite(res[i]["bound"]) and "mean" in res[i]
    # the others are the same fits as without the big window
    rest = fit_windows_batched(make, [data[0], data[1], data[2]], maxiter=5, batch=4)
    for i, j in ((0, 0), (2, 1), (3, 2)):
        assert abs(res[i]["bound"] - rest[j]["bound"]) <= 1e-9 * abs(rest[j]["bound"])


def test_a_failing_window_in_a_ragged_batch_is_retired_alone(gp_handle, monkeypatch):
    from gpitch_amd import windows as W
    _, _, data = _driver_windows(6, seed=2)
    counts = [w[2].shape[0] for w in data]
    assert len(set(counts)) >= 3, counts
    make = _make(data)
    groups, _ = W.ragged_batches(counts, 6)
    assert len(groups) == 1
    bad_window = groups[0][1][2]                     # the window in slot 2 of the sorted batch
    clean = W.fit_windows_batched(make, data, maxiter=5, batch=6, inflight=1)
    real_submit = W.SgprWindowBatch.submit

    def bad_submit(self, params_host, with_grad=True):
        p = np.array(params_host, dtype=np.float64, copy=True)
        if not any(np.array_equal(p[2], p[q]) for q in range(len(p)) if q != 2):     # slot 2 on parameters of its own
            p[2, 1] = -3.0                                                            # -> Kuu not positive definite
        return real_submit(self, p, with_grad)
    monkeypatch.setattr(W.SgprWindowBatch, "submit", bad_submit)
    res = W.fit_windows_batched(make, data, maxiter=5, batch=6, inflight=1)
    monkeypatch.setattr(W.SgprWindowBatch, "submit", real_submit)
    assert "error" in res[bad_window] and np.isnan(res[bad_window]["bound"])
    for i in range(len(data)):
        if i == bad_window:
            continue
        assert "error" not in res[i]
        assert res[i]["bound"] == clean[i]["bound"] and res[i]["nfev"] == clean[i]["nfev"]
        np.testing.assert_array_equal(res[i]["params"], clean[i]["params"])
    gp_handle.check(gp_handle.lib.gp_check_not_pd(gp_handle.h))
