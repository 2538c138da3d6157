"""Every caller-allocated workspace at exactly the size its *_workspace_bytes function returns: (a) nothing outside it is
written (64 KiB guard bands of a fixed byte on both sides), (b) the results equal those with a workspace twice as large,
(c) one 256-byte granule less is refused with GP_ERR_WORKSPACE before anything is launched (the whole allocation keeps
its fill byte).  The models allocate through Handle.workspace, which is replaced here by an allocator that hands out
the 256-byte aligned interior of a filled tensor with numel() == the requested size.

Covered: Pdgp (whitened / unwhitened x float64 / float32 / mixed, a Q-route plan with its far field, and a gp_pdgp_create_subset plan), SGPR (M = 64 and the
blocked factorisation at M = 320, float64 / float32, predict_source), the window batch (ragged counts, predict_f,
predict_source in chunks of 2), a PdgpBatch training plan, and the handle-free conditionals / KL / Kuu factorisation with a
32-partial Mercer kernel at N = 8 and 300, and a prediction-only PdgpBatch plan (predict, predict_moments)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GUARD = 64 * 1024
FILL = 0xA5


class _Guarded(object):
    def __init__(self, h, mode):
        self.h, self.mode, self.bufs = h, mode, []

    def __call__(self, nbytes):
        t = self.h.torch
        nbytes = int(nbytes)
        size = {"exact": nbytes, "double": 2 * nbytes, "short": max(nbytes - 256, 0)}[self.mode]
        buf = t.full((size + 2 * GUARD + 256,), FILL, dtype=t.uint8, device=self.h.device)
        off = GUARD + (-(buf.data_ptr() + GUARD)) % 256
        self.bufs.append((buf, off, size))
        return buf[off:off + size]

    def guards_hold(self):
        return all(bool((b[:o] == FILL).all()) and bool((b[o + s:] == FILL).all()) for b, o, s in self.bufs)

    def untouched(self):
        return all(bool((b == FILL).all()) for b, _, _ in self.bufs)


def _check(h, monkeypatch, run, exact_keys=(), short_untouched=True):
    """run() -> dict of arrays / floats, allocating through Handle.workspace.  short_untouched=False: a legal earlier
    call of run() writes to the short workspace before the refused one (guard bands only)"""
    from gpitch_amd import _lib
    out = {}
    for mode in ("exact", "double"):
        g = _Guarded(h, mode)
        monkeypatch.setattr(_lib.Handle, "workspace", lambda self, n, g=g: g(n))
        out[mode] = run()
        h.sync()
        assert g.bufs and g.guards_hold(), mode
    for k, ref in out["double"].items():
        got, ref = np.asarray(out["exact"][k]), np.asarray(ref)
        if k in exact_keys:
            assert np.array_equal(got, ref), k
        else:
            # the buffers keep their offsets whatever the size, so 1e-10 of the largest entry serves every call: tighter
            # than the 2e-7 ... 1e-8 the calls' own tests allow against the oracle, and not to be widened to those
            np.testing.assert_allclose(got, ref, rtol=0, atol=1e-10 * max(np.abs(ref).max(), 1e-300), err_msg=k)
    g = _Guarded(h, "short")
    monkeypatch.setattr(_lib.Handle, "workspace", lambda self, n, g=g: g(n))
    with pytest.raises(_lib.GpitchError) as e:
        run()
    h.sync()
    assert e.value.status == _lib.GP_ERR_WORKSPACE
    assert g.untouched() if short_untouched else g.guards_hold()


def _pdgp_problem():
    from gpitch_amd.synth import make_problem, uniform_inducing
    prob = make_problem(300, 64, 2, num_partials=3, seed=3)
    rq = np.random.RandomState(11)
    prob["zc"] = [uniform_inducing(prob["x"], 96) for _ in range(2)]
    prob["q_mu_com"] = [0.3 * rq.randn(96, 1) for _ in range(2)]
    prob["q_sqrt_com"] = [np.tril(np.eye(96) + 0.05 * rq.randn(96, 96))[:, :, None].copy() for _ in range(2)]
    prob["kern_act"][1], prob["kern_com"][0] = dict(prob["kern_com"][1]), dict(prob["kern_act"][0])   # one of each per role
    return prob


@pytest.mark.parametrize("float_type", [None, np.float32, (np.float64, np.float32)], ids=["f64", "f32", "mixed"])
@pytest.mark.parametrize("whiten", [True, False])
def test_pdgp_workspace(gp_handle, monkeypatch, whiten, float_type):
    from helpers import pdgp_from_problem
    prob = _pdgp_problem()

    def run():
        m = pdgp_from_problem(prob, whiten=whiten, handle=gp_handle, float_type=float_type)
        m._pack()
        return {"elbo": m._elbo(True), "grad": m._grad.cpu().numpy().copy()}
    _check(gp_handle, monkeypatch, run, exact_keys=("elbo",))


def test_pdgp_q_route_far_field_workspace(gp_handle, monkeypatch):
    """a plan whose components take the Q route with its far field forward and backward: the carve of T, Psi,
    CnF, CFF, cn, cF, Um / Vp, Wv, rng2 and tS between the guard bands and at its exact size, with ranges that differ per GP"""
    import test_gpu_qfar as tq
    from helpers import pdgp_from_problem
    prob = tq._problem(N=1024, M=128, P=2, ls=[8, 25])
    assert [r[:2] for r in tq._ranges(prob, 0)] != [r[:2] for r in tq._ranges(prob, 1)]

    def run():
        m = pdgp_from_problem(prob, handle=gp_handle)
        m.za.fixed = True
        m.zc.fixed = True
        m._pack()
        out = {"elbo": m._elbo(True), "grad": m._grad.cpu().numpy().copy()}
        assert int(gp_handle.lib.gp_pdgp_far_field(m._plan)) == 1 and int(gp_handle.lib.gp_pdgp_far_field_backward(m._plan)) == 1
        tq.assert_device_ranges(gp_handle, m, prob, 1, 1)
        return out
    _check(gp_handle, monkeypatch, run, exact_keys=("elbo",))


def test_pdgp_subset_plan_workspace(gp_handle, monkeypatch):
    from helpers import pdgp_from_problem
    prob = _pdgp_problem()

    def run():
        m = pdgp_from_problem(prob, handle=gp_handle, shard=("gp", 1, 2))
        m._pack()
        return {"send": m._gp_begin(True).cpu().numpy().copy(), "grad": m._grad.cpu().numpy().copy()}
    _check(gp_handle, monkeypatch, run)


@pytest.mark.parametrize("float_type", [None, np.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("M", [64, 320])
def test_sgpr_workspace(gp_handle, monkeypatch, M, float_type):
    from test_gpu_sgpr import _model, _problem
    X, Y, Z, kl = _problem(500, M, 2, 5)

    def run():
        m = _model(X, Y, Z, kl, 0.3, gp_handle, float_type=float_type)
        m._compile()
        m._pack()
        g = gp_handle.zeros(m._nparams)
        out = {"bound": m._bound(grad=g), "grad": g.cpu().numpy().copy()}
        if M == 64 and float_type is None:
            sm, sv = m.predict_s(X[::5])
            out["smean"], out["svar"] = np.stack(sm), np.stack(sv)
        m._destroy()
        return out
    _check(gp_handle, monkeypatch, run, exact_keys=("bound",))


def test_window_batch_workspace(gp_handle, monkeypatch):
    from gpitch_amd.windows import SgprWindowBatch
    from test_gpu_windows_ragged import _model, _params_vector, _ragged_windows
    N = 257
    wins = _ragged_windows([40, 64, 17], N, 3, seed0=7)
    pv = np.stack([_params_vector(0.2 + 0.05 * i, w[3]) for i, w in enumerate(wins)])
    xnews = [np.linspace(w[0].min(), w[0].max(), 100).reshape(-1, 1) for w in wins]

    def run():
        tmpl = _model(*wins[1][:3], wins[1][3], 0.3, gp_handle)
        dev = SgprWindowBatch(tmpl, 3, N, 64, handle=gp_handle)
        try:
            dev.load([w[0] for w in wins], [w[1] for w in wins], [w[2] for w in wins])
            b, g = dev.evaluate(pv, with_grad=True)
            fm, fv = dev.predict_f(pv, xnews)
            sm, sv = dev.predict_s(pv, xnews, chunk=2)
            return {"bound": np.array(b), "grad": np.array(g), "fm": fm, "fv": fv, "sm": sm, "sv": sv}
        finally:
            dev.close()
            tmpl._destroy()
    _check(gp_handle, monkeypatch, run, exact_keys=("bound",))


def test_pdgp_batch_training_workspace(gp_handle, monkeypatch):
    from gpitch_amd.pdgp_batch import PdgpBatch
    from gpitch_amd.synth import make_problem
    from helpers import pdgp_from_problem
    probs = [make_problem(64, M, 2, num_partials=2, seed=M) for M in (16, 32)]

    def run():
        res = PdgpBatch([pdgp_from_problem(p, handle=gp_handle) for p in probs], handle=gp_handle).objective_many()
        return {"f": np.array([r[0] for r in res]), "g": np.concatenate([np.ravel(r[1]) for r in res])}
    _check(gp_handle, monkeypatch, run, exact_keys=("f",))


@pytest.mark.parametrize("moments", [False, True], ids=["predict", "predict_moments"])
def test_pdgp_batch_predict_only_workspace(gp_handle, monkeypatch, moments):
    from gpitch_amd.pdgp_batch import predict_many, predict_sources_many
    from gpitch_amd.synth import make_problem
    from helpers import pdgp_from_problem
    probs = [make_problem(64, M, 2, num_partials=2, seed=M) for M in (16, 32)]
    models = [pdgp_from_problem(p, handle=gp_handle) for p in probs]
    xnews = [p["x"][:50] + 1e-5 for p in probs]
    ynews = [p["y"][:50] for p in probs]

    def run():
        if moments:
            res = predict_sources_many(models, xnews, ynews)
            return {"%s%d" % (name, k): np.asarray(r[name]) for k, r in enumerate(res) for name in r}
        return {"%d.%d" % (k, j): np.asarray(a) for k, r in enumerate(predict_many(models, xnews)) for j, a in enumerate(r)}
    # one granule short of predict_moments' size still holds gp_pdgpb_predict_prepare's regions: that call runs, the
    # moments call behind it is the one refused
    _check(gp_handle, monkeypatch, run, short_untouched=not moments)


def _mercer32():
    from gpitch_amd.matern12_spectral_mixture import MercerMatern12sm
    return MercerMatern12sm(1, energy=np.full(32, 1. / 32), frequency=110. * np.arange(1, 33), variance=1.0, lengthscales=0.1)


@pytest.mark.parametrize("N", [8, 300])
@pytest.mark.parametrize("call", ["diag", "diag_f32w", "full"])
@pytest.mark.parametrize("whiten", [True, False])
def test_handle_free_conditional_workspace(monkeypatch, call, whiten, N):
    from gpitch_amd import _lib
    from gpitch_amd.conditionals import conditional
    h = _lib.default_handle()
    rng = np.random.RandomState(N)
    M = 64
    x = np.linspace(0., (N - 1) / 16000., N).reshape(-1, 1)
    z = np.linspace(0., 299 / 16000., M).reshape(-1, 1) + 1e-5
    f, q = 0.3 * rng.randn(M, 1), np.tril(np.eye(M) + 0.05 * rng.randn(M, M))
    kern = _mercer32()

    def run():
        fm, fv = conditional(x, z, kern, f, full_cov=(call == "full"), q_sqrt=q, whiten=whiten,
                             float_type=np.float32 if call == "diag_f32w" else None)
        return {"mean": fm, "var": fv}
    _check(h, monkeypatch, run)


@pytest.mark.parametrize("N", [8, 300])
def test_handle_free_conditional_diag_f32_workspace(monkeypatch, N):
    """gp_conditional_diag_f32 (the whitened float32 form without a `whiten` argument), which conditional() does not call"""
    from gpitch_amd import _lib
    from gpitch_amd.conditionals import _kdesc
    h = _lib.default_handle()
    rng = np.random.RandomState(N)
    M = 64
    x = np.linspace(0., (N - 1) / 16000., N).reshape(-1, 1)
    z = np.linspace(0., 299 / 16000., M).reshape(-1, 1) + 1e-5
    f, q = 0.3 * rng.randn(M, 1), np.tril(np.eye(M) + 0.05 * rng.randn(M, M))
    kern = _mercer32()

    def run():
        d, th = _kdesc(h, kern)
        dx, dz, dmu, dq = h.to_device(x), h.to_device(z), h.to_device(f), h.to_device(q)
        fm, fv = h.empty(N), h.empty(N)
        ws = h.workspace(h.lib.gp_conditional_workspace_bytes(N, M))
        h.check(h.lib.gp_conditional_diag_f32(h.h, C.byref(d), dx.data_ptr(), N, dz.data_ptr(), M, dmu.data_ptr(),
                                              dq.data_ptr(), 1e-6, fm.data_ptr(), fv.data_ptr(), ws.data_ptr(), ws.numel()))
        return {"mean": fm.cpu().numpy(), "var": fv.cpu().numpy()}
    _check(h, monkeypatch, run)


def test_handle_free_kl_and_kuu_cholesky_workspace(monkeypatch):
    from gpitch_amd import _lib
    from gpitch_amd.conditionals import _kdesc, gauss_kl
    h = _lib.default_handle()
    rng = np.random.RandomState(2)
    M = 64
    z = np.linspace(0., 299 / 16000., M).reshape(-1, 1)
    mu, q = 0.3 * rng.randn(M, 1), np.tril(np.eye(M) + 0.05 * rng.randn(M, M))
    kern = _mercer32()
    K = np.exp(-np.abs(z - z.T) / 0.01) + 1e-6 * np.eye(M)
    _check(h, monkeypatch, lambda: {"kl": gauss_kl(mu, q)})
    _check(h, monkeypatch, lambda: {"kl": gauss_kl(mu, q, K)})

    def kl_kernel():
        d, th = _kdesc(h, kern)
        out = C.c_double()
        dmu, dq, dz = h.to_device(mu), h.to_device(q), h.to_device(z)
        ws = h.workspace(h.lib.gp_gauss_kl_workspace_bytes(M, 1))
        h.check(h.lib.gp_gauss_kl(h.h, dmu.data_ptr(), dq.data_ptr(), M, C.byref(d), dz.data_ptr(), 1e-6, C.byref(out),
                                  ws.data_ptr(), ws.numel()))
        return {"kl": out.value}
    _check(h, monkeypatch, kl_kernel)

    def chol():
        d, th = _kdesc(h, kern)
        dz, L, W = h.to_device(z), h.zeros(M, M), h.zeros(M, M)
        ws = h.workspace(h.lib.gp_chol_workspace_bytes(M))
        h.check(h.lib.gp_kuu_cholesky(h.h, C.byref(d), dz.data_ptr(), M, 1e-6, L.data_ptr(), W.data_ptr(), ws.data_ptr(),
                                      ws.numel()))
        return {"L": L.cpu().numpy(), "W": W.cpu().numpy()}
    _check(h, monkeypatch, chol)
