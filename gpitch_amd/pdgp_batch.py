"""Many small, independent Pdgp models trained together: one launch sequence per Adam step for all of them
(csrc/pdgp_batch.hip through gp_pdgpb_*).

    results = optimize_many(models, method=AdamOptimizer(0.0025), maxiter=1000)

replaces  for m in models: m.optimize(method=AdamOptimizer(0.0025), maxiter=1000)  — the per-note training behind
init_kernel_with_trained_models (gpitch/init_models.py:74-121) and the segments of a long recording — and leaves every
model as that loop would: parameters, Adam step count and moments, and the minibatch generators advanced by the same
draws (GPflow's final fresh-minibatch fun / jac evaluation included).  Whitened float64 unsharded models, Adam only;
everything else is refused by check_batchable() before any device work.
"""
import ctypes as C

import numpy as np

from . import _lib
from .methods import nlin_code
from .param import sorted_params
from .train import AdamOptimizer, OptimizeResult

MAX_M = 128            # inducing points per latent GP (one factor of 128 x 128 float64 in a workgroup's LDS)
MAX_MINIBATCH = 1024   # frames per model and step
MAX_PARTIALS = 32
_KERNELS = {_lib.KERN_MATERN12: "Matern12", _lib.KERN_MATERN32: "Matern32", _lib.KERN_MATERN52: "Matern52",
            _lib.KERN_RBF: "RBF", _lib.KERN_MERCER_MATERN12SM: "MercerMatern12sm", _lib.KERN_MATERN32SM: "Matern32sm"}
_SINGLE = "train this model on its own with Pdgp.optimize"


def check_batchable(models, method=None, callback=None):
    """Host-only scope check of optimize_many / PdgpBatch: raises NotImplementedError (a feature the batch does not
    have) or ValueError (a shape it does not take) naming the single-model path.  No device work."""
    from .pdgp import Pdgp
    if method is not None and not isinstance(method, AdamOptimizer):
        raise NotImplementedError("optimize_many trains with AdamOptimizer only (got %r); %s" % (method, _SINGLE))
    if callback is not None:
        raise NotImplementedError("optimize_many takes no callback; %s" % _SINGLE)
    models = list(models)
    if not models:
        raise ValueError("optimize_many needs at least one model")
    if len(set(id(m) for m in models)) != len(models):
        raise ValueError("optimize_many: the same model appears twice in the list")
    for k, m in enumerate(models):
        if not isinstance(m, Pdgp):
            raise ValueError("optimize_many: item %d is not a Pdgp" % k)
        if not m.whiten:
            raise NotImplementedError("model %d: whiten=False is not batched; %s" % (k, _SINGLE))
        if m._bits != 64:
            raise NotImplementedError("model %d: float_type %r is not batched (float64 only); %s" % (k, m._bits, _SINGLE))
        if m._shard is not None:
            raise NotImplementedError("model %d: sharded models are not batched; %s" % (k, _SINGLE))
        nlin_code(m.nlinfun)
        if m.minibatch_size > MAX_MINIBATCH or min(m.minibatch_size, m.num_data) > MAX_MINIBATCH:
            raise ValueError("model %d: minibatch of %d frames > %d; %s" % (k, m.minibatch_size, MAX_MINIBATCH, _SINGLE))
        for kern, M in [(m.kern_act[i], m.num_inducing_a[i]) for i in range(m.num_sources)] + \
                       [(m.kern_com[i], m.num_inducing_c[i]) for i in range(m.num_sources)]:
            if M > MAX_M:
                raise ValueError("model %d: %d inducing points in one latent GP > %d; %s" % (k, M, MAX_M, _SINGLE))
            t = getattr(kern, "type_code", None)
            if t not in _KERNELS:
                raise NotImplementedError("model %d: kernel %s is not batched (takes %s); %s"
                                          % (k, type(kern).__name__, ", ".join(sorted(_KERNELS.values())), _SINGLE))
            mp = int(kern.num_partials)
            if t in (_lib.KERN_MERCER_MATERN12SM, _lib.KERN_MATERN32SM) and not 1 <= mp <= MAX_PARTIALS:
                raise ValueError("model %d: %d partials outside 1..%d; %s" % (k, mp, MAX_PARTIALS, _SINGLE))
    return models


def _gps(m):
    """latent GPs in the plan's order: [g_0..g_{P-1}, f_0..f_{P-1}] (Pdgp._gps of an unsharded model)"""
    P = m.num_sources
    return ([(m.kern_act[i], m.za[i], m.q_mu_act[i], m.q_sqrt_act[i]) for i in range(P)] +
            [(m.kern_com[i], m.zc[i], m.q_mu_com[i], m.q_sqrt_com[i]) for i in range(P)])


def model_segments(m, base=0):
    """[(offset, Param)] of one model's block of the batch's parameter vector (include/gpitch_abi.h gp_pdgpb_config):
    [noise | per latent GP: theta | z | q_mu | q_sqrt], starting at `base`; also returns the block's length"""
    segs = [(base, m.likelihood.variance)]
    off = base + 1
    for kern, z, q_mu, q_sqrt in _gps(m):
        for j, p in enumerate(kern.theta_params()):
            segs.append((off + j, p))
        off += 2 + 2 * int(kern.num_partials)
        M = z.size
        segs += [(off, z), (off + M, q_mu), (off + 2 * M, q_sqrt)]
        off += 2 * M + M * M
    return segs, off - base


def free_index(m, segs):
    """entries of the batch vector that make up the model's GPflow free state, in GPflow's order (param.sorted_params:
    Params by attribute name, `.fixed` ones absent) — the order of Pdgp._objective / optimize's `x` and `jac`"""
    off = {id(p): o for o, p in segs}
    idx = [np.arange(off[id(p)], off[id(p)] + p.size) for p in sorted_params(m) if not p.fixed and id(p) in off]
    return np.concatenate(idx) if idx else np.zeros(0, dtype=np.int64)


def draw_indices(m, steps):
    """the next `steps` minibatches of model m exactly as Pdgp._batch draws them (sorted in time order), advancing
    m.x / m.y the same way; a (steps, B) int64 array.  A model whose minibatch covers its data draws nothing (_batch).
    With replacement (minibatch / N < 0.5) the steps are drawn as one block: randint(N, size=(k, B)) yields the stream
    and leaves the state of k single draws.  The permutation branch is drawn step by step."""
    N, B = m.num_data, m.minibatch_size
    if m.x.minibatch_size >= N and m.y.minibatch_size >= N:
        return np.tile(np.arange(N, dtype=np.int64), (steps, 1))
    rng = m.x.rng
    if float(m.x.minibatch_size) / float(N) < 0.5 and steps > 0:
        idx = rng.randint(N, size=(steps, m.x.minibatch_size))
    else:
        idx = np.stack([m.x.next_indices() for _ in range(steps)]) if steps else np.zeros((0, B), dtype=np.int64)
    if m.y.rng is not rng:
        if hasattr(rng, "get_state") and hasattr(m.y.rng, "set_state"):
            m.y.rng.set_state(rng.get_state())
        else:
            for _ in range(steps):
                m.y.next_indices()
    return np.sort(idx, axis=1, kind="stable")


def _describe_not_pd(code):
    """gp_pdgpb_not_pd's per-model word (1 + 128 row + pivot) as text"""
    row, pivot = divmod(int(code) - 1, MAX_M)
    return "latent GP row %d of [g_0..g_{P-1}, f_0..f_{P-1}], pivot %d" % (row, pivot)


class PdgpBatch(object):
    """The plan behind optimize_many: every model's parameters in one device vector, one gp_pdgpb plan sized by the
    batch's own shapes (no single-model engine plan is built)."""

    def __init__(self, models, handle=None):
        self.models = check_batchable(models)
        h = self._handle = handle or _lib.default_handle()
        self._segs, self._free_idx, self._range = [], [], []
        base = 0
        for m in self.models:
            segs, n = model_segments(m, base)
            self._segs.append(segs)
            self._range.append((base, base + n))
            base += n
        self.num_params = base
        i32 = C.c_int32
        gps = [g for m in self.models for g in _gps(m)]
        nm = len(self.models)
        self._cfg_keep = dict(
            P=(i32 * nm)(*[m.num_sources for m in self.models]),
            B=(i32 * nm)(*[min(m.minibatch_size, m.num_data) for m in self.models]),
            nlin=(i32 * nm)(*[nlin_code(m.nlinfun) for m in self.models]),
            N=(C.c_double * nm)(*[float(m.num_data) for m in self.models]),
            M=(i32 * len(gps))(*[g[1].size for g in gps]),
            kt=(i32 * len(gps))(*[g[0].type_code for g in gps]),
            mp=(i32 * len(gps))(*[int(g[0].num_partials) for g in gps]))
        k = self._cfg_keep
        from .pdgp import jitter
        cfg = _lib.PdgpBatchConfig(nm, k["P"], k["B"], k["nlin"], k["N"], k["M"], k["kt"], k["mp"], jitter)
        plan = C.c_void_p()
        h.check(h.lib.gp_pdgpb_create(h.h, C.byref(cfg), C.byref(plan)))
        self._plan = plan
        if int(h.lib.gp_pdgpb_num_params(plan)) != self.num_params:
            raise RuntimeError("gp_pdgpb layout disagrees with the host layout")
        self._ws = h.workspace(h.lib.gp_pdgpb_workspace_bytes(plan))
        h.check(h.lib.gp_pdgpb_set_workspace(plan, self._ws.data_ptr(), self._ws.numel()))
        self._batch_off = np.concatenate([[0], np.cumsum([min(m.minibatch_size, m.num_data) for m in self.models])])
        self._data_off = np.concatenate([[0], np.cumsum([m.num_data for m in self.models])])
        self._x = h.to_device(np.concatenate([m.x._array.reshape(-1) for m in self.models]))
        self._y = h.to_device(np.concatenate([m.y._array.reshape(-1) for m in self.models]))
        n = self.num_params
        self._params, self._free, self._grad = h.zeros(n), h.zeros(n), h.zeros(n)
        self._adam_m, self._adam_v = h.zeros(n), h.zeros(n)
        self._elbo = h.zeros(nm)
        self._tcode = h.torch.zeros(n, dtype=h.torch.uint8, device=h.device)

    # ------------------------------------------------------------------------------------------
    def _pack(self):
        """host Params -> device parameter vector, transform codes and free state; the free-state index and the
        gradients the backward pass skips follow the models' current `.fixed` flags"""
        h = self._handle
        self._free_idx = [free_index(m, segs) for m, segs in zip(self.models, self._segs)]
        g = 0
        for m in self.models:
            for kern, z, _, _ in _gps(m):
                need_theta = any(not p.fixed for p in kern.theta_params())
                h.check(h.lib.gp_pdgpb_set_grad_needs(self._plan, g, int(need_theta), int(not z.fixed)))
                g += 1
        host = np.zeros(self.num_params)
        tc = np.full(self.num_params, 2, dtype=np.uint8)
        for segs in self._segs:
            for off, p in segs:
                v = p.value.reshape(-1)
                host[off:off + v.size] = v
                tc[off:off + v.size] = 2 if p.fixed else p.transform.device_code(h)
        self._params.copy_(h.torch.as_tensor(host))
        self._tcode.copy_(h.torch.as_tensor(tc))
        h.check(h.lib.gp_transform_backward(h.h, self._params.data_ptr(), self._tcode.data_ptr(), self.num_params,
                                            self._free.data_ptr()))

    def _load_moments(self):
        """each model's Adam moments as its own optimize() would continue from them"""
        mom = np.zeros((2, self.num_params))
        for m, segs in zip(self.models, self._segs):
            state = m._adam_state()           # one (m, v) per Param, in the order of model_segments
            if state is None:
                continue
            for (off, p), (mv, vv) in zip(segs, state):
                mom[0, off:off + p.size] = mv
                mom[1, off:off + p.size] = vv
        t = self._handle.torch
        self._adam_m.copy_(t.as_tensor(mom[0]))
        self._adam_v.copy_(t.as_tensor(mom[1]))

    def _indices(self, draws):
        """per-model (steps, B) draws -> (steps, sum B) int32 indices into the concatenated frames"""
        cols = [d + self._data_off[k] for k, d in enumerate(draws)]
        return np.ascontiguousarray(np.concatenate(cols, axis=1).astype(np.int32))

    def _jac(self, k, free_host, grad_host):
        """-(d ELBO / d free state) of model k in GPflow's order (Pdgp._objective's chain rule)"""
        scale = np.zeros(self.num_params)
        for off, p in self._segs[k]:
            if not p.fixed:
                scale[off:off + p.size] = p.transform.dforward(free_host[off:off + p.size])
        idx = self._free_idx[k]
        return -(grad_host * scale)[idx]

    def _evaluate(self, draws):
        h = self._handle
        idx = h.torch.as_tensor(self._indices(draws)).to(h.device)
        h.check(h.lib.gp_pdgpb_objective(self._plan, self._params.data_ptr(), self._x.data_ptr(), self._y.data_ptr(),
                                         idx.data_ptr(), self._elbo.data_ptr(), self._grad.data_ptr()))
        return self._elbo.cpu().numpy(), self._grad.cpu().numpy()

    def not_pd(self, clear=True):
        """per model: 0, or 1 + 128 row + pivot of its failed Cholesky with the smallest (latent GP row, pivot)"""
        out = (C.c_int32 * len(self.models))()
        h = self._handle
        h.check(h.lib.gp_pdgpb_not_pd(self._plan, out, int(bool(clear))))
        return np.array(out[:], dtype=np.int64)

    def objective_many(self):
        """every model's (-ELBO, -gradient over its free state) on a fresh minibatch of its own, as Pdgp._objective at
        the models' current Params (same draws, same free-state order)"""
        self._pack()
        draws = [draw_indices(m, 1) for m in self.models]
        elbo, grad = self._evaluate(draws)
        free = self._free.cpu().numpy()
        bad = self.not_pd()
        out = []
        for k, m in enumerate(self.models):
            if bad[k]:
                raise _lib.NotPositiveDefiniteError(_lib.GP_ERR_NOT_PD, "model %d: Cholesky failed: %s"
                                                    % (k, _describe_not_pd(bad[k])))
            out.append((-float(elbo[k]), self._jac(k, free, grad)))
        return out

    def optimize(self, method, maxiter=1000, chunk=64):
        """`maxiter` Adam steps of every model (see optimize_many)"""
        check_batchable(self.models, method)
        h = self._handle
        self._pack()
        self._load_moments()
        self.not_pd(clear=True)
        nm = len(self.models)
        rng_keep = [(m.x.rng.get_state() if hasattr(m.x.rng, "get_state") else None,
                     m.y.rng.get_state() if hasattr(m.y.rng, "get_state") else None) for m in self.models]
        t0 = [m._adam_t for m in self.models]
        keep = []
        done = 0
        while done < maxiter:
            k = min(chunk, maxiter - done)
            idx = h.torch.as_tensor(self._indices([draw_indices(m, k) for m in self.models])).to(h.device)
            lr = np.empty((k, nm))
            for s in range(k):
                for j in range(nm):
                    t = t0[j] + done + s + 1
                    lr[s, j] = method.learning_rate * np.sqrt(1. - method.beta2 ** t) / (1. - method.beta1 ** t)
            lr_dev = h.torch.as_tensor(lr.reshape(-1)).to(h.device)
            keep.append((idx, lr_dev))
            h.check(h.lib.gp_pdgpb_adam(self._plan, self._free.data_ptr(), self._params.data_ptr(), self._tcode.data_ptr(),
                                        self._adam_m.data_ptr(), self._adam_v.data_ptr(), self._x.data_ptr(),
                                        self._y.data_ptr(), idx.data_ptr(), k, lr_dev.data_ptr(), method.beta1,
                                        method.beta2, method.epsilon))
            done += k
        bad = self.not_pd(clear=True)
        # GPflow evaluates the returned fun / jac on a fresh minibatch (Pdgp.optimize)
        draws = [draw_indices(m, 1) for m in self.models]
        elbo, grad = self._evaluate(draws)
        final_bad = self.not_pd(clear=True)     # a failure in the final evaluation voids that model's fun / jac
        bad = np.where(bad != 0, bad, final_bad)
        h.sync()
        del keep
        free = self._free.cpu().numpy()
        params = self._params.cpu().numpy()
        mom_m, mom_v = self._adam_m.cpu().numpy(), self._adam_v.cpu().numpy()
        results = []
        for k, m in enumerate(self.models):
            if bad[k]:
                # frozen since its failed step: the model keeps its Params, Adam state and generators
                xs, ys = rng_keep[k]
                if xs is not None:
                    m.x.rng.set_state(xs)
                if ys is not None:
                    m.y.rng.set_state(ys)
                msg = "Cholesky failed: %s" % _describe_not_pd(bad[k])
                results.append(OptimizeResult(fun=None, jac=None, x=None, success=False, status="error", message=msg,
                                              error=_lib.NotPositiveDefiniteError(_lib.GP_ERR_NOT_PD, msg)))
                continue
            idx = self._free_idx[k]
            for off, p in self._segs[k]:
                p.value = params[off:off + p.size]
            m._adam_t = t0[k] + maxiter
            m._set_adam_state([(mom_m[off:off + p.size].copy(), mom_v[off:off + p.size].copy())
                               for off, p in self._segs[k]])
            m._invalidate_device_state()
            results.append(OptimizeResult(fun=-float(elbo[k]), jac=self._jac(k, free, grad), x=free[idx].copy(),
                                          message='Finished iterations.', status='Finished iterations.', success=True))
        return results

    def __del__(self):
        try:
            if self._plan is not None and self._handle is not None and self._handle.h:
                self._handle.sync()
                self._handle.lib.gp_pdgpb_destroy(self._plan)
        except Exception:
            pass


def optimize_many(models, method=None, maxiter=1000, callback=None):
    """Train every model in `models` (ordinary Pdgp objects) as  m.optimize(method=method, maxiter=maxiter)  would, all
    of them together: one OptimizeResult per model.  A model whose Cholesky fails is frozen and its result carries
    `error`; the others go on.  method: an AdamOptimizer token shared by all models (default AdamOptimizer())."""
    method = AdamOptimizer() if method is None else method
    models = check_batchable(models, method, callback)
    return PdgpBatch(models).optimize(method, maxiter)
