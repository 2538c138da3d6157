"""Many-window SGPRSS fitting — the loop of AMT.optimize / SoSp.optimize (gpitch/transcription.py:265-288,
gpitch/separation.py:279-313) with the windows of one GPU spread over several HIP streams.

The reference fits its windows (ws = 2001 frames, 50 % overlap: window_overlap.py:7-16) one after another; each
L-BFGS-B evaluation is a few dozen small kernels, so one window cannot fill an MI355X.  Here `num_streams` worker
threads each own a HIP stream, a library handle and ONE model whose engine plan and workspace are reused for every
window they draw (the data holders are swapped, as transcription.py:253-263 does); kernels of different windows
overlap on the device.  Across GPUs the windows are dealt round-robin (dist.window_assignment); there is no
exchange between windows.
"""
import threading

import numpy as np

from . import sgpr_ss


def default_reset(model, x, y, z):
    """AMT.reset_model (transcription.py:253-263): new data, unit noise and kernel variances.  (The reference
    also scales y by 20 there and resets the lengthscales from its params file: callers do that in `reset`.)"""
    model.X = x
    model.Y = y
    model.Z = z
    model.likelihood.variance = 1.
    for k in model.kern.kern_list:
        k.variance = 1.


def fit_windows(make_model, windows, maxiter=10, num_streams=4, reset=default_reset, after_fit=None,
                method='L-BFGS-B', rank=0, world_size=1, carry_kernel_state=False):
    """Fit every window (x_i, y_i, z_i) in `windows` with its own L-BFGS-B run.

    carry_kernel_state=False: every window starts from the parameter values the model was built with, so the
    result does not depend on which worker fitted which window.  The reference never resets the energies and
    frequencies of its kernels between windows (they are trainable, matern12_spectral_mixture.py:86-94, and
    reset_model only touches variances / lengthscales), so there each window starts from the previous window's
    optimum: carry_kernel_state=True with num_streams=1 reproduces that sequential drift.

    make_model(handle) -> SGPRSS   built once per worker (any window's data; it is replaced by `reset`)
    reset(model, x, y, z)          puts a window into the model (default: AMT.reset_model)
    after_fit(model, index) -> obj what to keep per window (default: bound, nfev and the kernel variances, the
                                   piano-roll entries of transcription.py:286-288)
    Returns a list over windows (None for windows owned by other ranks)."""
    import torch
    from . import _lib
    from .dist import window_assignment
    mine = window_assignment(len(windows), world_size, rank)
    results = [None] * len(windows)
    lock = threading.Lock()
    cursor = [0]
    errors = []
    dev = _lib.default_handle().device      # also loads the library / binds the device in the main thread

    def keep(model, idx, res):
        if after_fit is not None:
            return after_fit(model, idx)
        return {"bound": -float(res.fun), "nfev": int(res.nfev),
                "variances": np.array([k.variance.value[0] for k in model.kern.kern_list]),
                "noise": float(model.likelihood.variance.value[0])}

    def worker():
        try:
            torch.cuda.set_device(dev)
            s = torch.cuda.Stream(device=dev)
            with torch.cuda.stream(s):
                h = _lib.Handle(dev.index, stream=s)
                model = make_model(h)
                params0 = [p.value.copy() for p in model._param_list()]
                while True:
                    with lock:
                        if cursor[0] >= len(mine):
                            break
                        idx = mine[cursor[0]]
                        cursor[0] += 1
                    x, y, z = windows[idx][:3]
                    if not carry_kernel_state:
                        for p, v in zip(model._param_list(), params0):
                            p.value = v
                    reset(model, x, y, z)
                    res = model.optimize(method=method, maxiter=maxiter)
                    results[idx] = keep(model, idx, res)
                model._destroy()
                s.synchronize()
                h.close()
        except Exception as e:     # surfaced to the caller below
            errors.append(e)

    n = max(1, min(int(num_streams), len(mine) or 1))
    threads = [threading.Thread(target=worker) for _ in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise errors[0]
    return results


# ----------------------------------------------------------------------------------------------------------------
# device-batched form: W windows per launch sequence (include/gpitch_abi.h gp_sgprb_*), scipy's L-BFGS-B per window
# driven in reverse communication (lbfgsb_batch.py)
class SgprWindowBatch(object):
    """Device side of a batch of W SGPRSS windows that share N and the kernel structure of `template` (an SGPRSS):
    bound and gradient of all of them from one launch sequence.  M is the largest inducing-point count a window may
    have; a window with fewer is padded exactly (gp_sgprb_set_inducing_counts)."""

    def __init__(self, template, num_windows, N, M, handle=None):
        import ctypes as C
        from . import _lib
        self.h = h = handle or template._handle or _lib.default_handle()
        kl = template.kern.kern_list
        P = len(kl)
        i32 = C.c_int32 * P
        self._keep = (i32(*[k.type_code for k in kl]), i32(*[int(k.num_partials) for k in kl]))
        self.P, self.codes = P, list(zip(self._keep[0], self._keep[1]))     # (type, partials) of every source
        cfg = _lib.SgprConfig(P, int(N), int(M), self._keep[0], self._keep[1], 1e-6, int(bool(template.reg)))
        plan = C.c_void_p()
        h.check(h.lib.gp_sgprb_create(h.h, C.byref(cfg), int(num_windows), C.byref(plan)))
        self.plan = plan
        self.W, self.N, self.M = int(num_windows), int(N), int(M)
        self.nparams = int(h.lib.gp_sgprb_num_params(plan))
        self._ws = h.workspace(h.lib.gp_sgprb_workspace_bytes(plan))
        h.check(h.lib.gp_sgprb_set_workspace(plan, self._ws.data_ptr(), self._ws.numel()))
        t = h.torch
        self.X, self.Y, self.Z = h.zeros(self.W, self.N), h.zeros(self.W, self.N), h.zeros(self.W, self.M)
        self.params, self.grad, self.bound = h.zeros(self.W, self.nparams), h.zeros(self.W, self.nparams), h.zeros(self.W)
        # pinned staging: parameter upload / result download without a pageable-memory synchronisation each round
        self._p_host = t.zeros(self.W, self.nparams, dtype=t.float64).pin_memory()
        self._g_host = t.zeros(self.W, self.nparams, dtype=t.float64).pin_memory()
        self._b_host = t.zeros(self.W, dtype=t.float64).pin_memory()
        self._st_host = t.zeros(4, dtype=t.int32).pin_memory()      # not-positive-definite status of the evaluation in flight
        self._ev, self._pending = None, None
        self.last_status = (0, 0, 0)
        self._ragged = False         # the plan holds inducing counts other than M

    def load(self, xs, ys, zs):
        """put `len(xs)` windows into the first slots (the others keep whatever they held: still valid problems).
        A window's Z may hold 1..M points: shorter ones are padded here (the pad is never read) and the counts go to the
        plan, which evaluates each window as its own-size problem.  All windows at M: no counts are set."""
        import ctypes as C
        h = self.h
        t = h.torch
        n = len(xs)
        zl = [np.asarray(z, dtype=np.float64).reshape(-1) for z in zs]
        counts = [int(z.size) for z in zl]
        for i, c in enumerate(counts):
            if not 1 <= c <= self.M:
                raise ValueError("SgprWindowBatch.load: window %d has %d inducing points; this plan takes 1..%d"
                                 % (i, c, self.M))
        ragged = any(c != self.M for c in counts)
        if ragged:
            zl = [np.concatenate([z, np.full(self.M - z.size, z[-1])]) for z in zl]
        self.X[:n].copy_(t.as_tensor(np.stack([np.asarray(x, dtype=np.float64).reshape(-1) for x in xs])))
        self.Y[:n].copy_(t.as_tensor(np.stack([np.asarray(y, dtype=np.float64).reshape(-1) for y in ys])))
        self.Z[:n].copy_(t.as_tensor(np.stack(zl)))
        if ragged or self._ragged:   # (back to all-M: the plan drops its counts, slots from n on take M)
            h.check(h.lib.gp_sgprb_set_inducing_counts(self.plan, (C.c_int32 * n)(*counts), n))
            self._ragged = ragged
        self.count = n
        self.counts = counts
        self._exact_order = None

    def _upload(self, params_host, cnt):
        """the constrained parameter vectors of the first `cnt` windows, through the pinned staging buffer"""
        self._p_host[:cnt].copy_(self.h.torch.as_tensor(np.asarray(params_host, dtype=np.float64)))
        self.params[:cnt].copy_(self._p_host[:cnt], non_blocking=True)

    def submit(self, params_host, with_grad=True):
        """enqueue one evaluation (parameter upload, the launch sequence, result download) and return at once; `collect`
        waits for exactly this evaluation — not for whatever else is queued on the stream (another batch's evaluation:
        `fit_windows_batched` keeps two batches in flight so that the host's L-BFGS-B stepping of one overlaps the
        device's evaluation of the other)"""
        h = self.h
        n = self.count
        self._upload(params_host, n)
        h.check(h.lib.gp_sgprb_bound_grad(self.plan, self.params.data_ptr(), self.X.data_ptr(), self.Y.data_ptr(),
                                          self.Z.data_ptr(), n, self.bound.data_ptr(),
                                          self.grad.data_ptr() if with_grad else None))
        self._b_host[:n].copy_(self.bound[:n], non_blocking=True)
        if with_grad:
            self._g_host[:n].copy_(self.grad[:n], non_blocking=True)
        # this evaluation's own status word, cleared behind the copy: a failed Cholesky is reported by the evaluation that
        # caused it (status[2] = window slot) and never leaks into the next batch / the next user of the handle
        h.check(h.lib.gp_take_not_pd(h.h, self._st_host.data_ptr()))
        if self._ev is None:
            self._ev = h.torch.cuda.Event()
        self._ev.record(h.torch.cuda.current_stream(h.device))
        self._pending = (n, bool(with_grad))

    def collect(self):
        """(bound, grad) of the evaluation in flight.  `self.last_status` = (flag, pivot, window slot) of the FIRST Cholesky
        failure in it (flag 0: none): that window's numbers — and possibly those of other windows that failed in the same
        evaluation, the device word keeps the first only — are not a bound; `fit_windows_batched` retires the window and
        evaluates again, `evaluate` raises."""
        n, with_grad = self._pending
        self._ev.synchronize()
        self._pending = None
        st = self._st_host.numpy()
        self.last_status = (int(st[0]), int(st[1]), int(st[2]))
        return self._b_host[:n].numpy().copy(), (self._g_host[:n].numpy().copy() if with_grad else None)

    def evaluate(self, params_host, with_grad=True):
        """params_host: (count, nparams) constrained parameter vectors -> (bound (count,), grad (count, nparams))"""
        self.submit(params_host, with_grad)
        out = self.collect()
        if self.last_status[0]:
            from ._lib import GP_ERR_NOT_PD, NotPositiveDefiniteError
            raise NotPositiveDefiniteError(GP_ERR_NOT_PD, "Cholesky failed: window %d of the batch is not positive "
                                           "definite (pivot %d)" % (self.last_status[2], self.last_status[1]))
        return out

    def _load_xnew(self, xnews, n_windows):
        t = self.h.torch
        if xnews is None:
            return self.X[:n_windows], self.N            # predict at the windows' own frames (separation.py:306, 311)
        xn = np.stack([np.asarray(x, dtype=np.float64).reshape(-1) for x in xnews])
        if xn.shape[0] != n_windows:
            raise ValueError("one Xnew per loaded window")
        return t.as_tensor(xn).to(self.X.device), int(xn.shape[1])

    def _timelines(self, xnews, xn, n):
        """every loaded window's smoother timeline (sgpr_ss.ssm_timeline of its frames and its new points `xn`), padded to
        N + n steps: (order (count, N + n), ostep (count, n), steps (count,)), int32"""
        cnt = self.count
        xh = self.X[:cnt].cpu().numpy()
        nh = xh if xnews is None else xn.cpu().numpy()
        order = np.zeros((cnt, self.N + n), dtype=np.int32)
        ostep = np.zeros((cnt, n), dtype=np.int32)
        steps = np.zeros(cnt, dtype=np.int32)
        for w in range(cnt):
            o, s, k = sgpr_ss.ssm_timeline(xh[w], nh[w])
            order[w, :k], ostep[w], steps[w] = o, s, k
        return order, ostep, steps

    @staticmethod
    def _chunks(cnt, chunk, per, cap):
        """the library calls that cover `cnt` windows, `chunk` at a time: (first window, windows) of each, the first one
        the largest.  chunk=None: as many windows as keep `per` bytes each below `cap`."""
        if chunk is None:
            chunk = cap // max(1, int(per))
        chunk = int(max(1, min(int(chunk), cnt)))
        return [(b0, min(chunk, cnt - b0)) for b0 in range(0, cnt, chunk)]

    def predict_f(self, params_host, xnews=None):
        """SGPRSS.predict_f of every loaded window at its parameters params_host[i] (constrained vectors, as
        `fit_windows_batched` returns them in "params"): (mean, var), each (count, n) — separation.py:306"""
        h = self.h
        cnt = self.count
        xn, n = self._load_xnew(xnews, cnt)
        if n > self.N:
            raise ValueError("window-batched predict_f takes at most N new points per window")
        self._upload(params_host, cnt)
        mean, var = h.empty(cnt, n), h.empty(cnt, n)
        h.check(h.lib.gp_sgprb_predict_f(self.plan, self.params.data_ptr(), self.X.data_ptr(), self.Y.data_ptr(),
                                         self.Z.data_ptr(), xn.data_ptr(), n, cnt, mean.data_ptr(), var.data_ptr()))
        return mean.cpu().numpy(), var.cpu().numpy()

    def predict_s(self, params_host, xnews=None, chunk=None):
        """SGPRSS.predict_s (the exact per-source posteriors, sgpr_ss.py:73-114) of every loaded window: (mean, var),
        each (count, P, n) — separation.py:311.  `chunk` windows share one launch sequence (default: as many as fit
        in ~16 GiB of workspace: the N x N factor and its inverse are 64 MB per window at N = 2001)."""
        h = self.h
        cnt = self.count
        xn, n = self._load_xnew(xnews, cnt)
        P = self.P
        self._upload(params_host, cnt)
        size = h.lib.gp_sgprb_predict_source_workspace_bytes
        calls = self._chunks(cnt, chunk, size(self.plan, 1, n), 16 << 30)
        ws = h.workspace(size(self.plan, calls[0][1], n))
        mean, var = h.empty(cnt, P, n), h.empty(cnt, P, n)
        for b0, c in calls:
            h.check(h.lib.gp_sgprb_predict_source(self.plan, self.params[b0:].data_ptr(), self.X[b0:].data_ptr(),
                                                  self.Y[b0:].data_ptr(), xn[b0:].data_ptr(), n, c,
                                                  mean[b0:].data_ptr(), var[b0:].data_ptr(), ws.data_ptr(), ws.numel()))
        return mean.cpu().numpy(), var.cpu().numpy()

    def predict_s_sparse(self, params_host, xnews=None):
        """SGPRSS.predict_s_sparse (the sparse per-source posteriors, gp_sgprb_predict_source_sparse) of every loaded
        window from one fused launch: (mean, var), each (count, P, n).  n may exceed N."""
        h = self.h
        cnt = self.count
        xn, n = self._load_xnew(xnews, cnt)
        P = self.P
        self._upload(params_host, cnt)
        mean, var = h.empty(cnt, P, n), h.empty(cnt, P, n)
        h.check(h.lib.gp_sgprb_predict_source_sparse(self.plan, self.params.data_ptr(), self.X.data_ptr(), self.Y.data_ptr(),
                                                     self.Z.data_ptr(), xn.data_ptr(), n, cnt, mean.data_ptr(),
                                                     var.data_ptr()))
        return mean.cpu().numpy(), var.cpu().numpy()

    def predict_s_ssm(self, params_host, xnews=None, chunk=None, return_loglik=False):
        """SGPRSS.predict_s_ssm (the exact per-source posteriors by the state-space smoother, gp_sgprb_predict_source_ssm) of
        every loaded window: (mean, var), each (count, P, n) [, the exact log-likelihoods (count,)].  One workgroup per
        window; `chunk` windows share a launch sequence (default: as many as keep the forward walk's history, steps * d^2
        doubles per window, below sgpr_ss.MAX_SSM_BYTES).  Chunking changes no bit of any window's result.  Z, the windows'
        inducing counts and the plan's precision play no part; n may exceed N."""
        h = self.h
        cnt = self.count
        d, P = sgpr_ss.ssm_state_dim(self.codes, "SgprWindowBatch.predict_s_ssm")    # raises before any device work
        xn, n = self._load_xnew(xnews, cnt)
        order, ostep, steps = self._timelines(xnews, xn, n)
        self._upload(params_host, cnt)
        smax = int(steps.max())
        size = h.lib.gp_ssm_smooth_workspace_bytes
        calls = self._chunks(cnt, chunk, size(d, smax, P, 1), sgpr_ss.MAX_SSM_BYTES)
        ws = h.workspace(size(d, smax, P, calls[0][1]))
        mean, var, ll = h.empty(cnt, P, n), h.empty(cnt, P, n), h.empty(cnt)
        for b0, c in calls:
            h.check(h.lib.gp_sgprb_predict_source_ssm(self.plan, self.params[b0:].data_ptr(), self.X[b0:].data_ptr(),
                                                      self.Y[b0:].data_ptr(), xn[b0:].data_ptr(), n, c,
                                                      order[b0:].ctypes.data, ostep[b0:].ctypes.data, steps[b0:].ctypes.data,
                                                      mean[b0:].data_ptr(), var[b0:].data_ptr(), ll[b0:].data_ptr(),
                                                      ws.data_ptr(), ws.numel()))
        out = (mean.cpu().numpy(), var.cpu().numpy())
        return out + (ll.cpu().numpy(),) if return_loglik else out

    def exact_loglik_grad(self, params_host, with_grad=True, chunk=None):
        """SGPRSS.exact_log_likelihood_and_grad of every loaded window at its constrained parameter vector params_host[i]
        (gp_sgprb_exact_loglik_grad: one workgroup per window): (loglik (count,), grad (count, nparams)); with_grad=False
        runs the forward walk alone and returns (loglik, None).  `chunk` windows share a launch sequence (default: as many as
        keep the forward walk's history below sgpr_ss.MAX_SSM_BYTES); chunking changes no bit of any window's result.  Z, the
        windows' inducing counts and the plan's precision play no part.  Synchronous."""
        h = self.h
        cnt, N = self.count, self.N
        d, P = sgpr_ss.ssm_state_dim(self.codes, "SgprWindowBatch.exact_loglik_grad")    # raises before any device work
        if self._exact_order is None:
            xh = self.X[:cnt].cpu().numpy()
            self._exact_order = np.ascontiguousarray(np.argsort(xh, axis=1, kind="stable").astype(np.int32))
        order = self._exact_order
        steps = np.full(cnt, N, dtype=np.int32)
        size = h.lib.gp_ssm_score_workspace_bytes if with_grad else h.lib.gp_ssm_smooth_workspace_bytes
        self._upload(params_host, cnt)
        calls = self._chunks(cnt, chunk, size(d, N, P, 1), sgpr_ss.MAX_SSM_BYTES)
        ws = h.workspace(size(d, N, P, calls[0][1]))
        ll = h.empty(cnt)
        grad = h.empty(cnt, self.nparams) if with_grad else None
        for b0, c in calls:
            if with_grad:
                h.check(h.lib.gp_sgprb_exact_loglik_grad(self.plan, self.params[b0:].data_ptr(), self.X[b0:].data_ptr(),
                                                         self.Y[b0:].data_ptr(), c, order[b0:].ctypes.data, ll[b0:].data_ptr(),
                                                         grad[b0:].data_ptr(), None, ws.data_ptr(), ws.numel()))
            else:
                h.check(h.lib.gp_sgprb_predict_source_ssm(self.plan, self.params[b0:].data_ptr(), self.X[b0:].data_ptr(),
                                                          self.Y[b0:].data_ptr(), None, 0, c, order[b0:].ctypes.data, None,
                                                          steps[b0:].ctypes.data, None, None, ll[b0:].data_ptr(),
                                                          ws.data_ptr(), ws.numel()))
        return ll.cpu().numpy(), (grad.cpu().numpy() if with_grad else None)

    def sample_s_sparse(self, params_host, xnews=None, num_samples=1, seed=None, eps=None):
        """SGPRSS.sample_s_sparse (joint posterior draws of every source, gp_sgprb_sample_source_sparse) of every loaded
        window from one launch sequence: (count, P, num_samples, n); ragged windows included.  eps=None: standard normals
        from a device generator seeded by `seed`, sgpr_ss.SAMPLE_EPS_BYTES per library call; otherwise
        eps=(eps_x (count, S, C, n), eps_z (count, S, C, M), eps_u (count, S, 2, M)) with M the plan's: rows of eps_z and
        eps_u past a window's own inducing-point count are never read."""
        h = self.h
        t = h.torch
        cnt, S, M, P = self.count, int(num_samples), self.M, self.P
        C = int(sum(sgpr_ss.sample_components(self.codes)))     # raises for an unsupported kernel, before any device work
        xn, n = self._load_xnew(xnews, cnt)
        if S < 1:
            raise ValueError("sample_s_sparse: needs at least one sample")
        shapes = [(cnt,) + sh for sh in sgpr_ss.sample_eps_shapes(self.codes, n, M, S)]
        if eps is not None:
            eps = sgpr_ss._check_eps("sample_s_sparse", ("eps_x", "eps_z", "eps_u"), eps, shapes)
        xh, zh = xn.cpu().numpy(), self.Z[:cnt].cpu().numpy()
        order = np.zeros((cnt, n + M), dtype=np.int32)
        for w in range(cnt):
            k = self.counts[w]
            order[w, :n + k] = sgpr_ss.merged_order(xh[w], zh[w, :k])
        self._upload(params_host, cnt)
        chunk = S if eps is not None else sgpr_ss._sample_chunk(S, cnt * (C * (n + M) + 2 * M))
        ws = h.workspace(h.lib.gp_sgpr_sample_source_workspace_bytes(M, P, C, n, chunk, cnt))
        gen = None if eps is not None else sgpr_ss._sample_generator(h, seed)
        res = np.empty((cnt, P, S, n))
        for s0 in range(0, S, chunk):
            sc = min(chunk, S - s0)
            if eps is not None:
                ex, ez, eu = (h.to_device(e) for e in eps)
            else:
                ex, ez, eu = (t.randn(cnt, sc, *sh[2:], dtype=t.float64, device=h.device, generator=gen) for sh in shapes)
            out = h.empty(cnt, P, sc, n)
            h.check(h.lib.gp_sgprb_sample_source_sparse(self.plan, self.params.data_ptr(), self.X.data_ptr(), self.Y.data_ptr(),
                                                        self.Z.data_ptr(), xn.data_ptr(), n, cnt, order.ctypes.data, sc,
                                                        ex.data_ptr(), ez.data_ptr(), eu.data_ptr(), out.data_ptr(),
                                                        ws.data_ptr(), ws.numel()))
            res[:, :, s0:s0 + sc] = out.cpu().numpy()
        return res

    def sample_s_ssm(self, params_host, xnews=None, num_samples=1, seed=None, eps=None, chunk=None):
        """SGPRSS.sample_s_ssm (joint draws of every source from the exact posterior by the simulation smoother,
        gp_sgprb_sample_source_ssm) of every loaded window: (count, P, num_samples, n).  One wavefront per (window, draw);
        `chunk` windows share a launch sequence (default: as many as keep a call's normals and workspace below
        sgpr_ss.MAX_SSM_BYTES).  Chunking changes no bit of any draw, seeded ones included: the normals are generated window
        by window.  eps=None: standard normals from a device generator seeded by `seed`, at most sgpr_ss.SAMPLE_EPS_BYTES of
        them per window at a time; otherwise eps=(eps_x (count, S, smax, d), eps_y (count, S, N)) with smax the longest
        timeline among the windows (sgpr_ss.ssm_timeline): a window reads its own first steps of eps_x.  Z, the windows'
        inducing counts and the plan's precision play no part; n may exceed N."""
        h = self.h
        t = h.torch
        cnt, N, S = self.count, self.N, int(num_samples)
        d, P = sgpr_ss.ssm_state_dim(self.codes, "SgprWindowBatch.sample_s_ssm")    # raises before any device work
        if S < 1:
            raise ValueError("sample_s_ssm: needs at least one sample")
        xn, n = self._load_xnew(xnews, cnt)
        if n < 1:
            raise ValueError("sample_s_ssm: needs at least one new point")
        order, ostep, steps = self._timelines(xnews, xn, n)
        smax = int(steps.max())
        shapes = [(cnt,) + sh for sh in sgpr_ss.ssm_sample_eps_shapes(self.codes, smax, N, S)]
        if eps is not None:
            eps = sgpr_ss._check_eps("sample_s_ssm", ("eps_x", "eps_y"), eps, shapes)
        self._upload(params_host, cnt)
        sch = S if eps is not None else sgpr_ss._sample_chunk(S, smax * d + N)
        size = h.lib.gp_ssm_sample_workspace_bytes
        per = int(size(d, smax, P, sch, 1)) + 8 * sch * (smax * d + N)      # a window's workspace and its normals
        calls = self._chunks(cnt, chunk, per, sgpr_ss.MAX_SSM_BYTES)
        ws = h.workspace(size(d, smax, P, sch, calls[0][1]))
        gen = None if eps is not None else sgpr_ss._sample_generator(h, seed)
        res = np.empty((cnt, P, S, n))
        for s0 in range(0, S, sch):
            sc = min(sch, S - s0)
            for b0, c in calls:
                sm = int(steps[b0:b0 + c].max())          # the library lays eps_x out on the call's own longest timeline
                if eps is not None:
                    ex, ey = h.to_device(np.ascontiguousarray(eps[0][b0:b0 + c, :, :sm])), h.to_device(eps[1][b0:b0 + c])
                else:
                    ex, ey = h.empty(c, sc, sm, d), h.empty(c, sc, N)
                    for w in range(c):                    # window by window on the batch's longest timeline: the same stream
                        ex[w].copy_(t.randn(sc, smax, d, dtype=t.float64, device=h.device, generator=gen)[:, :sm])
                        ey[w].copy_(t.randn(sc, N, dtype=t.float64, device=h.device, generator=gen))
                out = h.empty(c, P, sc, n)
                h.check(h.lib.gp_sgprb_sample_source_ssm(self.plan, self.params[b0:].data_ptr(), self.X[b0:].data_ptr(),
                                                         self.Y[b0:].data_ptr(), xn[b0:].data_ptr(), n, c,
                                                         order[b0:].ctypes.data, ostep[b0:].ctypes.data,
                                                         steps[b0:].ctypes.data, sc, ex.data_ptr(), ey.data_ptr(),
                                                         out.data_ptr(), ws.data_ptr(), ws.numel()))
                res[b0:b0 + c, :, s0:s0 + sc] = out.cpu().numpy()
        return res

    def close(self):
        if self.plan is not None:
            self.h.sync()
            self.h.lib.gp_sgprb_destroy(self.plan)
            self.plan = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def ragged_batches(counts, batch, granule=16, cap=256):
    """How fit_windows_batched groups windows by inducing-point count (host only).

    counts[i] = inducing points of window i.  Returns (batches, single): batches is a list of (plan_M, positions) with at
    most `batch` positions each, single the positions whose count exceeds `cap` (fitted one window at a time).  Equal
    counts: consecutive batches in input order on one plan of exactly that M (no padding).  Otherwise the windows are
    sorted by count (stable) and cut into runs of at most `batch`; a run's plan takes its largest count rounded up to a
    multiple of `granule`, at most `cap`, so that the padded work stays small and few plan sizes occur."""
    counts = [int(c) for c in counts]
    for i, c in enumerate(counts):
        if c < 1:
            raise ValueError("ragged_batches: window %d has no inducing point" % i)
    B = max(1, int(batch))
    single = [i for i, c in enumerate(counts) if c > cap]
    rest = [i for i, c in enumerate(counts) if c <= cap]
    if not rest:
        return [], single
    if len({counts[i] for i in rest}) == 1:
        return [(counts[rest[0]], rest[b0:b0 + B]) for b0 in range(0, len(rest), B)], single
    order = sorted(rest, key=lambda i: counts[i])       # (stable)
    out = []
    for b0 in range(0, len(order), B):
        ids = order[b0:b0 + B]
        m = max(counts[i] for i in ids)
        out.append((min(int(cap), -(-m // int(granule)) * int(granule)), ids))
    return out, single


# ---- shared by fit_windows_batched and fit_windows_exact ----
# `predict` of fit_windows_batched -> the per-source predictor, of SgprWindowBatch and of SGPRSS alike
_SOURCE_PREDICTOR = {True: "predict_s", "sparse": "predict_s_sparse", "ssm": "predict_s_ssm"}


def _refuse_mean_function(model, who, instead):
    if getattr(model, "mean_function", None) is not None and type(model.mean_function).__name__ != "Zero":
        raise NotImplementedError("%s: the template model has a mean_function; the batched plan has none (use %s)"
                                  % (who, instead))


def _free_state(model):
    """(st, ps, free_idx, vals0, back, var_idx) of the template: its _objective_setup(), the free state of its own parameter
    values (every window's starting point without params0) and where the kernel variances sit in a parameter vector"""
    st = model._objective_setup()
    ps, free_idx, vals0 = st["ps"], st["free_idx"], st["vals0"]
    back = np.array([ps[i].transform.backward(np.atleast_1d(vals0[i]))[0] for i in free_idx])
    var_idx = [int(o) for o in np.cumsum([1] + [2 + 2 * int(k.num_partials) for k in model.kern.kern_list])[:-1]]
    return st, ps, free_idx, vals0, back, var_idx


def _starting_points(ids, params0, ps, free_idx, vals0, back):
    """(base, x0s) of windows `ids`: their constrained parameter vectors (params0[i], or the template's) and free states"""
    if params0 is None:
        return np.tile(vals0, (len(ids), 1)), [back.copy() for _ in ids]
    base = np.stack([np.asarray(params0[i], dtype=np.float64) for i in ids])
    return base, [np.array([ps[j].transform.backward(np.atleast_1d(row[j]))[0] for j in free_idx]) for row in base]


def _constrained(st, base, Xf):
    """(parameter vectors, d constrained / d free) at the free states Xf: `base` with its free entries replaced"""
    y, dy = sgpr_ss.SGPRSS._free_to_params(st, Xf)
    pv = base.copy()
    pv[:, st["free_idx"]] = y
    return pv, dy


def _window_result(key, value, nfev, nit, params, var_idx, **more):
    return dict({key: value, "nfev": nfev, "nit": nit, "variances": params[var_idx].copy(), "noise": float(params[0]),
                 "params": params}, **more)


def fit_windows_batched(make_model, windows, maxiter=10, batch=64, reset=default_reset, handle=None, rank=0,
                        world_size=1, params0=None, predict=False, inflight=2):
    """fit_windows with the device work batched: `batch` windows go through every bound + gradient evaluation together
    (one launch sequence, gp_sgprb_bound_grad), each window driven by its own instance of scipy's L-BFGS-B routine
    (lbfgsb_batch.LbfgsbRC: the iterates of `model.optimize(maxiter=maxiter)` exactly, given the same f and g).

    Every window starts from the parameter values of make_model(handle) after `reset(model, x, y, z)` (unit noise and
    kernel variances by default, transcription.py:253-263) — i.e. carry_kernel_state=False of fit_windows — or from
    params0[i] (constrained vector [noise | theta_0 | ...]) when given.  All windows must share N (see below for M).
    predict=True adds what SoSp.optimize computes after every window's optimisation (separation.py:300-313), batched the
    same way: "mean", "var" (predict_f at the window's frames, (N, 1)) and "smean", "svar" (predict_s: lists over the
    sources of (N, 1) arrays).  predict="sparse" is the same with "smean", "svar" from the sparse per-source posterior
    (SGPRSS.predict_s_sparse: no N x N factorisation) instead of predict_s; predict="ssm" takes them from the state-space
    smoother (SGPRSS.predict_s_ssm: predict_s's exact posterior without the N x N factorisation, the variance from the
    source's own Kdiag; kernels with a Matern-1/2 envelope only).  `merge_sources` takes any of the three.
    Windows must share N; their inducing-point counts may differ (each window's Z from its own audio, as the drivers'
    init_liv picks it).  Windows of different counts are sorted by count and batched with their neighbours
    (`ragged_batches`), each batch on a plan sized by its largest count; plans are made when first needed and freed once no
    pending batch needs their size.  A window with more than 256 inducing points is fitted in the same call by the
    one-window engine (as fit_windows does it; "engine": "single" in its result).
    `inflight` batches are kept going at once (default 2: the host's stepping of one overlaps the device's evaluation of
    the other; 1 = one after another).
    `reset` is evaluated ONCE, on this rank's first window, to obtain the starting parameter values of every window (the
    default reset and AMT.reset_model set the same values for every window); per-window starting values go in `params0`.
    The template model must have no mean function and float64 strips (NotImplementedError otherwise).
    A window whose Kuu or B loses positive definiteness during its fit (the reference: tf.cholesky raises out of that
    window's optimize()) — or has them not positive definite at its STARTING parameters already — is retired with
    results[i]["error"] set, bound = nan and its starting parameters; the other windows of the batch are unaffected (their
    evaluation is repeated; the retired slot rides along on a healthy window's parameters, so it cannot fail again).  One
    repeat per failing window: the device's status word names the first failure of an evaluation only.
    Returns a list over windows of dicts: bound, nfev, nit, variances, noise, params [, error]."""
    from . import _lib, lbfgsb_batch
    from .dist import window_assignment
    if not lbfgsb_batch.available():
        raise RuntimeError("fit_windows_batched needs scipy >= 1.15 (its reverse-communication L-BFGS-B routine); "
                           "use fit_windows")
    if not (isinstance(predict, (bool, np.bool_)) or predict in ("sparse", "ssm")):
        raise ValueError('fit_windows_batched: predict is False, True, "sparse" or "ssm"')
    source = _SOURCE_PREDICTOR[predict if isinstance(predict, str) else True] if predict else None
    mine = window_assignment(len(windows), world_size, rank)
    results = [None] * len(windows)
    if not mine:
        return results
    # the windows' shapes, before any device work
    N = int(np.asarray(windows[mine[0]][0]).size)
    counts = []
    for i in mine:
        if np.asarray(windows[i][0]).size != N:
            raise ValueError("fit_windows_batched: all windows must have the same number of frames")
        counts.append(int(np.asarray(windows[i][2]).size))
        if counts[-1] < 1:
            raise ValueError("fit_windows_batched: window %d has no inducing point" % i)
    if handle is None:
        # a stream of its own: the launch sequence of an evaluation is recorded into a hipGraph and replayed, which the
        # legacy null stream cannot do
        import torch
        dev0 = _lib.default_handle().device
        s = torch.cuda.Stream(device=dev0)
        with torch.cuda.stream(s):
            hs = _lib.Handle(dev0.index, stream=s)
            try:
                return fit_windows_batched(make_model, windows, maxiter=maxiter, batch=batch, reset=reset, handle=hs,
                                           rank=rank, world_size=world_size, params0=params0, predict=predict,
                                           inflight=inflight)
            finally:
                s.synchronize()
                hs.close()
    h = handle
    model = make_model(h)
    if source == "predict_s_ssm":              # the smoother's scope, before any fitting
        sgpr_ss.ssm_state_dim(model.kern.kern_list, 'fit_windows_batched(predict="ssm")')
    init_vals = [p.value.copy() for p in model._param_list()]      # (the single-engine windows start from these)
    # what the batched plan takes from the template model: kernel structure, `reg`, the parameter values after ONE
    # reset() (on this rank's first window).  It does not carry a mean function or float32 strips: refuse, do not drop.
    _refuse_mean_function(model, "fit_windows_batched", "fit_windows")
    if getattr(model, "_bits", 64) != 64:
        raise NotImplementedError("fit_windows_batched runs in float64; the template model asks for float32 strips "
                                  "(use fit_windows)")
    x0w, y0w, z0w = windows[mine[0]][:3]
    reset(model, x0w, y0w, z0w)
    st, ps, free_idx, vals0, back, var_idx = _free_state(model)
    groups, single = ragged_batches(counts, batch)
    chunks = [(m, [mine[q] for q in ids]) for m, ids in groups]       # (plan M, window indices)
    single = [mine[q] for q in single]
    B = max(1, min(int(batch), sum(len(ids) for _, ids in chunks)))
    # Two batches in flight, each on a device plan of its own: while the host steps the L-BFGS-B instances of one batch
    # (setulb and the transforms: as long as a device evaluation at W = 256), the device evaluates the other.
    nslots = max(1, min(int(inflight), len(chunks)))
    # plans for the first batches up front; later ones when first needed.  A plan stays while a pending batch needs its
    # size and is freed when a new plan is made (sizes only grow along the sorted batches: at most 2 x inflight plans)
    idle = [SgprWindowBatch(model, B, N, m, handle=h) for m, _ in chunks[:nslots]]

    def plan_for(m):
        for d in idle:
            if d.M == m:
                idle.remove(d)
                return d
        for d in [d for d in idle if all(d.M != mm for mm, _ in pending)]:
            idle.remove(d)
            d.close()
        return SgprWindowBatch(model, B, N, m, handle=h)

    class _Run(object):
        pass

    def start(dev, ids):
        r = _Run()
        r.dev, r.ids, r.n = dev, ids, len(ids)
        dev.load([windows[i][0] for i in ids], [windows[i][1] for i in ids], [windows[i][2] for i in ids])
        r.base, x0s = _starting_points(ids, params0, ps, free_idx, vals0, back)
        r.runs = [lbfgsb_batch.LbfgsbRC(x0, maxiter=maxiter) for x0 in x0s]
        r.Xf = np.stack(x0s)
        r.active = list(range(r.n))
        r.failed = {}
        submit(r)
        return r

    def submit(r):
        pv, r.dy = _constrained(st, r.base, r.Xf)
        # retired windows ride along on the parameters of a healthy window (their own starting parameters may be what failed:
        # Kuu depends on the kernel parameters and Z alone, so a healthy window's parameters factorise in any slot)
        donor = r.active[0] if r.active else None
        for q in r.failed:
            pv[q] = pv[donor] if donor is not None else r.base[q]
        r.dev.submit(pv)

    def advance(r):
        """collect the evaluation in flight, step every active instance; True while the batch still needs evaluations"""
        bound, grad = r.dev.collect()
        flag, pivot, slot = r.dev.last_status
        if flag:
            # TF raises InvalidArgumentError out of the one session.run whose tf.cholesky failed and the reference's window
            # loop dies there (transcription.py:283); here that window alone is retired with the error, and the evaluation
            # is repeated for the others (the device word names the first failure only: another window may have failed in
            # the same evaluation — it is found by the repeat)
            if slot in r.failed or not (0 <= slot < r.n):
                # (a retired slot runs on a healthy window's parameters: it cannot be what failed unless the status word is wrong)
                raise _lib.NotPositiveDefiniteError(_lib.GP_ERR_NOT_PD, "Cholesky failed in window slot %d (pivot %d), which is %s"
                                                    % (slot, pivot, "already retired" if slot in r.failed else "outside the batch"))
            r.failed[slot] = "Cholesky failed: not positive definite (pivot %d) at evaluation %d" % (pivot, r.runs[slot].nfev + 1)
            r.active = [q for q in r.active if q != slot]
            if r.active:
                submit(r)
            return bool(r.active)
        nxt = []
        for q in r.active:
            g = -(grad[q, free_idx] * r.dy[q])
            r.runs[q].give(-bound[q], g)
            if r.runs[q].step():
                r.Xf[q] = r.runs[q].x
                nxt.append(q)
        r.active = nxt
        if nxt:
            submit(r)
        return bool(nxt)

    def finish(r):
        pfin, _ = _constrained(st, r.base, np.stack([q.x for q in r.runs]))
        for q in r.failed:
            pfin[q] = r.base[q]
        for q, i in enumerate(r.ids):
            results[i] = _window_result("bound", -r.runs[q].fun, r.runs[q].nfev, r.runs[q].nit, pfin[q].copy(), var_idx)
            if q in r.failed:
                results[i].update(error=r.failed[q], bound=float("nan"))
        if source:
            fm, fv = r.dev.predict_f(pfin)
            sm, sv = getattr(r.dev, source)(pfin)
            for q, i in enumerate(r.ids):
                if q in r.failed:           # (predicted at the starting parameters only to keep the batch whole)
                    continue
                results[i]["mean"], results[i]["var"] = fm[q].reshape(-1, 1), fv[q].reshape(-1, 1)
                results[i]["smean"] = [sm[q, k].reshape(-1, 1) for k in range(sm.shape[1])]
                results[i]["svar"] = [sv[q, k].reshape(-1, 1) for k in range(sv.shape[1])]

    pending = list(chunks)
    live = []
    while pending and len(live) < nslots:
        m, ids = pending.pop(0)
        live.append(start(plan_for(m), ids))
    while live:
        for r in list(live):
            if advance(r):
                continue
            finish(r)
            live.remove(r)
            idle.append(r.dev)
            if pending:
                m, ids = pending.pop(0)
                live.append(start(plan_for(m), ids))
    for dev in idle:
        dev.close()
    # windows beyond the batched plans' 256 inducing points: the one-window engine, as fit_windows fits a window
    for i in single:
        for p, v in zip(model._param_list(), init_vals):
            p.value = v
        x, y, z = windows[i][:3]
        reset(model, x, y, z)
        ps1 = model._param_list()
        if params0 is not None:
            for p, v in zip(ps1, np.asarray(params0[i], dtype=np.float64)):
                p.value = np.array([v])
        start_vals = np.array([float(p.value[0]) for p in ps1])
        try:
            res = model.optimize(method='L-BFGS-B', maxiter=maxiter)
        except _lib.NotPositiveDefiniteError as e:
            results[i] = _window_result("bound", float("nan"), 0, 0, start_vals, var_idx, engine="single", error=str(e))
            continue
        pv = np.array([float(p.value[0]) for p in ps1])
        results[i] = _window_result("bound", -float(res.fun), int(res.nfev), int(res.nit), pv, var_idx, engine="single")
        if source:
            m1, v1 = model.predict_f(x)
            ms, vs = getattr(model, source)(x)
            results[i].update(mean=m1, var=v1, smean=list(ms), svar=list(vs))
    model._destroy()
    return results


def fit_windows_exact(make_model, windows, maxiter=10, batch=64, params0=None, handle=None):
    """Fit every window (x_i, y_i[, z_i]) by exact maximum likelihood: SGPRSS.optimize(objective="exact") of each window,
    `batch` windows going through every evaluation of the exact log-likelihood and its gradient together
    (SgprWindowBatch.exact_loglik_grad), each driven by its own instance of scipy's L-BFGS-B routine
    (lbfgsb_batch.minimize_many: the iterates of the window's own optimize, given the same f and g).  Inducing inputs play no
    part: a window's z is ignored.

    Every window starts from the parameter values of make_model(handle), or from params0[i] (constrained vector
    [noise | theta_0 | ...]) when given; .fixed Params keep the template's values.  Windows must share N; the template must
    have no mean function, reg=False and kernels in the scope of predict_s_ssm (NotImplementedError otherwise, before any
    device work).  Synchronous: one evaluation at a time, no recorded graph, no batches in flight.
    Returns a list over windows of dicts: loglik, nfev, nit, variances, noise, params."""
    from . import _lib, lbfgsb_batch
    if not lbfgsb_batch.available():
        raise RuntimeError("fit_windows_exact needs scipy >= 1.15 (its reverse-communication L-BFGS-B routine)")
    results = [None] * len(windows)
    if not len(windows):
        return results
    N = int(np.asarray(windows[0][0]).size)
    for w in windows:
        if np.asarray(w[0]).size != N or np.asarray(w[1]).size != N:
            raise ValueError("fit_windows_exact: all windows must have the same number of frames (one output column)")
    model = make_model(handle)
    _refuse_mean_function(model, "fit_windows_exact", 'optimize(objective="exact") per window')
    if getattr(model, "_shard", None):
        raise NotImplementedError("fit_windows_exact: the template model is a frame-sharded window; the state-space walk is "
                                  "sequential in the frames (build it unsharded)")
    if model.reg:
        raise NotImplementedError("fit_windows_exact: reg=True adds its L1 term to the collapsed bound; the exact likelihood "
                                  "has none (build the template with reg=False)")
    sgpr_ss.ssm_state_dim(model.kern.kern_list, "fit_windows_exact")
    h = handle or model._handle or _lib.default_handle()
    st, ps, free_idx, vals0, back, var_idx = _free_state(model)
    z = model.Z._array.reshape(-1)
    B = max(1, min(int(batch), len(windows)))
    dev = SgprWindowBatch(model, B, N, z.size, handle=h)
    try:
        for b0 in range(0, len(windows), B):
            ids = list(range(b0, min(b0 + B, len(windows))))
            dev.load([windows[i][0] for i in ids], [windows[i][1] for i in ids], [z for _ in ids])
            base, x0s = _starting_points(ids, params0, ps, free_idx, vals0, back)

            def fg(Xf, active, base=base):
                pv, dy = _constrained(st, base, Xf)
                ll, grad = dev.exact_loglik_grad(pv)
                return -ll, -(grad[:, free_idx] * dy)

            runs = lbfgsb_batch.minimize_many(fg, x0s, maxiter=maxiter)
            pfin, _ = _constrained(st, base, np.stack([r.x for r in runs]))
            for q, i in enumerate(ids):
                results[i] = _window_result("loglik", -runs[q].fun, runs[q].nfev, runs[q].nit, pfin[q].copy(), var_idx)
    finally:
        dev.close()
        model._destroy()
        object.__setattr__(model, "_obj_state", None)
    return results



def merge_sources(results, ws, n):
    """SoSp.predict_s (separation.py:340-368): overlap-add the per-window source posteriors of
    `fit_windows_batched(..., predict=True)` into whole-signal estimates [[mean_1, var_1], [mean_2, var_2], ...]
    (window_overlap.merged_mean / merged_variance, Hann-weighted halves of 50 %-overlapping windows)."""
    from . import window_overlap
    num_sources = len(results[0]["smean"])
    out = []
    for k in range(num_sources):
        m = window_overlap.merged_mean(y=[r["smean"][k] for r in results], ws=ws, n=n)
        v = window_overlap.merged_variance(y=[r["svar"][k] for r in results], ws=ws, n=n)
        out.append([m, v])
    return out
