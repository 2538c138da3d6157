"""SGPRSS — sparse Gaussian process regression for source separation (gpitch/sgpr_ss.py:10-114), on the
HIP engine (csrc/sgpr.hip) through gp_sgpr_*.  Same constructor and method names as the reference:

    m = SGPRSS(X, Y, kern, Z, reg=False)       # kern: sum of pitch kernels (np.sum(list) -> Add, .kern_list)
    m.build_likelihood()                        # collapsed bound (sgpr_ss.py:29-71)
    mean, var = m.predict_f(Xnew)               # GPflow SGPR.build_predict (separation.py:306)
    smean, svar = m.predict_s(Xnew)             # per-source exact posterior (sgpr_ss.py:73-114)
"""
import ctypes as C

import numpy as np

from . import _lib
from .kernels import Add
from .param import DataHolder, Param, ParamList, Parameterized, transforms


class _Gaussian(Parameterized):
    """gpflow.likelihoods.Gaussian: variance Param (positive), initial value 1.0"""

    def __init__(self):
        self.variance = Param(1.0, transforms.positive)


# ---- joint posterior draws of the sources (csrc/sample.hip): host-only helpers, no device work ----
_KERN_NAMES = {_lib.KERN_MATERN12: "Matern12", _lib.KERN_MATERN32: "Matern32", _lib.KERN_MATERN52: "Matern52",
               _lib.KERN_RBF: "RBF", _lib.KERN_MERCER_MATERN12SM: "MercerMatern12sm", _lib.KERN_MATERN12SM: "Matern12sm",
               _lib.KERN_MATERN32SM: "Matern32sm", _lib.KERN_MERCER_MATERN52SM: "Matern52 * MercerCosMix"}
_SAMPLE_KERNS = (_lib.KERN_MERCER_MATERN12SM, _lib.KERN_MATERN12SM, _lib.KERN_MATERN12)
# eps=None: the standard normals of one library call stay below this many bytes (the draws are generated chunk by chunk)
SAMPLE_EPS_BYTES = 1 << 30


def _kern_codes(kern_list):
    """[(type_code, num_partials)] of kernel objects (an Add, a list) or of such pairs"""
    kl = getattr(kern_list, "kern_list", kern_list)
    return [(int(k[0]), int(k[1])) if isinstance(k, (tuple, list)) else (int(k.type_code), int(k.num_partials)) for k in kl]


def sample_components(kern_list, who="sample_s_sparse", what="joint draws need"):
    """Ornstein-Uhlenbeck components per source for sample_s_sparse: 2 m for a Matern-1/2 spectral mixture of m partials
    (a_k and b_k of every partial), 1 for Matern12.  Raises NotImplementedError, naming the kernel, for a sum that holds a
    kernel without a Matern-1/2 envelope: only those have the exact first-order prior sampler.  (`who`, `what`: the caller
    and its need, for the message: the state-space smoother asks the same question.)"""
    comps = []
    for i, (code, m) in enumerate(_kern_codes(kern_list)):
        if code not in _SAMPLE_KERNS:
            raise NotImplementedError("%s: kernel %d of the sum is %s; %s a Matern-1/2 envelope "
                                      "(supported: %s)" % (who, i, _KERN_NAMES.get(code, "type %d" % code), what,
                                                           ", ".join(_KERN_NAMES[c] for c in _SAMPLE_KERNS)))
        comps.append(1 if code == _lib.KERN_MATERN12 else 2 * m)
    return comps


def sample_eps_shapes(kern_list, n, M, num_samples=1):
    """shapes of the three standard-normal arrays of sample_s_sparse for one window and output column:
    eps_x (S, C, n), eps_z (S, C, M), eps_u (S, 2, M) with C = sum of sample_components(kern_list), the sources' blocks in
    kern_list order.  Blocks are indexed by the caller's own point order (Xnew, Z), not by the merged one."""
    C = int(sum(sample_components(kern_list)))
    S = int(num_samples)
    return (S, C, int(n)), (S, C, int(M)), (S, 2, int(M))


def merged_order(xnew, z):
    """stable ascending argsort of t = concat(xnew, z) as int32: entry < len(xnew) is a new frame, len(xnew) + i is z[i].
    Ties keep the caller's order (a frame that coincides with an inducing input comes first)."""
    t = np.concatenate([np.asarray(xnew, dtype=np.float64).reshape(-1), np.asarray(z, dtype=np.float64).reshape(-1)])
    return np.argsort(t, kind="stable").astype(np.int32)


# ---- the exact posterior by the state-space smoother (csrc/ssm_smooth.hip): host-only helpers, no device work ----
SSM_MAX_D = 128
# the forward walk's history (steps * d^2 doubles per window and a little more) of one library call stays below this many
# bytes: a batch of windows is cut into chunks, which changes no bit of any window's result
MAX_SSM_BYTES = 32 << 30


def ssm_state_dim(kern_list, who="predict_s_ssm"):
    """(d, P) of the state-space model of a kernel sum: d = the sum of sample_components.  Raises NotImplementedError
    naming the kernel and its index for a kernel without the Ornstein-Uhlenbeck form, and naming d for d > SSM_MAX_D."""
    comps = sample_components(kern_list, who, "the state-space smoother needs")
    d = int(sum(comps))
    if d > SSM_MAX_D:
        raise NotImplementedError("%s: the state dimension d = %d (the sources' components: %s) exceeds %d"
                                  % (who, d, comps, SSM_MAX_D))
    return d, len(comps)


def ssm_timeline(X, Xnew):
    """The smoother's timeline (order, out_step, steps), int32 / int32 / int: the N training frames in stable ascending
    order with, merged in, every distinct value of Xnew that is not bit-equal to a training frame.  order[j] < N is training
    frame X[order[j]] (an observed step), order[j] >= N new frame Xnew[order[j] - N] (the first with that value);
    out_step[i] is the step of new frame i.  A new frame bit-equal to a training frame shares that frame's step (the first of
    them, should the training frame repeat); duplicate training frames stay separate steps; a tie between a training frame
    and a new one that is equal but not bit-equal (0.0 and -0.0) keeps the training frame first."""
    X = np.ascontiguousarray(np.asarray(X, dtype=np.float64).reshape(-1))
    Xnew = np.ascontiguousarray(np.asarray(Xnew, dtype=np.float64).reshape(-1))
    N, n = X.size, Xnew.size
    if n == 0:
        return np.argsort(X, kind="stable").astype(np.int32), np.zeros(0, dtype=np.int32), N
    xb, nb = X.view(np.int64), Xnew.view(np.int64)
    ub, first, inv = np.unique(nb, return_index=True, return_inverse=True)
    inv = inv.reshape(-1)
    fresh = ~np.isin(ub, xb)                               # distinct new values that are no training frame
    reps = first[fresh]                                    # their first occurrence in Xnew
    t = np.concatenate([X, Xnew[reps]])
    ids = np.concatenate([np.arange(N), N + reps])
    order = ids[np.argsort(t, kind="stable")].astype(np.int32)
    steps = order.size
    step_of = np.full(N + n, -1, dtype=np.int64)
    step_of[order] = np.arange(steps)
    ustep = np.empty(ub.size, dtype=np.int64)              # the step of every distinct new value
    ustep[fresh] = step_of[N + reps]
    if (~fresh).any():
        tr = order[order < N]                              # training frames in step order
        tb, tfirst = np.unique(xb[tr], return_index=True)  # a value's first training frame along the timeline
        ustep[~fresh] = step_of[tr[tfirst[np.searchsorted(tb, ub[~fresh])]]]
    return order, ustep[inv].astype(np.int32), int(steps)


def ssm_sample_eps_shapes(kern_list, steps, N, num_samples=1):
    """shapes of the two standard-normal arrays of sample_s_ssm for one window and output column: eps_x (S, steps, d),
    STEP-major along the merged timeline of ssm_timeline(X, Xnew) (entry [s, j, i] drives coordinate i of the state at step
    j; d and the coordinates' order as ssm_state_dim / sample_components), and eps_y (S, N) in the caller's frame order."""
    d, _ = ssm_state_dim(kern_list, "sample_s_ssm")
    S = int(num_samples)
    return (S, int(steps), d), (S, int(N))


def _sample_chunk(num_samples, doubles_per_sample):
    """draws per library call so that their standard normals stay below SAMPLE_EPS_BYTES"""
    return int(max(1, min(int(num_samples), SAMPLE_EPS_BYTES // (8 * max(1, int(doubles_per_sample))))))


def _sample_generator(h, seed):
    g = h.torch.Generator(device=h.device)
    if seed is None:
        g.seed()
    else:
        g.manual_seed(int(seed))
    return g


def _check_eps(who, names, eps, shapes):
    """the caller's standard normals as float64 arrays, one per name and of the wanted shape each (ValueError otherwise)"""
    eps = [np.asarray(e, dtype=np.float64) for e in eps]
    if len(eps) != len(names) or any(e.shape != sh for e, sh in zip(eps, shapes)):
        raise ValueError("%s: eps must be (%s) of shapes %s" % (who, ", ".join(names), list(shapes)))
    return eps


class SGPRSS(Parameterized):
    def __init__(self, X, Y, kern, Z, mean_function=None, reg=False, handle=None, shard=None, float_type=None):
        """shard=(rank, world): ONE window spread over `world` GPUs by frames (one process each).  Every rank is
        built with the full X, Y; it uploads only its contiguous slice, and each bound / gradient evaluation
        exchanges one all-reduce of M^2 + M + 2 doubles (plus one of the small gradient vector): see
        include/gpitch_abi.h gp_sgpr_bound_begin / _end.  Predictions need the whole window on one GPU."""
        # mean_function (sgpr_ss.py:14,25): subtracted from Y in the bound (:40) and in the exact posterior (:90), added back
        # to predicted means (:95); gpitch_amd.mean_functions.Constant / Linear carry trainable Params as GPflow's do
        # (optimize() trains them unless .fixed), any other callable is a fixed function of the inputs
        if mean_function is not None and not callable(mean_function):
            raise TypeError("mean_function must be callable on an (n, 1) array (gpitch_amd.mean_functions)")
        object.__setattr__(self, "mean_function", mean_function)
        if not isinstance(kern, Add):
            kern = Add([kern])
        if reg:
            kern.var_vector = ParamList([k.variance for k in kern.kern_list])   # sgpr_ss.py:17-22
        Y = np.asarray(Y, dtype=np.float64)
        if Y.ndim != 2 or Y.shape[1] < 1:
            raise ValueError("Y must be N x D")
        self.X = DataHolder(np.asarray(X, dtype=np.float64).reshape(-1, 1))
        self.Y = DataHolder(Y)
        self.Z = DataHolder(np.asarray(Z, dtype=np.float64).reshape(-1, 1), on_shape_change='pass')   # :26
        self.kern = kern
        self.reg = reg
        self.likelihood = _Gaussian()
        # D = Y.shape[1] outputs share X, Z, the kernel and the noise (sgpr_ss.py:38 output_dim): the bound is the sum of
        # the D one-column bounds (every term of :55-62 is linear in the columns or carries the factor output_dim), so
        # D > 1 is D evaluations of the one-column launch sequence, summed on the device (_bound).  The reference's
        # callers only ever pass one column.
        self.num_latent = Y.shape[1]
        self._handle = handle
        self._plan = None
        self._plan_key = None
        if shard is not None:
            rank, world = int(shard[0]), int(shard[1])
            if not (0 <= rank < world):
                raise ValueError("shard=(rank, world) needs 0 <= rank < world")
            shard = (rank, world)
        object.__setattr__(self, "_shard", shard)
        # float_type: the reference's dtype setting (sgpr_ss.py:7 float_type = settings.dtypes.float_type); float32 puts
        # the M x N strips and the strip products on the float32 matrix path (gp_sgpr_set_precision)
        object.__setattr__(self, "_bits", _lib.precision_bits(float_type))

    def _frames(self):
        """frame indices this rank holds (all of them when unsharded): contiguous, sizes differ by at most one"""
        N = self.X.shape[0]
        if not self._shard:
            return slice(0, N)
        rank, world = self._shard
        base, extra = divmod(N, world)
        lo = rank * base + min(rank, extra)
        return slice(lo, lo + base + (1 if rank < extra else 0))

    # data can be swapped between windows (transcription.py:253-263: model.X = x; model.Y = 20*y; model.Z = z)
    def __setattr__(self, name, value):
        cur = self.__dict__.get(name)
        if isinstance(cur, DataHolder) and not isinstance(value, DataHolder):
            value = np.asarray(value, dtype=np.float64)
            if name == "Y" and value.ndim == 2:
                object.__setattr__(self, name, DataHolder(value))
                object.__setattr__(self, "num_latent", value.shape[1])
            else:
                object.__setattr__(self, name, DataHolder(value.reshape(-1, 1)))
        else:
            Parameterized.__setattr__(self, name, value)

    # ------------------------------------------------------------------------------------------
    def _compile(self, n_pred=0):
        h = self._handle = self._handle or _lib.default_handle()
        kl = self.kern.kern_list
        fr = self._frames()
        N, M = fr.stop - fr.start, self.Z.shape[0]
        if N < 1:
            raise ValueError("more ranks than frames")
        maxN = max(N, n_pred)
        key = (maxN, M, tuple((k.type_code, int(k.num_partials)) for k in kl), bool(self.reg))
        if self._plan is not None and self._plan_key == key:
            return
        self._destroy()
        P = len(kl)
        i32 = C.c_int32 * P
        self._keep = (i32(*[k.type_code for k in kl]), i32(*[int(k.num_partials) for k in kl]))
        cfg = _lib.SgprConfig(P, maxN, M, self._keep[0], self._keep[1], 1e-6, int(bool(self.reg)))
        plan = C.c_void_p()
        h.check(h.lib.gp_sgpr_create(h.h, C.byref(cfg), C.byref(plan)))
        self._plan, self._plan_key = plan, key
        if self._bits == 32:
            h.check(h.lib.gp_sgpr_set_precision(plan, 32))
        self._ws = h.workspace(h.lib.gp_sgpr_workspace_bytes(plan))
        h.check(h.lib.gp_sgpr_set_workspace(plan, self._ws.data_ptr(), self._ws.numel()))
        self._nparams = int(h.lib.gp_sgpr_num_params(plan))
        self._bound_dev = h.zeros(1)

    def _dev(self, name, host):
        """device copy of `host` in a buffer that is reused while the size stays the same: stable pointers let the
        engine keep its descriptors and replay the recorded evaluation graph across evaluations and windows"""
        h = self._handle
        host = np.ascontiguousarray(np.asarray(host, dtype=np.float64).reshape(-1))
        cur = self.__dict__.get(name)
        if cur is None or cur.numel() != host.size or cur.device != h.device:
            cur = h.empty(host.size)
            object.__setattr__(self, name, cur)
        cur.copy_(h.torch.as_tensor(host))
        return cur

    def _pack(self):
        vec = [self.likelihood.variance.value.reshape(-1)]
        for k in self.kern.kern_list:
            vec.append(k.theta())
        host = np.concatenate(vec)
        assert host.size == self._nparams
        fr = self._frames()
        self._dev("_params", host)
        self._dev("_Xd", self.X._array[fr])
        self._upload_err()
        self._dev("_Zd", self.Z._array)
        object.__setattr__(self, "_n_local", fr.stop - fr.start)
        object.__setattr__(self, "_obj_state", None)      # Param values / .fixed flags may have changed

    def _err_host(self):
        """err = Y - mean_function(X) on this rank's frames (sgpr_ss.py:40); a mean function of one column is
        subtracted from every column"""
        fr = self._frames()
        yv = self.Y._array[fr]
        if self.mean_function is not None:
            mv = np.asarray(self.mean_function(self.X._array[fr]), dtype=np.float64).reshape(yv.shape[0], -1)
            yv = yv - mv
        return yv

    def _upload_err(self):
        """the residual columns on the device: `_Yd` is the column the library reads (a stable pointer: the recorded
        launch sequence stays valid); with D > 1 `_Yall` holds all of them, column-major, and _bound copies each in turn"""
        err = self._err_host()
        if self.num_latent == 1:
            self._dev("_Yd", err)
            object.__setattr__(self, "_Yall", None)
            return
        self._dev("_Yall", np.ascontiguousarray(err.T))
        self._dev("_Yd", err[:, 0])

    def _columns(self):
        """iterate over the output columns with `_Yd` holding the current one"""
        D = self.num_latent
        if D == 1:
            yield 0
            return
        n = self._Yd.numel()
        for d in range(D):
            self._Yd.copy_(self._Yall[d * n:(d + 1) * n])
            yield d

    def _mean_params(self):
        """trainable Params of the mean function (gpflow.mean_functions.Constant.c, Linear.A / .b), [] for a plain callable"""
        mf = self.mean_function
        return list(mf.params()) if (mf is not None and hasattr(mf, "params") and hasattr(mf, "grad_from_residual")) else []

    def _bound(self, grad=None, per_column=None):
        """the bound (and its gradient into the device vector `grad`): the sum over the D output columns of the
        one-column evaluation (per_column(d) is called after each, while the plan still holds that column's state)"""
        D = self.num_latent
        if D == 1:
            v = self._bound_column(grad)
            if per_column is not None:
                per_column(0)
            return v
        h = self._handle
        total, gsum = 0.0, (None if grad is None else h.zeros(grad.numel()))
        for d in self._columns():
            total += self._bound_column(grad)
            if grad is not None:
                gsum += grad
            if per_column is not None:
                per_column(d)
        if self.reg:
            # every column's bound carries the whole L1 term -beta sum |variance_k| (sgpr_ss.py:64-68): keep one
            beta, off = 1000., 1
            corr = np.zeros(self._nparams)
            for k in self.kern.kern_list:
                th = k.theta()                    # th[0]: the kernel's variance in the library's layout
                total += (D - 1) * beta * abs(th[0])
                corr[off] = (D - 1) * beta * np.sign(th[0])
                off += th.size
            if grad is not None:
                gsum += h.to_device(corr)
        if grad is not None:
            grad.copy_(gsum)
        return total

    def _bound_column(self, grad=None):
        """one evaluation of the one-column bound (and gradient into the device vector `grad`) on this model's frames, for
        the residual column in `_Yd`; the frame-sharded form runs begin -> all-reduce -> end -> all-reduce(grad)"""
        h = self._handle
        out = C.c_double()
        n = self._n_local
        args = (self._plan, self._params.data_ptr(), self._Xd.data_ptr(), self._Yd.data_ptr(), n)
        if not self._shard:
            if grad is None:
                h.check(h.lib.gp_sgpr_bound(*args, self._Zd.data_ptr(), self._bound_dev.data_ptr(), C.byref(out)))
            else:
                h.check(h.lib.gp_sgpr_bound_grad(*args, self._Zd.data_ptr(), self._bound_dev.data_ptr(), C.byref(out),
                                                 grad.data_ptr()))
            return out.value
        from .dist import allreduce_sum_, rccl_comm
        xchg = self.__dict__.get("_xchg")
        need = int(h.lib.gp_sgpr_exchange_doubles(self._plan))
        if xchg is None or xchg.numel() != need:
            xchg = h.empty(need)
            object.__setattr__(self, "_xchg", xchg)
        if "_comm_cache" not in self.__dict__:
            object.__setattr__(self, "_comm_cache", rccl_comm(h, self._shard[1]))
        comm = self._comm_cache
        if comm is not None:
            # an RCCL group: begin -> all-reduce -> end -> all-reduce(grad) inside ONE library call (gp_sgpr_bound_grad_sharded)
            h.check(h.lib.gp_sgpr_bound_grad_sharded(args[0], comm, *args[1:], self.X.shape[0], self._Zd.data_ptr(), xchg.data_ptr(),
                                                     self._bound_dev.data_ptr(), C.byref(out),
                                                     None if grad is None else grad.data_ptr()))
            return out.value
        h.check(h.lib.gp_sgpr_bound_begin(*args, self._Zd.data_ptr(), xchg.data_ptr()))
        allreduce_sum_(xchg)
        h.check(h.lib.gp_sgpr_bound_end(*args, self.X.shape[0], self._Zd.data_ptr(), xchg.data_ptr(),
                                        self._bound_dev.data_ptr(), C.byref(out),
                                        None if grad is None else grad.data_ptr(), int(self._shard[0] == 0)))
        if grad is not None:
            allreduce_sum_(grad)
        return out.value

    def build_likelihood(self):
        """the bound on the marginal likelihood (sgpr_ss.py:29-71)"""
        self._compile()
        self._pack()
        return self._bound()

    def compute_log_likelihood(self):
        return self.build_likelihood()

    # ---- shared by the predictors and the samplers ----
    def _refuse_shard(self):
        if self._shard:
            raise NotImplementedError("predictions of a frame-sharded window: build the model unsharded on one GPU")

    def _source_columns(self, Xnew, call):
        """the column loop of the per-source predictors, after _compile / _pack: call(xs, mean, var, column) on every output
        column, with the device copy of Xnew and the (P, n) device arrays it fills: (means (P, n, D), variances (P, n))"""
        h, P, n = self._handle, len(self.kern.kern_list), Xnew.size
        xs, mean, var = h.to_device(Xnew), h.empty(P, n), h.empty(P, n)
        m = np.empty((P, n, self.num_latent))
        for d in self._columns():
            call(xs, mean, var, d)
            m[:, :, d] = mean.cpu().numpy()
        return m, var.cpu().numpy()

    def _per_source(self, m, v):
        """what the per-source predictors return: (list of P means (n, D), list of P variances tiled to (n, D))"""
        D = self.num_latent
        return [m[i] for i in range(m.shape[0])], [np.tile(v[i].reshape(-1, 1), (1, D)) for i in range(v.shape[0])]

    def predict_f(self, Xnew, full_cov=False):
        """mean and variance of the mixture at Xnew (GPflow 0.5 SGPR.build_predict; full_cov=True — `predict_f_full_cov`
        in GPflow — returns the n x n x 1 covariance)"""
        self._refuse_shard()
        Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        n = Xnew.size
        self._compile(n_pred=n)
        self._pack()
        h = self._handle
        xs = h.to_device(Xnew)
        mean, var = h.empty(n), h.empty(n)
        cov = h.empty(n, n) if full_cov else None
        D = self.num_latent
        mu = np.empty((n, D))
        for d in self._columns():                   # the mean is linear in the column, the variance does not see it
            if full_cov:
                h.check(h.lib.gp_sgpr_predict_f_full(self._plan, self._params.data_ptr(), self._Xd.data_ptr(),
                                                     self._Yd.data_ptr(), self.X.shape[0], self._Zd.data_ptr(), xs.data_ptr(),
                                                     n, mean.data_ptr(), var.data_ptr(), cov.data_ptr()))
            else:
                h.check(h.lib.gp_sgpr_predict_f(self._plan, self._params.data_ptr(), self._Xd.data_ptr(), self._Yd.data_ptr(),
                                                self.X.shape[0], self._Zd.data_ptr(), xs.data_ptr(), n, mean.data_ptr(),
                                                var.data_ptr()))
            mu[:, d] = mean.cpu().numpy()
        if self.mean_function is not None:          # SGPR.build_predict: + mean_function(Xnew)
            mu = mu + np.asarray(self.mean_function(Xnew.reshape(-1, 1)), dtype=np.float64).reshape(n, -1)
        if full_cov:                                # GPflow tiles the covariance over the D outputs
            return mu, np.tile(cov.cpu().numpy().reshape(n, n, 1), (1, 1, D))
        return mu, np.tile(var.cpu().numpy().reshape(-1, 1), (1, D))

    def predict_f_full_cov(self, Xnew):
        """GPflow's AutoFlow'd name for predict_f(full_cov=True)"""
        return self.predict_f(Xnew, full_cov=True)

    def build_predict_source(self, Xnew, full_cov=False):
        """p(source* | Y): exact GP on the N training frames, one posterior per kernel in kern_list
        (sgpr_ss.py:73-106; the variance uses the SUM kernel's Kdiag as the reference does)."""
        self._refuse_shard()
        Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        n, N, P = Xnew.size, self.X.shape[0], len(self.kern.kern_list)
        self._compile()
        self._pack()
        h = self._handle
        ws = h.workspace(h.lib.gp_sgpr_predict_source_workspace_bytes(N, n))
        cov = h.empty(P, n, n) if full_cov else None

        def call(xs, mean, var, _):                 # one exact posterior per column (the reference's callers have one)
            if full_cov:
                h.check(h.lib.gp_sgpr_predict_source_full(self._plan, self._params.data_ptr(), self._Xd.data_ptr(),
                                                          self._Yd.data_ptr(), N, xs.data_ptr(), n, mean.data_ptr(),
                                                          var.data_ptr(), cov.data_ptr(), ws.data_ptr(), ws.numel()))
            else:
                h.check(h.lib.gp_sgpr_predict_source(self._plan, self._params.data_ptr(), self._Xd.data_ptr(),
                                                     self._Yd.data_ptr(), N, xs.data_ptr(), n, mean.data_ptr(), var.data_ptr(),
                                                     ws.data_ptr(), ws.numel()))

        m, v = self._source_columns(Xnew, call)
        if self.mean_function is not None:          # sgpr_ss.py:95 adds it to EVERY source's mean
            m = m + np.asarray(self.mean_function(Xnew.reshape(-1, 1)), dtype=np.float64).reshape(1, n, -1)
        if full_cov:                                # sgpr_ss.py:95-99: tiled to n x n x D
            c = cov.cpu().numpy()
            return [m[i] for i in range(P)], [np.tile(c[i].reshape(n, n, 1), (1, 1, self.num_latent)) for i in range(P)]
        return self._per_source(m, v)               # :101-102

    def predict_s(self, Xnew):
        """sgpr_ss.py:108-114"""
        return self.build_predict_source(Xnew)

    def predict_s_sparse(self, Xnew):
        """Sparse posterior of every source at Xnew: (list of P means (n, D), list of P variances (n, D)).

        Source p under the optimal q(u) of the collapsed bound (gp_sgpr_predict_source_sparse): GPflow's
        SGPR.build_predict with the one kernel K_p in place of the sum, O(M^2 n) per source and independent of N, where
        predict_s factorises the N x N exact GP.  It approximates predict_s; the variance starts from the source's own
        Kdiag, not the sum kernel's (sgpr_ss.py:101).  The mean function is NOT added: the sources are zero-mean GPs, and
        sum_p smean_p + mean_function(Xnew) is predict_f's mean.  Xnew may be longer than the training window."""
        self._refuse_shard()
        Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        self._compile()
        self._pack()
        h = self._handle

        def call(xs, mean, var, _):                 # the mean is linear in the column, the variance does not see it
            h.check(h.lib.gp_sgpr_predict_source_sparse(self._plan, self._params.data_ptr(), self._Xd.data_ptr(),
                                                        self._Yd.data_ptr(), self.X.shape[0], self._Zd.data_ptr(),
                                                        xs.data_ptr(), Xnew.size, mean.data_ptr(), var.data_ptr()))

        return self._per_source(*self._source_columns(Xnew, call))

    def _ssm_call(self, Xnew, who):
        """the smoother on every output column: (means (P, n, D), variances (P, n), log-likelihoods (D,))"""
        self._refuse_shard()
        kl = self.kern.kern_list
        d, P = ssm_state_dim(kl, who)                 # raises for an unsupported kernel or d, before any device work
        Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        n, N = Xnew.size, self.X.shape[0]
        order, out_step, steps = ssm_timeline(self.X._array, Xnew)
        order, out_step = np.ascontiguousarray(order), np.ascontiguousarray(out_step)
        self._compile()
        self._pack()
        h = self._handle
        ll = h.empty(1)
        ws = h.workspace(h.lib.gp_ssm_smooth_workspace_bytes(d, steps, P, 1))
        lls = np.empty(self.num_latent)

        def call(xs, mean, var, c):                   # (no new point: the forward walk alone, nothing but ll is written)
            h.check(h.lib.gp_sgpr_predict_source_ssm(self._plan, self._params.data_ptr(), self._Xd.data_ptr(),
                                                     self._Yd.data_ptr(), N, xs.data_ptr() if n else None, n,
                                                     order.ctypes.data, out_step.ctypes.data if n else None, steps,
                                                     mean.data_ptr() if n else None, var.data_ptr() if n else None,
                                                     ll.data_ptr(), ws.data_ptr(), ws.numel()))
            lls[c] = float(ll.cpu().numpy()[0])

        return self._source_columns(Xnew, call) + (lls,)

    def predict_s_ssm(self, Xnew):
        """The exact posterior of every source at Xnew: (list of P means (n, D), list of P variances (n, D)).

        What predict_s computes (sgpr_ss.py:73-114), without its N x N factorisation: a sum of kernels with a Matern-1/2
        envelope (Matern12, MercerMatern12sm, Matern12sm) is a linear-Gaussian state-space model of dimension d = the sum of
        sample_components(kern), and a Kalman filter with a Bryson-Frazier backward pass (gp_sgpr_predict_source_ssm) gives
        p(f_p | y) at every frame in O((N + n) d^2), for any N, with no inducing points (Z plays no part).  Conventions as
        predict_s_sparse: the variance starts from the source's OWN k_p(x, x) where predict_s starts from the sum kernel's,
        so svar of predict_s = this variance + (Kdiag_sum - Kdiag_p); the mean function is NOT added (the residual
        Y - mean_function(X) is what is filtered); columns are looped, the variance computed once.  Exact for the idealised
        kernels r = |x - x'|: predict_s's kernels carry the reference's 1e-12 under the square root, a first-order
        difference that grows with 1 / noise variance (about 1e-6 of the mean at noise 0.01).  Xnew may lie on training frames,
        between them or outside the window, in any order, with repeats.  NotImplementedError, before any device work, for a
        kernel without the Ornstein-Uhlenbeck form (naming it and its index in the sum) and for d > 128 (naming d)."""
        m, v, _ = self._ssm_call(Xnew, "predict_s_ssm")
        return self._per_source(m, v)

    def exact_log_likelihood(self):
        """log p(Y | parameters) of the exact GP (the quantity the collapsed bound of build_likelihood lies below, at any
        Z), from the forward walk of the smoother alone: the sum over the D columns, the mean function subtracted.  Exact
        for the idealised kernels r = |x - x'|, so it differs from a dense evaluation with the reference's kernels (1e-12
        under the square root) in about the fifth significant digit.  Same scope as predict_s_ssm."""
        return float(self._ssm_call(np.zeros(0), "exact_log_likelihood")[2].sum())

    def _exact_setup(self, who):
        """what an evaluation of the exact likelihood and its gradient needs beside the parameters: the timeline of the
        training frames, the workspace and the result buffers.  Raises before any device work (scope as predict_s_ssm)."""
        if self._shard:
            raise NotImplementedError("%s: a frame-sharded window has no exact likelihood (the state-space walk is sequential "
                                      "in the frames): build the model unsharded on one GPU" % who)
        d, P = ssm_state_dim(self.kern.kern_list, who)
        N = self.X.shape[0]
        order = np.ascontiguousarray(np.argsort(self.X._array.reshape(-1), kind="stable").astype(np.int32))
        self._compile()
        self._pack()
        h = self._handle
        ex = {"N": N, "order": order, "ws": h.workspace(h.lib.gp_ssm_score_workspace_bytes(d, N, P, 1)), "ll": h.empty(1),
              "grad": h.empty(self._nparams), "resid": h.empty(N) if self._mean_params() else None}
        object.__setattr__(self, "_exact_st", ex)
        return ex

    def _exact_eval(self, ex, mean_grad):
        """(log-likelihood, its gradient in the engine's parameters, the mean function's entries) at the device's `_params` and
        residual columns: the sum over the D columns of gp_sgpr_exact_loglik_grad"""
        h = self._handle
        value, g = 0.0, np.zeros(self._nparams)
        mps = self._mean_params()
        gm = np.zeros(len(mps))
        r = ex["resid"] if mean_grad else None
        for _ in self._columns():
            h.check(h.lib.gp_sgpr_exact_loglik_grad(self._plan, self._params.data_ptr(), self._Xd.data_ptr(), self._Yd.data_ptr(),
                                                    ex["N"], ex["order"].ctypes.data, ex["ll"].data_ptr(), ex["grad"].data_ptr(),
                                                    r.data_ptr() if r is not None else None, ex["ws"].data_ptr(),
                                                    ex["ws"].numel()))
            value += float(ex["ll"].cpu().numpy()[0])
            g += ex["grad"].cpu().numpy()
            if r is not None:
                gm += np.concatenate(self.mean_function.grad_from_residual(self.X._array, r.cpu().numpy()))
        return value, g, gm

    def exact_log_likelihood_and_grad(self):
        """(exact_log_likelihood(), its gradient over _param_list() in constrained parameters): noise variance, every
        kernel's variance, lengthscale, energies and frequencies, then the mean function's Params.  One forward walk with
        its history and one backward walk that carries the score (gp_sgpr_exact_loglik_grad), O(N d^2) per column, summed
        over the D columns; Z plays no part.  The value has the bits of exact_log_likelihood().  Same scope as
        predict_s_ssm."""
        ex = self._exact_setup("exact_log_likelihood_and_grad")
        value, g, gm = self._exact_eval(ex, bool(self._mean_params()))
        object.__setattr__(self, "_exact_st", None)
        return value, np.concatenate([g, gm])

    def _draw(self, who, names, shapes, eps, Xnew, S, seed, doubles, ws_bytes, call):
        """The draw loop of sample_s_sparse / sample_s_ssm: a list of P arrays (S, n, D).  `shapes`: of the standard-normal
        arrays `names` for one column, S first; `eps`: the caller's (a leading D axis each when D > 1) or None for torch.randn
        from a generator seeded by `seed`, at most SAMPLE_EPS_BYTES of them (`doubles` per draw) per library call;
        ws_bytes(chunk): the workspace of `chunk` draws; call(xs, sc, es, out, ws): the library call for sc draws at the
        device copy xs of Xnew from the normals es into out (P, sc, n).  Both run after _compile, when the handle exists."""
        P, n, D = len(self.kern.kern_list), Xnew.size, self.num_latent
        if eps is not None:
            eps = _check_eps(who, names, eps, [((D,) if D > 1 else ()) + sh for sh in shapes])
            eps = [e.reshape((D,) + sh) for e, sh in zip(eps, shapes)]
        self._compile()
        self._pack()
        h = self._handle
        xs = h.to_device(Xnew)
        chunk = S if eps is not None else _sample_chunk(S, doubles)
        ws = h.workspace(ws_bytes(chunk))
        out = h.empty(P, chunk, n)
        gen = None if eps is not None else _sample_generator(h, seed)
        res = np.empty((P, S, n, D))
        for d in self._columns():
            for s0 in range(0, S, chunk):
                sc = min(chunk, S - s0)
                if eps is not None:
                    es = [h.to_device(e[d]) for e in eps]       # (to_device makes them contiguous)
                else:
                    es = [h.torch.randn(sc, *sh[1:], dtype=h.torch.float64, device=h.device, generator=gen) for sh in shapes]
                call(xs, sc, es, out, ws)
                res[:, s0:s0 + sc, :, d] = out.reshape(-1)[:P * sc * n].reshape(P, sc, n).cpu().numpy()
        return [res[i] for i in range(P)]

    def sample_s_sparse(self, Xnew, num_samples=1, seed=None, eps=None):
        """Joint posterior draws of every source at Xnew under the q(u) of predict_s_sparse: a list of P arrays
        (num_samples, n, D).  A draw is joint across the n frames and across the P sources (gp_sgpr_sample_source_sparse:
        Matheron's rule on an exact O(n) prior sampler, no n x n matrix); its mean over many draws is predict_s_sparse's
        mean and its spread the joint posterior covariance.  Every kernel needs a Matern-1/2 envelope (MercerMatern12sm,
        Matern12sm, Matern12); the mean function is NOT added, as in predict_s_sparse.

        eps=None: the standard normals are torch.randn on the handle's device from a generator seeded by `seed`, drawn
        SAMPLE_EPS_BYTES at a time (the same seed and chunk size give the same draws); output columns get independent ones.
        eps=(eps_x, eps_z, eps_u) of shapes sample_eps_shapes(kern, n, M, num_samples), each with a leading D axis when
        D > 1, supplies them: the map is affine in eps and eps = 0 returns the posterior mean."""
        self._refuse_shard()
        kl = self.kern.kern_list
        C = int(sum(sample_components(kl)))           # raises for an unsupported kernel, before any device work
        Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        n, P, M, S = Xnew.size, len(kl), self.Z.shape[0], int(num_samples)
        if n < 1 or S < 1:
            raise ValueError("sample_s_sparse: needs at least one new point and one sample")
        order = np.ascontiguousarray(merged_order(Xnew, self.Z._array))

        def call(xs, sc, es, out, ws):
            h = self._handle
            h.check(h.lib.gp_sgpr_sample_source_sparse(self._plan, self._params.data_ptr(), self._Xd.data_ptr(),
                                                       self._Yd.data_ptr(), self.X.shape[0], self._Zd.data_ptr(),
                                                       xs.data_ptr(), n, order.ctypes.data, sc, es[0].data_ptr(),
                                                       es[1].data_ptr(), es[2].data_ptr(), out.data_ptr(), ws.data_ptr(),
                                                       ws.numel()))

        return self._draw("sample_s_sparse", ("eps_x", "eps_z", "eps_u"), sample_eps_shapes(kl, n, M, S), eps, Xnew, S, seed,
                          doubles=C * (n + M) + 2 * M, call=call,
                          ws_bytes=lambda chunk: self._handle.lib.gp_sgpr_sample_source_workspace_bytes(M, P, C, n, chunk, 1))

    def sample_s_ssm(self, Xnew, num_samples=1, seed=None, eps=None):
        """Joint draws of every source at Xnew from the EXACT posterior of predict_s_ssm: a list of P arrays
        (num_samples, n, D).  A draw is joint across the n frames and across the P sources (gp_sgpr_sample_source_ssm: Durbin
        and Koopman's simulation smoother in its disturbance form, three O((N + n) d) walks per draw behind one gain walk; no
        inducing points, no d x d array per step, any N); its mean over many draws is predict_s_ssm's mean and its spread the
        joint posterior covariance.  Scope and conventions as predict_s_ssm: the mean function is NOT added, Xnew in any
        order, repeats repeat their value.  NotImplementedError, before any device work, for a kernel without the
        Ornstein-Uhlenbeck form and for d > 128.

        eps=None: the standard normals are torch.randn on the handle's device from a generator seeded by `seed`, drawn
        SAMPLE_EPS_BYTES at a time (the same seed and chunk size give the same draws); output columns get independent ones.
        eps=(eps_x, eps_y) of shapes ssm_sample_eps_shapes(kern, steps, N, num_samples), steps = ssm_timeline(X, Xnew)[2],
        each with a leading D axis when D > 1, supplies them: the map is affine in eps, and eps = 0 returns the exact
        posterior mean from a workspace without the smoother's steps * d^2 history.  eps_x is STEP-major and indexed along
        the MERGED timeline, unlike sample_s_sparse's component-major blocks: the same seed (or eps) with another Xnew is
        another draw, not the same path seen at other frames."""
        self._refuse_shard()
        kl = self.kern.kern_list
        d, P = ssm_state_dim(kl, "sample_s_ssm")      # raises for an unsupported kernel or d, before any device work
        Xnew = np.asarray(Xnew, dtype=np.float64).reshape(-1)
        n, N, S = Xnew.size, self.X.shape[0], int(num_samples)
        if n < 1 or S < 1:
            raise ValueError("sample_s_ssm: needs at least one new point and one sample")
        order, out_step, steps = ssm_timeline(self.X._array, Xnew)
        order, out_step = np.ascontiguousarray(order), np.ascontiguousarray(out_step)

        def call(xs, sc, es, out, ws):
            h = self._handle
            h.check(h.lib.gp_sgpr_sample_source_ssm(self._plan, self._params.data_ptr(), self._Xd.data_ptr(),
                                                    self._Yd.data_ptr(), N, xs.data_ptr(), n, order.ctypes.data,
                                                    out_step.ctypes.data, steps, sc, es[0].data_ptr(), es[1].data_ptr(),
                                                    out.data_ptr(), ws.data_ptr(), ws.numel()))

        return self._draw("sample_s_ssm", ("eps_x", "eps_y"), ssm_sample_eps_shapes(kl, steps, N, S), eps, Xnew, S, seed,
                          doubles=steps * d + N, call=call,
                          ws_bytes=lambda chunk: self._handle.lib.gp_ssm_sample_workspace_bytes(d, steps, P, chunk, 1))

    # ---- training: GPflow Model.optimize -> scipy L-BFGS-B on the free state (transcription.py:283) ----
    def _param_list(self):
        ps = [self.likelihood.variance]
        for k in self.kern.kern_list:
            ps.extend(k.theta_params())
        return ps + self._mean_params()     # (after the engine's parameter vector: they live on the host)

    def _objective_setup(self):
        """vectorised view of the free state for _objective (rebuilt by optimize(): .fixed flags, transforms and the
        values of the fixed Params are read once per optimisation, not once per evaluation)"""
        from .param import Identity, Log1pe, Logistic
        ps = self._param_list()
        free_idx = np.array([i for i, p in enumerate(ps) if not p.fixed], dtype=np.int64)
        kind = np.zeros(free_idx.size, dtype=np.int64)      # 0 identity, 1 positive, 2 logistic, 3 anything else
        lo = np.zeros(free_idx.size)
        span = np.ones(free_idx.size)
        other = {}
        for j, i in enumerate(free_idx):
            tr = ps[i].transform
            if isinstance(tr, Identity):
                kind[j] = 0
            elif isinstance(tr, Log1pe):
                kind[j] = 1
                lo[j] = tr._lower
            elif isinstance(tr, Logistic):
                kind[j] = 2
                lo[j], span[j] = tr.a, tr.b - tr.a
            else:
                kind[j] = 3
                other[j] = tr
        st = {"ps": ps, "free_idx": free_idx, "kind": kind, "lo": lo, "span": span, "other": other,
              "vals0": np.array([p.value[0] for p in ps])}
        object.__setattr__(self, "_obj_state", st)
        return st

    @staticmethod
    def _free_to_params(st, x):
        """forward transforms and their derivatives for the whole free vector at once"""
        x = np.asarray(x, dtype=np.float64)
        kind, lo, span = st["kind"], st["lo"], st["span"]
        sig = 1. / (1. + np.exp(-x))
        y = np.where(kind == 1, np.logaddexp(0., x) + lo, np.where(kind == 2, lo + span * sig, x))
        dy = np.where(kind == 1, sig, np.where(kind == 2, span * sig * (1. - sig), 1.))
        for j, tr in st["other"].items():       # (x may be one free vector or a (windows, n) stack of them)
            col = np.atleast_1d(x[..., j])
            y[..., j] = np.array([tr.forward(np.array([v]))[0] for v in col]).reshape(np.shape(x[..., j]))
            dy[..., j] = np.array([tr.dforward(np.array([v]))[0] for v in col]).reshape(np.shape(x[..., j]))
        return y, dy

    def _objective(self, x_free):
        """(-(bound), -d bound / d free-state) — GPflow Model._objective"""
        h = self._handle
        st = self.__dict__.get("_obj_state") or self._objective_setup()
        y, dy = self._free_to_params(st, x_free)
        vals = st["vals0"].copy()
        vals[st["free_idx"]] = y
        nd = self._nparams                        # the engine's parameters; the mean function's follow them
        mps = self._mean_params()
        train_mean = bool(mps) and bool(np.any(st["free_idx"] >= nd))
        if train_mean:                            # a new mean function: new residuals (same device buffer: the recorded
            for p_, v in zip(mps, vals[nd:]):     # launch sequence stays valid)
                p_._array = np.array([v], dtype=np.float64)
            self._upload_err()
        self._dev("_params", vals[:nd])
        grad = self.__dict__.get("_grad_dev")
        if grad is None or grad.numel() != nd:
            grad = h.empty(nd)
            object.__setattr__(self, "_grad_dev", grad)
        gm = np.zeros(len(mps))

        def mean_grad(d):
            # d bound / d err of the column just evaluated, chained through the mean function (shared by the columns)
            r = self.__dict__.get("_resid_dev")
            if r is None or r.numel() != self._n_local:
                r = h.empty(self._n_local)
                object.__setattr__(self, "_resid_dev", r)
            h.check(h.lib.gp_sgpr_residual_grad(self._plan, self._params.data_ptr(), self._Yd.data_ptr(), self._n_local,
                                                r.data_ptr()))
            gm[:] += np.concatenate(self.mean_function.grad_from_residual(self.X._array[self._frames()], r.cpu().numpy()))

        value = self._bound(grad, per_column=mean_grad if train_mean else None)
        g = grad.cpu().numpy()
        if mps:
            if train_mean:
                if self._shard:                   # a frame-sharded window: every rank holds its slice's share of the sums
                    from .dist import allreduce_sum_
                    gm = allreduce_sum_(h.torch.as_tensor(gm)).numpy()
            g = np.concatenate([g, gm])
        return -value, -(g[st["free_idx"]] * dy)

    def _objective_exact(self, x_free):
        """(-(exact log-likelihood), -d / d free-state): _objective with the state-space score in the bound's place"""
        st, ex = self._obj_state, self._exact_st
        y, dy = self._free_to_params(st, x_free)
        vals = st["vals0"].copy()
        vals[st["free_idx"]] = y
        nd = self._nparams
        mps = self._mean_params()
        train_mean = bool(mps) and bool(np.any(st["free_idx"] >= nd))
        if train_mean:
            for p_, v in zip(mps, vals[nd:]):
                p_._array = np.array([v], dtype=np.float64)
            self._upload_err()
        self._dev("_params", vals[:nd])
        value, g, gm = self._exact_eval(ex, train_mean)
        g = np.concatenate([g, gm])
        return -value, -(g[st["free_idx"]] * dy)

    def optimize(self, method='L-BFGS-B', tol=None, callback=None, maxiter=1000, disp=False, objective="bound", **kw):
        """GPflow's Model.optimize on the free state.  objective="bound" (the default) climbs the collapsed bound of
        build_likelihood; objective="exact" climbs exact_log_likelihood() by its exact gradient
        (exact_log_likelihood_and_grad): same driver, transforms and .fixed handling, Z plays no part, res.fun is minus the
        exact log-likelihood.  "exact" has the scope of predict_s_ssm and takes neither a frame-sharded window nor reg=True
        (the L1 term belongs to the bound): NotImplementedError before any device work."""
        from scipy.optimize import minimize
        if objective not in ("bound", "exact"):
            raise ValueError('optimize: objective is "bound" or "exact"')
        exact = objective == "exact"
        if exact:
            if self.reg:
                raise NotImplementedError('optimize(objective="exact"): reg=True adds its L1 term to the collapsed bound; the '
                                          'exact likelihood has none (build the model with reg=False)')
            self._exact_setup('optimize(objective="exact")')
        else:
            self._compile()
            self._pack()
        st = self._objective_setup()
        ps, free_idx = st["ps"], st["free_idx"]
        x0 = np.array([ps[i].transform.backward(ps[i].value)[0] for i in free_idx])
        try:
            res = minimize(self._objective_exact if exact else self._objective, x0, jac=True, method=method, tol=tol,
                           callback=callback, options=dict(maxiter=maxiter, disp=disp))
        finally:
            object.__setattr__(self, "_exact_st", None)
        y, _ = self._free_to_params(st, res.x)
        for j, i in enumerate(free_idx):
            ps[i].value = y[j:j + 1]
        object.__setattr__(self, "_obj_state", None)
        return res

    def _destroy(self):
        if self._plan is not None and self._handle is not None and self._handle.h:
            self._handle.sync()
            self._handle.lib.gp_sgpr_destroy(self._plan)
        self._plan = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass
