"""Pdgp — pitch detection using Gaussian processes: same constructor, attributes and methods as
gpitch/pdgp.py:48-208, executed by the HIP engine (csrc/pdgp.hip, bwd.hip) through the C-ABI.

    m = Pdgp(x, y, z, kern=[[kact...], [kcom...]], whiten=True, minibatch_size=None, nlinfun=logistic_tf)
    m.za.fixed = True; m.zc.fixed = True
    m.optimize(method=AdamOptimizer(0.005), maxiter=1000)
    mean_a, var_a, mean_c, var_c, mean_src = m.predict_act_n_com(xtest)
"""
import ctypes as C

import numpy as np

from . import _lib, flatvec
from .flatvec import col
from .likelihoods import MpdLik
from .methods import logistic, logistic_tf, nlin_code
from .sgpr_ss import _sample_chunk, _sample_generator, merged_order
from .param import MinibatchData, Param, ParamList, Parameterized, draw_in_lockstep, param_version
from .train import AdamOptimizer, NatGradAdam, OptimizeResult

jitter = 1e-6   # gpflow settings.numerics.jitter_level (pdgp.py:14)
# sample_sources: standard normals per point of the kernels that have an exact state-space prior sampler (0: 2 m)
_SAMPLE_COMPONENTS = {_lib.KERN_MATERN12: 1, _lib.KERN_MATERN32: 2, _lib.KERN_MERCER_MATERN12SM: 0, _lib.KERN_MATERN12SM: 0}


def predict_windowed(model, xnew, ws=1600):
    """gpitch/pdgp.py:17-44 (Python-2 integer division at :25 made explicit; the trailing remainder
    is dropped exactly as there).  NOTE the reference applies the *default* logistic for the source
    mean here (:35,:42) regardless of model.nlinfun; kept."""
    n = xnew.size
    P = model.num_sources
    m_a_l = [[] for _ in range(P)]
    v_a_l = [[] for _ in range(P)]
    m_c_l = [[] for _ in range(P)]
    v_c_l = [[] for _ in range(P)]
    m_s_l = [[] for _ in range(P)]
    for i in range(n // ws):
        x = xnew[i * ws:(i + 1) * ws].copy()
        m_a, v_a = model.predict_act(x)
        m_c, v_c = model.predict_com(x)
        for j in range(P):
            m_a_l[j].append(m_a[j].copy())
            v_a_l[j].append(v_a[j].copy())
            m_c_l[j].append(m_c[j].copy())
            v_c_l[j].append(v_c[j].copy())
    for j in range(P):
        m_a_l[j] = np.asarray(m_a_l[j]).reshape(-1, 1)
        v_a_l[j] = np.asarray(v_a_l[j]).reshape(-1, 1)
        m_c_l[j] = np.asarray(m_c_l[j]).reshape(-1, 1)
        v_c_l[j] = np.asarray(v_c_l[j]).reshape(-1, 1)
        m_s_l[j] = logistic(m_a_l[j]) * m_c_l[j]
    return m_a_l, v_a_l, m_c_l, v_c_l, m_s_l


def pitch_assignment(num_sources, world_size, rank):
    """pitches held by `rank` when one model is spread over `world_size` GPUs (pitch p -> rank p mod world)"""
    return list(range(rank, num_sources, world_size))


class Pdgp(Parameterized):
    def __init__(self, x, y, z, kern, whiten=True, minibatch_size=None, nlinfun=logistic_tf, handle=None,
                 max_predict_batch=None, shard=None, float_type=None):
        """Pitch detection using Gaussian process (pdgp.py:49-111).
        x, y: (N,1) arrays; z = [[za_0..], [zc_0..]]; kern = [[kern_act...], [kern_com...]].

        shard=(rank, world) spreads ONE model over `world` GPUs (one process each): this rank's engine plan holds
        the pitches {p : p mod world == rank} (both GPs of a pitch), the likelihood noise is replicated, and each
        ELBO evaluation exchanges one all-reduce of 3n+1 doubles (include/gpitch_abi.h: gp_pdgp_elbo_begin/_end).
        shard=("gp", rank, world) deals the 2P LATENT GPs instead (row g of [g_0..g_{P-1}, f_0..f_{P-1}] -> rank g mod
        world; 24 GPs on 8 GPUs = 3 each, where whole pitches give 2,2,2,2,1,1,1,1): one all-gather of (fmean, fvar)
        per step, the likelihood recomputed on every rank, backward local (gp_pdgp_cond_begin/_end).
        Every rank constructs the model with the same arguments.

        float_type: the reference's `settings.dtypes.float_type` (pdgp.py:13), np.float64 (default) or np.float32.
        With float32 the M x N strips (Kuf, Lm^-1 Kuf, Kuf_bar) and the four O(M^2 N) products are float32 on the
        float32 matrix cores; parameters, Kuu, its Cholesky factor, all reductions, the likelihood and the
        gradients stay float64 (include/gpitch_abi.h: gp_pdgp_set_precision); `whiten` and `float_type` are independent, as in
        the reference (pdgp.py:13,49,122-129).
        A pair `(float_type_act, float_type_com)` sets the strips' precision per group of latent GPs — activation GPs,
        component GPs — and `(np.float64, np.float32)` is the useful one: the activation GPs (Matern-3/2 on a 16-kHz
        grid, cond(Kuu) ~ 1e9) keep float64 strips, the component GPs run in float32 (gp_pdgp_set_gp_precision; float64
        latent GPs must precede float32 ones in the engine's order, so (float32, float64) is refused)."""
        if isinstance(float_type, (tuple, list)):
            if len(float_type) != 2:
                raise ValueError("float_type: one type or a pair (activation GPs, component GPs)")
            self._bits = tuple(_lib.precision_bits(f) for f in float_type)
            if self._bits[0] == self._bits[1]:
                self._bits = self._bits[0]
        else:
            self._bits = _lib.precision_bits(float_type)
        x = np.asarray(x, dtype=np.float64).reshape(-1, 1)
        y = np.asarray(y, dtype=np.float64).reshape(-1, 1)
        if minibatch_size is None:
            minibatch_size = x.shape[0]
        self.minibatch_size = int(minibatch_size)
        self.num_data = x.shape[0]
        self.num_sources = len(kern[0])
        self._gp_shard = None          # ("gp", rank, world): the latent GPs this rank holds, rows of [g_0.., f_0..]
        if shard is None:
            self._shard = None
            self._local = list(range(self.num_sources))
        elif len(shard) == 3 and shard[0] == "gp":
            rank, world = int(shard[1]), int(shard[2])
            if not (0 <= rank < world) or world > 2 * self.num_sources:
                raise ValueError('shard=("gp", rank, world) needs 0 <= rank < world <= 2 x number of sources')
            from .dist import gp_assignment
            self._shard = (rank, world)
            self._gp_shard = gp_assignment(2 * self.num_sources, world, rank)
            self._local = []           # no whole pitch lives here
        else:
            if len(shard) == 3 and shard[0] == "pitch":
                shard = shard[1:]
            rank, world = int(shard[0]), int(shard[1])
            if not (0 <= rank < world) or world > self.num_sources:
                raise ValueError("shard=(rank, world) needs 0 <= rank < world <= number of sources")
            self._shard = (rank, world)
            self._local = pitch_assignment(self.num_sources, world, rank)
        self.whiten = whiten
        self.nlinfun = nlinfun
        self.likelihood = MpdLik(nlinfun=self.nlinfun, num_sources=self.num_sources)
        self.x = MinibatchData(x, self.minibatch_size, np.random.RandomState(0))   # pdgp.py:76-77: same seed
        self.y = MinibatchData(y, self.minibatch_size, np.random.RandomState(0))
        self.kern_act = ParamList(kern[0])
        self.kern_com = ParamList(kern[1])
        self.num_inducing_a, self.num_inducing_c = [], []
        za_l, zc_l, q_mu_com_l, q_mu_act_l, q_sqrt_com_l, q_sqrt_act_l = [], [], [], [], [], []
        for i in range(self.num_sources):
            Ma, Mc = np.asarray(z[0][i]).size, np.asarray(z[1][i]).size
            self.num_inducing_a.append(Ma)
            self.num_inducing_c.append(Mc)
            za_l.append(Param(np.asarray(z[0][i], dtype=np.float64).reshape(-1, 1).copy()))
            zc_l.append(Param(np.asarray(z[1][i], dtype=np.float64).reshape(-1, 1).copy()))
            q_mu_act_l.append(Param(np.zeros((Ma, 1))))
            q_mu_com_l.append(Param(np.zeros((Mc, 1))))
            q_sqrt_act_l.append(Param(np.eye(Ma)[:, :, None].copy()))     # M x M x 1 (pdgp.py:102-103)
            q_sqrt_com_l.append(Param(np.eye(Mc)[:, :, None].copy()))
        self.za = ParamList(za_l)
        self.zc = ParamList(zc_l)
        self.q_mu_com = ParamList(q_mu_com_l)
        self.q_mu_act = ParamList(q_mu_act_l)
        self.q_sqrt_com = ParamList(q_sqrt_com_l)
        self.q_sqrt_act = ParamList(q_sqrt_act_l)
        # ---- engine state (created lazily; needs the GPU) ----
        self._handle = handle
        self._plan = None
        self._max_predict_batch = max_predict_batch
        self._adam_t = 0

    # ------------------------------------------------------------------------------------------
    # engine plumbing
    def _gps(self):
        """GP order of the engine: act then com of the pitches this rank holds (all of them when unsharded)"""
        return flatvec.latent_gps(self, self._rows())

    def _rows(self):
        """the engine's latent GPs as rows of the model's order [g_0..g_{P-1}, f_0..f_{P-1}]"""
        if self._gp_shard is not None:
            return list(self._gp_shard)
        return self._local + [self.num_sources + i for i in self._local]

    def _compile(self):
        if self._plan is not None:
            return
        h = self._handle = self._handle or _lib.default_handle()
        loc = self._local if self._gp_shard is None else list(range(self.num_sources))   # (GP-sharded: cfg = whole model)
        P = len(loc)
        i32 = C.c_int32 * P
        self._cfg_keep = dict(
            M_act=i32(*[self.num_inducing_a[i] for i in loc]), M_com=i32(*[self.num_inducing_c[i] for i in loc]),
            kt_act=i32(*[self.kern_act[i].type_code for i in loc]),
            kt_com=i32(*[self.kern_com[i].type_code for i in loc]),
            np_act=i32(*[int(self.kern_act[i].num_partials) for i in loc]),
            np_com=i32(*[int(self.kern_com[i].num_partials) for i in loc]))
        k = self._cfg_keep
        self._max_batch = max(self.minibatch_size, self._max_predict_batch or min(self.num_data, 32768))
        cfg = _lib.PdgpConfig(P, int(bool(self.whiten)), nlin_code(self.nlinfun), self._max_batch,
                              k["M_act"], k["M_com"], k["kt_act"], k["kt_com"], k["np_act"], k["np_com"], jitter)
        plan = C.c_void_p()
        if self._gp_shard is not None:
            idx = (C.c_int32 * len(self._gp_shard))(*self._gp_shard)
            h.check(h.lib.gp_pdgp_create_subset(h.h, C.byref(cfg), idx, len(self._gp_shard), C.byref(plan)))
        else:
            h.check(h.lib.gp_pdgp_create(h.h, C.byref(cfg), C.byref(plan)))
        self._plan = plan
        if self._bits == 32:
            h.check(h.lib.gp_pdgp_set_precision(plan, 32))
        elif isinstance(self._bits, tuple):
            rows = list(range(2 * P)) if self._gp_shard is None else list(self._gp_shard)
            bits = [self._bits[0] if r < P else self._bits[1] for r in rows]
            h.check(h.lib.gp_pdgp_set_gp_precision(plan, (C.c_int32 * len(bits))(*bits), len(bits)))
        n = self._nparams = int(h.lib.gp_pdgp_num_params(plan))
        self._layout = []
        for g in range(2 * P if self._gp_shard is None else len(self._gp_shard)):
            o = [C.c_int64() for _ in range(4)]
            h.check(h.lib.gp_pdgp_layout(plan, g, *[C.byref(v) for v in o]))
            self._layout.append(tuple(v.value for v in o))
        t = h.torch
        self._params = h.zeros(n)
        self._free = h.zeros(n)
        self._grad = h.zeros(n)
        self._adam_m = h.zeros(n)
        self._adam_v = h.zeros(n)
        self._tcode = t.zeros(n, dtype=t.uint8, device=h.device)
        self._elbo_dev = h.zeros(2)     # [ELBO, sum of KL terms]
        self._ws = h.workspace(h.lib.gp_pdgp_workspace_bytes(plan))
        h.check(h.lib.gp_pdgp_set_workspace(plan, self._ws.data_ptr(), self._ws.numel()))
        self._x_dev = h.to_device(self.x._array.reshape(-1))
        self._y_dev = h.to_device(self.y._array.reshape(-1))
        # _batch() hands over the resident frames as they lie, or a subset drawn in index order: every batch is in time order
        # exactly when the resident x is.  The engine may then contract Kuf_bar of its Matern-3/2 / 5/2 families along the
        # sorted frames (kuf_scan.hip); it re-checks neighbouring pairs on the device.
        xh = self.x._array.reshape(-1)
        h.check(h.lib.gp_pdgp_set_frames_ascending(plan, int(bool(np.all(xh[1:] >= xh[:-1])))))
        self._xchg = h.zeros(3 * self._max_batch + 1) if (self._shard and self._gp_shard is None) else None
        if self._gp_shard is not None:
            from .dist import gp_exchange_layout
            _, blk = gp_exchange_layout(2 * self.num_sources, self._shard[1], self._max_batch)
            self._gp_send = h.zeros(blk)
            self._gp_recv = h.zeros(blk * self._shard[1])
        pending = self.__dict__.pop("_pending_adam", None)
        if pending is not None:
            self._set_adam_state(pending)

    def _param_order(self):
        """every Param of the flat vector in the order of _segments(), without a plan"""
        out = [self.likelihood.variance]
        for kern, z, q_mu, q_sqrt in self._gps():
            out += list(kern.theta_params()) + [z, q_mu, q_sqrt]
        return out

    def _adam_state(self):
        """[(m, v)] per Param in _param_order(): the Adam moments the next optimize() continues from (None: fresh)"""
        if self._plan is None:
            return self.__dict__.get("_pending_adam")
        m, v = self._adam_m.cpu().numpy(), self._adam_v.cpu().numpy()
        return [(m[o:o + p.size].copy(), v[o:o + p.size].copy()) for o, p in self._segments()]

    def _set_adam_state(self, state):
        """install Adam moments trained elsewhere (pdgp_batch.optimize_many), one (m, v) per Param in _param_order();
        kept by position (so that a copy of the model keeps them too) until the plan exists"""
        if self._plan is None:
            self._pending_adam = [(np.array(a, copy=True), np.array(b, copy=True)) for a, b in state]
            return
        m, v = self._adam_m.cpu().numpy(), self._adam_v.cpu().numpy()
        for (o, p), (ms, vs) in zip(self._segments(), state):
            m[o:o + p.size], v[o:o + p.size] = ms, vs
        t = self._handle.torch
        self._adam_m.copy_(t.as_tensor(m))
        self._adam_v.copy_(t.as_tensor(v))

    def _invalidate_device_state(self):
        """Params were written from outside: drop the packed copy and the memoised prediction factorisation"""
        self._packed_key = None
        self._pred_state = None
        self._pred_memo = None

    def _segments(self):
        """[(offset, Param)] of every Param in the flat vector"""
        segs = [(0, self.likelihood.variance)]
        for g, (kern, z, q_mu, q_sqrt) in enumerate(self._gps()):
            o_th, o_z, o_mu, o_sq = self._layout[g]
            for j, p in enumerate(kern.theta_params()):
                segs.append((o_th + j, p))
            segs += [(o_z, z), (o_mu, q_mu), (o_sq, q_sqrt)]
        return segs

    def _pack(self):
        """host Param values -> device parameter vector, free state and transform codes"""
        self._compile()
        h = self._handle
        host, tc = flatvec.pack(self._segments(), self._nparams, h)     # padding slots: fixed
        self._params.copy_(h.torch.as_tensor(host))
        self._tcode.copy_(h.torch.as_tensor(tc))
        flatvec.set_grad_needs(h, h.lib.gp_pdgp_set_grad_needs, self._plan, self._gps())
        # bit 0: the Q route is allowed; bit 1: its inducing inputs ascend, so the product may take its far-field form; bit 2: so
        # may the backward pass's Kuf diag(2 gv) Kuf^T and Kuf gm
        allow = int(self._qform_admissible())
        h.check(h.lib.gp_pdgp_set_qform(self._plan, allow | (6 if allow and self._qform_z_ascending() else 0)))
        # the activations' far field: whitened, ascending inducing inputs, a lengthscale of at most
        # FAR_ACT_MAX_SPACINGS inducing spacings
        h.check(h.lib.gp_pdgp_set_far_act(self._plan, int(self._far_act_admissible())))
        h.check(h.lib.gp_transform_backward(h.h, self._params.data_ptr(), self._tcode.data_ptr(), self._nparams,
                                            self._free.data_ptr()))
        self._packed_key = self._host_key()

    # The far-field form of A = W Kuf and Lq^T A rounds the far entries of Kuf another way than the strip builder does, and W
    # carries the difference into the gradient in proportion to cond(Kuu).  Measured against the dense products:
    # 4.6e-10 of the lengthscale gradient at 250 inducing spacings, 5.2e-9 at 1000 — about the 1.75th power.  The project's bar
    # for two float64 forms of one gradient is 1e-9 of a block's scale, which that law meets at some 390 spacings; 300 leaves a
    # margin.  Beyond it the dense products stay.
    FAR_ACT_MAX_SPACINGS = 300.0

    def _far_act_admissible(self):
        """May the engine form A = W Kuf and Lq^T A of the Matern-3/2 latent GPs from near rows plus the exact far field
        ?  From the values being packed: the model is whitened, the inducing inputs of every such GP ascend (the
        route takes them fixed and walks them in order), and its lengthscale is at most FAR_ACT_MAX_SPACINGS times their median
        spacing.  The engine checks shapes, types and gradient needs itself."""
        if not self.whiten:
            return False
        found = False
        for kern, z in zip(list(self.kern_act) + list(self.kern_com), list(self.za) + list(self.zc)):
            if int(kern.type_code) != _lib.KERN_MATERN32:
                continue
            found = True
            zz = np.asarray(z.value, dtype=np.float64).reshape(-1)
            if zz.shape[0] < 2 or not np.all(zz[1:] >= zz[:-1]):
                return False
            spacing = float(np.median(np.diff(zz)))
            if not (float(np.ravel(kern.lengthscales.value)[0]) <= self.FAR_ACT_MAX_SPACINGS * spacing):
                return False
        return found

    def _qform_admissible(self):
        """May the engine take its Q route (one dense product where the Cholesky route needs three) for the
        MercerMatern12sm latent GPs?  The route inverts Kuu explicitly, so it wants Kuu + jitter I well conditioned.  A Matern-1/2
        envelope keeps it so when its lengthscale is near the inducing spacing (cond(Kuu) is bounded by the Ornstein-Uhlenbeck
        matrix's, whatever the cosine mixture) — the transcription model's components, not every model's: so the engine's own
        measure, tr(K) tr(K^-1) / M^2 >= cond(K) / M^2, is taken here from the values being packed, and the route is allowed at
        three quarters of the bound the engine's device-side guard enforces at every evaluation (switches.h GP_QFORM_COND_MAX
        = 4; the benchmark's twelve components sit at 1.1 - 2.7), which leaves training some room to move the lengthscale.  The engine checks shapes, types and gradient needs itself."""
        if not self.whiten:
            return False
        found = False
        for kern, z in zip(list(self.kern_act) + list(self.kern_com), list(self.za) + list(self.zc)):
            if int(kern.type_code) != _lib.KERN_MERCER_MATERN12SM:
                continue
            found = True
            zz = np.asarray(z.value, dtype=np.float64).reshape(-1)
            M = zz.shape[0]
            r = np.abs(zz[:, None] - zz[None, :])
            mix = sum(float(np.ravel(e.value)[0]) * np.cos(2.0 * np.pi * float(np.ravel(f.value)[0]) * r)
                      for e, f in zip(kern.energy, kern.frequency))
            K = float(np.ravel(kern.variance.value)[0]) * np.exp(-r / float(np.ravel(kern.lengthscales.value)[0])) * mix
            K[np.diag_indices(M)] += jitter
            try:
                bound = np.trace(K) * np.trace(np.linalg.inv(K))
            except np.linalg.LinAlgError:
                return False
            if not (bound <= 3.0 * M * M):
                return False
        return found

    def _qform_z_ascending(self):
        """Do the inducing inputs of every MercerMatern12sm latent GP ascend?  Checked beside the conditioning measure, from the
        values being packed: the Q route fixes them, and the far-field form of its product walks them in
        order."""
        for kern, z in zip(list(self.kern_act) + list(self.kern_com), list(self.za) + list(self.zc)):
            if int(kern.type_code) != _lib.KERN_MERCER_MATERN12SM:
                continue
            zz = np.asarray(z.value, dtype=np.float64).reshape(-1)
            if not np.all(zz[1:] >= zz[:-1]):
                return False
        return True

    def _host_key(self):
        """what the packed device copy depends on: every Param value (param_version) and the `.fixed` flags"""
        return (param_version(), tuple(p.fixed for _, p in self._segments()))

    def _free_index(self):
        """engine offsets of the entries of GPflow's free-state vector, in GPflow's order (param.sorted_params: Params by
        attribute name, `.fixed` ones absent) — the `x` / `jac` layout of optimize(), its callback and _objective()"""
        key = tuple(p.fixed for _, p in self._segments())
        memo = self.__dict__.get("_free_index_memo")
        if memo is None or memo[0] != key:
            idx = flatvec.free_index(self, self._segments())
            memo = (key, idx, self._handle.torch.as_tensor(idx, device=self._handle.device))
            self._free_index_memo = memo
        return memo[1], memo[2]

    def _unpack(self):
        host = self._params.cpu().numpy()
        for off, p in self._segments():
            p.value = host[off:off + p.size]
        self._packed_key = self._host_key()

    def _batch(self):
        """fresh minibatch (x and y generators are seeded identically so rows stay paired: pdgp.py:76-77)"""
        # The batch is a SET of frames (the ELBO sums over it): handing it to the engine in time order changes nothing but
        # the order of that sum, and lets the covariance kernels factorise the envelope away from the diagonal band
        # (cov.hip: separable envelope) — with a shuffled batch every 64-column tile straddles the whole signal.
        n_all = int(self._x_dev.shape[0])
        if self.x.minibatch_size >= n_all and self.y.minibatch_size >= n_all:
            # minibatch_size = N (the benchmark configurations): GPflow draws rng.permutation(N)[:N] — every draw is the
            # whole data set, whatever the order; in time order that is the data as it lies in memory.  No draw, no sort,
            # no index upload, no gather: at 4-5 ms per step the two 32768-element permutations and the sort were 1.7 ms
            # of host time per step, as much as the rest of the step's launches (tools/host_profile.py).
            return self._x_dev, self._y_dev, n_all
        idx = draw_in_lockstep(self.x, self.y, self.x.next_indices)
        ti = self._upload_indices(idx)
        return self._x_dev.index_select(0, ti).contiguous(), self._y_dev.index_select(0, ti).contiguous(), idx.size

    def _upload_indices(self, idx):
        """The step's index vector goes up through a small ring of pinned host buffers with a non-blocking copy: a
        plain `as_tensor(idx, device=...)` is a synchronous copy from pageable memory, i.e. one host-device sync per
        step, after which the device sits idle until the host has issued the next step's first launches."""
        h = self._handle
        torch = h.torch
        if h.device.type != "cuda":
            return torch.as_tensor(idx, device=h.device)
        n = int(idx.size)
        ring = getattr(self, "_idx_ring", None)
        if ring is None or ring[0][0].numel() < n:
            cap = max(n, int(self.minibatch_size))
            ring = [(torch.empty(cap, dtype=torch.int64).pin_memory(),
                     torch.empty(cap, dtype=torch.int64, device=h.device), torch.cuda.Event()) for _ in range(3)]
            self._idx_ring, self._idx_pos = ring, 0
        pinned, dev, ev = ring[self._idx_pos % len(ring)]
        self._idx_pos += 1
        ev.synchronize()                     # the copy that last read this pinned buffer has run
        pinned[:n].numpy()[...] = idx
        dev[:n].copy_(pinned[:n], non_blocking=True)
        ev.record()
        return dev[:n]

    def _sharded_comm(self):
        """the handle's RCCL communicator when this sharded model can use the one-call forms (gp_pdgp_elbo_pitch_sharded /
        gp_pdgp_elbo_gp_sharded: begin -> exchange -> end [-> Adam] inside the library): an nccl process group of the
        model's world size (or no group at all for a one-rank model).  None: the torch.distributed exchange between the two
        stages (gloo rehearsals, emulated ranks)."""
        if "_comm_cache" not in self.__dict__:
            from .dist import rccl_comm
            object.__setattr__(self, "_comm_cache", rccl_comm(self._handle, self._shard[1]))
        return self._comm_cache

    def _elbo_one_call(self, comm, want_grad, sync, adam):
        """a sharded evaluation (and, with `adam`, the optimiser step behind it) as ONE library call"""
        h = self._handle
        xb, yb, n = self._batch()
        self._last_batch = (xb, yb)
        out = C.c_double()
        grad = self._grad.data_ptr() if want_grad else None
        aa = C.byref(adam) if adam is not None else None
        if self._gp_shard is not None:
            from .dist import gp_exchange_layout
            G, world = 2 * self.num_sources, self._shard[1]
            per, blk = gp_exchange_layout(G, world, n)
            full = self.__dict__.get("_gp_full")
            if full is None or full.numel() < 2 * G * n + 8:
                full = h.empty(2 * G * self._max_batch + 8)
                object.__setattr__(self, "_gp_full", full)
            h.check(h.lib.gp_pdgp_elbo_gp_sharded(self._plan, comm, self._params.data_ptr(), xb.data_ptr(), yb.data_ptr(), n,
                                                  float(self.num_data), G, len(self._gp_shard), self._gp_send.data_ptr(),
                                                  self._gp_recv.data_ptr(), full.data_ptr(), self._elbo_dev.data_ptr(),
                                                  C.byref(out) if sync else None, grad, aa))
        else:
            h.check(h.lib.gp_pdgp_elbo_pitch_sharded(self._plan, comm, self._params.data_ptr(), xb.data_ptr(), yb.data_ptr(), n,
                                                     float(self.num_data), self._xchg.data_ptr(), self._elbo_dev.data_ptr(),
                                                     C.byref(out) if sync else None, grad, aa))
        return out.value if sync else None

    def _elbo(self, want_grad, sync=True, adam=None):
        h = self._handle
        self._pred_state = None      # the engine drops its prediction factorisation on every ELBO evaluation
        if self._shard:
            comm = self._sharded_comm()
            if comm is not None:
                return self._elbo_one_call(comm, want_grad, sync, adam)
        assert adam is None
        if self._gp_shard is not None:
            from .dist import allgather_
            send = self._gp_begin(want_grad)
            recv = self._gp_recv[:send.numel() * self._shard[1]]
            allgather_(recv, send)
            return self._gp_end(want_grad, recv, sync)
        if self._shard:
            xchg = self._elbo_begin(want_grad)
            from .dist import allreduce_sum_
            allreduce_sum_(xchg)
            return self._elbo_end(want_grad, sync)
        xb, yb, n = self._batch()
        self._last_batch = (xb, yb)   # keep alive while the stream uses them
        out = C.c_double()
        h.check(h.lib.gp_pdgp_elbo(self._plan, self._params.data_ptr(), xb.data_ptr(), yb.data_ptr(), n,
                                   float(self.num_data), self._elbo_dev.data_ptr(), C.byref(out) if sync else None,
                                   self._grad.data_ptr() if want_grad else None))
        return out.value if sync else None

    def _elbo_begin(self, want_grad):
        """pitch-sharded stage 1: returns the exchange tensor [A | B | D | sum KL] (3n+1) to be summed over ranks"""
        h = self._handle
        self._pred_state = None
        xb, yb, n = self._batch()
        self._last_batch = (xb, yb)
        xchg = self._xchg[:3 * n + 1]
        h.check(h.lib.gp_pdgp_elbo_begin(self._plan, self._params.data_ptr(), xb.data_ptr(), yb.data_ptr(), n,
                                         self._grad.data_ptr() if want_grad else None, xchg.data_ptr()))
        return xchg

    def _gp_begin(self, want_grad):
        """GP-sharded stage 1: conditionals of this rank's latent GPs, written straight into the all-gather's send block
        [fmean rows | fvar rows | sum of the local KL terms] (dist.gp_exchange_layout)"""
        from .dist import gp_exchange_layout
        h = self._handle
        self._pred_state = None
        xb, yb, n = self._batch()
        self._last_batch = (xb, yb)
        per, blk = gp_exchange_layout(2 * self.num_sources, self._shard[1], n)
        send = self._gp_send[:blk]
        if len(self._gp_shard) < per:
            send.zero_()                  # this rank's last row slot is padding
        h.check(h.lib.gp_pdgp_cond_begin(self._plan, self._params.data_ptr(), xb.data_ptr(), n,
                                         self._grad.data_ptr() if want_grad else None, send.data_ptr(),
                                         send[per * n:].data_ptr(), send[2 * per * n:].data_ptr()))
        return send

    def _gp_end(self, want_grad, gathered, sync=True):
        """GP-sharded stage 2 on the all-gather's output (world x block): the whole model's likelihood, local backward"""
        from .dist import gp_assemble
        h = self._handle
        xb, yb = self._last_batch
        n = xb.numel()
        fm, fv, kl = gp_assemble(gathered, 2 * self.num_sources, self._shard[1], n)
        self._gp_keep = (fm, fv, kl)      # alive while the stream uses them
        out = C.c_double()
        h.check(h.lib.gp_pdgp_cond_end(self._plan, self._params.data_ptr(), xb.data_ptr(), yb.data_ptr(), n,
                                       float(self.num_data), fm.data_ptr(), fv.data_ptr(), kl.data_ptr(),
                                       self._elbo_dev.data_ptr(), C.byref(out) if sync else None,
                                       self._grad.data_ptr() if want_grad else None))
        return out.value if sync else None

    def _elbo_end(self, want_grad, sync=True):
        """pitch-sharded stage 2 on the rank-summed exchange tensor"""
        h = self._handle
        xb, yb = self._last_batch
        n = xb.numel()
        out = C.c_double()
        h.check(h.lib.gp_pdgp_elbo_end(self._plan, self._params.data_ptr(), xb.data_ptr(), yb.data_ptr(), n,
                                       float(self.num_data), self._xchg.data_ptr(), self._elbo_dev.data_ptr(),
                                       C.byref(out) if sync else None, self._grad.data_ptr() if want_grad else None))
        return out.value if sync else None

    # ------------------------------------------------------------------------------------------
    # reference API
    def build_prior_kl(self):
        """compute KL divergences (pdgp.py:113-131)"""
        from .conditionals import gauss_kl
        if not self.whiten or self._shard:
            # K = Kuu + jitter I (pdgp.py:126-129): evaluated by the engine next to the conditionals
            self._pack()
            self._elbo(False)
            return float(self._elbo_dev[1].item())
        kl = 0.
        for i in range(self.num_sources):
            kl += gauss_kl(self.q_mu_act[i].value, self.q_sqrt_act[i].value)
            kl += gauss_kl(self.q_mu_com[i].value, self.q_sqrt_com[i].value)
        return kl

    def build_likelihood(self):
        """Compute the objective function (pdgp.py:133-170): the ELBO on a fresh minibatch."""
        self._pack()
        return self._elbo(False)

    def compute_log_likelihood(self):
        return self.build_likelihood()

    def _objective(self, x_free):
        """GPflow Model._objective: (-(ELBO), -grad wrt the free state) in float64"""
        h = self._handle
        if self._plan is None or self.__dict__.get("_packed_key") != self._host_key():
            self._pack()       # (inside optimize()'s loop the device copy is ahead of the host Params and is left alone)
        idx, idx_dev = self._free_index()
        xf = np.zeros(self._nparams)
        xf[idx] = np.asarray(x_free, dtype=np.float64).reshape(-1)
        self._free.index_copy_(0, idx_dev, h.torch.as_tensor(xf[idx]).to(h.device))
        h.check(h.lib.gp_transform_forward(h.h, self._free.data_ptr(), self._tcode.data_ptr(), self._nparams,
                                           self._params.data_ptr()))
        f = self._elbo(True)
        g = flatvec.free_gradient(self._segments(), xf, self._grad.cpu().numpy())
        return -f, -g[idx]

    def get_free_state(self):
        """GPflow Model.get_free_state: the non-fixed Params' unconstrained values, ordered by name"""
        self._pack()
        return self._free.index_select(0, self._free_index()[1]).cpu().numpy()

    def optimize(self, method='L-BFGS-B', tol=None, callback=None, maxiter=1000, disp=False, **kw):
        """GPflow Model.optimize.  `method` is an AdamOptimizer token (demo-modgp.py:44-45), a NatGradAdam token
        (natural-gradient steps on q(u) of every latent GP whose q_mu and q_sqrt are free, Adam on the rest: train.py)
        or a scipy.optimize.minimize method name."""
        natgrad = isinstance(method, NatGradAdam)
        if natgrad:
            step_gps = self._natgrad_gps(method)        # refusals come before any device work
        self._pack()
        h = self._handle
        adaptive = natgrad and method.adaptive()     # per-role lengths / halving: gp_pdgp_natgrad_step_adaptive
        if natgrad:
            step_gps = (C.c_int32 * len(step_gps))(*step_gps)
            if adaptive:
                gammas = method.role_gammas(self.num_sources)
                gammas = (C.c_double * len(gammas))(*gammas)
                if self.__dict__.get("_nga_ws") is None:
                    self._nga_ws = h.workspace(h.lib.gp_pdgp_natgrad_adaptive_workspace_bytes(self._plan))
                # the call's counters start from zero; they are read once, after the last iteration
                h.check(h.lib.gp_pdgp_natgrad_counts(self._plan, self._nga_ws.data_ptr(), None, None, 1))
            elif self.__dict__.get("_ng_ws") is None:
                self._ng_ws = h.workspace(h.lib.gp_pdgp_natgrad_workspace_bytes(self._plan))
        if natgrad or isinstance(method, AdamOptimizer):
            flag = C.c_int32(0)
            one_call = not natgrad and bool(self._shard) and self._sharded_comm() is not None
            for it in range(maxiter):
                self._adam_t += 1
                if natgrad:
                    # the same evaluation an Adam iteration makes; the step on q(u) reads its blocks of the gradient and
                    # zeroes them, so that Adam behind it (zero gradient, zero moments: an update of exactly 0) moves
                    # the noise variance, the kernels and the inducing inputs only
                    self._elbo(True, sync=False)
                    if adaptive:
                        h.check(h.lib.gp_pdgp_natgrad_step_adaptive(
                            self._plan, self._params.data_ptr(), self._free.data_ptr(), self._grad.data_ptr(), gammas,
                            method.halvings, step_gps, self._nga_ws.data_ptr(), self._nga_ws.numel()))
                    else:
                        h.check(h.lib.gp_pdgp_natgrad_step(self._plan, self._params.data_ptr(), self._free.data_ptr(),
                                                           self._grad.data_ptr(), method.gamma, step_gps,
                                                           self._ng_ws.data_ptr(), self._ng_ws.numel()))
                    h.check(h.lib.gp_adam_step(h.h, self._free.data_ptr(), self._params.data_ptr(), self._grad.data_ptr(),
                                               self._tcode.data_ptr(), self._adam_m.data_ptr(), self._adam_v.data_ptr(),
                                               self._nparams, self._adam_t, method.learning_rate, method.beta1,
                                               method.beta2, method.epsilon))
                elif one_call:
                    # a sharded model on an RCCL group: conditionals -> exchange -> likelihood + backward -> Adam, one call
                    aa = _lib.AdamArgs(self._free.data_ptr(), self._tcode.data_ptr(), self._adam_m.data_ptr(),
                                       self._adam_v.data_ptr(), self._nparams, self._adam_t, method.learning_rate,
                                       method.beta1, method.beta2, method.epsilon)
                    self._elbo(True, sync=False, adam=aa)
                else:
                    self._elbo(True, sync=False)
                    h.check(h.lib.gp_adam_step(h.h, self._free.data_ptr(), self._params.data_ptr(), self._grad.data_ptr(),
                                               self._tcode.data_ptr(), self._adam_m.data_ptr(), self._adam_v.data_ptr(),
                                               self._nparams, self._adam_t, method.learning_rate, method.beta1,
                                               method.beta2, method.epsilon))
                # a failed Cholesky freezes the optimiser state on the device (gp_adam_step); the loop itself stops at
                # the next poll that has seen the flag — no host synchronisation per step
                h.check(h.lib.gp_poll_not_pd(h.h, C.byref(flag)))
                if flag.value:
                    self._check_not_pd(method)              # raises NotPositiveDefiniteError with the pivot index
                if callback is not None:
                    callback(self._free.index_select(0, self._free_index()[1]).cpu().numpy())
            self._check_not_pd(method)                      # a failure in the last few steps, not polled yet
            # GPflow evaluates the returned `fun`/`jac` on a fresh minibatch (demo_modgp.ipynb:140-146)
            x_final = self._free.index_select(0, self._free_index()[1]).cpu().numpy()
            f, g = self._objective(x_final)
            self._unpack()
            if self._shard:
                self.sync_params()
            res = OptimizeResult(fun=f, jac=g, x=x_final, message='Finished iterations.', status='Finished iterations.',
                                 success=True)
            if adaptive:
                res["natgrad"] = self._natgrad_counts(method)
            return res
        if self._shard:
            # each rank owns a different slice of the free state: only element-wise update rules (Adam) stay
            # consistent across ranks without exchanging it
            raise NotImplementedError("a pitch-sharded Pdgp is trained with AdamOptimizer")
        from scipy.optimize import minimize
        idx_dev = self._free_index()[1]
        x0 = self._free.index_select(0, idx_dev).cpu().numpy()
        res = minimize(self._objective, x0, jac=True, method=method, tol=tol, callback=callback,
                       options=dict(maxiter=maxiter, disp=disp))
        self._free.index_copy_(0, idx_dev, h.torch.as_tensor(res.x).to(h.device))
        h.check(h.lib.gp_transform_forward(h.h, self._free.data_ptr(), self._tcode.data_ptr(), self._nparams,
                                           self._params.data_ptr()))
        self._unpack()
        return res

    def _natgrad_gps(self, method):
        """one flag per latent GP in the engine's order [g_0..g_{P-1}, f_0..f_{P-1}]: does NatGradAdam step its q(u)?
        Both of q_mu and q_sqrt free: yes; both fixed: no; one of the two fixed has no natural-gradient step (ValueError
        naming the GP).  No device work."""
        if not (0.0 < method.gamma <= 1.0):
            raise ValueError("NatGradAdam: gamma must be a number in (0, 1], not %r" % (method.gamma,))
        if getattr(method, "gamma_com", None) is not None:       # (a token changed after it was made)
            method.check_gamma("gamma_com", method.gamma_com)
        method.check_halvings(getattr(method, "halvings", 0))
        if self._shard:
            raise NotImplementedError("NatGradAdam on a sharded model: build the model unsharded on one GPU "
                                      "(a sharded Pdgp is trained with AdamOptimizer)")
        flags = []
        for role, q_mu, q_sqrt in (("activation", self.q_mu_act, self.q_sqrt_act), ("component", self.q_mu_com, self.q_sqrt_com)):
            for i in range(self.num_sources):
                fm, fs = bool(q_mu[i].fixed), bool(q_sqrt[i].fixed)
                if fm != fs:
                    raise ValueError("NatGradAdam: the %s GP %d has %s fixed and %s free; a natural-gradient step moves both, "
                                     "fix both or neither" % ((role, i) + (("q_mu", "q_sqrt") if fm else ("q_sqrt", "q_mu"))))
                flags.append(int(not fm))
        return flags

    def _natgrad_counts(self, method):
        """the adaptive step's counters of this optimize() call, rows [g_0..g_{P-1}, f_0..f_{P-1}] (one read, after the loop);
        the shortest length starts at the GP's own gamma_r (the device reports +inf for a GP that took no step)"""
        h, G = self._handle, 2 * self.num_sources
        hv, sg = (C.c_int64 * G)(), (C.c_double * G)()
        h.check(h.lib.gp_pdgp_natgrad_counts(self._plan, self._nga_ws.data_ptr(), hv, sg, 0))
        return {"halvings": [int(v) for v in hv],
                "shortest_gamma": [min(float(v), g) for v, g in zip(sg, method.role_gammas(self.num_sources))]}

    def _check_not_pd(self, method):
        """gp_check_not_pd; a refusal that a NatGradAdam step raised itself (its I - 2 gamma P was not positive definite:
        natgrad.hip leaves the GP in the first words of its workspace) is reported as such"""
        h = self._handle
        try:
            h.check(h.lib.gp_check_not_pd(h.h))
        except _lib.NotPositiveDefiniteError as e:
            if not isinstance(method, NatGradAdam):
                raise
            adaptive = method.adaptive()
            rep = (self._nga_ws if adaptive else self._ng_ws)[:16].view(h.torch.int32).cpu().numpy()
            if int(rep[0]) != 1:
                raise
            g, P = int(rep[1]), self.num_sources
            if adaptive:
                last = method.role_gammas(P)[g] * 2.0 ** -method.halvings
                raise _lib.NotPositiveDefiniteError(
                    e.status, "NatGradAdam: the natural-gradient step was too long: I - 2 gamma P of the %s GP %d (latent GP %d) "
                              "is not positive definite (pivot %d) at gamma = %g, the last length tried after halvings = %d; no "
                              "parameter was changed, take a smaller gamma or more halvings"
                              % ("activation" if g < P else "component", g if g < P else g - P, g, int(rep[2]), last,
                                 method.halvings))
            raise _lib.NotPositiveDefiniteError(
                e.status, "NatGradAdam: the natural-gradient step was too long: I - 2 gamma P of the %s GP %d (latent GP %d) is "
                          "not positive definite (pivot %d) at gamma = %g; no parameter was changed, take a smaller gamma"
                          % ("activation" if g < P else "component", g if g < P else g - P, g, int(rep[2]), method.gamma))

    def _pred_key(self):
        """what a prediction's factorisation depends on: every Param value and the Adam steps taken (`.fixed` flags do
        not matter here)"""
        return (param_version(), self._adam_t)

    def _predict_chunks(self, xnew, entry, chunk):
        """The loop of _predict and _predict_moments: xnew goes to the engine `_max_batch` frames at a time through
        chunk(call, s, xs) — xs the device copy of xnew[s:s + _max_batch], call the library entry to use.  While no
        Param changed, Kuu / its Cholesky factor / inverse of the previous prediction are reused instead of rebuilt:
        `call` is `entry` after a fresh _pack(), its `_reuse` form when the engine still holds the factorisation of
        these Params, and always from the second chunk on.  The factorisation is recorded only once a chunk has run
        (an empty xnew factors nothing)."""
        state = self._pred_key()
        reuse = self._plan is not None and getattr(self, "_pred_state", None) == state
        if not reuse:
            self._pack()
        h = self._handle
        call = getattr(h.lib, entry + "_reuse" if reuse else entry)
        for s in range(0, xnew.size, self._max_batch):
            chunk(call, s, h.to_device(xnew[s:s + self._max_batch]))
            call = getattr(h.lib, entry + "_reuse")
        if xnew.size:
            self._pred_state = state

    def _predict(self, xnew, want_source):
        xnew = np.asarray(xnew, dtype=np.float64).reshape(-1)
        # predict_act followed by predict_com at the same inputs (pdgp.py:17-44 does exactly that per window) is one
        # engine evaluation
        state = self._pred_key()
        memo = getattr(self, "_pred_memo", None)
        if memo is not None and memo[0] == state and memo[1].shape == xnew.shape and np.array_equal(memo[1], xnew):
            return memo[2]
        P, n = self.num_sources, xnew.size
        loc = self._local
        gp_mode = self._gp_shard is not None
        rows = np.array(self._rows())      # engine row -> model row [g_0..g_{P-1}, f_0..f_{P-1}]
        fmean = np.zeros((2 * P, n))
        fvar = np.zeros((2 * P, n))
        src = np.zeros((P, n))

        def chunk(predict, s, xs):
            h, c = self._handle, xs.numel()
            fm, fv, ms = h.empty(len(rows), c), h.empty(len(rows), c), (None if gp_mode else h.empty(len(loc), c))
            h.check(predict(self._plan, self._params.data_ptr(), xs.data_ptr(), c, fm.data_ptr(), fv.data_ptr(),
                            None if gp_mode else ms.data_ptr()))
            fmean[rows, s:s + c] = fm.cpu().numpy()
            fvar[rows, s:s + c] = fv.cpu().numpy()
            if not gp_mode:
                src[loc, s:s + c] = ms.cpu().numpy()

        self._predict_chunks(xnew, "gp_pdgp_predict", chunk)
        h = self._handle
        if self._shard:
            # rows of other ranks are zero here: a sum over ranks assembles the full prediction (emulated ranks — a test
            # driving several shards in one process — pass allow_local=True through _pred_allow_local and get their rows only)
            from .dist import allreduce_sum_, require_group
            if not self.__dict__.get("_pred_allow_local", False):
                require_group(self._shard[1], "Pdgp.predict")
            t = h.torch
            for a in ((fmean, fvar) if gp_mode else (fmean, fvar, src)):
                a[...] = allreduce_sum_(t.as_tensor(a)).numpy()
        if gp_mode:
            # an activation GP and its component GP may live on different ranks: the source mean (pdgp.py:207) is formed
            # from the assembled rows — complete only once the sum over ranks has run (a rank on its own sees its rows)
            src = self.nlinfun(fmean[:P]) * fmean[P:]
        self._pred_memo = (state, xnew.copy(), (fmean, fvar, src))
        return fmean, fvar, src

    def sync_params(self):
        """pitch-sharded model: after training, give every rank the Param values of every pitch"""
        import torch.distributed as dist
        if not (self._shard and dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return
        P = self.num_sources
        mine = {}
        for g in self._rows():
            i, act = (g, True) if g < P else (g - P, False)
            kname = "kern_act" if act else "kern_com"
            mine[(kname, i)] = [q.value.copy() for q in getattr(self, kname)[i].theta_params()]
            for name in (("za", "q_mu_act", "q_sqrt_act") if act else ("zc", "q_mu_com", "q_sqrt_com")):
                mine[(name, i)] = getattr(self, name)[i].value.copy()
        everyone = [None] * dist.get_world_size()
        dist.all_gather_object(everyone, mine)
        for part in everyone:
            for (name, i), val in part.items():
                if (name, i) in mine:
                    continue
                if name.startswith("kern"):
                    for q, v in zip(getattr(self, name)[i].theta_params(), val):
                        q.value = v
                else:
                    getattr(self, name)[i].value = val

    def predict_act(self, xnew):
        """pdgp.py:172-179"""
        P = self.num_sources
        fm, fv, _ = self._predict(xnew, False)
        return [col(fm, i).copy() for i in range(P)], [col(fv, i).copy() for i in range(P)]

    def predict_com(self, xnew):
        """pdgp.py:181-188"""
        P = self.num_sources
        fm, fv, _ = self._predict(xnew, False)
        return [col(fm, P + i).copy() for i in range(P)], [col(fv, P + i).copy() for i in range(P)]

    def predict_act_n_com(self, xnew):
        """pdgp.py:190-208"""
        P = self.num_sources
        fm, fv, src = self._predict(xnew, True)
        return ([col(fm, i).copy() for i in range(P)], [col(fv, i).copy() for i in range(P)],
                [col(fm, P + i).copy() for i in range(P)], [col(fv, P + i).copy() for i in range(P)],
                [col(src, i).copy() for i in range(P)])

    # ------------------------------------------------------------------------------------------
    # posterior of the sources, of the mixture, and held-out density (csrc/lik.hip mpd_moments_kernel through
    # gp_pdgp_predict_moments: the conditionals stay on the device, only the requested arrays come back)
    def _predict_moments(self, xnew, ynew=None, sources=False, y=False, logp=False, noise=True):
        """(smean, svar) P x n, (ymean, yvar) n, logp n — None for what was not asked for.  Chunked by _max_batch with
        the factorisation reused, as _predict; the prediction memo of _predict is neither read nor written."""
        xnew = np.asarray(xnew, dtype=np.float64)
        if xnew.ndim > 2 or (xnew.ndim == 2 and xnew.shape[1] != 1):
            raise ValueError("xnew has shape %r, not (n,) or (n, 1)" % (xnew.shape,))
        xnew = xnew.reshape(-1)
        P, n = self.num_sources, xnew.size
        if logp:
            if ynew is None:
                raise ValueError("expected_log_density needs ynew")
            ynew = np.asarray(ynew, dtype=np.float64)
            if ynew.ndim > 2 or (ynew.ndim == 2 and ynew.shape[1] != 1) or ynew.size != n:
                raise ValueError("ynew has shape %r for %d inputs in xnew" % (ynew.shape, n))
            ynew = ynew.reshape(-1)
        if self._shard:
            # the rows are assembled over the ranks as _predict does; the operator entry runs on the assembled rows
            fm, fv, _ = self._predict(xnew, False)
            return self.likelihood._moments(fm.T, fv.T, ynew, sources=sources, y=y, logp=logp, noise=noise)
        sm, sv = (np.zeros((P, n)), np.zeros((P, n))) if sources else (None, None)
        ym, yv = (np.zeros(n), np.zeros(n)) if y else (None, None)
        lp = np.zeros(n) if logp else None
        ptr = lambda t: None if t is None else t.data_ptr()

        def chunk(call, s, xs):
            h, c = self._handle, xs.numel()
            ys = h.to_device(ynew[s:s + c]) if logp else None
            dsm, dsv = (h.empty(P, c), h.empty(P, c)) if sources else (None, None)
            dym, dyv = (h.empty(c), h.empty(c)) if y else (None, None)
            dlp = h.empty(c) if logp else None
            h.check(call(self._plan, self._params.data_ptr(), xs.data_ptr(), c, ptr(ys), int(bool(noise)), ptr(dsm),
                         ptr(dsv), ptr(dym), ptr(dyv), ptr(dlp)))
            for dst, src in ((sm, dsm), (sv, dsv), (ym, dym), (yv, dyv), (lp, dlp)):
                if dst is not None:
                    dst[..., s:s + c] = src.cpu().numpy()

        self._predict_chunks(xnew, "gp_pdgp_predict_moments", chunk)
        return sm, sv, ym, yv, lp

    def predict_sources(self, xnew):
        """posterior mean and variance under q of every source nlin(g_i) f_i at xnew: (mean_s, var_s), lists of P (n, 1)
        arrays.  mean_s[i] = E[nlin(g_i)] E[f_i] with the nonlinearity integrated by the likelihood's 20-point rule
        (predict_act_n_com's mean_source plugs the activation's mean in instead)."""
        sm, sv, _, _, _ = self._predict_moments(xnew, sources=True)
        P = self.num_sources
        return [col(sm, i).copy() for i in range(P)], [col(sv, i).copy() for i in range(P)]

    def predict_y(self, xnew):
        """GPflow Model.predict_y: mean and variance of the observed mixture at xnew, (n, 1) each; the sources are
        independent under q, the variance includes the noise variance"""
        _, _, ym, yv, _ = self._predict_moments(xnew, y=True)
        return ym.reshape(-1, 1), yv.reshape(-1, 1)

    def predict_mixture(self, xnew):
        """mean and variance of the latent mixture sum_i nlin(g_i) f_i at xnew (predict_y without the noise variance)"""
        _, _, ym, yv, _ = self._predict_moments(xnew, y=True, noise=False)
        return ym.reshape(-1, 1), yv.reshape(-1, 1)

    def expected_log_density(self, xnew, ynew):
        """E_q[log p(ynew_n | g, f)] per frame, (n, 1): MpdLik.variational_expectations at the posterior's moments at xnew,
        not scaled by N / B and without the KL terms — on the training data, the data term of the ELBO"""
        return self._predict_moments(xnew, ynew, logp=True)[4].reshape(-1, 1)

    # ------------------------------------------------------------------------------------------
    # joint posterior draws of the latent GPs and the sources (csrc/sample.hip through gp_pdgp_sample)
    def _sample_components(self):
        """standard normals per point of every latent GP, rows [g_0..g_{P-1}, f_0..f_{P-1}]: 1 for Matern12, 2 for
        Matern32 (the state (f, f')), 2 m for a Matern-1/2 spectral mixture of m partials.  Raises NotImplementedError,
        naming the GP and its kernel, for a kernel without an exact state-space prior sampler.  No device work."""
        from .sgpr_ss import _KERN_NAMES
        comps = []
        for role, kerns in (("activation", self.kern_act), ("component", self.kern_com)):
            for i in range(self.num_sources):
                code, m = int(kerns[i].type_code), int(kerns[i].num_partials)
                if code not in _SAMPLE_COMPONENTS:
                    raise NotImplementedError(
                        "sample_sources: the %s GP %d has kernel %s; joint draws need an exact state-space prior sampler "
                        "(supported: %s)" % (role, i, _KERN_NAMES.get(code, "type %d" % code),
                                             ", ".join(_KERN_NAMES[c] for c in sorted(_SAMPLE_COMPONENTS))))
                comps.append(_SAMPLE_COMPONENTS[code] or 2 * m)
        return comps

    def sample_eps_shapes(self, n, num_samples=1):
        """shapes of the standard normals of sample_sources at n frames: three lists (eps_x, eps_z, eps_u) of 2P shapes,
        rows [g_0..g_{P-1}, f_0..f_{P-1}]: (S, c_r, n), (S, c_r, M_r), (S, 2, M_r).  Blocks are indexed by the caller's own
        point order (xnew, Z_r), not by the merged one."""
        S, n = int(num_samples), int(n)
        comps = self._sample_components()
        Ms = list(self.num_inducing_a) + list(self.num_inducing_c)
        return ([(S, c, n) for c in comps], [(S, c, M) for c, M in zip(comps, Ms)], [(S, 2, M) for M in Ms])

    def sample_sources(self, xnew, num_samples=1, seed=0, eps=None, return_latents=False):
        """Joint posterior draws under q of every source nlin(g_i) f_i across all frames of xnew: `src` of shape
        (P, num_samples, n); with return_latents=True also the draws of the activations g and components f it was formed
        from, `(src, g, f)`, each (P, num_samples, n).  A draw is a whole path: each latent GP is drawn by Matheron's rule
        on an exact O(n + M) state-space prior sampler along sorted time (gp_pdgp_sample; no n x n matrix), so functionals
        of a path (an envelope, a spectrogram, an onset time) can be evaluated draw by draw.  Activation and component
        kernels need such a sampler: Matern12, Matern32, MercerMatern12sm, Matern12sm (NotImplementedError otherwise,
        before any device work).  Observation noise is not added.  float64 whatever the model's float_type.

        eps=None: the standard normals are torch.randn on the handle's device from a generator seeded by `seed`, drawn
        sgpr_ss.SAMPLE_EPS_BYTES at a time (the same seed and chunk size give the same draws).  eps=(eps_x, eps_z, eps_u),
        three lists of 2P arrays of shapes sample_eps_shapes(n, num_samples), supplies them: the map is affine in eps per
        GP, eps = 0 returns predict_act / predict_com's means and predict_act_n_com's mean_source.  All of xnew is one
        call: a joint draw cannot be cut into frame chunks, so n is bounded by device memory, not by max_predict_batch.
        The factorisation of a previous prediction or draw is reused while no Param changed; the prediction memo is
        neither read nor written."""
        if self._shard:
            raise NotImplementedError("sample_sources of a sharded model: build the model unsharded on one GPU")
        comps = self._sample_components()              # raises for an unsupported kernel, before any device work
        xnew = np.asarray(xnew, dtype=np.float64)
        if xnew.ndim > 2 or (xnew.ndim == 2 and xnew.shape[1] != 1):
            raise ValueError("xnew has shape %r, not (n,) or (n, 1)" % (xnew.shape,))
        xnew = xnew.reshape(-1)
        if isinstance(num_samples, bool) or int(num_samples) != num_samples or int(num_samples) < 1:
            raise ValueError("num_samples must be a positive integer, not %r" % (num_samples,))
        P, n, S = self.num_sources, xnew.size, int(num_samples)
        Ms = list(self.num_inducing_a) + list(self.num_inducing_c)
        shapes = self.sample_eps_shapes(n, S)
        if eps is not None:
            if len(eps) != 3 or any(len(e) != 2 * P for e in eps):
                raise ValueError("eps must be (eps_x, eps_z, eps_u), three lists of %d arrays" % (2 * P))
            eps = [[np.asarray(a, dtype=np.float64) for a in e] for e in eps]
            for name, e, sh in zip(("eps_x", "eps_z", "eps_u"), eps, shapes):
                for r in range(2 * P):
                    if e[r].shape != sh[r]:
                        raise ValueError("%s[%d] has shape %r, not %r (sample_eps_shapes)" % (name, r, e[r].shape, sh[r]))
        if n == 0:
            out = tuple(np.zeros((P, S, 0)) for _ in range(3))
            return out if return_latents else out[0]
        zs = [z.value.reshape(-1) for z in list(self.za) + list(self.zc)]
        order = np.ascontiguousarray(np.concatenate([merged_order(xnew, z) for z in zs]))
        state = self._pred_key()
        reuse = self._plan is not None and getattr(self, "_pred_state", None) == state
        if not reuse:
            self._pack()
        h = self._handle
        t = h.torch
        xs = h.to_device(xnew)
        C_all, maxM = int(sum(comps)), int(max(Ms))
        per_draw = sum(c * (n + M) + 2 * M for c, M in zip(comps, Ms))
        chunk = S if eps is not None else _sample_chunk(S, per_draw)
        ws = h.workspace(h.lib.gp_pdgp_sample_workspace_bytes(2 * P, maxM, C_all, n, chunk))
        lat, dsrc = h.empty(2 * P * chunk * n), h.empty(P * chunk * n)
        gen = None if eps is not None else _sample_generator(h, seed)
        src = np.empty((P, S, n))
        g, f = (np.empty((P, S, n)), np.empty((P, S, n))) if return_latents else (None, None)
        call = h.lib.gp_pdgp_sample_reuse if reuse else h.lib.gp_pdgp_sample
        for s0 in range(0, S, chunk):
            sc = min(chunk, S - s0)
            if eps is not None:
                ex, ez, eu = (h.to_device(np.concatenate([a.reshape(-1) for a in e])) for e in eps)
            else:
                ex, ez, eu = (t.randn(sc * sum(int(np.prod(sh[1:])) for sh in shs), dtype=t.float64, device=h.device,
                                      generator=gen) for shs in shapes)
            h.check(call(self._plan, self._params.data_ptr(), xs.data_ptr(), n, order.ctypes.data, sc, ex.data_ptr(),
                         ez.data_ptr(), eu.data_ptr(), lat.data_ptr(), dsrc.data_ptr(), ws.data_ptr(), ws.numel()))
            call = h.lib.gp_pdgp_sample_reuse
            self._pred_state = state
            src[:, s0:s0 + sc] = dsrc[:P * sc * n].reshape(P, sc, n).cpu().numpy()
            if return_latents:
                l = lat[:2 * P * sc * n].reshape(2 * P, sc, n).cpu().numpy()
                g[:, s0:s0 + sc], f[:, s0:s0 + sc] = l[:P], l[P:]
        return (src, g, f) if return_latents else src

    def __del__(self):
        try:
            if self._plan is not None and self._handle is not None and self._handle.h:
                self._handle.sync()
                self._handle.lib.gp_pdgp_destroy(self._plan)
        except Exception:
            pass
