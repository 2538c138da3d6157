"""Many small, independent Pdgp models trained together: one launch sequence per Adam step for all of them
(csrc/pdgp_batch.hip through gp_pdgpb_*).

    results = optimize_many(models, method=AdamOptimizer(0.0025), maxiter=1000)

replaces  for m in models: m.optimize(method=AdamOptimizer(0.0025), maxiter=1000)  — the per-note training behind
init_kernel_with_trained_models (gpitch/init_models.py:74-121) and the segments of a long recording — and leaves every
model as that loop would: parameters, Adam step count and moments, and the minibatch generators advanced by the same
draws (GPflow's final fresh-minibatch fun / jac evaluation included).  Whitened float64 unsharded models; everything
else is refused by check_batchable() before any device work.

    results = optimize_many(models, method=NatGradAdam(0.1, 0.0025), maxiter=1000)

replaces the same loop with the second optimiser token: per iteration a natural-gradient step on q(u) of every latent GP
whose q_mu and q_sqrt are both free, Adam on the rest, two more launches per iteration whatever the number of models
(gp_pdgpb_natgrad; check_batchable_natgrad() is its host check).  A model whose step is too long (I - 2 gamma P of one
of its GPs not positive definite) is refused on its own: it is left as it was and its result carries the error, the
others go on.

    results = optimize_many(segments, method=..., maxiter=1000, tied=tie_groups(segments))

trains the segments of one recording as ONE model of it: the Params of each group in `tied` are one parameter (one noise
variance, one set of kernels; q(u) and by default the inducing inputs stay each segment's own), the objective is the sum of
the segments' ELBOs, and one more launch per iteration hands every member the group's summed gradient (check_tied() is the
host check, gp_pdgpb_set_ties the device entry).  Models joined by ties stop together when one of them fails.

    preds = predict_many(models, xnews)

replaces  [m.predict_act_n_com(x) for m, x in zip(models, xnews)]  with one factorisation launch for every latent GP and
one launch for every (latent GP, frame tile) pair, without building any single-model engine plan (check_predictable()
takes the same models, without the minibatch limit).

    draws = sample_sources_many(models, xnews, num_samples=16, seed=0)

replaces  [m.sample_sources(x, 16) for m, x in zip(models, xnews)]  — joint posterior draws of every source of every model
(csrc/pdgp_batch.hip gp_pdgpb_sample over the state-space core of csrc/sample.hip; check_sampleable()).
"""
import contextlib
import ctypes as C

import numpy as np

from . import _lib, flatvec
from .flatvec import col, free_index, latent_gps  # noqa: F401  (free_index: part of this module's interface)
from .methods import nlin_code
from .param import Logistic, Param, ParamList, Parameterized, draw_in_lockstep
from .pdgp import Pdgp, jitter
from .sgpr_ss import _KERN_NAMES, _sample_generator, merged_order
from .train import AdamOptimizer, NatGradAdam, OptimizeResult

MAX_M = 128            # inducing points per latent GP (one factor of 128 x 128 float64 in a workgroup's LDS)
MAX_MINIBATCH = 1024   # frames per model and step
MAX_PARTIALS = 32
_KERNELS = {_lib.KERN_MATERN12: "Matern12", _lib.KERN_MATERN32: "Matern32", _lib.KERN_MATERN52: "Matern52",
            _lib.KERN_RBF: "RBF", _lib.KERN_MERCER_MATERN12SM: "MercerMatern12sm", _lib.KERN_MATERN32SM: "Matern32sm"}
_SINGLE = "train this model on its own with Pdgp.optimize"


def _check_models(models, entry, single, minibatch):
    """the scope both batched entries share (check_batchable, check_predictable): a list of distinct whitened float64
    unsharded Pdgp models whose latent GPs the batch's kernels take; `minibatch` adds the training minibatch limit"""
    models = list(models)
    if not models:
        raise ValueError("%s needs at least one model" % entry)
    if len(set(id(m) for m in models)) != len(models):
        raise ValueError("%s: the same model appears twice in the list" % entry)
    for k, m in enumerate(models):
        if not isinstance(m, Pdgp):
            raise ValueError("%s: item %d is not a Pdgp" % (entry, k))
        if not m.whiten:
            raise NotImplementedError("model %d: whiten=False is not batched; %s" % (k, single))
        if m._bits != 64:
            raise NotImplementedError("model %d: float_type %r is not batched (float64 only); %s" % (k, m._bits, single))
        if m._shard is not None:
            raise NotImplementedError("model %d: sharded models are not batched; %s" % (k, single))
        nlin_code(m.nlinfun)
        if minibatch and (m.minibatch_size > MAX_MINIBATCH or min(m.minibatch_size, m.num_data) > MAX_MINIBATCH):
            raise ValueError("model %d: minibatch of %d frames > %d; %s" % (k, m.minibatch_size, MAX_MINIBATCH, single))
        for kern, M in [(m.kern_act[i], m.num_inducing_a[i]) for i in range(m.num_sources)] + \
                       [(m.kern_com[i], m.num_inducing_c[i]) for i in range(m.num_sources)]:
            if M > MAX_M:
                raise ValueError("model %d: %d inducing points in one latent GP > %d; %s" % (k, M, MAX_M, single))
            t = getattr(kern, "type_code", None)
            if t not in _KERNELS:
                raise NotImplementedError("model %d: kernel %s is not batched (takes %s); %s"
                                          % (k, type(kern).__name__, ", ".join(sorted(_KERNELS.values())), single))
            mp = int(kern.num_partials)
            if t in (_lib.KERN_MERCER_MATERN12SM, _lib.KERN_MATERN32SM) and not 1 <= mp <= MAX_PARTIALS:
                raise ValueError("model %d: %d partials outside 1..%d; %s" % (k, mp, MAX_PARTIALS, single))
    return models


def check_batchable(models, method=None, callback=None):
    """Host-only scope check of optimize_many / PdgpBatch: raises NotImplementedError (a feature the batch does not
    have) or ValueError (a shape it does not take) naming the single-model path.  No device work."""
    if method is not None and not isinstance(method, AdamOptimizer):
        raise NotImplementedError("optimize_many trains with AdamOptimizer only (got %r); %s" % (method, _SINGLE))
    if callback is not None:
        raise NotImplementedError("optimize_many takes no callback; %s" % _SINGLE)
    return _check_models(models, "optimize_many", _SINGLE, minibatch=True)


def check_batchable_natgrad(models, method, callback=None):
    """Host-only scope check of optimize_many / PdgpBatch.optimize with a NatGradAdam token (check_batchable stays the
    Adam path's): the models' scope as there, no callback, and per model Pdgp._natgrad_gps(method) — gamma outside
    (0, 1] on a token changed after construction, or one of a q_mu / q_sqrt pair fixed, is a ValueError that names the
    model; a GP with both fixed is skipped.  Returns the models and one list of flags per model, rows
    [g_0..g_{P-1}, f_0..f_{P-1}]: does the step move that GP's q(u)?  No device work."""
    if not isinstance(method, NatGradAdam):
        raise NotImplementedError("check_batchable_natgrad takes a NatGradAdam token (got %r)" % (method,))
    if callback is not None:
        raise NotImplementedError("optimize_many takes no callback; %s" % _SINGLE)
    models = _check_models(models, "optimize_many", _SINGLE, minibatch=True)
    flags = []
    for k, m in enumerate(models):
        try:
            flags.append(m._natgrad_gps(method))
        except ValueError as e:
            raise ValueError("model %d: %s" % (k, e))
    return models, flags


def _check_for(models, method, callback=None):
    """the host check of the token's type: (models, NatGradAdam's per-model flags or None)"""
    if isinstance(method, NatGradAdam):
        return check_batchable_natgrad(models, method, callback)
    return check_batchable(models, method, callback), None


def model_segments(m, base=0):
    """[(offset, Param)] of one model's block of the batch's parameter vector (include/gpitch_abi.h gp_pdgpb_config):
    [noise | per latent GP: theta | z | q_mu | q_sqrt], starting at `base`; also returns the block's length"""
    segs = [(base, m.likelihood.variance)]
    off = base + 1
    for kern, z, q_mu, q_sqrt in latent_gps(m):
        for j, p in enumerate(kern.theta_params()):
            segs.append((off + j, p))
        off += 2 + 2 * int(kern.num_partials)
        M = z.size
        segs += [(off, z), (off + M, q_mu), (off + 2 * M, q_sqrt)]
        off += 2 * M + M * M
    return segs, off - base


def _segments(models):
    """model_segments of every model back to back: per model its segments and its (first, end) slots; the vector's length"""
    segs, ranges, base = [], [], 0
    for m in models:
        sm, n = model_segments(m, base)
        segs.append(sm)
        ranges.append((base, base + n))
        base += n
    return segs, ranges, base


# ------------------------------------------------------------------------------------------------------------------
# tied parameters: Params of one model or of several that are ONE parameter (csrc/pdgp_batch.hip pdgpb_tie_kernel,
# gp_pdgpb_set_ties)
def _param_names(kern):
    """id(Param) -> its name in the kernel ("lengthscales", "energy[1]"), through nested kernels; theta_params() names a
    Param by its position ("theta[j]") when no attribute holds it"""
    names = {}

    def walk(obj, prefix):
        for name in sorted(obj.__dict__):
            v = obj.__dict__[name]
            if isinstance(v, Param):
                names.setdefault(id(v), prefix + name)
            elif isinstance(v, (list, tuple, ParamList)):
                for j, it in enumerate(v):
                    if isinstance(it, Param):
                        names.setdefault(id(it), "%s%s[%d]" % (prefix, name, j))
                    elif isinstance(it, Parameterized):
                        walk(it, "%s%s[%d]." % (prefix, name, j))
            elif isinstance(v, Parameterized):
                walk(v, prefix + name + ".")

    walk(kern, "")
    for j, p in enumerate(kern.theta_params()):
        names.setdefault(id(p), "theta[%d]" % j)
    return names


def _tie_roles(models, segs):
    """id(Param) -> (model, offset, role text, is it q(u)?) of every Param of the batch's parameter vector"""
    roles = {}
    for k, m in enumerate(models):
        off = {id(p): o for o, p in segs[k]}
        P = m.num_sources
        v = m.likelihood.variance
        roles[id(v)] = (k, off[id(v)], "model %d, noise, variance" % k, False)
        for r, (kern, z, q_mu, q_sqrt) in enumerate(latent_gps(m)):
            gp = "model %d, %s %d" % (k, "act" if r < P else "com", r if r < P else r - P)
            names = _param_names(kern)
            for p in kern.theta_params():
                roles[id(p)] = (k, off[id(p)], "%s, %s" % (gp, names[id(p)]), False)
            roles[id(z)] = (k, off[id(z)], "%s, %s" % (gp, "za" if r < P else "zc"), False)
            roles[id(q_mu)] = (k, off[id(q_mu)], "%s, q_mu" % gp, True)
            roles[id(q_sqrt)] = (k, off[id(q_sqrt)], "%s, q_sqrt" % gp, True)
    return roles


def tie_groups(models, noise=True, kernels=True, inducing=False):
    """The `tied=` groups that make structurally identical models — the segments of one recording — one model of it: one
    group per noise variance (noise), one per position of every latent GP's kernel.theta_params() (kernels) and, with
    inducing=True, one per za[i] / zc[i] (which needs equal M; q(u) stays each model's own).  Identical: the same P and,
    latent GP by latent GP in the order [g_0..g_{P-1}, f_0..f_{P-1}], the same kernel type and partial count; ValueError
    names the first model that differs from model 0.  Host only; reads no value and changes none (whether the members' values,
    transforms and flags agree is check_tied's matter)."""
    models = list(models)
    if not models:
        raise ValueError("tie_groups needs at least one model")
    shape = lambda m: [(type(g[0]).__name__, int(g[0].num_partials)) for g in latent_gps(m)]
    first = shape(models[0])
    for k, m in enumerate(models[1:], 1):
        if m.num_sources != models[0].num_sources:
            raise ValueError("tie_groups: model %d has %d sources, model 0 has %d" % (k, m.num_sources, models[0].num_sources))
        for r, (a, b) in enumerate(zip(shape(m), first)):
            if a != b:
                raise ValueError("tie_groups: model %d: latent GP %d of [g_0..g_{P-1}, f_0..f_{P-1}] has kernel %s with %d "
                                 "partials, model 0 has %s with %d" % (k, r, a[0], a[1], b[0], b[1]))
        if inducing:
            for r, (g, g0) in enumerate(zip(latent_gps(m), latent_gps(models[0]))):
                if g[1].size != g0[1].size:
                    raise ValueError("tie_groups: inducing=True: model %d: latent GP %d has %d inducing points, model 0 has %d"
                                     % (k, r, g[1].size, g0[1].size))
    groups = []
    if noise:
        groups.append([m.likelihood.variance for m in models])
    gps = [latent_gps(m) for m in models]
    for r in range(len(first)):
        if kernels:
            groups += [list(ps) for ps in zip(*[g[r][0].theta_params() for g in gps])]
        if inducing:
            groups.append([g[r][1] for g in gps])
    return groups


def _tie_list(tied):
    """`tied` as a list of lists (None: no group)"""
    return [] if tied is None else [list(g) for g in tied]


def check_tied(models, tied):
    """Host-only scope check of `tied=` (optimize_many, PdgpBatch), in the style of check_batchable: run before any device
    work, it builds no plan.  tied: an iterable of groups, each an iterable of one or more Params of the listed models —
    likelihood.variance, a Param of a kernel's theta_params(), za[i] / zc[i] — that are ONE parameter.  ValueError names the
    group's index and the offending Param's role (model, noise / act i / com i, Param name) for: a Param of none of the
    models; a Param named twice, in one group or in two; a q_mu / q_sqrt Param (q(u) is each model's own); members whose
    shapes, transforms (type, Logistic bounds), `.fixed` flags, current values (bit for bit) or stored Adam moments differ;
    models joined by a group whose _adam_t differ (their bias-corrected step lengths would).
    Returns the scalar groups the device takes: per group of free Params with two members or more and per element (array
    Params tie element by element) the members' offsets into the batch's parameter vector (model_segments, models back to
    back), in the listed order.  A group whose members are all `.fixed`, and a group of one member, pass the checks and
    yield nothing."""
    models = list(models)
    tied = _tie_list(tied)
    if not tied:
        return []
    segs, _, _ = _segments(models)
    roles = _tie_roles(models, segs)
    moments = {}

    def moment(p):
        k = roles[id(p)][0]
        if k not in moments:
            state = models[k]._adam_state()
            moments[k] = {} if state is None else {id(q): mv for (_, q), mv in zip(segs[k], state)}
        zero = np.zeros(p.size)
        mv = moments[k].get(id(p), (zero, zero))
        return np.asarray(mv[0], dtype=np.float64).reshape(-1), np.asarray(mv[1], dtype=np.float64).reshape(-1)

    same_bits = lambda a, b: a.shape == b.shape and a.tobytes() == b.tobytes()
    seen, out = {}, []
    for gi, group in enumerate(tied):
        if not group:
            raise ValueError("check_tied: group %d is empty" % gi)
        for j, p in enumerate(group):
            if not isinstance(p, Param) or id(p) not in roles:
                raise ValueError("check_tied: group %d: member %d (%r) is not a Param of the listed models (taken: "
                                 "likelihood.variance, a kernel's theta_params(), za[i] / zc[i])" % (gi, j, p))
            k, _, role, is_q = roles[id(p)]
            if id(p) in seen:
                raise ValueError("check_tied: group %d: %s appears twice (first in group %d)" % (gi, role, seen[id(p)]))
            seen[id(p)] = gi
            if is_q:
                raise ValueError("check_tied: group %d: %s: q(u) is never tied (it is what differs per model, and the "
                                 "natural-gradient step moves it per latent GP)" % (gi, role))
        p0 = group[0]
        k0, _, role0, _ = roles[id(p0)]
        for p in group[1:]:
            k, _, role, _ = roles[id(p)]
            what = None
            t, t0 = p.transform, p0.transform
            if p.shape != p0.shape:
                what = "has shape %r, %s has %r" % (p.shape, role0, p0.shape)
            elif type(t) is not type(t0) or (isinstance(t, Logistic) and (t.a, t.b) != (t0.a, t0.b)):
                describe = lambda u: "Logistic(%r, %r)" % (u.a, u.b) if isinstance(u, Logistic) else type(u).__name__
                what = "has transform %s, %s has %s" % (describe(t), role0, describe(t0))
            elif bool(p.fixed) != bool(p0.fixed):
                what = "has fixed=%s, %s has fixed=%s" % (bool(p.fixed), role0, bool(p0.fixed))
            elif not same_bits(p._array, p0._array):
                what = "holds %s, %s holds %s (tied Params start from the same value, bit for bit)" % (
                    np.array2string(p._array.reshape(-1), threshold=4), role0, np.array2string(p0._array.reshape(-1), threshold=4))
            elif not p.fixed and not all(same_bits(a, b) for a, b in zip(moment(p), moment(p0))):
                what = "and %s have different stored Adam moments" % role0
            elif not p.fixed and models[k]._adam_t != models[k0]._adam_t:
                what = "belongs to a model at Adam step %d, %s to one at step %d (their step lengths would differ)" % (
                    models[k]._adam_t, role0, models[k0]._adam_t)
            if what is not None:
                raise ValueError("check_tied: group %d: %s %s" % (gi, role, what))
        if len(group) >= 2 and not p0.fixed:
            offs = [roles[id(p)][1] for p in group]
            out += [[o + e for o in offs] for e in range(p0.size)]
    return out


def _tied_sets(models, segs, groups):
    """the tied sets of scalar groups (check_tied's result): lists of model indices, ascending, that a chain of groups
    joins — two models or more; what gp_pdgpb_set_ties derives on its side"""
    starts = np.array([s[0][0] for s in segs])
    root = list(range(len(models)))

    def find(k):
        while root[k] != k:
            root[k] = root[root[k]]
            k = root[k]
        return k

    for g in groups:
        ks = [find(int(np.searchsorted(starts, o, side="right")) - 1) for o in g]
        for k in ks:
            root[find(k)] = find(min(ks))
    sets = {}
    for k in range(len(models)):
        sets.setdefault(find(k), []).append(k)
    return [s for s in sets.values() if len(s) >= 2]


def _config(models, train):
    """gp_pdgpb_config of the models — a training plan's with the minibatch sizes B and the data counts N, a predict-only
    plan's without — and the ctypes arrays it points to, which the caller keeps alive as long as the config"""
    i32, nm = C.c_int32, len(models)
    gps = [g for m in models for g in latent_gps(m)]
    keep = dict(
        P=(i32 * nm)(*[m.num_sources for m in models]),
        B=(i32 * nm)(*[min(m.minibatch_size, m.num_data) for m in models]) if train else None,
        nlin=(i32 * nm)(*[nlin_code(m.nlinfun) for m in models]),
        N=(C.c_double * nm)(*[float(m.num_data) for m in models]) if train else None,
        M=(i32 * len(gps))(*[g[1].size for g in gps]),
        kt=(i32 * len(gps))(*[g[0].type_code for g in gps]),
        mp=(i32 * len(gps))(*[int(g[0].num_partials) for g in gps]))
    k = keep
    return _lib.PdgpBatchConfig(nm, k["P"], k["B"], k["nlin"], k["N"], k["M"], k["kt"], k["mp"], jitter), keep


def draw_indices(m, steps):
    """the next `steps` minibatches of model m exactly as Pdgp._batch draws them (sorted in time order), advancing
    m.x / m.y the same way; a (steps, B) int64 array.  A model whose minibatch covers its data draws nothing (_batch).
    With replacement (minibatch / N < 0.5) the steps are drawn as one block: randint(N, size=(k, B)) yields the stream
    and leaves the state of k single draws.  The permutation branch is drawn step by step."""
    N, B = m.num_data, m.minibatch_size
    if m.x.minibatch_size >= N and m.y.minibatch_size >= N:
        return np.tile(np.arange(N, dtype=np.int64), (steps, 1))

    def draw():
        if float(m.x.minibatch_size) / float(N) < 0.5 and steps > 0:
            return m.x.rng.randint(N, size=(steps, m.x.minibatch_size))
        return np.stack([m.x.next_indices() for _ in range(steps)]) if steps else np.zeros((0, B), dtype=np.int64)

    return draw_in_lockstep(m.x, m.y, draw, steps)


def _describe_not_pd(code):
    """gp_pdgpb_not_pd's per-model word (1 + 128 row + pivot) as text"""
    row, pivot = divmod(int(code) - 1, MAX_M)
    return "latent GP row %d of [g_0..g_{P-1}, f_0..f_{P-1}], pivot %d" % (row, pivot)


def _describe_refused(k, code, P, gamma, method=None):
    """gp_pdgpb_natgrad_refused's word of model k (the same 1 + 128 row + pivot) as the refusal's message; `method`: the
    token of a call through gp_pdgpb_natgrad_adaptive, whose message names the last length tried and the halvings"""
    row, pivot = divmod(int(code) - 1, MAX_M)
    if method is not None:
        last = method.role_gammas(P)[row] * 2.0 ** -method.halvings
        return ("NatGradAdam: model %d: the natural-gradient step was too long: I - 2 gamma P of the %s GP %d (latent GP %d) "
                "is not positive definite (pivot %d) at gamma = %g, the last length tried after halvings = %d; the model was "
                "left as it was, take a smaller gamma or more halvings"
                % (k, "activation" if row < P else "component", row if row < P else row - P, row, pivot, last,
                   method.halvings))
    return ("NatGradAdam: model %d: the natural-gradient step was too long: I - 2 gamma P of the %s GP %d (latent GP %d) "
            "is not positive definite (pivot %d) at gamma = %g; the model was left as it was, take a smaller gamma"
            % (k, "activation" if row < P else "component", row if row < P else row - P, row, pivot, gamma))


class PdgpBatch(object):
    """The plan behind optimize_many: every model's parameters in one device vector, one gp_pdgpb plan sized by the
    batch's own shapes (no single-model engine plan is built)."""

    def __init__(self, models, handle=None, tied=None):
        self.models = check_batchable(models)
        self._tied = _tie_list(tied)               # the groups as given: optimize() checks them again at every call
        groups = check_tied(self.models, self._tied)
        h = self._handle = handle or _lib.default_handle()
        self._free_idx = []
        self._segs, self._range, self.num_params = _segments(self.models)
        nm = len(self.models)
        cfg, self._cfg_keep = _config(self.models, train=True)
        plan = C.c_void_p()
        h.check(h.lib.gp_pdgpb_create(h.h, C.byref(cfg), C.byref(plan)))
        self._plan = plan
        if int(h.lib.gp_pdgpb_num_params(plan)) != self.num_params:
            raise RuntimeError("gp_pdgpb layout disagrees with the host layout")
        self._ws = h.workspace(h.lib.gp_pdgpb_workspace_bytes(plan))
        h.check(h.lib.gp_pdgpb_set_workspace(plan, self._ws.data_ptr(), self._ws.numel()))
        self._data_off = np.concatenate([[0], np.cumsum([m.num_data for m in self.models])])
        self._x = h.to_device(np.concatenate([m.x._array.reshape(-1) for m in self.models]))
        self._y = h.to_device(np.concatenate([m.y._array.reshape(-1) for m in self.models]))
        n = self.num_params
        self._params, self._free, self._grad = h.zeros(n), h.zeros(n), h.zeros(n)
        self._adam_m, self._adam_v = h.zeros(n), h.zeros(n)
        self._elbo = h.zeros(nm)
        self._tcode = h.torch.zeros(n, dtype=h.torch.uint8, device=h.device)
        self._ng_ws = None             # gp_pdgpb_natgrad's workspace, from the first NatGradAdam call on
        self._nga_ws = None            # gp_pdgpb_natgrad_adaptive's (per-role lengths / halving), likewise
        self._ng_last = None           # the one of the two the plan has seen last (its refusal words)
        self._tie_groups, self._tie_sets, self._tie_ws = [], [], None
        self._set_ties(groups)

    # ------------------------------------------------------------------------------------------
    def _pack(self):
        """host Params -> device parameter vector, transform codes and free state; the free-state index and the
        gradients the backward pass skips follow the models' current `.fixed` flags"""
        h = self._handle
        self._free_idx = [free_index(m, segs) for m, segs in zip(self.models, self._segs)]
        flatvec.set_grad_needs(h, h.lib.gp_pdgpb_set_grad_needs, self._plan,
                               [g for m in self.models for g in latent_gps(m)])
        host, tc = flatvec.pack([sp for segs in self._segs for sp in segs], self.num_params, h)
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
        return -flatvec.free_gradient(self._segs[k], free_host, grad_host)[self._free_idx[k]]

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

    def refused(self, clear=True):
        """per model: 0, or 1 + 128 row + pivot of its refused natural-gradient step with the smallest (latent GP row,
        pivot); all 0 before the first NatGradAdam call"""
        if self._ng_last is None:
            return np.zeros(len(self.models), dtype=np.int64)
        out = (C.c_int32 * len(self.models))()
        h = self._handle
        h.check(h.lib.gp_pdgpb_natgrad_refused(self._plan, out, int(bool(clear))))
        return np.array(out[:], dtype=np.int64)

    def _set_ties(self, groups):
        """hand the plan the scalar tie groups of check_tied (none: clear its ties) in a workspace of their own"""
        if groups == self._tie_groups:
            return
        h = self._handle
        if not groups:
            h.check(h.lib.gp_pdgpb_set_ties(self._plan, 0, None, None, None, 0))
            self._tie_groups, self._tie_sets, self._tie_ws = [], [], None
            return
        start = np.concatenate([[0], np.cumsum([len(g) for g in groups])])
        gs = (C.c_int32 * start.size)(*[int(v) for v in start])
        mem = (C.c_int64 * int(start[-1]))(*[int(o) for g in groups for o in g])
        h.sync()                                   # nothing in flight still reads the workspace this one replaces
        ws = h.workspace(h.lib.gp_pdgpb_ties_workspace_bytes(len(groups), int(start[-1]), len(self.models)))
        h.check(h.lib.gp_pdgpb_set_ties(self._plan, len(groups), gs, mem, ws.data_ptr(), ws.numel()))
        self._tie_groups, self._tie_sets, self._tie_ws = groups, _tied_sets(self.models, self._segs, groups), ws

    def set_tied(self, tied):
        """replace the plan's tie groups (None or []: no ties, optimize() then launches what it launches without them)"""
        tied = _tie_list(tied)
        groups = check_tied(self.models, tied)
        self._tied = tied
        self._set_ties(groups)

    def ties_frozen(self, clear=True):
        """per model: 0, or 1 + the index of the lowest failed model of its tied set at the iteration the set stopped; all
        0 without ties"""
        if not self._tie_groups:
            return np.zeros(len(self.models), dtype=np.int64)
        out = (C.c_int32 * len(self.models))()
        h = self._handle
        h.check(h.lib.gp_pdgpb_ties_frozen(self._plan, out, int(bool(clear))))
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
        """`maxiter` iterations of every model with an AdamOptimizer or a NatGradAdam token (see optimize_many)"""
        _, flags = _check_for(self.models, method)
        groups = check_tied(self.models, self._tied)     # values, flags and moments may have changed since the last call
        natgrad = flags is not None
        h = self._handle
        self._set_ties(groups)
        self.ties_frozen(clear=True)
        self._pack()
        self._load_moments()
        self.not_pd(clear=True)
        nm = len(self.models)
        adaptive = natgrad and method.adaptive()     # per-role lengths / halving: gp_pdgpb_natgrad_adaptive
        if natgrad:
            step_gps = [f for fl in flags for f in fl]
            step_gps = (C.c_int32 * len(step_gps))(*step_gps)
            if self._ng_last is not None:
                self.refused(clear=True)
            if adaptive:
                gammas = [g for m in self.models for g in method.role_gammas(m.num_sources)]
                gammas = (C.c_double * len(gammas))(*gammas)
                if self._nga_ws is None:
                    self._nga_ws = h.workspace(h.lib.gp_pdgpb_natgrad_adaptive_workspace_bytes(self._plan))
                else:                                # the call's counters start from zero
                    h.check(h.lib.gp_pdgpb_natgrad_counts(self._plan, None, None, 1))
            elif self._ng_ws is None:
                self._ng_ws = h.workspace(h.lib.gp_pdgpb_natgrad_workspace_bytes(self._plan))
            self._ng_last = self._nga_ws if adaptive else self._ng_ws
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
            args = (self._plan, self._free.data_ptr(), self._params.data_ptr(), self._tcode.data_ptr(),
                    self._adam_m.data_ptr(), self._adam_v.data_ptr(), self._x.data_ptr(), self._y.data_ptr(),
                    idx.data_ptr(), k, lr_dev.data_ptr(), method.beta1, method.beta2, method.epsilon)
            if adaptive:
                h.check(h.lib.gp_pdgpb_natgrad_adaptive(*(args + (gammas, method.halvings, step_gps,
                                                                  self._nga_ws.data_ptr(), self._nga_ws.numel()))))
            elif natgrad:
                # the same evaluation; the step on q(u) reads its blocks of the gradient and zeroes them, so that Adam
                # behind it (zero gradient, zero moments: an update of exactly 0) moves everything else only
                h.check(h.lib.gp_pdgpb_natgrad(*(args + (method.gamma, step_gps, self._ng_ws.data_ptr(),
                                                         self._ng_ws.numel()))))
            else:
                h.check(h.lib.gp_pdgpb_adam(*args))
            done += k
        bad = self.not_pd(clear=True)
        # a model whose Kuu failed is reported as that (its garbage gradient may have raised the refusal word as well)
        refused = self.refused(clear=True) if natgrad else np.zeros(nm, dtype=np.int64)
        frozen = self.ties_frozen(clear=True)
        counts = self._natgrad_counts(method) if adaptive else None      # one read, after the last iteration
        # GPflow evaluates the returned fun / jac on a fresh minibatch (Pdgp.optimize)
        draws = [draw_indices(m, 1) for m in self.models]
        elbo, grad = self._evaluate(draws)
        final_bad = self.not_pd(clear=True)     # a failure in the final evaluation voids that model's fun / jac
        bad = np.where(bad != 0, bad, final_bad)
        for tset in self._tie_sets:             # a set whose only failure is the final evaluation's stops together as well
            failed = [k for k in tset if bad[k] or refused[k]]
            for k in tset:
                if failed and not frozen[k]:
                    frozen[k] = 1 + failed[0]
        h.sync()
        del keep
        free = self._free.cpu().numpy()
        params = self._params.cpu().numpy()
        mom_m, mom_v = self._adam_m.cpu().numpy(), self._adam_v.cpu().numpy()
        results = []
        for k, m in enumerate(self.models):
            if bad[k] or refused[k] or frozen[k]:
                # frozen since its failed step (or that of a model it is tied to): the model keeps its Params, Adam state
                # and generators
                xs, ys = rng_keep[k]
                if xs is not None:
                    m.x.rng.set_state(xs)
                if ys is not None:
                    m.y.rng.set_state(ys)
                j = k if bad[k] or refused[k] else int(frozen[k]) - 1      # the model whose failure stopped this one
                if bad[j]:
                    msg = "Cholesky failed: %s" % _describe_not_pd(bad[j])
                else:
                    msg = _describe_refused(j, refused[j], self.models[j].num_sources, method.gamma,
                                            method if adaptive else None)
                if j != k:
                    msg = "model %d: stopped together with model %d, to which it is tied: %s" % (k, j, msg)
                results.append(OptimizeResult(fun=None, jac=None, x=None, success=False, status="error", message=msg,
                                              error=_lib.NotPositiveDefiniteError(_lib.GP_ERR_NOT_PD, msg)))
                if adaptive:                         # what it had accumulated up to the refusing iteration
                    results[-1]["natgrad"] = counts[k]
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
            if adaptive:
                results[-1]["natgrad"] = counts[k]
        return results

    def _natgrad_counts(self, method):
        """per model the adaptive step's counters of this call, rows [g_0..g_{P-1}, f_0..f_{P-1}]; the shortest length starts
        at the GP's own gamma_r (the device reports +inf for a GP that took no step)"""
        h = self._handle
        G = sum(2 * m.num_sources for m in self.models)
        hv, sg = (C.c_int64 * G)(), (C.c_double * G)()
        h.check(h.lib.gp_pdgpb_natgrad_counts(self._plan, hv, sg, 0))
        out, g0 = [], 0
        for m in self.models:
            n = 2 * m.num_sources
            out.append({"halvings": [int(v) for v in hv[g0:g0 + n]],
                        "shortest_gamma": [min(float(v), g) for v, g in zip(sg[g0:g0 + n], method.role_gammas(m.num_sources))]})
            g0 += n
        return out

    def __del__(self):
        try:
            if self._plan is not None and self._handle is not None and self._handle.h:
                self._handle.sync()
                self._handle.lib.gp_pdgpb_destroy(self._plan)
        except Exception:
            pass


def optimize_many(models, method=None, maxiter=1000, callback=None, tied=None):
    """Train every model in `models` (ordinary Pdgp objects) as  m.optimize(method=method, maxiter=maxiter)  would, all
    of them together: one OptimizeResult per model.  A model whose Cholesky fails is frozen and its result carries
    `error`; the others go on.  method: an AdamOptimizer or a NatGradAdam token shared by all models (default
    AdamOptimizer()).

    NatGradAdam(gamma, learning_rate, ...): per iteration the Adam branch's evaluation, a natural-gradient step on q(u)
    of every latent GP whose q_mu and q_sqrt are both free (both fixed: skipped; one of the two: ValueError), then Adam
    on the rest (train.NatGradAdam).  A model whose step is too long — I - 2 gamma P of one of its GPs is
    not positive definite — is refused on its own: none of its GPs is stepped, it is frozen from that iteration on and
    ends as a model with a failed Cholesky does (Params, Adam state, _adam_t and generators as before the call,
    success=False, error a NotPositiveDefiniteError naming NatGradAdam, the model, the GP, the pivot and gamma).  The
    Moments that an earlier AdamOptimizer run left on q_mu / q_sqrt are not cleared: Adam then keeps coasting on them
    beside the step, as in Pdgp.optimize.  Start NatGradAdam on fresh models, or accept that.

    tied: groups of Params that are ONE parameter (check_tied; tie_groups builds them for the segments of one recording:
    one noise variance, one set of kernels, q(u) and by default the inducing inputs per segment).  The objective is then
    the sum of the models' ELBOs: per iteration the shared parameter's gradient is the sum over the group's members, one
    Adam update is applied, and every member ends on the same value and the same Adam moments, bit for bit (DESIGN.md
    3l).  One result per model as without ties, `fun` / `jac` / `x` its own.  Models that ties join, directly or through
    a chain, stop together: when one of them fails, all of them are frozen at that iteration and end as a failed model
    does; the others' messages name the model they are tied to and repeat its cause.  Without `tied` nothing changes."""
    method = AdamOptimizer() if method is None else method
    models, _ = _check_for(models, method, callback)
    return PdgpBatch(models, tied=tied).optimize(method, maxiter)


# ------------------------------------------------------------------------------------------------------------------
# prediction: Pdgp.predict_act_n_com of many models (csrc/pdgp_batch.hip pdgpb_pred_*, gp_pdgpb_predict)
MAX_PREDICT_FRAMES = 1 << 22   # latent-GP frames (2 P x frames, summed over models) per gp_pdgpb_predict launch
PREDICT_TILE = 64              # frames per (latent GP, frame tile) entry of pdgpb_pred_kernel (PB_PT)
_SINGLE_PREDICT = "predict this model on its own with Pdgp.predict_act_n_com"


def _frames(x, k):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim > 2 or (a.ndim == 2 and a.shape[1] != 1):
        raise ValueError("predict_many: inputs of model %d have shape %r, not (n,) or (n, 1)" % (k, a.shape))
    return a.reshape(-1)


def check_predictable(models, xnews):
    """Host-only scope check of predict_many, in the style of check_batchable: NotImplementedError (a feature the batch
    does not have) or ValueError (a shape it does not take) naming the single-model path.  No minibatch limit: the
    prediction does not use the minibatch.  Returns the models and their inputs as flat float64 arrays; `xnews` is a
    list with one array per model or one array for every model."""
    models = _check_models(models, "predict_many", _SINGLE_PREDICT, minibatch=False)
    if isinstance(xnews, (list, tuple)):
        if len(xnews) != len(models):
            raise ValueError("predict_many: %d input arrays for %d models" % (len(xnews), len(models)))
        xs = [_frames(x, k) for k, x in enumerate(xnews)]
    else:
        x = _frames(xnews, 0)
        xs = [x] * len(models)
    return models, xs


def predict_layout(num_sources, counts, tile=PREDICT_TILE):
    """The work list and output offsets of one gp_pdgpb_predict call (what the call builds from xnew_off), host only.
    Latent GPs are listed model by model, rows [g_0..g_{P-1}, f_0..f_{P-1}].  Returns a dict of int64 arrays:
      tile_start [G + 1]  first (latent GP, frame tile) entry of each GP, GP-major; the last item is the entry count
      gp_out [G]          each GP's first element in fmean / fvar (model-major: per model 2 P rows of n_k frames)
      gp_src [G]          activation rows: the source's first element in mean_source (P rows of n_k per model), else -1
      out_base, src_base [num_models + 1]  each model's block in fmean / fvar and in mean_source
      x_off [num_models + 1]  each model's first frame in xnew (the call's xnew_off)"""
    P = np.asarray(num_sources, dtype=np.int64)
    n = np.asarray(counts, dtype=np.int64)
    assert P.shape == n.shape and np.all(P >= 1) and np.all(n >= 0)
    cum = lambda a: np.concatenate([[0], np.cumsum(a)]).astype(np.int64)
    out_base, src_base, x_off = cum(2 * P * n), cum(P * n), cum(n)
    gp_out, gp_src, ntile = [], [], []
    for k in range(P.size):
        for r in range(2 * int(P[k])):
            gp_out.append(out_base[k] + r * n[k])
            gp_src.append(src_base[k] + r * n[k] if r < P[k] else -1)
            ntile.append((n[k] + tile - 1) // tile)
    i64 = lambda a: np.asarray(a, dtype=np.int64)
    return dict(tile_start=cum(i64(ntile)), gp_out=i64(gp_out), gp_src=i64(gp_src), out_base=out_base,
                src_base=src_base, x_off=x_off)


def predict_chunks(num_sources, counts, limit=MAX_PREDICT_FRAMES):
    """Split the frames of one predict_many call into launches of at most `limit` latent-GP frames (2 P per frame of a
    model; a single frame of a model with 2 P > limit goes alone).  Each chunk is a (num_models, 2) int64 array of
    (first frame, frame count) per model, models in order, frames in order; together they cover every frame once."""
    nm = len(counts)
    chunks, cur, used = [], np.zeros((nm, 2), dtype=np.int64), 0
    for k in range(nm):
        per = 2 * int(num_sources[k])
        start, left = 0, int(counts[k])
        while left > 0:
            take = min(left, (limit - used) // per)
            if take == 0:
                if used == 0:
                    take = 1
                else:
                    chunks.append(cur)
                    cur, used = np.zeros((nm, 2), dtype=np.int64), 0
                    continue
            cur[k] = (start, take)
            start, left, used = start + take, left - take, used + take * per
    if used > 0 or not chunks:
        chunks.append(cur)
    return chunks


@contextlib.contextmanager
def _predict_plan(h, models):
    """a predict-only gp_pdgpb plan of the models (no minibatch, no training state), destroyed behind the stream's work"""
    cfg, keep = _config(models, train=False)
    plan = C.c_void_p()
    h.check(h.lib.gp_pdgpb_create(h.h, C.byref(cfg), C.byref(plan)))
    try:
        yield plan
    finally:
        h.sync()
        h.lib.gp_pdgpb_destroy(plan)


def _predict_batch(entry, models, xs, ys, blocks, ws_bytes, launch):
    """The device work of predict_many and predict_sources_many (`entry` names the caller in messages), after the host
    checks: one predict-only plan, every Param uploaded once, gp_pdgpb_predict_prepare, then one launch(...) per
    MAX_PREDICT_FRAMES chunk of the inputs xs (and targets ys, or None) with one copy back each.

    blocks names each output array by the predict_layout key of its per-model offsets: "out_base" (2 P_k rows of n_k
    frames per model), "src_base" (P_k rows) or "x_off" (one row).  ws_bytes(lib, plan, latent) sizes the workspace,
    `latent` being the largest chunk's count of latent-GP frames; launch(lib, plan, params, xd, off, yd, out, ws, nws)
    runs one chunk, `out` holding a device pointer per block.  Returns per model one (rows, n_k) array per block."""
    h = _lib.default_handle()
    t = h.torch
    nm = len(models)
    P = [m.num_sources for m in models]
    counts = [x.size for x in xs]
    rows = lambda key, k: {"out_base": 2 * P[k], "src_base": P[k], "x_off": 1}[key]
    segs, _, base = _segments(models)
    # host results in the layout of one call over every frame: a call that fits one launch lands there directly, the
    # chunks of a larger one are copied into it; every model's arrays are views of these buffers
    whole = predict_layout(P, counts)
    chunks = predict_chunks(P, counts, MAX_PREDICT_FRAMES)
    res = [np.zeros(int(whole[key][-1])) for key in blocks]
    with _predict_plan(h, models) as plan:
        if int(h.lib.gp_pdgpb_num_params(plan)) != base:
            raise RuntimeError("gp_pdgpb layout disagrees with the host layout")
        # every Param written once into a page-locked vector, copied to the device on the stream
        ppin = t.empty(base, dtype=t.float64, pin_memory=True)
        flatvec.pack([sp for sm in segs for sp in sm], base, out=ppin.numpy())
        params = ppin.to(h.device, non_blocking=True)
        latent = max(int(np.dot(2 * np.asarray(P, dtype=np.int64), c[:, 1])) for c in chunks)
        ws = h.workspace(ws_bytes(h.lib, plan, latent))
        h.check(h.lib.gp_pdgpb_predict_prepare(plan, params.data_ptr(), ws.data_ptr(), ws.numel()))
        for chunk in chunks:
            c = chunk[:, 1]
            if not c.any():
                continue
            lay = predict_layout(P, c)
            nx = int(lay["x_off"][-1])
            # transfers go through page-locked staging buffers (torch's caching host allocator): pageable copies of
            # tens of MB cost several times the kernels
            xpin = t.empty(nx * (2 if ys is not None else 1), dtype=t.float64, pin_memory=True)
            np.concatenate([xs[k][s:s + n] for k, (s, n) in enumerate(chunk)], out=xpin.numpy()[:nx])
            if ys is not None:
                np.concatenate([ys[k][s:s + n] for k, (s, n) in enumerate(chunk)], out=xpin.numpy()[nx:])
            xd = xpin.to(h.device, non_blocking=True)
            starts = np.concatenate([[0], np.cumsum([int(lay[key][-1]) for key in blocks])])
            buf = h.empty(int(starts[-1]))              # the blocks one after another: one copy back to the host
            off = (C.c_int64 * (nm + 1))(*[int(v) for v in lay["x_off"]])
            h.check(launch(h.lib, plan, params.data_ptr(), xd.data_ptr(), off,
                           xd[nx:].data_ptr() if ys is not None else None,
                           [buf[int(a):].data_ptr() for a in starts[:-1]], ws.data_ptr(), ws.numel()))
            pin = t.empty(int(starts[-1]), dtype=t.float64, pin_memory=True)
            pin.copy_(buf, non_blocking=True)
            h.sync()
            got = pin.numpy().copy()                    # the results live in ordinary memory; the staging goes back
            del xpin, pin
            for j, key in enumerate(blocks):
                g = got[int(starts[j]):int(starts[j + 1])]
                if len(chunks) == 1:
                    res[j] = g
                    continue
                for k, (s, n) in enumerate(chunk):
                    if n:
                        d = res[j][whole[key][k]:whole[key][k + 1]].reshape(rows(key, k), counts[k])
                        d[:, s:s + n] = g[lay[key][k]:lay[key][k + 1]].reshape(rows(key, k), n)
        del ppin
        bad = (C.c_int32 * nm)()
        h.check(h.lib.gp_pdgpb_not_pd(plan, bad, 1))
    for k in range(nm):
        if bad[k]:
            raise _lib.NotPositiveDefiniteError(_lib.GP_ERR_NOT_PD, "%s: model %d: Cholesky failed: %s"
                                                % (entry, k, _describe_not_pd(bad[k])))
    return [[res[j][whole[key][k]:whole[key][k + 1]].reshape(rows(key, k), counts[k]) for j, key in enumerate(blocks)]
            for k in range(nm)]


def predict_many(models, xnews):
    """Pdgp.predict_act_n_com of every model at its own inputs, all models together:

        preds = predict_many(models, xnews)
        preds[k] == models[k].predict_act_n_com(xnews[k])   # (mu_a, var_a, mu_c, var_c, m_src), lists of (n_k, 1)

    xnews: one array per model or one array for every model.  Reads each model's current Params and changes nothing
    (no Param, flag, generator or Adam state; no single-model engine plan, no prediction memo).  One launch factors
    every latent GP's Kuu, then one launch per MAX_PREDICT_FRAMES chunk predicts every (latent GP, frame tile) pair and
    one more forms the source means.  A failed Kuu factorisation raises NotPositiveDefiniteError naming the model."""
    models, xs = check_predictable(models, xnews)
    got = _predict_batch(
        "predict_many", models, xs, None, ("out_base", "out_base", "src_base"),      # fmean | fvar | mean_source
        lambda lib, plan, latent: lib.gp_pdgpb_predict_workspace_bytes(plan),
        lambda lib, plan, params, xd, off, yd, out, ws, nws: lib.gp_pdgpb_predict(plan, params, xd, off, *out, ws, nws))
    out = []
    for m, (fm, fv, src) in zip(models, got):
        r = range(m.num_sources)
        out.append(([col(fm, i) for i in r], [col(fv, i) for i in r],
                    [col(fm, len(r) + i) for i in r], [col(fv, len(r) + i) for i in r], [col(src, i) for i in r]))
    return out


# ------------------------------------------------------------------------------------------------------------------
# posterior of the sources, predictive moments of the mixture and held-out density of many models
# (csrc/pdgp_batch.hip pdgpb_pred_moments_kernel, gp_pdgpb_predict_moments)
def _targets(ynews, xs):
    """ynews as flat float64 arrays, one per model, each as long as the model's inputs (ValueError otherwise)"""
    if ynews is None:
        return None
    if isinstance(ynews, (list, tuple)):
        if len(ynews) != len(xs):
            raise ValueError("predict_sources_many: %d target arrays for %d models" % (len(ynews), len(xs)))
        ys = list(ynews)
    else:
        ys = [ynews] * len(xs)
    out = []
    for k, (yk, x) in enumerate(zip(ys, xs)):
        a = np.asarray(yk, dtype=np.float64)
        if a.ndim > 2 or (a.ndim == 2 and a.shape[1] != 1) or a.size != x.size:
            raise ValueError("predict_sources_many: targets of model %d have shape %r for %d inputs" % (k, a.shape, x.size))
        out.append(a.reshape(-1))
    return out


def predict_sources_many(models, xnews, ynews=None):
    """Pdgp.predict_sources, predict_y and (with ynews) expected_log_density of every model at its own inputs, all models
    together:

        res = predict_sources_many(models, xnews, ynews)
        res[k]["mean_s"], res[k]["var_s"]   # lists of P_k (n_k, 1) arrays: models[k].predict_sources(xnews[k])
        res[k]["mean_y"], res[k]["var_y"]   # (n_k, 1): models[k].predict_y(xnews[k])
        res[k]["logp"]                      # (n_k, 1): models[k].expected_log_density(xnews[k], ynews[k]); absent without ynews

    Scope, chunking and staging are predict_many's (check_predictable, predict_chunks, page-locked buffers); the moments
    of the 2P latent GPs stay in the device workspace: the largest chunk's fmean / fvar live behind the factors.
    xnews / ynews: one array per model or one array for every model; ynews[k] must be as long as xnews[k].  Reads each
    model's current Params and changes nothing."""
    models, xs = check_predictable(models, xnews)
    ys = _targets(ynews, xs)
    names = ("mean_s", "var_s", "mean_y", "var_y") + (("logp",) if ys is not None else ())
    got = _predict_batch(
        "predict_sources_many", models, xs, ys, ("src_base", "src_base") + ("x_off",) * (len(names) - 2),
        lambda lib, plan, latent: lib.gp_pdgpb_predict_moments_workspace_bytes(plan, latent),
        lambda lib, plan, params, xd, off, yd, out, ws, nws: lib.gp_pdgpb_predict_moments(
            plan, params, xd, off, yd, *(out + [None])[:5], ws, nws))
    res = []
    for m, arrays in zip(models, got):
        item = dict(zip(names, arrays))
        for name in names[:2]:
            item[name] = [col(item[name], i) for i in range(m.num_sources)]
        for name in names[2:]:
            item[name] = item[name].reshape(-1, 1)
        res.append(item)
    return res


# ------------------------------------------------------------------------------------------------------------------
# joint posterior draws of the sources of many models (csrc/pdgp_batch.hip gp_pdgpb_sample)
MAX_SAMPLE_BYTES = 1 << 30     # device bytes of one gp_pdgpb_sample call's normals and draws (beside sgpr_ss.SAMPLE_EPS_BYTES)
SAMPLE_DRAW_BLOCK = 16         # draws per block of a model's seeded stream; draw chunks are whole blocks
MAX_SAMPLE_GPS = 32767         # latent GPs per gp_pdgpb_sample call
_SINGLE_SAMPLE = "sample this model on its own with Pdgp.sample_sources"
_SAMPLERS = {_lib.KERN_MATERN12: 1, _lib.KERN_MATERN32: 2, _lib.KERN_MERCER_MATERN12SM: 0}   # normals per point (0: 2 m)


def _sample_comps(m, k):
    """normals per point of model k's latent GPs, rows [g_0..g_{P-1}, f_0..f_{P-1}]; NotImplementedError, naming model, role,
    GP and kernel, for a batched kernel without an exact state-space prior sampler"""
    comps = []
    for role, kerns in (("activation", m.kern_act), ("component", m.kern_com)):
        for i in range(m.num_sources):
            code = int(kerns[i].type_code)
            if code not in _SAMPLERS:
                raise NotImplementedError(
                    "sample_sources_many: model %d: the %s GP %d has kernel %s; joint draws need an exact state-space prior "
                    "sampler (supported: %s)" % (k, role, i, _KERN_NAMES.get(code, "type %d" % code),
                                                 ", ".join(_KERN_NAMES[c] for c in sorted(_SAMPLERS))))
            comps.append(_SAMPLERS[code] or 2 * int(kerns[i].num_partials))
    return comps


def check_sampleable(models, xnews):
    """Host-only scope check of sample_sources_many, in the style of check_predictable: everything that one refuses, and every
    latent GP needs a kernel that both the batch and the state-space sampler take (Matern12, Matern32, MercerMatern12sm).
    NotImplementedError names the model, the GP's role and index and its kernel (Matern52, RBF, Matern32sm: batched, no
    sampler) or Pdgp.sample_sources as the single-model path (Matern12sm: sampled, not batched).  No device work.  Returns
    the models and their inputs as flat float64 arrays."""
    models = _check_models(models, "sample_sources_many", _SINGLE_SAMPLE, minibatch=False)
    for k, m in enumerate(models):
        _sample_comps(m, k)
    if isinstance(xnews, (list, tuple)):
        if len(xnews) != len(models):
            raise ValueError("sample_sources_many: %d input arrays for %d models" % (len(xnews), len(models)))
        xs = [_sample_frames(x, k) for k, x in enumerate(xnews)]
    else:
        xs = [_sample_frames(xnews, 0)] * len(models)
    return models, xs


def _sample_frames(x, k):
    a = np.asarray(x, dtype=np.float64)
    if a.ndim > 2 or (a.ndim == 2 and a.shape[1] != 1):
        raise ValueError("sample_sources_many: inputs of model %d have shape %r, not (n,) or (n, 1)" % (k, a.shape))
    return a.reshape(-1)


def sample_layout(num_sources, counts, Ms, comps):
    """Offsets of one gp_pdgpb_sample call at ONE draw, host only (include/gpitch_abi.h).  num_sources, counts: per model
    P_k and n_k; Ms, comps: per latent GP (models in order, rows [g_0..g_{P-1}, f_0..f_{P-1}]) M_r and its normals per point
    c_r.  Returns a dict of int64 arrays, each ending with its total:
      order [G + 1]                  each GP's first entry of order_host (n_k + M_r entries; does not grow with the draws)
      eps_x, eps_z, eps_u [G + 1]    each GP's first double per draw: c_r n_k, c_r M_r, 2 M_r per draw (S draws: times S)
      latents, sources [num_models + 1]   each model's first double per draw: 2 P_k n_k and P_k n_k (S draws: times S)
      x_off [num_models + 1]         the call's xnew_off"""
    P = np.asarray(num_sources, dtype=np.int64)
    n = np.asarray(counts, dtype=np.int64)
    M = np.asarray(Ms, dtype=np.int64)
    c = np.asarray(comps, dtype=np.int64)
    assert P.shape == n.shape and M.shape == c.shape and M.size == 2 * P.sum() and np.all(n >= 0)
    cum = lambda a: np.concatenate([[0], np.cumsum(a)]).astype(np.int64)
    owner = np.repeat(np.arange(P.size), 2 * P)
    ng = n[owner]
    return dict(order=cum(ng + M), eps_x=cum(c * ng), eps_z=cum(c * M), eps_u=cum(2 * M),
                latents=cum(2 * P * n), sources=cum(P * n), x_off=cum(n))


def sample_bytes_per_draw(models, xs):
    """device bytes of ONE draw of each model at its inputs xs[k] (flat arrays): its normals (eps_x, eps_z, eps_u) and its
    draws (2 P latent rows and P source rows of n_k frames) — what sample_split weighs against the budget"""
    out = []
    for m, x in zip(models, xs):
        shapes = m.sample_eps_shapes(x.size, 1)
        out.append(8 * (sum(int(np.prod(sh)) for part in shapes for sh in part) + 3 * m.num_sources * x.size))
    return out


def sample_split(per_draw, gps, num_samples, budget, block=SAMPLE_DRAW_BLOCK, max_gps=MAX_SAMPLE_GPS):
    """The calls of one sample_sources_many: [(first model, end model, [(first draw, draws), ...])], host only.  per_draw:
    device bytes of one draw of each model (normals and draws); gps: its latent GPs.  A joint draw cannot be cut along
    frames, so the models are cut first: consecutive models share a group while one block of min(num_samples, block) draws of
    all of them stays within `budget` bytes and their latent GPs within max_gps; a model too large for that goes alone.
    Each group's draws then go in chunks of whole blocks, as many as the budget holds (at least one): chunk borders are
    multiples of `block`, the unit of the seeded streams.  Every (model, draw) is covered once, in order."""
    S, nb = int(num_samples), min(int(num_samples), block)
    groups, k0, used, ng = [], 0, 0, 0
    for k, (b, g) in enumerate(zip(per_draw, gps)):
        if k > k0 and ((used + int(b)) * nb > budget or ng + g > max_gps):
            groups.append((k0, k, used))
            k0, used, ng = k, 0, 0
        used, ng = used + int(b), ng + g
    groups.append((k0, len(per_draw), used))
    out = []
    for k0, k1, used in groups:
        chunk = S if S <= block else max(1, int(budget // max(1, used * block))) * block
        out.append((k0, k1, [(s0, min(chunk, S - s0)) for s0 in range(0, S, chunk)]))
    return out


def _sample_eps(eps, shapes):
    """caller-supplied eps as float64 arrays, checked against each model's sample_eps_shapes (ValueError otherwise)"""
    if eps is None:
        return None
    if not isinstance(eps, (list, tuple)) or len(eps) != len(shapes):
        raise ValueError("sample_sources_many: eps must be a list with one (eps_x, eps_z, eps_u) triple per model (%d)" % len(shapes))
    out = []
    for k, (e, shs) in enumerate(zip(eps, shapes)):
        G = len(shs[0])
        if not isinstance(e, (list, tuple)) or len(e) != 3 or any(len(a) != G for a in e):
            raise ValueError("sample_sources_many: eps of model %d must be (eps_x, eps_z, eps_u), three lists of %d arrays" % (k, G))
        e = [[np.asarray(a, dtype=np.float64) for a in part] for part in e]
        for name, part, sh in zip(("eps_x", "eps_z", "eps_u"), e, shs):
            for r in range(G):
                if part[r].shape != sh[r]:
                    raise ValueError("sample_sources_many: model %d: %s[%d] has shape %r, not %r (sample_eps_shapes)"
                                     % (k, name, r, part[r].shape, sh[r]))
        out.append(e)
    return out


def _sample_group(h, models, xs, first, chunks, eps, gens, out):
    """one group of sample_split on the device: a predict-only plan, every Param uploaded once, gp_pdgpb_predict_prepare with
    the largest chunk's workspace, then per chunk of draws the normals (staged from the caller's eps or drawn block by block
    from each model's generator), gp_pdgpb_sample and one copy back.  out[k] = [src, g, f] (g, f None when not wanted)"""
    t, lib, nm = h.torch, h.lib, len(models)
    P = [m.num_sources for m in models]
    gps = [g for m in models for g in latent_gps(m)]
    lay = sample_layout(P, [x.size for x in xs], [g[1].size for g in gps],
                        [c for k, m in enumerate(models) for c in _sample_comps(m, first + k)])
    keys = ("eps_x", "eps_z", "eps_u")
    want_lat = out[first][1] is not None
    segs, _, base = _segments(models)
    order = np.ascontiguousarray(np.concatenate(
        [merged_order(xs[k], z.value.reshape(-1)) for k, m in enumerate(models) for _, z, _, _ in latent_gps(m)]))
    assert order.size == lay["order"][-1]
    # the GPs of each model: [first, end) among the group's
    gp0 = np.concatenate([[0], np.cumsum([2 * p for p in P])])
    with _predict_plan(h, models) as plan:
        if int(lib.gp_pdgpb_num_params(plan)) != base:
            raise RuntimeError("gp_pdgpb layout disagrees with the host layout")
        ppin = t.empty(base, dtype=t.float64, pin_memory=True)
        flatvec.pack([sp for sm in segs for sp in sm], base, out=ppin.numpy())
        params = ppin.to(h.device, non_blocking=True)
        nx = int(lay["x_off"][-1])
        xpin = t.empty(nx, dtype=t.float64, pin_memory=True)
        np.concatenate(xs, out=xpin.numpy())
        xd = xpin.to(h.device, non_blocking=True)
        off = (C.c_int64 * (nm + 1))(*[int(v) for v in lay["x_off"]])
        ws = h.workspace(lib.gp_pdgpb_sample_workspace_bytes(plan, off, max(sc for _, sc in chunks)))
        h.check(lib.gp_pdgpb_predict_prepare(plan, params.data_ptr(), ws.data_ptr(), ws.numel()))
        # page-locked staging, allocated once at the largest chunk: the caller's eps going in, the results coming back
        most = max(sc for _, sc in chunks)
        nback = int(lay["sources"][-1]) + (int(lay["latents"][-1]) if want_lat else 0)
        pin = t.empty(most * nback, dtype=t.float64, pin_memory=True)
        epin = None if eps is None else t.empty(most * sum(int(lay[key][-1]) for key in keys), dtype=t.float64, pin_memory=True)
        for s0, sc in chunks:
            tot = [sc * int(lay[key][-1]) for key in keys]
            if eps is not None:
                # the caller's arrays cut to the chunk's draws, in the call's layout (the previous chunk's copy is done: it
                # was synchronised with its results)
                np.concatenate([eps[k][a][r][s0:s0 + sc].reshape(-1) for a in range(3) for k in range(nm)
                                for r in range(2 * P[k])], out=epin.numpy()[:sum(tot)])
                ed = epin[:sum(tot)].to(h.device, non_blocking=True)
                bufs = [ed[sum(tot[:a]):sum(tot[:a + 1])] for a in range(3)]
            else:
                bufs = [h.empty(v) for v in tot]
                for k in range(nm):
                    for b0 in range(s0, s0 + sc, SAMPLE_DRAW_BLOCK):
                        nb = min(SAMPLE_DRAW_BLOCK, s0 + sc - b0)
                        for key, buf in zip(keys, bufs):
                            o = lay[key]
                            m0, m1 = int(o[gp0[k]]), int(o[gp0[k + 1]])
                            if nb == sc:          # the chunk is this block: the stream lands in the call's layout as it is
                                buf[sc * m0:sc * m1].normal_(generator=gens[first + k])
                                continue
                            blk = h.empty(nb * (m1 - m0)).normal_(generator=gens[first + k])
                            for r in range(gp0[k], gp0[k + 1]):
                                a0, a1 = int(o[r]), int(o[r + 1])
                                if a1 > a0:
                                    buf[sc * a0:sc * a1].view(sc, a1 - a0)[b0 - s0:b0 - s0 + nb] = \
                                        blk[nb * (a0 - m0):nb * (a1 - m0)].view(nb, a1 - a0)
            nlat, nsrc = sc * int(lay["latents"][-1]), sc * int(lay["sources"][-1])
            res = h.empty(nsrc + nlat)                  # sources | latents: one copy back (the sources alone without latents)
            h.check(lib.gp_pdgpb_sample(plan, params.data_ptr(), xd.data_ptr(), off, order.ctypes.data, sc,
                                        bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), res[nsrc:].data_ptr(),
                                        res.data_ptr(), ws.data_ptr(), ws.numel()))
            ncopy = sc * nback
            pin[:ncopy].copy_(res[:ncopy], non_blocking=True)
            h.sync()
            got = pin.numpy()[:ncopy]
            for k in range(nm):
                n = xs[k].size
                if n == 0:
                    continue
                src, g, f = out[first + k]
                src[:, s0:s0 + sc] = got[sc * lay["sources"][k]:sc * lay["sources"][k + 1]].reshape(P[k], sc, n)
                if want_lat:
                    l = got[nsrc + sc * lay["latents"][k]:nsrc + sc * lay["latents"][k + 1]].reshape(2 * P[k], sc, n)
                    g[:, s0:s0 + sc], f[:, s0:s0 + sc] = l[:P[k]], l[P[k]:]
            del bufs
        del ppin, xpin, pin, epin
        bad = (C.c_int32 * nm)()
        h.check(lib.gp_pdgpb_not_pd(plan, bad, 1))
    for k in range(nm):
        if bad[k]:
            raise _lib.NotPositiveDefiniteError(_lib.GP_ERR_NOT_PD, "sample_sources_many: model %d: Cholesky failed: %s"
                                                % (first + k, _describe_not_pd(bad[k])))


def sample_sources_many(models, xnews, num_samples=1, seed=0, eps=None, return_latents=False):
    """Pdgp.sample_sources of every model at its own inputs, all models together: joint posterior draws under q of every
    source nlin(g_i) f_i across all frames of a model's inputs.

        draws = sample_sources_many(models, xnews, num_samples=S)
        draws[k]   # src (P_k, S, n_k); with return_latents=True (src, g, f), each (P_k, S, n_k)

    xnews: one array per model or one array for every model; a model without frames returns (P_k, S, 0) arrays, and a call
    without any frame does no device work.  eps: None, or one (eps_x, eps_z, eps_u) triple per model with exactly the shapes
    of models[k].sample_eps_shapes(n_k, S), in the caller's own point order: with the same eps the draws are those of
    models[k].sample_sources(xnews[k], S, eps=eps[k]) to rounding, and eps = 0 gives predict_many's means and mean_source.
    seed: one int (or None) per model, or one int s standing for [s + k].  Model k's normals come from its own torch generator
    on the handle's device, drawn SAMPLE_DRAW_BLOCK draws at a time: they depend on seeds[k], the model's shapes and
    num_samples only — not on the other models, their order, or how the call is split.  A seeded batch draw is its OWN
    stream, not that of Pdgp.sample_sources(seed=...), whose chunks are sized per model: only caller-supplied eps
    reproduces the single-model call.
    Scope: check_sampleable (raises before any device work).  Reads each model's current Params and changes nothing (no
    Param, flag, generator, Adam state, single-model plan or prediction memo).  A failed Kuu factorisation raises
    NotPositiveDefiniteError naming the model.  A call whose normals and draws pass MAX_SAMPLE_BYTES on the device is split
    into groups of models, then into chunks of draws (sample_split); the draws are bit-identical however it is split, and
    draw s of model k whatever num_samples and whatever else is in the list."""
    models, xs = check_sampleable(models, xnews)
    if isinstance(num_samples, bool) or int(num_samples) != num_samples or int(num_samples) < 1:
        raise ValueError("sample_sources_many: num_samples must be a positive integer, not %r" % (num_samples,))
    S, nm = int(num_samples), len(models)
    if isinstance(seed, (list, tuple, np.ndarray)):
        if len(seed) != nm:
            raise ValueError("sample_sources_many: %d seeds for %d models" % (len(seed), nm))
        seeds = list(seed)
    else:
        seeds = [None if seed is None else int(seed) + k for k in range(nm)]
    shapes = [m.sample_eps_shapes(x.size, S) for m, x in zip(models, xs)]
    eps = _sample_eps(eps, shapes)
    out = [[np.zeros((m.num_sources, S, x.size))] +
           [np.zeros((m.num_sources, S, x.size)) if return_latents else None for _ in range(2)] for m, x in zip(models, xs)]
    if any(x.size for x in xs):
        h = _lib.default_handle()
        gens = None if eps is not None else [_sample_generator(h, sd) for sd in seeds]
        per_draw = sample_bytes_per_draw(models, xs)
        for k0, k1, chunks in sample_split(per_draw, [2 * m.num_sources for m in models], S, MAX_SAMPLE_BYTES):
            if any(x.size for x in xs[k0:k1]):
                _sample_group(h, models[k0:k1], xs[k0:k1], k0, chunks, None if eps is None else eps[k0:k1], gens, out)
    return [tuple(o) if return_latents else o[0] for o in out]
