"""Checkpoints: save and load trained models, resume training bit for bit.

    gpitch_amd.save(path, obj, data=True)          # obj: a Pdgp, an SGPRSS, a kernel, or a list / tuple / dict of these
    obj = gpitch_amd.load(path, data=None, handle=None, float_type=None)
    state = m.state_dict(data=True)                # {"meta": JSON-able dict, "arrays": {key: numpy array}}
    m.load_state_dict(state)                       # into an EXISTING object of the same structure

Host code only: neither save nor load touches the device, a loaded model is freshly constructed and uncompiled.

The file is one `.npz` read with np.load(path, allow_pickle=False): `__meta__` is UTF-8 JSON as a uint8 array (format
version, the structure tree, settings, `.fixed` flags, transform arguments, generator scalars), every other entry is an
array named by its Param path behind the container's path — float64 Param values and Adam moments, the uint32[624]
Mersenne key of each minibatch generator.  No number that training depends on passes through decimal text.

The exactness contract.
1. Train, save, load, train.  Pdgp.optimize with an AdamOptimizer or a NatGradAdam token (one length, or gamma_com= /
   halvings=), optimize_many / PdgpBatch.optimize with the same tokens, with or without tied=: call it with maxiter=a,
   save, load (in this process or another), call it with maxiter=b.  The loaded model ends bit-identical to a twin that
   made the two calls back to back in one process: every Param, _adam_state(), _adam_t, the generators' next draws, and
   the returned fun / jac / x (and natgrad counts).  Both paths run the same _pack() on the same float64 bits with the
   same moments, step count and index stream.  Ties are not stored: tie_groups(models, ...) on the loaded models gives
   the same groups.
2. Chunked training is not uninterrupted training.  optimize() evaluates its returned fun / jac on a fresh minibatch, so
   a + b iterations in two calls draw one minibatch more than a + b iterations in one call.  The contract is stated
   against two calls, with a file between them or not.
3. Predict and sample after load.  The outputs of a loaded model are bit-identical to those of the live model it was
   saved from: Pdgp.predict_act_n_com / predict_sources / predict_y / expected_log_density / sample_sources(seed=...),
   SGPRSS.compute_log_likelihood / predict_f / predict_s / predict_s_sparse / sample_s_sparse(seed=...).
4. SGPRSS.optimize (L-BFGS-B) keeps no state between calls: a checkpoint between two calls is exact in the sense of 1,
   nothing more is promised.

Not held: `shard` (a loaded model is unsharded; build a sharded model by hand and load_state_dict into it), the handle
and the compiled plan, ties, a mean function that is an arbitrary callable (TypeError), and the state of a minibatch
generator without get_state / set_state of numpy's RandomState: that one is saved as "no generator state", the loaded
model has the constructor's RandomState(0), and resume is NOT exact in that case."""
import json
import os

import numpy as np

from . import mean_functions, methods
from .flatvec import latent_gps
from .kernels import RBF, Add, Kern, Matern12, Matern32, Matern32sm, Matern52, MercerCosMix, Prod
from .matern12_spectral_mixture import Matern12sm, MercerMatern12sm
from .param import Identity, Log1pe, Logistic, Param, ParamList, Parameterized
from .pdgp import Pdgp
from .sgpr_ss import SGPRSS

FORMAT_VERSION = 1
META_KEY = "__meta__"

_KERNELS = {c.__name__: c for c in (Matern12, Matern32, Matern52, RBF, Matern12sm, MercerMatern12sm, Matern32sm,
                                    MercerCosMix, Prod, Add)}
_NLINS = {f.__name__: f for f in (methods.logistic_tf, methods.softplus_tf, methods.gaussfun_tf)}
_MEANS = {c.__name__: c for c in (mean_functions.Zero, mean_functions.Constant, mean_functions.Linear)}


# ---- Params and transforms --------------------------------------------------------------------------------------------------
def _transform_meta(tr):
    if type(tr) is Identity:
        return {"class": "Identity"}
    if type(tr) is Log1pe:
        return {"class": "Log1pe", "lower": float(tr._lower)}
    if type(tr) is Logistic:
        return {"class": "Logistic", "a": float(tr.a), "b": float(tr.b)}
    raise TypeError("checkpoint: a Param has the transform %r; Identity, Log1pe and Logistic can be saved" % (tr,))


def _make_transform(meta):
    if meta["class"] == "Identity":
        return Identity()
    if meta["class"] == "Log1pe":
        return Log1pe(meta["lower"])
    if meta["class"] == "Logistic":
        return Logistic(meta["a"], meta["b"])
    raise ValueError("checkpoint: unknown transform %r" % (meta["class"],))


def _walk(obj, prefix, out, seen):
    """(path, Param) of every Param under `obj`, attributes by name (ParamLists and kern_list in list order).  Attributes
    whose name starts with an underscore are derived state (Matern32sm._unit, Prod._variance, the _kern_params views)
    and are rebuilt, not saved; a Param reached twice (Add.var_vector) keeps its first path."""
    for name in sorted(obj.__dict__):
        if name.startswith("_"):
            continue
        v = obj.__dict__[name]
        path = prefix + name
        if isinstance(v, Param):
            if id(v) not in seen:
                seen.add(id(v))
                out.append((path, v))
        elif isinstance(v, (ParamList, list, tuple)):
            for j, it in enumerate(v):
                if isinstance(it, Param):
                    if id(it) not in seen:
                        seen.add(id(it))
                        out.append(("%s[%d]" % (path, j), it))
                elif isinstance(it, Parameterized):
                    _walk(it, "%s[%d]." % (path, j), out, seen)
        elif isinstance(v, Parameterized):
            _walk(v, path + ".", out, seen)
    return out


def _kern_params(kern, prefix=""):
    return _walk(kern, prefix, [], set())


def _kern_meta(kern):
    name = type(kern).__name__
    if _KERNELS.get(name) is not type(kern):
        raise TypeError("checkpoint: kernel class %s cannot be saved (known: %s)" % (name, ", ".join(sorted(_KERNELS))))
    meta = {"class": name}
    if isinstance(kern, (Add, Prod)):
        meta["kern_list"] = [_kern_meta(k) for k in kern.kern_list]
    elif isinstance(kern, MercerCosMix):
        meta["num_features"] = int(kern.num_features)
    elif isinstance(kern, (Matern12sm, MercerMatern12sm, Matern32sm)):
        meta["num_partials"] = int(kern.num_partials)
    return meta


def _make_kern(meta):
    """a kernel of the saved structure with constructor values; its Params are installed afterwards"""
    name = meta["class"]
    if name not in _KERNELS:
        raise ValueError("checkpoint: unknown kernel class %r" % (name,))
    cls = _KERNELS[name]
    if cls is Add:
        return Add([_make_kern(k) for k in meta["kern_list"]])
    if cls is Prod:
        return Prod(*[_make_kern(k) for k in meta["kern_list"]])
    if cls is MercerCosMix:
        n = int(meta["num_features"])
        return MercerCosMix(1, energy=np.ones(n), frequency=np.ones(n))
    if cls is Matern32sm:
        return Matern32sm(1, int(meta["num_partials"]))
    if cls in (Matern12sm, MercerMatern12sm):
        n = int(meta["num_partials"])
        return cls(1, energy=np.ones(n), frequency=np.ones(n))
    return cls(1)


def _kern_signature(meta, path, out):
    """(path, what, value) of the kernel classes; partial and inducing counts show as Param paths (_check_params)"""
    out.append((path, "kernel class", meta["class"]))
    for j, k in enumerate(meta.get("kern_list", ())):
        _kern_signature(k, "%s%skern_list[%d]" % (path, "." if path else "", j), out)
    if "kern_list" in meta:
        out.append((path, "number of kernels", len(meta["kern_list"])))


def _params_meta(named):
    return [{"path": path, "shape": [int(s) for s in p.shape], "fixed": bool(p.fixed),
             "transform": _transform_meta(p.transform)} for path, p in named]


def _params_arrays(named):
    return {path: np.array(p._array, dtype=np.float64) for path, p in named}


def _check_params(kind, named, state):
    """every structural comparison of load_state_dict before anything is written: the target's Params against the saved
    ones, path by path in walk order; ValueError names the first path that differs"""
    saved, arrays = state["meta"]["params"], state["arrays"]
    for i in range(max(len(named), len(saved))):
        if i >= len(saved):
            raise ValueError("%s.load_state_dict: %s is not in the state" % (kind, named[i][0]))
        path = saved[i]["path"]
        if i >= len(named):
            raise ValueError("%s.load_state_dict: the state holds %s, the target does not" % (kind, path))
        if named[i][0] != path:
            raise ValueError("%s.load_state_dict: the target has %s where the state has %s" % (kind, named[i][0], path))
        shape = tuple(saved[i]["shape"])
        if tuple(named[i][1].shape) != shape:
            raise ValueError("%s.load_state_dict: %s has shape %r in the target and %r in the state"
                             % (kind, path, tuple(named[i][1].shape), shape))
        a = arrays.get(path)
        if a is None or a.dtype != np.float64 or tuple(a.shape) != shape:
            raise ValueError("%s.load_state_dict: the state's array %s is missing or is not float64 of shape %r"
                             % (kind, path, shape))
        _make_transform(saved[i]["transform"])


def _check_signature(kind, mine, theirs):
    for i in range(max(len(mine), len(theirs))):
        a = mine[i] if i < len(mine) else None
        b = theirs[i] if i < len(theirs) else None
        if a != b:
            path, what = (a or b)[0], (a or b)[1]
            raise ValueError("%s.load_state_dict: %s: %s is %r in the target and %r in the state"
                             % (kind, path or "the kernel", what, a and a[2], b and b[2]))


def _install_params(named, state):
    saved, arrays = state["meta"]["params"], state["arrays"]
    for (path, p), s in zip(named, saved):
        p.value = arrays[path]
        p.fixed = bool(s["fixed"])
        if _transform_meta(p.transform) != s["transform"]:
            p.transform = _make_transform(s["transform"])


def _state_parts(state, kind):
    if not isinstance(state, dict) or "meta" not in state or "arrays" not in state:
        raise ValueError("%s.load_state_dict: not a state_dict (a dict with 'meta' and 'arrays')" % kind)
    if state["meta"].get("class") != kind:
        raise ValueError("%s.load_state_dict: the state is that of a %s" % (kind, state["meta"].get("class")))
    return state["meta"], state["arrays"]


# ---- kernels ------------------------------------------------------------------------------------------------------------------
def kern_state_dict(self, data=True):
    """{"meta", "arrays"} of a kernel: its class tree (Add / Prod kern_list, partial counts) and every Param — value,
    shape, `.fixed`, transform and its arguments.  Matern32sm._unit and Prod._variance are derived and not saved.  `data`
    is accepted for symmetry with the models."""
    named = _kern_params(self)
    return {"meta": {"class": "Kern", "kern": _kern_meta(self), "params": _params_meta(named)},
            "arrays": _params_arrays(named)}


def kern_load_state_dict(self, state):
    """install a kernel's state into this kernel of the same structure (ValueError naming the first path that differs;
    nothing is changed then)"""
    meta, _ = _state_parts(state, "Kern")
    mine, theirs = [], []
    _kern_signature(_kern_meta(self), "", mine)
    _kern_signature(meta["kern"], "", theirs)
    _check_signature("Kern", mine, theirs)
    named = _kern_params(self)
    _check_params("Kern", named, state)
    _install_params(named, state)
    if isinstance(self, Prod):
        self._sync_variance()


# ---- minibatch generators ------------------------------------------------------------------------------------------------------
def _rng_state(holder, name, arrays):
    """the generator's state into `arrays`, its scalars returned for the meta; None: no generator state (a generator
    without RandomState's get_state: resume is not exact then)"""
    rng = holder.rng
    if not (hasattr(rng, "get_state") and hasattr(rng, "set_state")):
        return None
    st = rng.get_state()
    if not (isinstance(st, tuple) and len(st) == 5 and st[0] == "MT19937"):
        return None
    arrays[name + ".rng.key"] = np.array(st[1], dtype=np.uint32)
    arrays[name + ".rng.cached_gaussian"] = np.array([st[4]], dtype=np.float64)
    return {"kind": "MT19937", "pos": int(st[2]), "has_gauss": int(st[3])}


def _rng_tuple(meta, name, arrays, kind):
    if meta is None:
        return None
    key, g = arrays.get(name + ".rng.key"), arrays.get(name + ".rng.cached_gaussian")
    if meta.get("kind") != "MT19937" or key is None or key.dtype != np.uint32 or key.shape != (624,) or g is None:
        raise ValueError("%s.load_state_dict: the generator state of %s is not a Mersenne key of 624 uint32" % (kind, name))
    return ("MT19937", key.copy(), int(meta["pos"]), int(meta["has_gauss"]), float(g[0]))


# ---- Pdgp ---------------------------------------------------------------------------------------------------------------------
def _pdgp_params(m):
    named = [("likelihood.variance", m.likelihood.variance)]
    for name in ("kern_act", "kern_com"):
        for i, k in enumerate(getattr(m, name)):
            named += _kern_params(k, "%s[%d]." % (name, i))
    for name in ("za", "zc", "q_mu_act", "q_mu_com", "q_sqrt_act", "q_sqrt_com"):
        named += [("%s[%d]" % (name, i), p) for i, p in enumerate(getattr(m, name))]
    return named


def _pdgp_full_order(m):
    """Pdgp._param_order() of the unsharded model: the order the saved Adam moments are laid out in"""
    out = [m.likelihood.variance]
    for kern, z, q_mu, q_sqrt in latent_gps(m):
        out += list(kern.theta_params()) + [z, q_mu, q_sqrt]
    return out


def _pdgp_signature(meta):
    sig = [("", "number of sources", meta["num_sources"])]
    for name in ("kern_act", "kern_com"):
        for i, k in enumerate(meta[name]):
            _kern_signature(k, "%s[%d]" % (name, i), sig)
    return sig


def _pdgp_meta(m):
    nl = getattr(m.nlinfun, "__name__", None)
    if _NLINS.get(nl) is not m.nlinfun:
        raise TypeError("checkpoint: nlinfun %r cannot be saved (logistic_tf, softplus_tf, gaussfun_tf)" % (m.nlinfun,))
    return {"class": "Pdgp", "num_sources": int(m.num_sources), "whiten": bool(m.whiten),
            "minibatch_size": int(m.minibatch_size), "num_data": int(m.num_data), "nlinfun": nl,
            "bits": list(m._bits) if isinstance(m._bits, tuple) else int(m._bits),
            "max_predict_batch": None if m._max_predict_batch is None else int(m._max_predict_batch),
            "kern_act": [_kern_meta(k) for k in m.kern_act], "kern_com": [_kern_meta(k) for k in m.kern_com]}


def pdgp_state_dict(self, data=True):
    """Where training stands, as {"meta": JSON-able dict, "arrays": {key: array}}: every Param (value, shape, `.fixed`,
    transform), the kernels' class trees, whiten / minibatch_size / num_data / nlinfun / float_type bits /
    max_predict_batch, _adam_t, the Adam moments of _adam_state() (None stays None; "adam_m" / "adam_v" are the moments
    of _param_order() back to back), the states of x.rng and y.rng, and with data=True x and y.  Reads the device only
    for the moments of a compiled model.  A generator without get_state is saved as "no generator state": resume is not
    exact then.  `shard` is not saved; a sharded model that carries Adam moments holds its own rows' only and is refused."""
    named = _pdgp_params(self)
    meta = _pdgp_meta(self)
    arrays = _params_arrays(named)
    meta["params"] = _params_meta(named)
    meta["adam_t"] = int(self._adam_t)
    adam = self._adam_state()
    if adam is not None and self._shard:
        raise NotImplementedError("state_dict of a sharded Pdgp with Adam moments: each rank holds its own rows' only")
    meta["adam"] = adam is not None
    if adam is not None:
        arrays["adam_m"] = np.concatenate([np.asarray(a, dtype=np.float64).reshape(-1) for a, _ in adam])
        arrays["adam_v"] = np.concatenate([np.asarray(b, dtype=np.float64).reshape(-1) for _, b in adam])
    meta["rng"] = {"x": _rng_state(self.x, "x", arrays), "y": _rng_state(self.y, "y", arrays)}
    meta["data"] = bool(data)
    if data:
        arrays["x"] = np.array(self.x._array, dtype=np.float64)
        arrays["y"] = np.array(self.y._array, dtype=np.float64)
    return {"meta": meta, "arrays": arrays}


def pdgp_load_state_dict(self, state):
    """Install a state_dict into this EXISTING Pdgp — one built by hand: sharded, of another float type, on another
    handle.  The whole structure is checked first (source count, kernel classes, partial counts, inducing counts per
    role and source, whiten, nlinfun); a mismatch is a ValueError naming the first Param path that differs and changes
    nothing.  Installed: Param values, `.fixed` flags, transforms, _adam_t, the Adam moments, the generators' states.
    Left as the target has them: x, y, minibatch_size, float_type, shard, handle.  Ends with
    _invalidate_device_state(), so the next call repacks."""
    meta, arrays = _state_parts(state, "Pdgp")
    _check_signature("Pdgp", _pdgp_signature(_pdgp_meta(self)), _pdgp_signature(meta))
    named = _pdgp_params(self)
    _check_params("Pdgp", named, state)
    for key in ("whiten", "nlinfun"):
        if _pdgp_meta(self)[key] != meta[key]:
            raise ValueError("Pdgp.load_state_dict: %s is %r in the target and %r in the state"
                             % (key, _pdgp_meta(self)[key], meta[key]))
    am, av = arrays.get("adam_m"), arrays.get("adam_v")
    if meta["adam"]:
        # (counted from the shapes: a Prod answers theta_params() only once its factors' flags are installed)
        total = 1 + sum(2 + 2 * int(k.num_partials) + 2 * z.size + z.size * z.size for k, z, _, _ in latent_gps(self))
        for nm, a in (("adam_m", am), ("adam_v", av)):
            if a is None or a.dtype != np.float64 or a.shape != (total,):
                raise ValueError("Pdgp.load_state_dict: %s is missing or is not float64 of %d entries" % (nm, total))
    rngs = [(h, _rng_tuple(meta["rng"][n], n, arrays, "Pdgp")) for n, h in (("x", self.x), ("y", self.y))]
    for h, st in rngs:
        if st is not None and not hasattr(h.rng, "set_state"):
            raise ValueError("Pdgp.load_state_dict: the target's minibatch generator has no set_state")
    # ---- nothing was changed up to here ----
    _install_params(named, state)
    for k in list(self.kern_act) + list(self.kern_com):
        if isinstance(k, Prod):
            k._sync_variance()
    self._adam_t = int(meta["adam_t"])
    if meta["adam"]:
        by_id, off = {}, 0
        for p in _pdgp_full_order(self):
            by_id[id(p)] = (am[off:off + p.size].copy(), av[off:off + p.size].copy())
            off += p.size
        self._set_adam_state([by_id[id(p)] for p in self._param_order()])      # (a sharded target: its own rows)
    else:
        self.__dict__.pop("_pending_adam", None)
        if self._plan is not None:
            self._adam_m.zero_()
            self._adam_v.zero_()
    for h, st in rngs:
        if st is not None:
            h.rng.set_state(st)
    self._invalidate_device_state()


def _float_type(bits):
    one = lambda b: np.float32 if int(b) == 32 else np.float64
    return tuple(one(b) for b in bits) if isinstance(bits, (list, tuple)) else one(bits)


def _take_data(meta, arrays, names, data, kind):
    """the two data arrays of a model: from the file, or from load's `data` when the file was saved with data=False"""
    if data is None:
        if not meta["data"]:
            raise ValueError("load: this %s was saved with data=False: pass data=(%s, %s) (for a container, a list or "
                             "dict of such pairs of the same shape)" % (kind, names[0], names[1]))
        return arrays[names[0]], arrays[names[1]]
    if not isinstance(data, (tuple, list)) or len(data) != 2:
        raise ValueError("load: data for a %s is a pair (%s, %s)" % (kind, names[0], names[1]))
    a, b = (np.asarray(d, dtype=np.float64) for d in data)
    for nm, d in zip(names, (a, b)):
        n = d.shape[0] if d.ndim else 1
        if n != int(meta["num_data"]):
            raise ValueError("load: %s has %d frames, the saved %s has num_data = %d" % (nm, n, kind, meta["num_data"]))
    return a, b


def _pdgp_from_state(state, data, handle, float_type):
    meta, arrays = state["meta"], state["arrays"]
    x, y = _take_data(meta, arrays, ("x", "y"), data, "Pdgp")
    shapes = {p["path"]: p["shape"] for p in meta["params"]}
    P = int(meta["num_sources"])
    z = [[np.zeros(shapes["%s[%d]" % (n, i)][0]) for i in range(P)] for n in ("za", "zc")]
    kern = [[_make_kern(k) for k in meta[n]] for n in ("kern_act", "kern_com")]
    m = Pdgp(x, y, z, kern, whiten=meta["whiten"], minibatch_size=meta["minibatch_size"], nlinfun=_NLINS[meta["nlinfun"]],
             handle=handle, max_predict_batch=meta["max_predict_batch"],
             float_type=_float_type(meta["bits"]) if float_type is None else float_type)
    m.load_state_dict(state)
    return m


# ---- SGPRSS -------------------------------------------------------------------------------------------------------------------
def _mean_meta(mf):
    if mf is None:
        return None
    name = type(mf).__name__
    if _MEANS.get(name) is not type(mf):
        raise TypeError("checkpoint: the mean function %r is an arbitrary callable and cannot be saved "
                        "(gpitch_amd.mean_functions Zero, Constant and Linear can)" % (mf,))
    return {"class": name}


def _sgpr_params(m):
    named = [("likelihood.variance", m.likelihood.variance)] + _kern_params(m.kern, "kern.")
    mf = m.mean_function
    if mf is not None:
        named += [("mean_function." + n, p) for n, p in sorted(vars(mf).items()) if isinstance(p, Param)]
    return named


def _sgpr_meta(m):
    return {"class": "SGPRSS", "reg": bool(m.reg), "bits": int(m._bits), "D": int(m.num_latent),
            "num_data": int(m.X.shape[0]), "num_inducing": int(m.Z.shape[0]), "kern": _kern_meta(m.kern),
            "mean_function": _mean_meta(m.mean_function)}


def _sgpr_signature(meta):
    sig = []
    _kern_signature(meta["kern"], "kern", sig)
    sig.append(("Z", "number of inducing points", meta["num_inducing"]))
    sig.append(("Y", "D", meta["D"]))
    sig.append(("mean_function", "class", meta["mean_function"] and meta["mean_function"]["class"]))
    return sig


def sgpr_state_dict(self, data=True):
    """{"meta", "arrays"} of an SGPRSS: Z, reg, float_type bits, the noise variance, the Add kernel and the mean function
    (Zero / Constant / Linear with its Params, or none; any other callable: TypeError naming it) — every Param with
    value, shape, `.fixed` and transform — and with data=True X and Y (N x D)."""
    named = _sgpr_params(self)
    meta = _sgpr_meta(self)
    meta["params"] = _params_meta(named)
    meta["data"] = bool(data)
    arrays = _params_arrays(named)
    arrays["Z"] = np.array(self.Z._array, dtype=np.float64)
    if data:
        arrays["X"] = np.array(self.X._array, dtype=np.float64)
        arrays["Y"] = np.array(self.Y._array, dtype=np.float64)
    return {"meta": meta, "arrays": arrays}


def sgpr_load_state_dict(self, state):
    """Install a state_dict into this EXISTING SGPRSS of the same structure (kernel classes, partial counts, inducing
    count, D, mean function class; a mismatch is a ValueError naming the first path that differs and changes nothing):
    Param values, `.fixed` flags, transforms and Z.  X, Y, reg, float_type, shard and handle stay the target's."""
    meta, arrays = _state_parts(state, "SGPRSS")
    _check_signature("SGPRSS", _sgpr_signature(_sgpr_meta(self)), _sgpr_signature(meta))
    named = _sgpr_params(self)
    _check_params("SGPRSS", named, state)
    Z = arrays.get("Z")
    if Z is None or Z.dtype != np.float64 or Z.shape != tuple(self.Z.shape):
        raise ValueError("SGPRSS.load_state_dict: Z is missing or is not float64 of shape %r" % (tuple(self.Z.shape),))
    _install_params(named, state)
    self.Z = Z
    object.__setattr__(self, "_obj_state", None)


def _sgpr_from_state(state, data, handle, float_type):
    meta, arrays = state["meta"], state["arrays"]
    X, Y = _take_data(meta, arrays, ("X", "Y"), data, "SGPRSS")
    Y = np.asarray(Y, dtype=np.float64)
    if Y.ndim != 2 or Y.shape[1] != int(meta["D"]):
        raise ValueError("load: Y has shape %r, the saved SGPRSS has D = %d columns" % (Y.shape, meta["D"]))
    mf = meta["mean_function"]
    if mf is not None and mf["class"] not in _MEANS:
        raise ValueError("checkpoint: unknown mean function class %r" % (mf["class"],))
    m = SGPRSS(X, Y, _make_kern(meta["kern"]), np.zeros(int(meta["num_inducing"])),
               mean_function=None if mf is None else _MEANS[mf["class"]](), reg=meta["reg"], handle=handle,
               float_type=_float_type(meta["bits"]) if float_type is None else float_type)
    m.load_state_dict(state)
    return m


def _kern_from_state(state, data, handle, float_type):
    k = _make_kern(state["meta"]["kern"])
    k.load_state_dict(state)
    return k


_BUILDERS = {"Pdgp": _pdgp_from_state, "SGPRSS": _sgpr_from_state, "Kern": _kern_from_state}

Kern.state_dict, Kern.load_state_dict = kern_state_dict, kern_load_state_dict
Pdgp.state_dict, Pdgp.load_state_dict = pdgp_state_dict, pdgp_load_state_dict
SGPRSS.state_dict, SGPRSS.load_state_dict = sgpr_state_dict, sgpr_load_state_dict


# ---- containers and the file ----------------------------------------------------------------------------------------------------
def _join(prefix, path):
    return path if not prefix else (prefix + path if path.startswith("[") else prefix + "." + path)


def _gather(obj, prefix, data, arrays):
    """the structure tree of `obj` for the meta; every leaf's arrays go into `arrays` behind the leaf's container path"""
    if isinstance(obj, (Pdgp, SGPRSS, Kern)):
        st = obj.state_dict(data=data)
        for key, a in st["arrays"].items():
            full = _join(prefix, key)
            if full in arrays or full == META_KEY:
                raise ValueError("save: two entries would be named %r" % (full,))
            arrays[full] = a
        return {"node": "object", "prefix": prefix, "meta": st["meta"]}
    if isinstance(obj, (list, tuple)):
        return {"node": "tuple" if isinstance(obj, tuple) else "list",
                "items": [_gather(it, "%s[%d]" % (prefix, i), data, arrays) for i, it in enumerate(obj)]}
    if isinstance(obj, dict):
        for k in obj:
            if not isinstance(k, str) or not k or any(c in k for c in ".[]/\\"):
                raise TypeError("save: dict keys are non-empty strings without . [ ] / \\, not %r" % (k,))
        return {"node": "dict", "keys": list(obj), "items": [_gather(obj[k], _join(prefix, k), data, arrays) for k in obj]}
    raise TypeError("save: %r is not a Pdgp, an SGPRSS, a kernel, or a list / tuple / dict of these" % (type(obj).__name__,))


def save(path, obj, data=True):
    """Write `obj` — a Pdgp, an SGPRSS, a kernel, or a list / tuple / dict of these, nested — to the `.npz` file `path`
    (written as given, no extension is added).  data=False leaves x, y (X, Y of an SGPRSS) out; load(path, data=...)
    then takes them.  The file is written to path + ".tmp" and moved over `path`, so a save that fails leaves the file
    that was there as it was.  No device work beyond reading the Adam moments of a compiled Pdgp.  See the module's
    docstring for the format and the exactness contract."""
    path = os.fspath(path)
    arrays = {}
    tree = _gather(obj, "", data, arrays)
    meta = {"format_version": FORMAT_VERSION, "tree": tree}
    blob = np.frombuffer(json.dumps(meta, allow_nan=False).encode("utf-8"), dtype=np.uint8)
    tmp = path + ".tmp"
    try:
        with open(tmp, "wb") as f:
            np.savez(f, **{META_KEY: blob}, **arrays)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _build(node, arrays, data, handle, float_type, where):
    kind = node["node"]
    if kind == "object":
        prefix = node["prefix"]
        own = {}
        for key, a in arrays.items():
            if not prefix:
                own[key] = a
            elif key.startswith(prefix) and key[len(prefix):len(prefix) + 1] in (".", "["):
                own[key[len(prefix) + 1:] if key[len(prefix)] == "." else key[len(prefix):]] = a
        cls = node["meta"].get("class")
        if cls not in _BUILDERS:
            raise ValueError("load: unknown object class %r" % (cls,))
        return _BUILDERS[cls]({"meta": node["meta"], "arrays": own}, data, handle, float_type)
    if kind in ("list", "tuple"):
        if data is not None and (not isinstance(data, (list, tuple)) or len(data) != len(node["items"])):
            raise ValueError("load: data for %s is a list of %d entries" % (where or "the file's list", len(node["items"])))
        out = [_build(it, arrays, None if data is None else data[i], handle, float_type, "%s[%d]" % (where, i))
               for i, it in enumerate(node["items"])]
        return tuple(out) if kind == "tuple" else out
    if kind == "dict":
        if data is not None and (not isinstance(data, dict) or any(k not in data for k in node["keys"])):
            raise ValueError("load: data for %s is a dict with the keys %r" % (where or "the file's dict", node["keys"]))
        return {k: _build(it, arrays, None if data is None else data[k], handle, float_type, _join(where, k))
                for k, it in zip(node["keys"], node["items"])}
    raise ValueError("load: unknown node %r in the structure tree" % (kind,))


def load(path, data=None, handle=None, float_type=None):
    """Read what save() wrote and return the same structure: models freshly constructed and uncompiled (_plan is None,
    no device work), kernels, and the lists / tuples / dicts around them.  `handle` and `float_type` are runtime choices
    and override what was saved; `shard` is not saved, a loaded model is unsharded.  data: for a file saved with
    data=False, (x, y) for a single model — (X, Y) for an SGPRSS — or a list / dict of such pairs of the container's
    shape (None for a kernel); missing data and data whose frame count differs from the saved num_data are ValueErrors.
    A file of another FORMAT_VERSION is a ValueError naming both versions; a truncated or foreign file raises, no partial
    model is returned."""
    with np.load(os.fspath(path), allow_pickle=False) as f:
        if META_KEY not in f.files:
            raise ValueError("load: %s is not a gpitch_amd checkpoint (no %s entry)" % (path, META_KEY))
        arrays = {k: f[k] for k in f.files}
    blob = arrays.pop(META_KEY)
    if blob.dtype != np.uint8 or blob.ndim != 1:
        raise ValueError("load: %s of %s is not a uint8 vector" % (META_KEY, path))
    meta = json.loads(blob.tobytes().decode("utf-8"))
    version = meta.get("format_version") if isinstance(meta, dict) else None
    if version != FORMAT_VERSION:
        raise ValueError("load: %s has format version %r, this library reads version %d" % (path, version, FORMAT_VERSION))
    return _build(meta["tree"], arrays, data, handle, float_type, "")
