"""gpitch_amd.checkpoint on the host: state_dict / load_state_dict / save / load of kernels, Pdgp, SGPRSS and containers,
and the file's hygiene.  No device: the models are never compiled (tests/test_gpu_checkpoint.py proves the exactness
contract on the device)."""
import json
import os

import numpy as np
import pytest

import gpitch_amd
from gpitch_amd import checkpoint, mean_functions, param
from gpitch_amd.kernels import RBF, Add, Matern12, Matern32, Matern32sm, Matern52, MercerCosMix, Prod
from gpitch_amd.matern12_spectral_mixture import Matern12sm, MercerMatern12sm
from gpitch_amd.param import Identity, Log1pe, Logistic
from gpitch_amd.pdgp import Pdgp
from gpitch_amd.sgpr_ss import SGPRSS


def _transform_key(t):
    if isinstance(t, Log1pe):
        return ("Log1pe", t._lower)
    if isinstance(t, Logistic):
        return ("Logistic", t.a, t.b)
    assert type(t) is Identity
    return ("Identity",)


def _randomise(obj, rng):
    """seeded random values inside every transform's range, and a mix of `.fixed` flags"""
    for p in param.sorted_params(obj):
        t = p.transform
        u = rng.uniform(0.05, 0.95, size=p.shape)
        p.value = t.a + (t.b - t.a) * u if isinstance(t, Logistic) else (u * 3.0 if isinstance(t, Log1pe) else u - 0.5)
        p.fixed = bool(rng.randint(2))


def _sm(cls, m, rng):
    return cls(1, energy=rng.uniform(0.1, 1.0, m), frequency=rng.uniform(100., 900., m))


def _prod(features_as_params):
    k = Matern52(1) * MercerCosMix(1, energy=np.ones(3), frequency=np.array([110., 220., 330.]),
                                   features_as_params=features_as_params)
    return k


def _kernel_cases():
    rng = np.random.RandomState(11)
    cases = {"Matern12": Matern12(1), "Matern32": Matern32(1), "Matern52": Matern52(1), "RBF": RBF(1),
             "Matern12sm": _sm(Matern12sm, 3, rng), "MercerMatern12sm-1": _sm(MercerMatern12sm, 1, rng),
             "MercerMatern12sm-4": _sm(MercerMatern12sm, 4, rng), "Matern32sm": Matern32sm(1, 3),
             "Prod": _prod(False), "Prod-features": _prod(True),
             "Add": Add([Matern32(1), _sm(MercerMatern12sm, 2, rng), Matern32sm(1, 2)])}
    for name, k in cases.items():
        _randomise(k, rng)
        _rebuild_derived(k)
        if name == "Prod":                  # without features_as_params the features stay fixed
            k.kern_list[1].energy.fixed = True
            k.kern_list[1].frequency.fixed = True
    return cases


def _rebuild_derived(k):
    """_randomise went through the derived Params too: Matern32sm's unit variance slot is 1 and fixed, the engine carries
    the two variances of a Prod as one fixed product"""
    for c in getattr(k, "kern_list", []):
        _rebuild_derived(c)
    if isinstance(k, Matern32sm):
        k._unit.value = 1.0
        k._unit.fixed = True
    if isinstance(k, Prod):
        k.kern_list[0].variance.fixed = True
        k.kern_list[1].variance.fixed = True
        k._sync_variance()


_KERNELS = _kernel_cases()


def _classes(k):
    return (type(k).__name__, int(getattr(k, "num_partials", 0)), [_classes(c) for c in getattr(k, "kern_list", [])])


def _same_params(a, b):
    pa, pb = param.sorted_params(a), param.sorted_params(b)
    assert len(pa) == len(pb)
    for p, q in zip(pa, pb):
        assert p.shape == q.shape
        assert p._array.dtype == q._array.dtype == np.float64
        assert np.array_equal(p._array.view(np.uint64), q._array.view(np.uint64))
        assert p.fixed == q.fixed
        assert _transform_key(p.transform) == _transform_key(q.transform)


def _same_kernel(a, b):
    assert _classes(a) == _classes(b)
    _same_params(a, b)
    if not isinstance(a, Add):
        assert np.array_equal(a.theta().view(np.uint64), b.theta().view(np.uint64))
        assert [p.fixed for p in a.theta_params()] == [p.fixed for p in b.theta_params()]
    else:
        for x, y in zip(a.kern_list, b.kern_list):
            assert np.array_equal(x.theta().view(np.uint64), y.theta().view(np.uint64))


@pytest.mark.parametrize("name", sorted(_KERNELS))
def test_kernel_round_trip(tmp_path, name):
    k = _KERNELS[name]
    path = str(tmp_path / "k.npz")
    gpitch_amd.save(path, k)
    back = gpitch_amd.load(path)
    assert back is not k
    _same_kernel(k, back)
    # state_dict -> load_state_dict into a kernel built by hand
    twin = checkpoint._make_kern(k.state_dict()["meta"]["kern"])
    twin.load_state_dict(k.state_dict())
    _same_kernel(k, twin)


def test_features_as_params_shows_in_the_flags(tmp_path):
    for name, want in (("Prod", True), ("Prod-features", False)):
        path = str(tmp_path / (name + ".npz"))
        k = _KERNELS[name]
        flags = [p.fixed for p in list(k.kern_list[1].energy) + list(k.kern_list[1].frequency)]
        gpitch_amd.save(path, k)
        back = gpitch_amd.load(path)
        assert [p.fixed for p in list(back.kern_list[1].energy) + list(back.kern_list[1].frequency)] == flags
        if want:
            assert all(flags)
        # Prod._variance is rebuilt from the factors, not trusted
        assert back._sync_variance().value[0] == k.kern_list[0].variance.value[0] * k.kern_list[1].variance.value[0]


# ---- Pdgp -------------------------------------------------------------------------------------------------------------------
def _pdgp(minibatch, seed=3, N=64):
    rng = np.random.RandomState(seed)
    x = np.linspace(0., 1., N).reshape(-1, 1)
    y = rng.randn(N, 1)
    Ma, Mc = (5, 7), (6, 4)
    z = [[np.sort(rng.uniform(0, 1, M)) for M in Ma], [np.sort(rng.uniform(0, 1, M)) for M in Mc]]
    kern = [[Matern32(1), Matern32(1)], [_sm(MercerMatern12sm, 3, rng), _sm(MercerMatern12sm, 2, rng)]]
    m = Pdgp(x, y, z, kern, whiten=False, minibatch_size=minibatch, nlinfun=gpitch_amd.softplus_tf,
             float_type=(np.float64, np.float32), max_predict_batch=48)
    _randomise(m, rng)
    m._set_adam_state([(rng.randn(p.size), rng.rand(p.size)) for p in m._param_order()])     # flat, as the device's are
    m._adam_t = 17
    for _ in range(3):
        param.draw_in_lockstep(m.x, m.y, m.x.next_indices)
    return m


def _same_pdgp(a, b, data=True):
    _same_params(a, b)
    for ka, kb in zip(list(a.kern_act) + list(a.kern_com), list(b.kern_act) + list(b.kern_com)):
        _same_kernel(ka, kb)
    assert (a.whiten, a.minibatch_size, a.num_data, a._bits, a._adam_t, a._max_predict_batch, a.num_sources) == \
           (b.whiten, b.minibatch_size, b.num_data, b._bits, b._adam_t, b._max_predict_batch, b.num_sources)
    assert a.nlinfun is b.nlinfun and a.likelihood.nlinfun is b.likelihood.nlinfun
    assert a.num_inducing_a == b.num_inducing_a and a.num_inducing_c == b.num_inducing_c
    sa, sb = a._adam_state(), b._adam_state()
    assert (sa is None) == (sb is None)
    if sa is not None:
        assert len(sa) == len(sb)
        for (m1, v1), (m2, v2) in zip(sa, sb):
            assert np.array_equal(m1, m2) and np.array_equal(v1, v2)
    assert a._plan is None and b._plan is None
    if data:
        assert np.array_equal(a.x._array, b.x._array) and np.array_equal(a.y._array, b.y._array)


def _next_draws(m, n=5):
    return [(m.x.next_indices(), m.y.next_indices()) for _ in range(n)]


@pytest.mark.parametrize("minibatch", (10, 40))       # with replacement; the permutation branch
def test_pdgp_round_trip(tmp_path, minibatch):
    m = _pdgp(minibatch)
    path = str(tmp_path / "m.npz")
    gpitch_amd.save(path, m)
    back = gpitch_amd.load(path)
    _same_pdgp(m, back)
    for (xa, ya), (xb, yb) in zip(_next_draws(m), _next_draws(back)):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb)


def test_pdgp_with_derived_kernel_params_round_trips(tmp_path):
    """Matern32sm and Matern52 * MercerCosMix put derived Params (_unit, _variance) into _param_order(): the moments keep
    their places, and a Prod whose factors are not yet fixed is never asked for its theta"""
    rng = np.random.RandomState(2)
    x, y = np.linspace(0., 1., 32), rng.randn(32)
    prod = _prod(True)
    prod.kern_list[0].variance.fixed = True
    prod.kern_list[1].variance.fixed = True
    prod.kern_list[1].variance.value = 0.2
    z = [[np.linspace(0, 1, 4), np.linspace(0, 1, 5)], [np.linspace(0, 1, 6), np.linspace(0, 1, 3)]]
    m = Pdgp(x, y, z, [[Matern32(1), Matern12(1)], [Matern32sm(1, 2), prod]])
    m._set_adam_state([(rng.randn(p.size), rng.rand(p.size)) for p in m._param_order()])
    m._adam_t = 4
    path = str(tmp_path / "m.npz")
    gpitch_amd.save(path, m)
    back = gpitch_amd.load(path)
    _same_pdgp(m, back)
    assert [p.fixed for p in back._param_order()] == [p.fixed for p in m._param_order()]


def test_pdgp_without_adam_state_and_runtime_overrides(tmp_path):
    m = _pdgp(10)
    m.__dict__.pop("_pending_adam")
    path = str(tmp_path / "m.npz")
    gpitch_amd.save(path, m)
    back = gpitch_amd.load(path, float_type=np.float32)
    assert back._adam_state() is None and back._bits == 32 and back._shard is None
    _same_params(m, back)


def test_generator_without_get_state_is_saved_as_none(tmp_path):
    class Plain(object):
        def randint(self, N, size):
            return np.zeros(size, dtype=np.int64)

    m = _pdgp(10)
    m.x.rng = Plain()
    path = str(tmp_path / "m.npz")
    gpitch_amd.save(path, m)
    back = gpitch_amd.load(path)
    assert np.array_equal(back.x.rng.get_state()[1], np.random.RandomState(0).get_state()[1])     # the constructor's
    assert np.array_equal(back.y.rng.get_state()[1], m.y.rng.get_state()[1])


# ---- SGPRSS -------------------------------------------------------------------------------------------------------------------
def _sgpr(mean_function="linear", seed=5, N=40, M=9):
    rng = np.random.RandomState(seed)
    X = np.linspace(0., 1., N).reshape(-1, 1)
    Y = rng.randn(N, 2)
    Z = np.sort(rng.uniform(0, 1, M)).reshape(-1, 1)
    kern = np.sum([_sm(MercerMatern12sm, 2, rng) for _ in range(3)])
    mf = mean_functions.Linear(A=0.3, b=-1.25) if mean_function == "linear" else mean_function
    m = SGPRSS(X, Y, kern, Z, mean_function=mf, reg=True, float_type=np.float32)
    _randomise(m.kern, rng)
    m.likelihood.variance = 0.37
    if mean_function == "linear":
        m.mean_function.b.fixed = True
    return m


def _same_sgpr(a, b):
    _same_kernel(a.kern, b.kern)
    _same_params(a.likelihood, b.likelihood)
    assert (a.reg, a._bits, a.num_latent) == (b.reg, b._bits, b.num_latent)
    for n in ("X", "Y", "Z"):
        assert np.array_equal(getattr(a, n)._array, getattr(b, n)._array)
    assert type(a.mean_function) is type(b.mean_function)
    if a.mean_function is not None and hasattr(a.mean_function, "params"):
        for p, q in zip(a.mean_function.params(), b.mean_function.params()):
            assert np.array_equal(p._array, q._array) and p.fixed == q.fixed
    # reg=True: var_vector is the kernels' own variances again
    assert [id(p) for p in b.kern.var_vector] == [id(k.variance) for k in b.kern.kern_list]
    assert a._plan is None and b._plan is None


def test_sgprss_round_trip(tmp_path):
    m = _sgpr()
    path = str(tmp_path / "s.npz")
    gpitch_amd.save(path, m)
    back = gpitch_amd.load(path)
    _same_sgpr(m, back)
    assert back.mean_function.A.value[0] == 0.3 and back.mean_function.b.value[0] == -1.25
    for mf in (None, mean_functions.Zero(), mean_functions.Constant(2.5)):
        m2 = _sgpr(mf)
        gpitch_amd.save(path, m2)
        _same_sgpr(m2, gpitch_amd.load(path))


# ---- containers ---------------------------------------------------------------------------------------------------------------
def test_containers(tmp_path):
    path = str(tmp_path / "c.npz")
    models = [_pdgp(10, seed=s) for s in (1, 2, 3)]
    gpitch_amd.save(path, models)
    back = gpitch_amd.load(path)
    assert isinstance(back, list) and len(back) == 3
    for a, b in zip(models, back):
        _same_pdgp(a, b)

    mixed = {"model": models[0], "kernels": [_KERNELS["Matern32"], _KERNELS["Add"]]}
    gpitch_amd.save(path, mixed)
    back = gpitch_amd.load(path)
    assert list(back) == ["model", "kernels"] and isinstance(back["kernels"], list)
    _same_pdgp(mixed["model"], back["model"])
    for a, b in zip(mixed["kernels"], back["kernels"]):
        _same_kernel(a, b)

    nested = {"notes": [{"pdgp": models[1], "window": _sgpr()}, (models[2], _KERNELS["Prod"])], "prior": _KERNELS["RBF"]}
    gpitch_amd.save(path, nested)
    back = gpitch_amd.load(path)
    assert isinstance(back["notes"][1], tuple)
    _same_pdgp(models[1], back["notes"][0]["pdgp"])
    _same_sgpr(nested["notes"][0]["window"], back["notes"][0]["window"])
    _same_pdgp(models[2], back["notes"][1][0])
    _same_kernel(_KERNELS["Prod"], back["notes"][1][1])
    _same_kernel(_KERNELS["RBF"], back["prior"])

    with pytest.raises(TypeError):
        gpitch_amd.save(path, [models[0], 3.0])


# ---- the file -----------------------------------------------------------------------------------------------------------------
def test_file_holds_plain_arrays_and_json(tmp_path):
    path = str(tmp_path / "f.npz")
    gpitch_amd.save(path, {"m": _pdgp(10), "s": _sgpr()})
    with np.load(path, allow_pickle=False) as f:
        assert "__meta__" in f.files
        for k in f.files:
            assert f[k].dtype != object, k
        meta = json.loads(f["__meta__"].tobytes().decode("utf-8"))
        assert f["__meta__"].dtype == np.uint8
        assert f["m.x.rng.key"].dtype == np.uint32 and f["m.x.rng.key"].shape == (624,)
        assert f["m.kern_com[0].frequency[2]"].dtype == np.float64
        assert f["m.adam_m"].dtype == np.float64
        assert f["s.kern.kern_list[1].energy[0]"].dtype == np.float64
    assert meta["format_version"] == checkpoint.FORMAT_VERSION == 1
    assert not os.path.exists(path + ".tmp")


def test_wrong_version_names_both(tmp_path, monkeypatch):
    path = str(tmp_path / "v.npz")
    monkeypatch.setattr(checkpoint, "FORMAT_VERSION", 7)
    gpitch_amd.save(path, _KERNELS["RBF"])
    monkeypatch.setattr(checkpoint, "FORMAT_VERSION", 1)
    with pytest.raises(ValueError) as e:
        gpitch_amd.load(path)
    assert "7" in str(e.value) and "version 1" in str(e.value)


def test_truncated_and_foreign_files_raise(tmp_path):
    path = str(tmp_path / "t.npz")
    gpitch_amd.save(path, _pdgp(10))
    blob = open(path, "rb").read()
    with open(path, "wb") as f:
        f.write(blob[:len(blob) // 2])
    with pytest.raises(Exception):
        gpitch_amd.load(path)
    np.savez(path, a=np.zeros(3))
    with pytest.raises(ValueError):
        gpitch_amd.load(path)


def test_data_false(tmp_path):
    path = str(tmp_path / "d.npz")
    m = _pdgp(10)
    gpitch_amd.save(path, m, data=False)
    with np.load(path, allow_pickle=False) as f:
        assert "x" not in f.files and "y" not in f.files
    with pytest.raises(ValueError) as e:
        gpitch_amd.load(path)
    assert "data=(x, y)" in str(e.value)
    back = gpitch_amd.load(path, data=(m.x.value, m.y.value))
    _same_pdgp(m, back)
    with pytest.raises(ValueError) as e:
        gpitch_amd.load(path, data=(m.x.value[:-1], m.y.value[:-1]))
    assert "63" in str(e.value) and "64" in str(e.value)

    s = _sgpr()
    gpitch_amd.save(path, [m, s], data=False)
    with pytest.raises(ValueError) as e:
        gpitch_amd.load(path)
    back = gpitch_amd.load(path, data=[(m.x.value, m.y.value), (s.X.value, s.Y.value)])
    _same_pdgp(m, back[0])
    _same_sgpr(s, back[1])
    with pytest.raises(ValueError):
        gpitch_amd.load(path, data=[(m.x.value, m.y.value)])


def test_failed_save_leaves_the_old_file(tmp_path):
    path = str(tmp_path / "o.npz")
    gpitch_amd.save(path, _KERNELS["Add"])
    before = open(path, "rb").read()
    bad = _sgpr(lambda X: np.zeros((np.asarray(X).shape[0], 1)))
    with pytest.raises(TypeError) as e:
        gpitch_amd.save(path, [_KERNELS["RBF"], bad])
    assert "lambda" in str(e.value)
    assert open(path, "rb").read() == before
    assert os.listdir(str(tmp_path)) == ["o.npz"]


# ---- load_state_dict ------------------------------------------------------------------------------------------------------------
def _snapshot(m):
    return [(p._array.copy(), p.fixed, _transform_key(p.transform)) for p in param.sorted_params(m)], m._adam_t, \
        m.x.rng.get_state()[1].copy()


def _unchanged(m, snap):
    now = _snapshot(m)
    assert now[1] == snap[1] and np.array_equal(now[2], snap[2])
    for (a, fa, ta), (b, fb, tb) in zip(now[0], snap[0]):
        assert np.array_equal(a, b) and fa == fb and ta == tb


def test_load_state_dict_names_the_path_and_changes_nothing():
    state = _pdgp(10).state_dict()
    rng = np.random.RandomState(0)
    x, y = np.linspace(0, 1, 64), rng.randn(64)

    def target(partials=(3, 2), Ma=(5, 7), kact=Matern32):
        z = [[np.linspace(0, 1, M) for M in Ma], [np.linspace(0, 1, M) for M in (6, 4)]]
        kern = [[kact(1), Matern32(1)], [_sm(MercerMatern12sm, p, rng) for p in partials]]
        return Pdgp(x, y, z, kern, whiten=False, minibatch_size=10, nlinfun=gpitch_amd.softplus_tf)

    for t, where in ((target(partials=(3, 5)), "kern_com[1].energy[2]"), (target(Ma=(5, 8)), "za[1]"),
                     (target(kact=Matern12), "kern_act[0]")):
        snap = _snapshot(t)
        with pytest.raises(ValueError) as e:
            t.load_state_dict(state)
        assert where in str(e.value), str(e.value)
        _unchanged(t, snap)
    ok = target()
    ok.load_state_dict(state)
    src = _pdgp(10)
    _same_params(src, ok)
    assert ok._adam_t == 17 and ok._bits == 64 and ok.__dict__["_packed_key"] is None     # float_type stays the target's
    for (m1, v1), (m2, v2) in zip(src._adam_state(), ok._adam_state()):
        assert np.array_equal(m1, m2) and np.array_equal(v1, v2)
    for (xa, ya), (xb, yb) in zip(_next_draws(src), _next_draws(ok)):
        assert np.array_equal(xa, xb) and np.array_equal(ya, yb)

    s = _sgpr()
    for other in (SGPRSS(s.X.value, s.Y.value, np.sum([_sm(MercerMatern12sm, 2, rng) for _ in range(2)]), s.Z.value),
                  SGPRSS(s.X.value, s.Y.value[:, :1], np.sum([_sm(MercerMatern12sm, 2, rng) for _ in range(3)]), s.Z.value,
                         mean_function=mean_functions.Linear())):
        before = [p._array.copy() for p in param.sorted_params(other.kern)]
        with pytest.raises(ValueError):
            other.load_state_dict(s.state_dict())
        assert all(np.array_equal(a, p._array) for a, p in zip(before, param.sorted_params(other.kern)))


def test_pickling_hooks_are_not_added():
    import copy
    for cls in (Pdgp, SGPRSS, Matern32, Add, Prod):
        for name in ("__reduce__", "__getstate__", "__setstate__"):
            assert name not in cls.__dict__
    m = _pdgp(10)
    twin = copy.deepcopy(m)
    _same_params(m, twin)
    assert len(twin._adam_state()) == len(m._adam_state())
