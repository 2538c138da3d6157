"""sample_sources_many, host side (no device): the scope check and every refusal, empty models, the offsets of one
gp_pdgpb_sample call, the split of a call into groups of models and chunks of draws, and the conditioning of the inputs that
test_gpu_pdgp_sample_many.py holds against the numpy restatement (tests/pdgp_sample_ref.py)."""
import numpy as np
import pytest

import pdgp_sample_many_cases as cs
import pdgp_sample_ref as ref
from gpitch_amd.pdgp_batch import check_sampleable, sample_layout, sample_sources_many, sample_split
from gpitch_amd.synth import pdgp_from_problem


def _prob(**kw):
    return ref.problem(8, 6, 2, 2, 128, seed=3, **kw)


def _sm(kind):
    return {"type": kind, "variance": 1.0, "lengthscales": 0.01, "energy": [0.1, 0.1], "frequency": [100., 200.]}


REFUSALS = ["whiten", "float32", "shard", "M", "duplicate", "empty", "not_a_model", "matern52_act", "rbf_com",
            "matern32sm_com", "matern12sm", "xnews_length", "xnew_shape", "num_samples", "eps_triples", "eps_shape",
            "eps_not_triple", "seed_length"]


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals_before_any_device_work(what):
    err, kw, says = NotImplementedError, {}, []
    models = None
    if what == "whiten":
        models, says = [pdgp_from_problem(_prob(), whiten=False)], ["model 0", "Pdgp.sample_sources"]
    elif what == "float32":
        models, says = [pdgp_from_problem(_prob(), float_type=np.float32)], ["model 0", "Pdgp.sample_sources"]
    elif what == "shard":
        models, says = [pdgp_from_problem(_prob()), pdgp_from_problem(_prob(), shard=(0, 2))], ["model 1", "Pdgp.sample_sources"]
    elif what == "M":
        models, err, says = [pdgp_from_problem(ref.problem(129, 6, 1, 2, 600, seed=3))], ValueError, ["model 0", "129"]
    elif what == "duplicate":
        m = pdgp_from_problem(_prob())
        models, err = [m, m], ValueError
    elif what == "empty":
        models, err, kw = [], ValueError, dict(xnews=[])
    elif what == "not_a_model":
        models, err = [pdgp_from_problem(_prob()), object()], ValueError
    elif what in ("matern52_act", "rbf_com", "matern32sm_com"):
        p = _prob()
        role, i, kern, name = {"matern52_act": ("kern_act", 1, ref._plain("matern52", 1.0, 0.01), "Matern52"),
                               "rbf_com": ("kern_com", 0, ref._plain("rbf", 1.0, 0.01), "RBF"),
                               "matern32sm_com": ("kern_com", 1, _sm("matern32sm"), "Matern32sm")}[what]
        p[role][i] = kern
        models = [pdgp_from_problem(_prob()), pdgp_from_problem(p)]
        says = ["model 1", "%s GP %d" % ("activation" if role == "kern_act" else "component", i), name, "MercerMatern12sm"]
    elif what == "matern12sm":
        p = _prob()
        p["kern_com"][0] = _sm("matern12sm")
        models, says = [pdgp_from_problem(p)], ["model 0", "Matern12sm", "Pdgp.sample_sources"]
    else:
        err = ValueError
        models = [pdgp_from_problem(_prob()), pdgp_from_problem(_prob())]
        good = [tuple([np.zeros(s) for s in shs] for shs in m.sample_eps_shapes(5, 2)) for m in models]
        if what == "xnews_length":
            kw = dict(xnews=[np.zeros(3)])
        elif what == "xnew_shape":
            kw = dict(xnews=[np.zeros(3), np.zeros((4, 2))])
        elif what == "num_samples":
            kw = dict(num_samples=0)
        elif what == "eps_triples":
            kw = dict(num_samples=2, eps=good[:1])
        elif what == "eps_shape":
            good[1][1][2] = np.zeros((2, 4, 7))
            kw = dict(num_samples=2, eps=good)
        elif what == "eps_not_triple":
            kw = dict(num_samples=2, eps=[good[0], good[1][:2]])
        else:
            kw = dict(seed=[1, 2, 3])
    xnews = kw.pop("xnews", [np.linspace(0., 0.005, 5) for _ in models])
    if what in REFUSALS[:13]:                     # the scope check itself refuses these
        with pytest.raises(err) as e:
            check_sampleable(models, xnews)
        for word in says:
            assert word in str(e.value), (word, str(e.value))
    else:
        check_sampleable(models, xnews)
    with pytest.raises(err) as e:                 # and so does the public entry, before any device work (no GPU here)
        sample_sources_many(models, xnews, **kw)
    for word in says:
        assert word in str(e.value), (word, str(e.value))
    for m in models:
        if hasattr(m, "_plan"):
            assert m._plan is None


def test_scope_check_returns_flat_inputs():
    ms = [pdgp_from_problem(_prob()), pdgp_from_problem(_prob(act="matern12", com="matern32"))]
    got, xs = check_sampleable(ms, [np.zeros((4, 1)), np.zeros(0)])
    assert got == ms and [x.shape for x in xs] == [(4,), (0,)] and all(x.dtype == np.float64 for x in xs)
    _, xs = check_sampleable(ms, np.arange(3, dtype=np.float32))
    assert len(xs) == 2 and all(x.shape == (3,) and x.dtype == np.float64 for x in xs)


def test_empty_models_return_shaped_arrays_without_a_device():
    ms = [pdgp_from_problem(_prob()), pdgp_from_problem(ref.problem(5, 4, 1, 2, 64, seed=4))]
    out = sample_sources_many(ms, [np.zeros(0), np.zeros((0, 1))], num_samples=3)
    assert [a.shape for a in out] == [(2, 3, 0), (1, 3, 0)]
    out = sample_sources_many(ms, np.zeros(0), num_samples=4, return_latents=True, seed=[5, 6])
    assert [len(o) for o in out] == [3, 3]
    assert all(a.shape == (P, 4, 0) for o, P in zip(out, (2, 1)) for a in o)
    assert all(m._plan is None for m in ms)


def test_offsets_of_a_small_ragged_call():
    """P = (1, 3), n = (5, 0); model 0: M = (4, 3), c = (2, 4); model 1: M = (2, 2, 2, 6, 6, 6), c = (1, 1, 1, 2, 2, 2)"""
    lay = sample_layout([1, 3], [5, 0], [4, 3, 2, 2, 2, 6, 6, 6], [2, 4, 1, 1, 1, 2, 2, 2])
    np.testing.assert_array_equal(lay["order"], [0, 9, 17, 19, 21, 23, 29, 35, 41])
    np.testing.assert_array_equal(lay["eps_x"], [0, 10, 30, 30, 30, 30, 30, 30, 30])
    np.testing.assert_array_equal(lay["eps_z"], [0, 8, 20, 22, 24, 26, 38, 50, 62])
    np.testing.assert_array_equal(lay["eps_u"], [0, 8, 14, 18, 22, 26, 38, 50, 62])
    np.testing.assert_array_equal(lay["latents"], [0, 10, 10])
    np.testing.assert_array_equal(lay["sources"], [0, 5, 5])
    np.testing.assert_array_equal(lay["x_off"], [0, 5, 5])
    assert all(v.dtype == np.int64 for v in lay.values())


@pytest.mark.parametrize("S", [1, 5, 16, 33, 100])
def test_split_covers_every_model_and_draw_once_in_order(S):
    per_draw, gps = [800, 2400, 160, 8000, 40], [2, 6, 2, 2, 4]
    seen_groups = set()
    nb = min(S, 16)
    for budget in (10 ** 9, nb * 8200, nb * 3400, nb * 2500, nb * 800, 100, 1):        # 1, 2, 3, .. and 5 groups
        split = sample_split(per_draw, gps, S, budget)
        seen_groups.add(len(split))
        at = 0
        for k0, k1, chunks in split:
            assert k0 == at and k1 > k0                          # consecutive models, none left out
            at = k1
            used = sum(per_draw[k0:k1])
            assert k1 - k0 == 1 or used * min(S, 16) <= budget   # only a single model may pass the budget
            s = 0
            for s0, sc in chunks:
                assert s0 == s and sc >= 1 and s0 % 16 == 0      # whole blocks of the seeded streams, in order
                s += sc
                assert sc <= 16 or used * sc <= budget
            assert s == S
        assert at == len(per_draw)
    assert {1, 2, 5} <= seen_groups
    many = sample_split(per_draw, gps, S, 1)
    assert [c for _, _, c in many] == [[(s0, min(16, S - s0)) for s0 in range(0, S, 16)]] * 5
    assert [g[:2] for g in sample_split(per_draw, gps, S, 10 ** 9, max_gps=8)] == [(0, 2), (2, 5)]   # the latent-GP limit cuts too


@pytest.mark.parametrize("name", cs.NAMES)
def test_gpu_inputs_are_well_conditioned(name):
    """a condition on the inputs, not a measurement: the two host routes of the restatement (triangular solves; products
    with the explicit W = L^-1, as the device holds it) agree within a tenth of the rule.  Worst ratios to that tenth:
    A 0.014, B 0.026, C 0.164, D 0.000, E 0.000, F 0.017."""
    prob, xs, nlin, _ = cs.case(name)
    for S in (5, 33):
        e = cs.eps(name, S)
        a = ref.sample_sources(prob, xs, e, True, nlin, route="solve")
        b = ref.sample_sources(prob, xs, e, True, nlin, route="W")
        for what, u, v in zip(("src", "g", "f"), b, a):
            err, bar = cs.rule(u, v)
            print("%s S = %d %s: routes differ by %.3e, a tenth of the rule %.3e" % (name, S, what, err, 0.1 * bar))
            assert err <= 0.1 * bar
