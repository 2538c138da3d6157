"""Tied Params of optimize_many / PdgpBatch, host side (gpitch_amd.pdgp_batch.tie_groups / check_tied, the workspace size of
gp_pdgpb_set_ties): no device."""
import copy
import ctypes as C

import numpy as np
import pytest

from tied_ref import segment_model, segments


def _offsets(models):
    """id(Param) -> its offset in the batch's parameter vector (model_segments, models back to back)"""
    from gpitch_amd.pdgp_batch import model_segments
    off, base = {}, 0
    for m in models:
        segs, n = model_segments(m, base)
        off.update({id(p): o for o, p in segs})
        base += n
    return off


def test_tie_groups_of_three_identical_models():
    from gpitch_amd import tie_groups
    ms = segments(3)
    before = [[p.value for p in k.theta_params()] for m in ms for k in list(m.kern_act) + list(m.kern_com)]
    groups = tie_groups(ms)
    # noise, then per latent GP one group per theta position: two Matern32 (2 each), Mercer m = 2 (6), Matern32sm m = 2 (6)
    assert len(groups) == 1 + 2 + 2 + 6 + 6
    assert all(len(g) == 3 for g in groups)
    assert [id(p) for p in groups[0]] == [id(m.likelihood.variance) for m in ms]
    assert [id(p) for p in groups[2]] == [id(m.kern_act[0].lengthscales) for m in ms]
    assert [id(p) for p in groups[5 + 1]] == [id(m.kern_com[0].lengthscales) for m in ms]
    assert [id(p) for p in groups[-1]] == [id(m.kern_com[1].frequency[1]) for m in ms]
    assert len(tie_groups(ms, noise=False)) == 16 and len(tie_groups(ms, kernels=False)) == 1
    withz = tie_groups(ms, noise=False, kernels=False, inducing=True)
    assert [[id(p) for p in g] for g in withz] == [[id(m.za[i]) for m in ms] for i in range(2)] + \
        [[id(m.zc[i]) for m in ms] for i in range(2)]
    after = [[p.value for p in k.theta_params()] for m in ms for k in list(m.kern_act) + list(m.kern_com)]
    assert all(np.array_equal(a, b) for x, y in zip(before, after) for a, b in zip(x, y))
    assert all(m._plan is None for m in ms)


def test_tie_groups_names_the_model_that_differs():
    from gpitch_amd import tie_groups
    ms = segments(2) + [segment_model(75, com=[2, 3])]          # the second component kernel has 3 partials
    with pytest.raises(ValueError, match=r"model 2: latent GP 3 .*3 partials"):
        tie_groups(ms)
    with pytest.raises(ValueError, match=r"model 1 has 1 sources"):
        tie_groups([ms[0], segment_model(76, P=1)])
    ms = segments(2) + [segment_model(77, M=24)]
    assert len(tie_groups(ms)) == 17                               # M may differ while z is not tied
    with pytest.raises(ValueError, match=r"inducing=True: model 2: latent GP 0 has 24 inducing points"):
        tie_groups(ms, inducing=True)


def _refused(ms, tied, pattern):
    from gpitch_amd import check_tied
    with pytest.raises(ValueError, match=pattern):
        check_tied(ms, tied)
    assert all(m._plan is None for m in ms)


def test_check_tied_refusals_name_group_and_role():
    from gpitch_amd.param import Param, transforms
    ms = segments(3)
    ok = [m.likelihood.variance for m in ms]
    ls = [m.kern_com[1].lengthscales for m in ms]
    # a Param of none of the models
    _refused(ms, [ok, [ls[0], Param(0.1)]], r"group 1: member 1 .*not a Param of the listed models")
    _refused(ms, [[ls[0], segment_model(80).kern_com[1].lengthscales]], r"group 0: member 1 .*not a Param")
    # twice: in one group, in two groups
    _refused(ms, [[ls[0], ls[1], ls[0]]], r"group 0: model 0, com 1, lengthscales appears twice \(first in group 0\)")
    _refused(ms, [ok, ls, [ms[1].kern_act[0].variance, ls[2]]],
             r"group 2: model 2, com 1, lengthscales appears twice \(first in group 1\)")
    # q(u)
    _refused(ms, [ok, [ms[0].q_mu_act[1], ms[1].q_mu_act[1]]], r"group 1: model 0, act 1, q_mu: q\(u\) is never tied")
    _refused(ms, [[ms[0].q_sqrt_com[0], ms[2].q_sqrt_com[0]]], r"group 0: model 0, com 0, q_sqrt: q\(u\) is never tied")
    # shapes
    other = segment_model(78, M=24)
    _refused(ms[:2] + [other], [[ms[0].za[1], other.za[1]]], r"group 0: model 2, act 1, za has shape \(24, 1\)")
    # transforms: the type, and Logistic's bounds
    _refused(ms, [ok, [ms[0].kern_com[0].lengthscales, ms[1].kern_com[1].lengthscales]],
             r"group 1: model 1, com 1, lengthscales has transform Logistic\(0.0, 2.0\), model 0, com 0, lengthscales has Log1pe")
    b = copy.deepcopy(ms)
    b[2].kern_com[1].lengthscales.transform = transforms.Logistic(0., 3.)
    _refused(b, [[m.kern_com[1].lengthscales for m in b]],
             r"group 0: model 2, com 1, lengthscales has transform Logistic\(0.0, 3.0\)")
    # fixed flags
    b = copy.deepcopy(ms)
    b[1].kern_act[0].variance.fixed = True
    _refused(b, [[m.kern_act[0].variance for m in b]], r"group 0: model 1, act 0, variance has fixed=True")
    # values, bit for bit
    b = copy.deepcopy(ms)
    b[1].kern_com[0].energy[1].value = np.nextafter(b[1].kern_com[0].energy[1].value, 1.0)
    _refused(b, [[m.likelihood.variance for m in b], [m.kern_com[0].energy[1] for m in b]],
             r"group 1: model 1, com 0, energy\[1\] holds")
    # stored Adam moments
    b = copy.deepcopy(ms)
    state = [(np.zeros(p.size), np.zeros(p.size)) for p in b[2]._param_order()]
    state[0] = (np.full(1, 1e-3), np.full(1, 1e-6))
    b[2]._set_adam_state(state)
    _refused(b, [[m.likelihood.variance for m in b]], r"group 0: model 2, noise, variance and model 0, noise, variance have "
                                                     r"different stored Adam moments")
    # Adam step counts of models that a tie joins
    b = copy.deepcopy(ms)
    b[1]._adam_t = 5
    _refused(b, [[b[0].likelihood.variance, b[2].likelihood.variance], [m.kern_act[1].lengthscales for m in b]],
             r"group 1: model 1, act 1, lengthscales belongs to a model at Adam step 5")


def test_check_tied_accepts_fixed_and_single_groups_and_returns_offsets():
    from gpitch_amd import check_tied, tie_groups
    ms = segments(2, zfixed=False) + [segment_model(79, P=3, zfixed=False)]
    off = _offsets(ms)
    for m in ms:
        m.kern_com[0].frequency.fixed = True
    fixed = [[ms[0].kern_com[0].frequency[j], ms[1].kern_com[0].frequency[j]] for j in range(2)]
    unit = [[ms[0].kern_com[1]._unit, ms[1].kern_com[1]._unit]]      # Matern32sm's unit variance slot is always fixed
    single = [[ms[0].likelihood.variance], [ms[1].za[0]]]
    assert check_tied(ms, None) == [] and check_tied(ms, []) == []
    assert check_tied(ms, fixed + unit + single) == []
    # a z group ties element by element; a within-model group lists offsets of one model
    zg = [ms[0].zc[1], ms[1].zc[1]]
    inner = [k.lengthscales for k in ms[2].kern_act]
    got = check_tied(ms, fixed + [zg] + single + [inner])
    M = zg[0].size
    assert len(got) == M + 1
    assert got[:M] == [[off[id(zg[0])] + e, off[id(zg[1])] + e] for e in range(M)]
    assert got[M] == [off[id(p)] for p in inner]
    # tie_groups' groups of two identical models: every free position, in model_segments' order of model 0
    got = check_tied(ms[:2], tie_groups(ms[:2]))
    want = [[off[id(p)] for p in g] for g in tie_groups(ms[:2]) if not g[0].fixed]
    assert got == want and len(got) == 1 + 2 + 2 + 4 + 5
    assert all(m._plan is None for m in ms)


def test_ties_workspace_bytes_and_exported_symbols():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    size = lib.gp_pdgpb_ties_workspace_bytes
    up = lambda n, a: (n + a - 1) // a * a
    # the documented carve: [group_start (ngroups + 1 int32) | members (int64) | set_start (nmodels / 2 + 1 int32) |
    # set_models (nmodels int32) | frozen (nmodels int32)], every region rounded up to the arena's 256 bytes, plus the
    # batch plans' margin of 256 bytes
    doc = lambda g, n, k: up(4 * (g + 1), 256) + up(8 * n, 256) + up(4 * (k // 2 + 1), 256) + 2 * up(4 * k, 256) + 256
    for g, n, k in ((1, 2, 2), (17, 51, 3), (300, 2400, 88), (63, 64, 5), (64, 64, 5), (4096, 100000, 1000)):
        assert size(g, n, k) == doc(g, n, k), (g, n, k)
        assert size(g, n, k) % 256 == 0
    assert size(1, 2, 2) < size(1000, 2, 2) < size(1000, 5000, 2) < size(1000, 5000, 900)
    assert size(0, 0, 3) == 0 and size(0, 10, 3) == 0
    for name in ("gp_pdgpb_ties_workspace_bytes", "gp_pdgpb_set_ties", "gp_pdgpb_ties_frozen"):
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name
    # without a plan the other two entries refuse a null plan instead of touching it
    assert lib.gp_pdgpb_set_ties(None, 0, None, None, None, 0) == _lib.GP_ERR_BAD_ARG
    assert lib.gp_pdgpb_ties_frozen(None, (C.c_int32 * 1)(), 0) == _lib.GP_ERR_BAD_ARG
