"""The activations' H = A diag(2 gv) A^T and u = A gm from the stored A once and its factors once (hfar.hip)
against the dense split-K product ON ONE HANDLE AND ONE MODEL: the plan's permission gp_pdgp_set_h_far switches between them.
The forward pass is untouched, so the ELBO is bit-equal; H and u feed the activations' q_mu, q_sqrt, variance and lengthscale
gradients only, so every component block and the noise gradient is bit-equal too, and the activations' blocks — two float64
forms of one product — agree to 1e-9 of their scale, the project's bar.  Cases: the layouts of test_gpu_afar.py, the
matrix-core product's (afar_mfma_cases.py: one tile, five tiles, near ranges off multiples of 64, every count of near tiles),
and one at 250 spacings."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                    # (the child process below starts this file without conftest.py)
    sys.path.insert(0, ROOT)

import afar_mfma_cases as mc
import test_gpu_afar as ta
from helpers import pdgp_from_problem, model_grad_dict

pytestmark = pytest.mark.gpu

TWO_FORMS = 1e-9            # x block scale: the project's bar for two float64 forms of one gradient (FAR_VS_DENSE)
CHILD_CASE = "plain_128x8192"

CASES = {name: (ta._problem, c) for name, c in ta.CASES.items()}
CASES.update({name: (mc.problem, c) for name, c in mc.CASES.items()})
CASES["long_128x8192"] = (ta._problem, dict(N=8192, M=128, P=1, ls=250))


def _problem(name):
    build, c = CASES[name]
    return build(**c)


def _is_act_block(name):
    return name.startswith("act") or name.startswith("q_mu_act") or name.startswith("q_sqrt_act") or name.startswith("za")


def _model(prob, h, overlap=None):
    model = pdgp_from_problem(prob, handle=h)
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    if overlap is not None:
        h.check(h.lib.gp_pdgp_set_overlap(model._plan, overlap))
    return model


def _evaluate(model, h, h_far=None, count=False):
    """(ELBO, gradient vector, gradient by name, launches under the `nt_gemm` timer or None, form reported)"""
    if h_far is not None:
        h.check(h.lib.gp_pdgp_set_h_far(model._plan, int(h_far)))
    if count:
        h.check(h.lib.gp_timers_enable(h.h, 1))
        h.check(h.lib.gp_timers_reset(h.h))
    try:
        f = model._elbo(True)
        h.sync()
        launches = h.timers()["nt_gemm"][1] if count else None
    finally:
        if count:
            h.check(h.lib.gp_timers_enable(h.h, 0))
    return f, model._grad.cpu().numpy().copy(), model_grad_dict(model), launches, int(h.lib.gp_pdgp_h_far(model._plan))


def _compare(tag, on, off):
    """the factored form against the dense product: everything bit-equal but the activations' blocks, those within the bar"""
    f1, _, g1, _, _ = on
    f0, _, g0, _, _ = off
    assert f1 == f0, tag
    worst = 0.0
    for name in g0:
        if _is_act_block(name):
            d = np.abs(g1[name] - g0[name]).max() / max(np.abs(g0[name]).max(), 1e-300)
            print("%s %s: from the factors vs the dense product %.2e of its scale" % (tag, name, d))
            worst = max(worst, d)
        else:
            assert np.array_equal(g1[name], g0[name]), (tag, name)
    assert worst <= TWO_FORMS, (tag, worst)


@pytest.mark.parametrize("case", sorted(CASES))
def test_factored_h_against_the_dense_product(gp_handle, case):
    h = gp_handle
    prob = _problem(case)
    model = _model(prob, h)
    on = _evaluate(model, h, count=True)                 # the default: permission given
    assert int(h.lib.gp_pdgp_far_field_act(model._plan)) == 1 and on[4] == 1, case
    off = _evaluate(model, h, h_far=0, count=True)
    assert off[4] == 0 and on[3] == off[3], (case, on[3], off[3])
    _compare(case, on, off)
    # a second evaluation, and the permission back on after it was off: the same bits
    again = _evaluate(model, h, h_far=1)
    assert again[4] == 1 and again[0] == on[0] and np.array_equal(again[1], on[1]), case
    again = _evaluate(model, h)
    assert again[0] == on[0] and np.array_equal(again[1], on[1]), case
    # overlap levels 0 and 2 on fresh models, launch counts included
    for level in (0, 2):
        other = _evaluate(_model(prob, h, overlap=level), h, count=True)
        assert other[4] == 1 and other[0] == on[0] and np.array_equal(other[1], on[1]) and other[3] == on[3], (case, level)


def test_one_plan_while_the_lengthscale_moves(gp_handle):
    """25 -> 4 -> 25 -> 8 spacings on one plan, as training moves it (the near ranges do not move with it, what is summed over
    them does): evaluations 1 and 3 bit-equal, each equal to a fresh model's"""
    h = gp_handle
    c = ta.CASES["plain_128x8192"]
    unit = (c["N"] / float(c["M"])) / ta.FS
    model = _model(ta._problem(**c), h)
    got = []
    for s in (25, 4, 25, 8):
        model.kern_act[0].lengthscales.value = s * unit
        model._pack()
        on = _evaluate(model, h)
        fresh = _evaluate(_model(ta._problem(**dict(c, ls=s)), h), h)
        assert on[4] == 1 and fresh[4] == 1
        assert on[0] == fresh[0] and np.array_equal(on[1], fresh[1]), s
        _compare("l = %d spacings" % s, on, _evaluate(model, h, h_far=0))
        h.check(h.lib.gp_pdgp_set_h_far(model._plan, 1))
        got.append(on)
    assert got[0][0] == got[2][0] and np.array_equal(got[0][1], got[2][1])
    assert got[0][0] != got[1][0] and got[0][0] != got[3][0]


@pytest.mark.parametrize("which", ["act_far_withheld", "float32", "mixed", "ragged_n", "short_strip"])
def test_fallbacks_keep_the_dense_product(gp_handle, which):
    """everything the selection does not admit: the form is reported not taken, the permission changes neither a bit nor a
    launch under the `nt_gemm` timer"""
    h = gp_handle
    base = ta.CASES["plain_128x8192"]
    prob, kw, far_act = {
        "act_far_withheld": (ta._problem(**base), {}, 0),
        "float32": (ta._problem(**base), dict(float_type=np.float32), None),
        "mixed": (ta._problem(**base), dict(float_type=(np.float64, np.float32)), None),
        "ragged_n": (ta._problem(**dict(base, N=8192 + 64)), {}, None),
        "short_strip": (ta._problem(**dict(base, N=4096)), {}, None),
    }[which]
    model = pdgp_from_problem(prob, handle=h, **kw)
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    if far_act is not None:
        h.check(h.lib.gp_pdgp_set_far_act(model._plan, far_act))
    on = _evaluate(model, h, h_far=1, count=True)
    off = _evaluate(model, h, h_far=0, count=True)
    assert on[4] == 0 and off[4] == 0, which
    assert on[3] == off[3] and on[0] == off[0] and np.array_equal(on[1], off[1]), which


def _child(path):
    from gpitch_amd import _lib
    h = _lib.Handle(0)
    f, v, _, n, took = _evaluate(_model(_problem(CHILD_CASE), h), h, count=True)
    np.savez(path, f=f, v=v, n=np.array([n]), d=np.array([took]))


def test_switch_off_is_the_library_without_the_form(gp_handle, tmp_path):
    """GPITCH_AMD_SWITCHES=h_far=0 in a child process against the permission withheld here: ELBO, gradient vector and launch
    count equal, the getter 0"""
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, GPITCH_AMD_SWITCHES="h_far=0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    ref = np.load(path)
    assert tuple(ref["d"]) == (0,)
    f, v, _, n, took = _evaluate(_model(_problem(CHILD_CASE), gp_handle), gp_handle, h_far=0, count=True)
    assert took == 0
    assert f == float(ref["f"]) and np.array_equal(v, ref["v"]) and n == int(ref["n"][0])


if __name__ == "__main__":
    _child(sys.argv[1])
