"""The scan's chunk moments and near sums from the activations' far field (kuf_scan_far_moments_kernel in
kuf_scan.hip) against the pass over the stored A (kuf_scan_stream_kernel) ON ONE HANDLE AND ONE MODEL: the plan's permission
gp_pdgp_set_scan_far switches between them.  Both forms feed the same prefix and far launches, and nothing else of the step
reads what they write, so the ELBO and every gradient block but the activations' variance and lengthscale must be bit-equal;
those two are two float64 forms of one sum and must agree to 1e-9 of their scale, the project's bar.  Cases: the matrix-core
product's (afar_mfma_cases.py), the layouts of test_gpu_afar.py, and one whose thresholds all lie inside one group."""
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

TWO_FORMS = 1e-9            # x block scale: the project's bar for two float64 forms of one gradient
CHILD_CASE = "plain_128x8192"

LAYOUTS = ("plain_128x8192", "clustered_128x8192", "one_group_128x8192", "frame_gap_128x8192")
CASES = {name: (mc.problem, c) for name, c in mc.CASES.items()}
CASES.update({name: (ta._problem, ta.CASES[name]) for name in LAYOUTS})
# every inducing input of the GP inside group 9 (122 frames of it: two of its four chunks hold all 64 thresholds)
CASES["one_group_64x16384"] = (ta._problem, dict(N=16384, M=64, P=1, ls=8, z=(1.9, {9: 64})))


def _problem(name):
    build, c = CASES[name]
    return build(**c)


def _is_scan_block(name):
    return name.startswith("act") and (name.endswith(".variance") or name.endswith(".lengthscales"))


def _model(prob, h, overlap=None, **kw):
    model = pdgp_from_problem(prob, handle=h, **kw)
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    if overlap is not None:
        h.check(h.lib.gp_pdgp_set_overlap(model._plan, overlap))
    return model


def _evaluate(model, h, scan_far=None, count=False):
    """(ELBO, gradient vector, gradient by name, launches under the `hyper` timer or None, form reported)"""
    if scan_far is not None:
        h.check(h.lib.gp_pdgp_set_scan_far(model._plan, int(scan_far)))
    if count:
        h.check(h.lib.gp_timers_enable(h.h, 1))
        h.check(h.lib.gp_timers_reset(h.h))
    try:
        f = model._elbo(True)
        h.sync()
        launches = h.timers()["hyper"][1] if count else None
    finally:
        if count:
            h.check(h.lib.gp_timers_enable(h.h, 0))
    return f, model._grad.cpu().numpy().copy(), model_grad_dict(model), launches, int(h.lib.gp_pdgp_scan_far(model._plan))


def _compare(tag, on, off):
    """the far-field form against the pass over A: everything bit-equal but the two sums, those within the bar"""
    f1, _, g1, _, _ = on
    f0, _, g0, _, _ = off
    assert f1 == f0, tag
    worst = 0.0
    for name in g0:
        if _is_scan_block(name):
            d = np.abs(g1[name] - g0[name]).max() / max(np.abs(g0[name]).max(), 1e-300)
            print("%s %s: far-field moments vs the pass over A %.2e of its scale" % (tag, name, d))
            worst = max(worst, d)
        else:
            assert np.array_equal(g1[name], g0[name]), (tag, name)
    assert worst <= TWO_FORMS, (tag, worst)


@pytest.mark.parametrize("case", sorted(CASES))
def test_far_moments_against_the_pass_over_a(gp_handle, case):
    h = gp_handle
    prob = _problem(case)
    model = _model(prob, h)
    on = _evaluate(model, h, count=True)                 # the default: permission given
    assert int(h.lib.gp_pdgp_far_field_act(model._plan)) == 1 and on[4] == 1, case
    off = _evaluate(model, h, scan_far=0, count=True)
    assert off[4] == 0 and on[3] == off[3], (case, on[3], off[3])
    _compare(case, on, off)
    # a second evaluation, and the permission back on after it was off: the same bits
    again = _evaluate(model, h, scan_far=1)
    assert again[4] == 1 and again[0] == on[0] and np.array_equal(again[1], on[1]), case
    again = _evaluate(model, h)
    assert again[0] == on[0] and np.array_equal(again[1], on[1]), case
    # overlap levels 0 and 2 on fresh models, and the forward-only ELBO
    for level in (0, 2):
        m = _model(prob, h, overlap=level)
        other = _evaluate(m, h)
        assert other[4] == 1 and other[0] == on[0] and np.array_equal(other[1], on[1]), (case, level)
    assert _model(prob, h)._elbo(False) == on[0], case


def test_one_plan_while_the_lengthscale_moves(gp_handle):
    """8 -> 250 -> 8 spacings on one plan: each evaluation bit-equal to a fresh model's, the first and the third to each other,
    and at 250 spacings (cond(Kuu) ~ 4e8) the two forms still within the bar"""
    h = gp_handle
    c = ta.CASES["plain_128x8192"]
    unit = (c["N"] / float(c["M"])) / ta.FS
    model = _model(ta._problem(**c), h)
    got = []
    for s in (8, 250, 8):
        model.kern_act[0].lengthscales.value = s * unit
        model._pack()
        on = _evaluate(model, h, scan_far=1)
        fresh = _evaluate(_model(ta._problem(**dict(c, ls=s)), h), h)
        assert on[4] == 1 and fresh[4] == 1
        assert on[0] == fresh[0] and np.array_equal(on[1], fresh[1]), s
        _compare("l = %d spacings" % s, on, _evaluate(model, h, scan_far=0))
        got.append(on)
    assert got[0][0] == got[2][0] and np.array_equal(got[0][1], got[2][1])
    assert got[0][0] != got[1][0]


def test_descending_frames_are_an_error_and_the_handle_goes_on(gp_handle):
    """two neighbouring frames exchanged under the promise of ascending frames: the new kernel checks the pairs it reads, as
    the pass over A does; the evaluation returns GP_ERR_BAD_ARG and the handle works afterwards"""
    from gpitch_amd import _lib
    h = gp_handle
    prob = _problem("plain_128x8192")
    good = _evaluate(_model(prob, h), h)
    bad = dict(prob)
    bad["x"], bad["y"] = prob["x"].copy(), prob["y"].copy()
    j = 5 * 256 + 77
    bad["x"][[j, j + 1]] = bad["x"][[j + 1, j]]
    model = _model(bad, h)                        # pdgp.py saw the descending pair and withheld the promise
    assert np.isfinite(model._elbo(True)) and int(h.lib.gp_pdgp_scan_far(model._plan)) == 0
    h.check(h.lib.gp_pdgp_set_frames_ascending(model._plan, 1))
    with pytest.raises(_lib.GpitchError) as err:
        model._elbo(True)
    assert err.value.status == _lib.GP_ERR_BAD_ARG and "not ascending" in str(err.value)
    assert int(h.lib.gp_pdgp_scan_far(model._plan)) == 1
    after = _evaluate(_model(prob, h), h)
    assert after[4] == 1 and after[0] == good[0] and np.array_equal(after[1], good[1])


def _fallbacks():
    base = ta.CASES["plain_128x8192"]
    m52 = ta._problem(**base)
    m52["kern_act"][0]["type"] = "matern52"
    return {
        "matern52": (m52, {}, None),
        "act_far_withheld": (ta._problem(**base), {}, 0),
        "float32": (ta._problem(**base), dict(float_type=np.float32), None),
        "mixed": (ta._problem(**base), dict(float_type=(np.float64, np.float32)), None),
        "ragged_n": (ta._problem(**dict(base, N=8192 + 64)), {}, None),
        "short_strip": (ta._problem(**dict(base, N=4096)), {}, None),
    }


@pytest.mark.parametrize("which", ["matern52", "act_far_withheld", "float32", "mixed", "ragged_n", "short_strip"])
def test_fallbacks_keep_the_pass_over_a(gp_handle, which):
    """everything the selection does not admit: the form is reported not taken, the permission changes neither a bit nor a
    launch under the `hyper` timer"""
    h = gp_handle
    prob, kw, far_act = _fallbacks()[which]
    model = _model(prob, h, **kw)
    if far_act is not None:
        h.check(h.lib.gp_pdgp_set_far_act(model._plan, far_act))
    on = _evaluate(model, h, scan_far=1, count=True)
    off = _evaluate(model, h, scan_far=0, count=True)
    assert on[4] == 0 and off[4] == 0, which
    assert on[3] == off[3] and on[0] == off[0] and np.array_equal(on[1], off[1]), which


def _child(path):
    from gpitch_amd import _lib
    h = _lib.Handle(0)
    f, v, _, n, took = _evaluate(_model(_problem(CHILD_CASE), h), h, count=True)
    np.savez(path, f=f, v=v, n=np.array([n]), d=np.array([took]))


def test_switch_off_is_the_library_without_the_form(gp_handle, tmp_path):
    """GPITCH_AMD_SWITCHES=scan_far=0 in a child process against the permission withheld here: ELBO, gradient vector and launch
    count equal, the getter 0"""
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, GPITCH_AMD_SWITCHES="scan_far=0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    ref = np.load(path)
    assert tuple(ref["d"]) == (0,)
    f, v, _, n, took = _evaluate(_model(_problem(CHILD_CASE), gp_handle), gp_handle, scan_far=0, count=True)
    assert took == 0
    assert f == float(ref["f"]) and np.array_equal(v, ref["v"]) and n == int(ref["n"][0])


def test_workspace_at_its_exact_size(gp_handle, monkeypatch):
    """an activation plan that takes the form, between guard bands at exactly gp_pdgp_workspace_bytes and one granule short
    (test_gpu_workspace_bounds.py's check): the tables of the forward pass (rng, T, Psi, the Kuf strip, W) that the backward
    window now reads have homes of their own in the carve, and nothing of the backward pass writes there"""
    import test_gpu_workspace_bounds as wb
    prob = ta._problem(**ta.CASES["two_gps_192x5632"])

    def run():
        m = _model(prob, gp_handle)
        out = {"elbo": m._elbo(True), "grad": m._grad.cpu().numpy().copy()}
        assert int(gp_handle.lib.gp_pdgp_scan_far(m._plan)) == 1
        return out
    wb._check(gp_handle, monkeypatch, run, exact_keys=("elbo",))


if __name__ == "__main__":
    _child(sys.argv[1])
