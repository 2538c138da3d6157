"""The Q route's backward products from the far field (Qbar = Kuf diag(2 gv) Kuf^T and v = Kuf gm from the rows near
each 256-frame group plus the far tables, qbar.hip) against the dense split-K product in the same process: bit 2 of the plan's
permission switches between them.  pdgp.py sets 7; a plan given 3 (or 1) runs the backward pass that existed before, which a
child process with GPITCH_AMD_SWITCHES=qform_qbar=0 — a library that never takes the new path — confirms bit for bit.
Shapes and models: test_gpu_qfar.py's eight cases."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                    # (the child process below starts this file without conftest.py)
    sys.path.insert(0, ROOT)

import qbar_rule as qb
import test_gpu_qfar as tq
from helpers import pdgp_from_problem, model_grad_dict

pytestmark = pytest.mark.gpu

CASES = tq.CASES
COUNTED = tq.COUNTED
FAR_VS_DENSE = 1e-9         # x block scale: test_gpu_qfar.py's bar for two float64 forms
CHILD_CASE = "128x1024x1_l8"


def _evaluate(prob, h, qform=None, overlap=None, count=False):
    """(ELBO, gradient vector, gradient by name, launches per timer of COUNTED or None, forward far field, backward far field)"""
    model = pdgp_from_problem(prob, handle=h)
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    if qform is not None:
        h.check(h.lib.gp_pdgp_set_qform(model._plan, int(qform)))
    if overlap is not None:
        h.check(h.lib.gp_pdgp_set_overlap(model._plan, overlap))
    if count:
        h.check(h.lib.gp_timers_enable(h.h, 1))
        h.check(h.lib.gp_timers_reset(h.h))
    try:
        f = model._elbo(True)
        h.sync()
        launches = tuple(h.timers()[k][1] for k in COUNTED) if count else None
    finally:
        if count:
            h.check(h.lib.gp_timers_enable(h.h, 0))
    return (f, model._grad.cpu().numpy().copy(), model_grad_dict(model), launches, int(h.lib.gp_pdgp_far_field(model._plan)),
            int(h.lib.gp_pdgp_far_field_backward(model._plan)))


def test_ranges_of_the_cases_are_monotone():
    for name, c in CASES.items():
        assert qb.is_monotone(tq._ranges(tq._problem(**c))), name


@pytest.mark.parametrize("case", sorted(CASES))
def test_far_field_backward_against_split_k_product(gp_handle, case):
    prob = tq._problem(**CASES[case])
    f1, v1, g1, n1, far1, bar1 = _evaluate(prob, gp_handle, count=True)              # as pdgp.py decides: 7
    f0, v0, g0, n0, far0, bar0 = _evaluate(prob, gp_handle, qform=3, count=True)
    assert (far1, bar1) == (1, 1) and (far0, bar0) == (1, 0)
    assert n1 == n0, (n1, n0)
    assert f1 == f0, (f1, f0)                                                         # the forward pass is the same
    worst = 0.0
    for name in g0:
        scale = max(np.abs(g0[name]).max(), 1e-12)
        d = np.abs(g1[name] - g0[name]).max() / scale
        print("%s %s: far field vs split-K %.2e" % (case, name, d))
        worst = max(worst, d)
    print("%s gradient blocks: far field vs split-K, worst %.2e of a block's scale" % (case, worst))
    assert worst <= FAR_VS_DENSE, worst
    # determinism: a second run, and everything in line instead of on the helper stream
    f_b, v_b, _, _, _, bar_b = _evaluate(prob, gp_handle, overlap=2)
    f_c, v_c, _, n_c, _, bar_c = _evaluate(prob, gp_handle, overlap=0, count=True)
    assert bar_b == 1 and bar_c == 1 and n_c == n1
    assert f1 == f_b == f_c
    assert np.array_equal(v1, v_b)
    assert np.array_equal(v1, v_c)


def test_all_near_ranges_stay_within_the_bar(gp_handle):
    """test_gpu_qfar.py's largest admissible lengthscale whose ranges are all [0, M) (25 spacings: the guard on Kuu's conditioning
    stops 10 000), over two groups instead of its one — a batch of one group keeps the split-K product (qbar_takes): every pair
    of tiles is near x near, no far run"""
    c = dict(N=512, M=64, P=1, ls=25)
    prob = tq._problem(**c)
    assert all(kb == 0 and ke == c["M"] for kb, ke, _, _ in tq._ranges(prob))
    f1, _, g1, n1, _, bar1 = _evaluate(prob, gp_handle, count=True)
    f0, _, g0, n0, _, bar0 = _evaluate(prob, gp_handle, qform=3, count=True)
    assert bar1 == 1 and bar0 == 0 and n1 == n0 and f1 == f0
    worst = max(np.abs(g1[k] - g0[k]).max() / max(np.abs(g0[k]).max(), 1e-12) for k in g0)
    print("all near: far field vs split-K, worst %.2e of a block's scale" % worst)
    assert worst <= FAR_VS_DENSE, worst


def _child(path):
    from gpitch_amd import _lib
    h = _lib.Handle(0)
    prob = tq._problem(**CASES[CHILD_CASE])
    out = {}
    for perm in (None, 1):
        f, v, _, n, far, bar = _evaluate(prob, h, qform=perm, count=True)
        out["f%s" % perm], out["v%s" % perm], out["n%s" % perm], out["d%s" % perm] = f, v, np.array(n), np.array([far, bar])
    np.savez(path, **out)


def test_cleared_bit_is_the_library_without_the_new_path(gp_handle, tmp_path):
    """permission 3 and permission 1 (and 5: bit 2 means nothing without bit 1) against a child process whose library has the
    switch off, where pdgp.py's own permission runs the backward pass as it was: ELBO, gradient and launch counts equal"""
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, GPITCH_AMD_SWITCHES="qform_qbar=0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    ref = np.load(path)
    assert tuple(ref["dNone"]) == (1, 0) and tuple(ref["d1"]) == (0, 0)
    prob = tq._problem(**CASES[CHILD_CASE])
    for perm, key, diag in ((3, "None", (1, 0)), (1, "1", (0, 0)), (5, "1", (0, 0))):
        f, v, _, n, far, bar = _evaluate(prob, gp_handle, qform=perm, count=True)
        assert (far, bar) == diag, (perm, far, bar)
        assert f == float(ref["f" + key]) and np.array_equal(v, ref["v" + key]), perm
        assert n == tuple(int(k) for k in ref["n" + key]), perm


if __name__ == "__main__":
    _child(sys.argv[1])
