"""The Q route's backward products from the far field (Qbar = Kuf diag(2 gv) Kuf^T and v = Kuf gm from the rows near
each 256-frame group plus the far tables, qbar.hip) against the dense split-K product in the same process: bit 2 of the plan's
permission switches between them.  pdgp.py sets 7; a plan given 3 (or 1) runs the backward pass that existed before, which a
child process with GPITCH_AMD_SWITCHES=qform_qbar=0 — a library that never takes the new path — confirms bit for bit.
Shapes and models: test_gpu_qfar.py's cases; every evaluation also compares the device's ranges, widened ranges and tile tables
with the numpy rules (test_gpu_qfar.assert_device_ranges).  One test keeps a plan while the lengthscale moves, as training does."""
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
    far, bar = int(h.lib.gp_pdgp_far_field(model._plan)), int(h.lib.gp_pdgp_far_field_backward(model._plan))
    tq.assert_device_ranges(h, model, prob, far, bar)      # the device's ranges, widened ranges and tile tables: the numpy rules'
    return f, model._grad.cpu().numpy().copy(), model_grad_dict(model), launches, far, bar


def test_ranges_of_the_cases_are_monotone():
    """... of every latent GP, but for the cases with a gap in the frame times, which are there because theirs are not"""
    for name, c in CASES.items():
        prob = tq._problem(**c)
        for p in range(c["P"]):
            assert qb.is_monotone(tq._ranges(prob, p)) == (not c.get("nonmonotone")), (name, p)


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


MOVING_LS = (25, 4, 25, 8)      # inducing spacings, in this order on one plan


def _free_model(prob, h):
    model = pdgp_from_problem(prob, handle=h)
    model.za.fixed = True
    model.zc.fixed = True
    return model


def _objective(model, x_free, h, prob):
    """one evaluation through the model's own free-state entry: (ELBO, free gradient, gradient by name, far, bar, range lists)"""
    f, g = model._objective(x_free)
    h.sync()
    far, bar = int(h.lib.gp_pdgp_far_field(model._plan)), int(h.lib.gp_pdgp_far_field_backward(model._plan))
    return -f, -np.asarray(g), model_grad_dict(model), far, bar, tq.assert_device_ranges(h, model, prob, far, bar)


def test_one_plan_while_the_lengthscale_moves(gp_handle):
    """Training keeps one plan, its workspace and the device-side transform while the lengthscale moves, so ranges, tile tables and
    the blocks written only where a run ends (Um, Vp, Wv, CnF) live on from a step with other ranges.  Four evaluations through
    Pdgp._objective on one model, packed once, at 25, 4, 25 and 8 spacings: after each the device's tables are the numpy
    rule's at that lengthscale, each agrees bit for bit with a fresh model evaluated once at that lengthscale through the same
    entry, and the first and third agree bit for bit.  The same walk on plans with permission 3 (split-K backward) and 1
    (dense product) stays within the bars between forms at every step."""
    h = gp_handle
    c = CASES["128x1024x1_l8"]
    fresh = {}
    for ls in sorted(set(MOVING_LS)):
        prob = tq._problem(**dict(c, ls=ls))
        model = _free_model(prob, h)
        x = model.get_free_state()
        fresh[ls] = (x,) + _objective(model, x, h, prob)
        assert fresh[ls][4:6] == (1, 1), ls
    xs = [fresh[ls][0] for ls in sorted(fresh)]
    assert all(int((xs[0] != x).sum()) == 1 for x in xs[1:])             # the states differ in the lengthscale alone
    prob = tq._problem(**c)
    model = _free_model(prob, h)
    packs, pack = [], model._pack
    object.__setattr__(model, "_pack", lambda: (packs.append(1), pack())[1])
    walk = []
    for ls in MOVING_LS:
        step = _objective(model, fresh[ls][0], h, prob)
        want = fresh[ls]
        assert step[3:5] == (1, 1), ls
        assert step[5] == want[6], ls                                    # (both already equal the numpy rule at the device's lengthscale)
        assert step[0] == want[1] and np.array_equal(step[1], want[2]), (ls, step[0], want[1])
        walk.append(step)
    assert len(packs) == 1
    assert all(a[5] != b[5] for a, b in zip(walk, walk[1:]))             # the ranges moved at every step
    assert walk[0][0] == walk[2][0] and np.array_equal(walk[0][1], walk[2][1])
    for perm, flags in ((3, (1, 0)), (1, (0, 0))):
        other = _free_model(prob, h)
        other._pack()
        h.check(h.lib.gp_pdgp_set_qform(other._plan, perm))
        for k, ls in enumerate(MOVING_LS):
            f0, _, g0, far, bar, _ = _objective(other, fresh[ls][0], h, prob)
            assert (far, bar) == flags, (perm, ls)
            f1, g1 = walk[k][0], walk[k][2]
            dev = abs(f1 - f0) / abs(f0)
            worst = max(np.abs(g1[n] - g0[n]).max() / max(np.abs(g0[n]).max(), 1e-12) for n in g0)
            print("step %d (l = %d spacings) against permission %d: ELBO %.2e relative, gradient blocks worst %.2e" % (k, ls, perm, dev, worst))
            if perm == 3:
                assert f1 == f0, (f1, f0)                                # the forward pass is the same
            assert dev <= tq.FAR_VS_DENSE_ELBO and worst <= FAR_VS_DENSE, (perm, ls, dev, worst)


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
