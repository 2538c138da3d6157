"""The activations' H = A diag(2 gv) A^T and u = A gm from the stored A once and its factors once on the host:
hfar_rule.py's restatement of hfar.hip against long double, beside the dense form it replaces and the two-sided form that
factors both sides.  test_scan_far_cpu.py's eight setups (M = 128, N = 8192, Matern-3/2, jitter 1e-6, four layouts, lengthscales
of 8 and 250 inducing spacings); the reference takes the SAME float64 W and carries everything behind it in long double.
Asserted: the one-sided form's lower triangle and u lie within the larger of ten times the dense-A form's own deviation and
1e-13 of scale; at 250 spacings the two-sided form does NOT — that is the mutation this file exists for.  And the store of Y:
the near (tile, group) pairs number at most M / 16 + N / 256 - 1 and no two share a slot tile + group, on these layouts and on
the GPU tests' case tables."""
import numpy as np
import pytest

import afar_mfma_cases as mc
import afar_rule as af
import hfar_rule as hf
import test_gpu_afar as ta
from test_scan_far_cpu import _setup

LD = np.longdouble
FLOOR = 1e-13
LAYOUTS = ["grid", "off_grid", "clustered", "frame_gap"]


def _forms(name, spacings):
    s = _setup(name, spacings)
    z, x, ls, var, W, gv, gm, rng = (s[k] for k in ("z", "x", "ls", "var", "W", "gv", "gm", "rng"))
    A_ld = W.astype(LD) @ af.kuf(z, x, var, ls, dtype=LD)
    H_ref, u_ref = hf.h_dense(A_ld, gv, gm)
    A = af.product_far(W, s["K"], rng, s["T"], s["Psi"], lower=True)          # the stored strip as afar.hip leaves it
    H_d, u_d = hf.h_dense(A, gv, gm)
    H_1, u_1 = hf.h_one_sided(A, s["K"], W, rng, s["T"], s["Psi"], gv, gm)
    H_2 = hf.h_two_sided(s["K"], W, rng, s["T"], s["Psi"], gv)
    hs, us = float(np.abs(H_ref).max()), float(np.abs(u_ref).max())
    dev = lambda H: float(np.abs(H - H_ref).max()) / hs
    return dict(dense=dev(H_d), one=dev(H_1), two=dev(H_2), u_dense=float(np.abs(u_d - u_ref).max()) / us,
                u_one=float(np.abs(u_1 - u_ref).max()) / us)


@pytest.mark.parametrize("spacings", [8, 250])
@pytest.mark.parametrize("name", LAYOUTS)
def test_three_forms_against_long_double(name, spacings):
    d = _forms(name, spacings)
    tag = "%s, l = %d spacings" % (name, spacings)
    print("%s H lower triangle: dense A %.2e, one-sided %.2e, two-sided %.2e of scale" % (tag, d["dense"], d["one"], d["two"]))
    print("%s u: dense A %.2e, one-sided %.2e of scale" % (tag, d["u_dense"], d["u_one"]))
    bar = max(10.0 * d["dense"], FLOOR)
    assert d["one"] <= bar, (tag, d)
    assert d["u_one"] <= max(10.0 * d["u_dense"], FLOOR), (tag, d)
    if spacings == 250:
        assert d["two"] > 10.0 * bar, (tag, d)       # the form that carries W's rounding twice misses the bar by more than ten


def _assert_store(tag, z, x):
    rng = af.ranges(np.ravel(z), np.ravel(x))
    M, ng = np.ravel(z).shape[0], len(rng)
    pairs = hf.near_pairs(rng)
    assert af.is_monotone(rng), tag
    assert len(pairs) <= hf.slot_count(M, ng), (tag, len(pairs))
    assert not hf.slots_collide(rng), tag
    assert all(0 <= t + S < hf.slot_count(M, ng) for t, S in pairs), tag
    return len(pairs)


@pytest.mark.parametrize("name", LAYOUTS)
def test_pair_bound_and_slots_on_the_layouts(name):
    s = _setup(name, 8)
    n = _assert_store(name, s["z"], s["x"])
    print("%s: %d near pairs of at most %d" % (name, n, hf.slot_count(s["z"].shape[0], len(s["rng"]))))


def test_pair_bound_and_slots_on_the_gpu_cases():
    for name, c in ta.CASES.items():
        prob = ta._problem(**c)
        for p in range(c["P"]):
            _assert_store(name, prob["za"][p], prob["x"])
    for name, c in mc.CASES.items():
        prob = mc.problem(**c)
        for p in range(c["P"]):
            _assert_store(name, prob["za"][p], prob["x"])


def test_a_tie_on_both_sides_collides():
    """equal frames across a group boundary together with equal inducing inputs across a tile boundary: two pairs on one
    anti-diagonal, which hfar_check_kernel refuses"""
    x = np.arange(512) / 16000.0
    x[256] = x[255]
    z = np.concatenate([x[255] - 1e-3 + 1e-6 * np.arange(15), [x[255]], [x[255]], x[255] + 1e-3 + 1e-6 * np.arange(15)])
    rng = af.ranges(z, x)
    assert [r[:2] for r in rng] == [(0, 32), (0, 32)]
    assert hf.slots_collide(rng)
