"""The far fields' table kernels and the Q route's guard in their staged forms (switch far_tables) against the
forms they replace.

Operators (gp_debug_far_tables: ONE launch of a table kernel on this file's buffers, ranges and reference points written here,
no cols kernel): for every case of far_tables_cases.py the table T of form 1 (afar_t_tiled_kernel / qfar_t_lds_kernel) equals
form 0's (afar_t_kernel / qfar_t_kernel) BYTE FOR BYTE, between guard bands that keep their sentinel.  Each table is also compared
with the numpy rule (afar_rule.tables / qfar_rule.tables) — a guard against a mis-wired entry, not the accuracy bar: the rule and
the device differ in exp's last bits and in the order the rows of one step enter.

Form 0's largest deviation from the numpy rule, relative to the table's largest entry, measured per case on MI355X with
afar_t_kernel / qfar_t_kernel (this file prints it for either form; profiles/r14/rule_dev.txt).  afar, largest 4.635e-16:
    all_at_step0_1024x2 4.635e-16; backwards_48x5 1.958e-16; clustered_1024x5 2.081e-16; clustered_16x5 0.000e+00;
    clustered_272x1 1.770e-16; clustered_272x128 3.739e-16; clustered_48x2 1.506e-16; frame_gap_272x5 1.594e-16;
    grid_1024x1 3.493e-16; grid_1024x128 1.813e-16; grid_16x1 0.000e+00; grid_16x128 0.000e+00; grid_272x2 1.930e-16;
    grid_48x5 1.965e-16; nan_above_1024x2 2.287e-16; nan_above_16x2 0.000e+00; nan_above_272x5 2.508e-16;
    none_272x5 0.000e+00; off_grid_1024x2 2.966e-16; off_grid_16x2 0.000e+00; off_grid_272x5 1.895e-16;
    off_grid_48x1 0.000e+00; off_grid_48x128 2.200e-16; ragged_48x5 1.613e-16
qfar, largest 1.293e-15:
    all_above_128x48x3 1.293e-15; all_below_128x48x3 1.274e-16; all_near_64x8x3 0.000e+00; clustered_1024x64x1 1.187e-15;
    clustered_1024x8x2 1.248e-15; clustered_128x40x2 7.009e-16; clustered_64x48x3 2.011e-16; clustered_64x8x257 1.015e-16;
    frame_gap_128x40x8 1.390e-16; grid_1024x40x3 1.224e-15; grid_128x48x1 1.988e-16; grid_64x40x255 0.000e+00;
    grid_64x64x2 1.016e-16; grid_64x8x1 0.000e+00; grid_64x8x300 0.000e+00; off_grid_1024x48x2 9.774e-16;
    off_grid_128x64x3 3.407e-16; off_grid_128x8x3 2.713e-16; off_grid_64x40x2 2.102e-16; off_grid_64x8x256 1.350e-16
Form 1 is asserted within 4 x the largest recorded value.

Guard and whole models: far_tables=1 here against GPITCH_AMD_SWITCHES=far_tables=0 in ONE child process — the guard's verdict and
GP index for a benign and an ill-conditioned Kuu at N = 4096, M = 64 and 128 (as test_gpu_qform.py's
test_an_ill_conditioned_kuu_is_an_error_not_a_less_accurate_result raises it), and ELBO and gradient vector of one case each of
test_gpu_afar.py's and test_gpu_qfar.py's tables and of per_gp_128x1024x3, at overlap 2 and 0, np.array_equal."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                    # (the child process below starts this file without conftest.py)
    sys.path.insert(0, ROOT)
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import far_tables_cases as fc

pytestmark = pytest.mark.gpu

# measured with form 0 (the docstring's tables): the largest over the cases, per kernel
RULE_DEV_AFAR = 4.635e-16
RULE_DEV_QFAR = 1.293e-15
SENTINEL = -1.2345678e300
BAND = 64                                   # doubles in front of and behind T

AFAR = {c["name"]: c for c in fc.afar_cases()}
QFAR = {c["name"]: c for c in fc.qfar_cases()}


def _ranges_dev(h, case):
    rng = np.array([[kb, ke] for kb, ke, _, _ in case["rng"]], dtype=np.int32)
    ref = np.array([[lo, hi] for _, _, lo, hi in case["rng"]], dtype=np.float64)
    return h.torch.as_tensor(rng, device=h.device), h.to_device(ref)


def _launch(h, which, form, case):
    """T [ng][M][width] of one launch, read back; the guard bands are checked here"""
    M, ng, N = case["M"], case["ng"], case["N"]
    rng, ref = _ranges_dev(h, case)
    z = h.to_device(case["z"])
    if which == 0:
        width, nf = 8, 0
        X, X2, fz = h.to_device(case["W"]), h.to_device(case["C"]), None
        theta = h.to_device(np.array([1.3, case["ls"]]))
    else:
        nf = case["nf"]
        width = 2 * nf
        X, X2, fz = h.to_device(case["Q"]), None, h.to_device(case["fz"])
        theta = h.to_device(np.array([1.0, case["ls"]]))
    n = ng * M * width
    buf = h.torch.full((n + 2 * BAND,), SENTINEL, dtype=h.torch.float64, device=h.device)
    ws = h.workspace(256)
    h.torch.cuda.synchronize()
    st = h.lib.gp_debug_far_tables(h.h, which, form, C.c_void_p(X.data_ptr()), C.c_void_p(X2.data_ptr()) if X2 is not None else None,
                                   C.c_void_p(z.data_ptr()), C.c_void_p(theta.data_ptr()),
                                   C.c_void_p(fz.data_ptr()) if fz is not None else None, C.c_void_p(rng.data_ptr()),
                                   C.c_void_p(ref.data_ptr()), C.c_void_p(buf.data_ptr() + 8 * BAND), M, N, nf,
                                   C.c_void_p(ws.data_ptr()), 256)
    h.check(st)
    h.sync()
    out = buf.cpu().numpy()
    assert np.all(out[:BAND] == SENTINEL) and np.all(out[-BAND:] == SENTINEL), "%s form %d wrote outside T" % (case["name"], form)
    return out[BAND:-BAND].reshape(ng, M, width).copy()


def _rule_dev(T, want):
    return float(np.abs(T - want).max() / max(np.abs(want).max(), 1e-300))


def _check(h, which, case, want, bar):
    T0, T1 = _launch(h, which, 0, case), _launch(h, which, 1, case)
    assert not np.any(T0 == SENTINEL) and not np.any(T1 == SENTINEL), case["name"]
    d0, d1 = _rule_dev(T0, want), _rule_dev(T1, want)
    print("%s %s: form 0 vs rule %.3e, form 1 vs rule %.3e of the largest entry %.3e"
          % ("afar" if which == 0 else "qfar", case["name"], d0, d1, np.abs(want).max()))
    assert np.array_equal(T0.view(np.int64), T1.view(np.int64)), \
        (case["name"], int((T0.view(np.int64) != T1.view(np.int64)).sum()), float(np.nanmax(np.abs(T0 - T1))))
    assert np.all(np.isfinite(T1)), case["name"]
    assert d1 <= 4.0 * bar, (case["name"], d1)
    T1b = _launch(h, which, 1, case)                                     # two runs agree
    assert np.array_equal(T1.view(np.int64), T1b.view(np.int64)), case["name"]


@pytest.mark.parametrize("name", sorted(AFAR))
def test_afar_tables_tiled_equal_the_chain_per_thread_bytes(gp_handle, name):
    case = AFAR[name]
    _check(gp_handle, 0, case, fc.afar_rule_tables(case), RULE_DEV_AFAR)


@pytest.mark.parametrize("name", sorted(QFAR))
def test_qfar_tables_staged_equal_the_element_per_thread_bytes(gp_handle, name):
    case = QFAR[name]
    _check(gp_handle, 1, case, fc.qfar_rule_tables(case), RULE_DEV_QFAR)


def test_debug_entry_refuses_what_the_kernels_do_not_take(gp_handle):
    from gpitch_amd import _lib
    h = gp_handle
    t = h.zeros(4096)
    p = C.c_void_p(t.data_ptr())
    for args in ((0, 0, p, p, p, p, None, p, p, p, 24, 256, 0),          # M no multiple of 16
                 (0, 1, p, p, p, p, None, p, p, p, 16, 200, 0),          # no whole group
                 (1, 1, p, None, p, p, p, p, p, p, 32, 256, 8),          # M no multiple of 64
                 (1, 1, p, None, p, p, p, p, p, p, 64, 256, 12),         # nf no multiple of 8
                 (2, 0, p, p, p, p, None, p, p, p, 16, 256, 0)):
        st = h.lib.gp_debug_far_tables(h.h, *args, p, 256)
        assert st == _lib.GP_ERR_BAD_ARG, args
    h.sync()


# ---- the guard and whole models: this process (far_tables = 1) against a child with far_tables = 0 ----------------------
GUARD_CASES = [(64, None), (64, 1.0), (128, None), (128, 1.0)]   # M; the components' lengthscale: test_gpu_qform.py's own, or its ill-conditioned 1 s
MODEL_CASES = [("afar", "plain_128x8192"), ("qfar", "128x1024x1_l8"), ("qfar", "per_gp_128x1024x3")]


def _guard_verdict(h, M, ls_com):
    """what an evaluation with the Q route forced on says: ("ok", ELBO) or ("error", status, message — it names the latent GP)"""
    import test_gpu_qform as tf
    from gpitch_amd import _lib
    from helpers import pdgp_from_problem
    prob = tf._problem(N=4096, M=M, P=1) if ls_com is None else tf._problem(N=4096, M=M, P=1, ls_com=ls_com)
    model = pdgp_from_problem(prob, handle=h)
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    h.check(h.lib.gp_pdgp_set_qform(model._plan, 1))
    out = []
    for _ in range(2):                                                   # two evaluations agree
        try:
            out.append(["ok", float(model._elbo(True)).hex()])
        except _lib.GpitchError as e:
            out.append(["error", int(e.status), str(e)])
    assert out[0] == out[1], out
    return out[0]


def _model_bits(h, kind, name, overlap):
    if kind == "afar":
        import test_gpu_afar as ta
        prob = ta._problem(**ta.CASES[name])
        f, v, _, _, took, _ = ta._evaluate(prob, h, overlap=overlap)
    else:
        import test_gpu_qfar as tq
        prob = tq._problem(**tq.CASES[name])
        f, v, _, _, took = tq._evaluate(prob, h, overlap=overlap)
    assert took == 1, (kind, name)
    return float(f), v


def _everything(h):
    out = {"guard": [_guard_verdict(h, M, ls) for M, ls in GUARD_CASES]}
    arrays = {}
    for kind, name in MODEL_CASES:
        for overlap in (2, 0):
            f, v = _model_bits(h, kind, name, overlap)
            out["f_%s_%d" % (name, overlap)] = f.hex()
            arrays["v_%s_%d" % (name, overlap)] = v
    return out, arrays


@pytest.fixture(scope="module")
def switch_off(tmp_path_factory):
    """the child's verdicts and bits with GPITCH_AMD_SWITCHES=far_tables=0"""
    path = str(tmp_path_factory.mktemp("far_tables") / "child")
    env = dict(os.environ, GPITCH_AMD_SWITCHES="far_tables=0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    with open(path + ".json") as fh:
        return json.load(fh), np.load(path + ".npz")


@pytest.fixture(scope="module")
def switch_on(gp_handle):
    assert "far_tables=0" not in os.environ.get("GPITCH_AMD_SWITCHES", "")
    return _everything(gp_handle)


def test_guard_gives_the_verdict_of_the_guard_it_replaces(switch_on, switch_off):
    on, off = switch_on[0]["guard"], switch_off[0]["guard"]
    for (M, ls), a, b in zip(GUARD_CASES, on, off):
        print("guard M %d ls_com %s: %s" % (M, ls, a))
        assert a == b, (M, ls, a, b)
    kinds = [a[0] for a in on]
    assert kinds == ["ok", "error", "ok", "error"], kinds                # benign, ill-conditioned, per M
    assert all("qform" in a[2] for a in on if a[0] == "error")


@pytest.mark.parametrize("kind,name", MODEL_CASES)
def test_whole_models_keep_every_bit(switch_on, switch_off, kind, name):
    for overlap in (2, 0):
        k = "%s_%d" % (name, overlap)
        assert switch_on[0]["f_" + k] == switch_off[0]["f_" + k], (k, switch_on[0]["f_" + k], switch_off[0]["f_" + k])
        assert np.array_equal(switch_on[1]["v_" + k], switch_off[1]["v_" + k]), k
    assert switch_on[0]["f_%s_2" % name] == switch_on[0]["f_%s_0" % name]


def _child(path):
    from gpitch_amd import _lib
    out, arrays = _everything(_lib.Handle(0))
    with open(path + ".json", "w") as fh:
        json.dump(out, fh)
    np.savez(path + ".npz", **arrays)


if __name__ == "__main__":
    _child(sys.argv[1])
