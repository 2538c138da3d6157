"""Which route a bound batch takes (DESIGN.md 3.04's table), asked through the public entries alone: the permission setters,
gp_pdgp_set_grad_needs (through `.fixed`), the five getters and gp_pdgp_workspace_bytes.  Every case is evaluated once with a
gradient and once without, each on a bind of its own (the gradient pointer is part of the bind's key): the getters are what
include/gpitch_abi.h promises for the case — the backward forms' getters 0 after the bind without a gradient — and the two
ELBOs are one double.  The workspace sizes are the recorded ones: no permission, set before or after the carve, moves a byte.
The numbers behind the routes are the other route tests' business (test_gpu_qform / qfar / qbar / afar / scan_far / hfar).

Models: Matern-3/2 activations, MercerMatern12sm components, 8 inducing spacings of lengthscale for the former (test_gpu_afar.py's
plain case) and a lengthscale the Q route's conditioning guard admits for the latter.  Shapes are the smallest at which a rule
can flip: the Q side at N = 1024 (test_gpu_qfar.py's 128x1024x1_l8), where the activations' strip has 2^17 entries and their far
field is off by shape; the activation side at N = 8192, M = 128, a strip of exactly 2^20 entries."""
import numpy as np
import pytest

from helpers import pdgp_from_problem

pytestmark = pytest.mark.gpu

FS = 16000.0
GETTERS = ("gp_pdgp_far_field", "gp_pdgp_far_field_backward", "gp_pdgp_far_field_act", "gp_pdgp_scan_far", "gp_pdgp_h_far")
F64_F32 = (np.float64, np.float32)

# gp_pdgp_workspace_bytes per model shape, as the commit before the routes became one record reports them
WORKSPACE = {
    "q_1024": 13674240, "q_1024_unwhitened": 14139904, "q_1024_f32": 8757504, "q_1000": 11583488,
    "a_8192": 76320768, "a_8192_unwhitened": 88962048, "a_8192_f64_f32": 61520384, "a_4096": 38768128,
    "both_8192x2": 152596992, "unequal_8192x2": 130764544,
}

# the shapes: make_problem's N, M, P and partial count, the components' lengthscale in inducing spacings, the model's options
Q_SIDE = dict(N=1024, M=128, P=1, m=20, ls_com=8)
A_SIDE = dict(N=8192, M=128, P=1, m=3, ls_com=2)
BOTH = dict(N=8192, M=128, P=2, m=3, ls_com=2)
SHAPES = {
    "q_1024": Q_SIDE, "q_1024_unwhitened": dict(Q_SIDE, whiten=False), "q_1024_f32": dict(Q_SIDE, float_type=np.float32),
    "q_1000": dict(Q_SIDE, N=1000),
    "a_8192": A_SIDE, "a_8192_unwhitened": dict(A_SIDE, whiten=False), "a_8192_f64_f32": dict(A_SIDE, float_type=F64_F32),
    "a_4096": dict(A_SIDE, N=4096),
    "both_8192x2": BOTH, "unequal_8192x2": dict(BOTH, M_act0=64),
}

# (case, shape, permissions and `.fixed` flags that differ from ON / fixed, getters of the gradient evaluation)
# permissions: frames (gp_pdgp_set_frames_ascending), qform (the bit mask), far_act, scan_far, h_far
ON = dict(frames=1, qform=7, far_act=1, scan_far=1, h_far=1, za_fixed=True, zc_fixed=True)
CASES = [
    # Q side: far_field needs bits 0 and 1 and ascending frames, far_field_backward bit 2 as well; the activations' getters are 0
    ("q_qform0", "q_1024", dict(qform=0), (0, 0, 0, 0, 0)),
    ("q_qform1", "q_1024", dict(qform=1), (0, 0, 0, 0, 0)),
    ("q_qform3", "q_1024", dict(qform=3), (1, 0, 0, 0, 0)),
    ("q_qform7", "q_1024", dict(), (1, 1, 0, 0, 0)),
    ("q_qform7_frames_not_promised", "q_1024", dict(frames=0), (0, 0, 0, 0, 0)),
    ("q_qform5_is_qform1", "q_1024", dict(qform=5), (0, 0, 0, 0, 0)),
    ("q_qform7_zc_free", "q_1024", dict(zc_fixed=False), (0, 0, 0, 0, 0)),
    ("q_qform7_unwhitened", "q_1024_unwhitened", dict(), (0, 0, 0, 0, 0)),
    ("q_qform7_float32", "q_1024_f32", dict(), (0, 0, 0, 0, 0)),
    ("q_qform7_n1000", "q_1000", dict(), (0, 0, 0, 0, 0)),
    # activation side (no Q permission): the far field, and on it the scan's moments and H from the factors
    ("a_far0", "a_8192", dict(qform=0, far_act=0), (0, 0, 0, 0, 0)),
    ("a_far1", "a_8192", dict(qform=0), (0, 0, 1, 1, 1)),
    ("a_far1_scan_far0", "a_8192", dict(qform=0, scan_far=0), (0, 0, 1, 0, 1)),
    ("a_far1_h_far0", "a_8192", dict(qform=0, h_far=0), (0, 0, 1, 1, 0)),
    ("a_far1_frames_not_promised", "a_8192", dict(qform=0, frames=0), (0, 0, 0, 0, 0)),
    ("a_far1_za_free", "a_8192", dict(qform=0, za_fixed=False), (0, 0, 0, 0, 0)),
    ("a_far1_unwhitened", "a_8192_unwhitened", dict(qform=0), (0, 0, 0, 0, 0)),
    # (float64 activations, float32 components: the far field may stay, the two forms that want float64 strips throughout do not)
    ("a_far1_f64_f32", "a_8192_f64_f32", dict(qform=0), (0, 0, 1, 0, 0)),
    ("a_far1_n4096", "a_4096", dict(qform=0), (0, 0, 0, 0, 0)),
    # both sides, every permission: every form; the split-K product has no latent GP left, and the GPs beside the Q run are one run
    ("both_all_on", "both_8192x2", dict(), (1, 1, 1, 1, 1)),
    # activations of M = 64 and 128: not the batch's one M
    ("unequal_activations", "unequal_8192x2", dict(qform=0), (0, 0, 0, 0, 0)),
]


def _problem(N, M, P, m, ls_com, M_act0=None, **_):
    from gpitch_amd.synth import make_problem, uniform_inducing
    prob = make_problem(N, M, P, num_partials=m, seed=5)
    spacing = (N // M) / FS
    for p in range(P):
        prob["kern_act"][p]["lengthscales"] = 8 * spacing
        prob["kern_com"][p]["lengthscales"] = ls_com * spacing
    if M_act0 is not None:
        prob["za"][0] = uniform_inducing(prob["x"], M_act0)
        prob["q_mu_act"][0] = prob["q_mu_act"][0][:M_act0].copy()
        prob["q_sqrt_act"][0] = prob["q_sqrt_act"][0][:M_act0, :M_act0].copy()
    return prob


def _set(h, model, frames, qform, far_act, scan_far, h_far, **_):
    lib, plan = h.lib, model._plan
    h.check(lib.gp_pdgp_set_frames_ascending(plan, frames))
    h.check(lib.gp_pdgp_set_qform(plan, qform))
    h.check(lib.gp_pdgp_set_far_act(plan, far_act))
    h.check(lib.gp_pdgp_set_scan_far(plan, scan_far))
    h.check(lib.gp_pdgp_set_h_far(plan, h_far))


def _model(h, shape, perms):
    """the model packed (which sets the gradient needs from `.fixed`), its workspace size checked, the permissions as given"""
    kw = SHAPES[shape]
    model = pdgp_from_problem(_problem(**kw), whiten=kw.get("whiten", True), handle=h, float_type=kw.get("float_type"))
    model.za.fixed = perms["za_fixed"]
    model.zc.fixed = perms["zc_fixed"]
    model._pack()
    if perms["qform"] & 1 and kw.get("whiten", True):
        assert model._qform_admissible() and model._qform_z_ascending(), shape     # (else the device's guard fails the evaluation)
    ws = int(h.lib.gp_pdgp_workspace_bytes(model._plan))
    print("workspace %s: %d bytes" % (shape, ws))
    _set(h, model, **perms)
    assert int(h.lib.gp_pdgp_workspace_bytes(model._plan)) == ws, shape
    return model, ws


def _getters(h, model):
    return tuple(int(getattr(h.lib, name)(model._plan)) for name in GETTERS)


def _check(h, model, want, what):
    """one evaluation with a gradient, one without; `want`: the getters of the former.  Returns the ELBO."""
    f1 = model._elbo(True)
    g1 = _getters(h, model)
    f0 = model._elbo(False)
    g0 = _getters(h, model)
    print("%s: getters %s with a gradient, %s without; ELBO %r / %r" % (what, g1, g0, f1, f0))
    assert g1 == tuple(want), (what, g1, want)
    assert g0 == tuple(want[:3]) + (0, 0), (what, g0, want)
    assert f1 == f0, (what, f1, f0)
    return f1


@pytest.mark.parametrize("case,shape,changes,want", CASES, ids=[c[0] for c in CASES])
def test_routes_of_the_bound_batch(gp_handle, case, shape, changes, want):
    model, ws = _model(gp_handle, shape, dict(ON, **changes))
    _check(gp_handle, model, want, case)
    assert ws == WORKSPACE[shape], (shape, ws)


def _rule(perms):
    """include/gpitch_abi.h's rules on the both-sides model, where every shape and type condition holds"""
    frames, q = perms["frames"], perms["qform"]
    far = int(frames and (q & 3) == 3)
    act = int(frames and perms["far_act"])
    return (far, int(far and (q & 7) == 7), act, int(act and perms["scan_far"]), int(act and perms["h_far"]))


def test_toggling_permissions_on_one_plan(gp_handle):
    """every permission off, on, off on one model, in turn: the getters follow, and with all of them off the ELBO is the double
    of a model that never had one"""
    h = gp_handle
    perms = dict(ON)
    model, ws = _model(h, "both_8192x2", perms)
    assert ws == WORKSPACE["both_8192x2"]
    f_on = _check(h, model, (1, 1, 1, 1, 1), "all on")
    f = None
    for name in ("h_far", "scan_far", "far_act", "qform", "frames"):
        for value in (0, ON[name], 0):
            perms[name] = value
            _set(h, model, **perms)
            f = _check(h, model, _rule(perms), "%s=%d" % (name, value))
    assert _rule(perms) == (0, 0, 0, 0, 0)
    never, _ = _model(h, "both_8192x2", dict(ON, frames=0, qform=0, far_act=0))
    assert _check(h, never, (0, 0, 0, 0, 0), "never permitted") == f
    _set(h, model, **ON)
    assert _check(h, model, (1, 1, 1, 1, 1), "all on again") == f_on
