"""The far-field form of the Q route's product (G = Q Kuf from the rows near each 256-frame group plus two tables
of rank 2 mpad) against the dense product (gemm_wave.hip role 6) in the same process: the plan's permission bit 1 — the caller's
word that the inducing inputs ascend — switches between them, and without it the path is the one GPITCH_AMD_SWITCHES=qform_far=0
selects.  Models as in test_gpu_qform.py: MercerMatern12sm components over fixed inducing inputs, a Matern-3/2 activation family."""
import numpy as np
import pytest

import qfar_rule as qf
from helpers import pdgp_from_problem, model_grad_dict

pytestmark = pytest.mark.gpu

FAR_VS_DENSE_ELBO = 1e-12   # relative (test_gpu_qform.py's bar for two float64 forms)
FAR_VS_DENSE = 1e-9         # x block scale
COUNTED = ("cond_A", "cond_LTA", "kuf_bar", "nt_gemm", "hyper")
LS_ACT = 0.002              # as test_gpu_qform.py: 8 spacings for the Matern-3/2 activations
SPACING_LS = 0.00025        # one inducing spacing, in _problem's lengthscale unit

# M x N x P, the components' lengthscale in inducing spacings, partials, and what the case is there for ("two": a group with
# far rows on both sides; "groups": that many column groups)
CASES = {
    "128x1024x1_l25": dict(N=1024, M=128, P=1, ls=25),
    "128x1024x1_l8": dict(N=1024, M=128, P=1, ls=8),
    "192x768x2_l8": dict(N=768, M=192, P=2, ls=8, groups=3),                 # odd tile count, three groups
    "256x2048x1_l8": dict(N=2048, M=256, P=1, ls=8, two=True),               # two-sided far field
    "64x4096x2_l8": dict(N=4096, M=64, P=2, ls=8),                           # the helper streams build the tables
    "128x1024x1_m3": dict(N=1024, M=128, P=1, ls=2, m=3, two=True),          # padded features: nf = 8, one chunk per side
    # off-grid clustered inducing inputs, 5.8 frames apart in the first, second and last group: several per group, one with none
    "128x1024x1_clustered": dict(N=1024, M=128, P=1, ls=8, z=(5.8, [44, 42, 0, 42]), two=True),
    # the same with clusters that end on tile edges and two empty groups: the second has no near row at all
    "128x1280x1_gap": dict(N=1280, M=128, P=1, ls=8, z=(5.2, [48, 32, 0, 0, 48]), two=True, empty=True),
}


def _problem(N, M, P, ls, m=20, z=None, seed=5, **_):
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=m, seed=seed)
    spacing = (N / float(M)) / 4.0
    unit = spacing
    if isinstance(z, tuple):
        fs, (step, per) = float(prob["fs"]), z
        zz = np.concatenate([(g * 256 + 0.37 + step * np.arange(k)) / fs for g, k in enumerate(per)])
        assert zz.shape[0] == M
        prob["zc"] = [zz.reshape(-1, 1).copy() for _ in range(P)]
        unit = step / 4.0
    elif z == "unsorted":
        perm = np.random.RandomState(11).permutation(M)
        prob["zc"] = [zc[perm].copy() for zc in prob["zc"]]
    for d in prob["kern_act"]:
        d["lengthscales"] = LS_ACT * spacing
    for d in prob["kern_com"]:
        d["lengthscales"] = ls * SPACING_LS * unit
    return prob


def _ranges(prob):
    return qf.ranges(np.ravel(prob["zc"][0]), np.ravel(prob["x"]), float(prob["kern_com"][0]["lengthscales"]))


def _evaluate(prob, h, qform=None, overlap=None, ascending=None, count=False):
    """(ELBO, gradient vector, gradient by name, launches per timer of COUNTED or None, far field taken).  qform None: as pdgp.py decides."""
    model = pdgp_from_problem(prob, handle=h)
    model.za.fixed = True
    model.zc.fixed = True
    model._pack()
    if qform is not None:
        h.check(h.lib.gp_pdgp_set_qform(model._plan, int(qform)))
    if overlap is not None:
        h.check(h.lib.gp_pdgp_set_overlap(model._plan, overlap))
    if ascending is not None:
        h.check(h.lib.gp_pdgp_set_frames_ascending(model._plan, int(ascending)))
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
    return f, model._grad.cpu().numpy().copy(), model_grad_dict(model), launches, int(h.lib.gp_pdgp_far_field(model._plan))


def test_cases_are_admissible_and_have_their_far_fields():
    """on the host: pdgp.py allows the Q route for every case, finds its inducing inputs ascending, and the numpy range rule
    gives each case the groups it is there for"""
    for name, c in CASES.items():
        prob = _problem(**c)
        model = pdgp_from_problem(prob)
        assert model._qform_admissible(), name
        assert model._qform_z_ascending(), name
        rng = _ranges(prob)
        both, one, none = qf.sides(rng, c["M"])
        print("%s: ranges %s" % (name, [(kb, ke) for kb, ke, _, _ in rng]))
        assert both + one > 0, name
        if c.get("two"):
            assert both > 0, name
        if c.get("groups"):
            assert len(rng) == c["groups"], name
        if c.get("empty"):
            assert any(kb == ke for kb, ke, _, _ in rng), name


@pytest.mark.parametrize("case", sorted(CASES))
def test_far_field_against_dense_product(gp_handle, case):
    prob = _problem(**CASES[case])
    f1, v1, g1, n1, far1 = _evaluate(prob, gp_handle, count=True)
    f0, v0, g0, n0, far0 = _evaluate(prob, gp_handle, qform=1, count=True)
    assert far1 == 1 and far0 == 0
    assert n1 == n0, (n1, n0)
    assert dict(zip(COUNTED, n1))["kuf_bar"] == 0
    dev = abs(f1 - f0) / abs(f0)
    print("%s ELBO: far field vs dense %.2e relative" % (case, dev))
    worst = 0.0
    for name in g0:
        scale = max(np.abs(g0[name]).max(), 1e-12)
        d = np.abs(g1[name] - g0[name]).max() / scale
        print("%s %s: far field vs dense %.2e" % (case, name, d))
        worst = max(worst, d)
    print("%s gradient blocks: far field vs dense, worst %.2e of a block's scale" % (case, worst))
    assert dev <= FAR_VS_DENSE_ELBO, (f1, f0)
    assert worst <= FAR_VS_DENSE, worst
    # determinism: a second run, and the tables in line instead of on the helper stream
    f_b, v_b, _, _, _ = _evaluate(prob, gp_handle, overlap=2)
    f_c, v_c, _, n_c, far_c = _evaluate(prob, gp_handle, overlap=0, count=True)
    assert far_c == 1 and n_c == n1
    assert f1 == f_b == f_c
    assert np.array_equal(v1, v_b)
    assert np.array_equal(v1, v_c)


def test_all_near_ranges_give_the_dense_bits(gp_handle):
    """A lengthscale of 10 000 spacings is far beyond the guard on Kuu's conditioning (4 M^2: test_gpu_qform.py's last test), so
    the largest admissible case whose ranges are all [0, M): one group that holds every inducing input.  The second loop
    never runs and the bits are role 6's."""
    c = dict(N=256, M=64, P=1, ls=25)
    prob = _problem(**c)
    assert all(kb == 0 and ke == c["M"] for kb, ke, _, _ in _ranges(prob))
    f1, v1, _, n1, far1 = _evaluate(prob, gp_handle, count=True)
    f0, v0, _, n0, far0 = _evaluate(prob, gp_handle, qform=1, count=True)
    assert far1 == 1 and far0 == 0 and n1 == n0
    assert f1 == f0 and np.array_equal(v1, v0)


def test_unsorted_inducing_inputs_keep_the_dense_product(gp_handle):
    prob = _problem(**dict(CASES["128x1024x1_l8"], z="unsorted"))
    assert not pdgp_from_problem(prob)._qform_z_ascending()
    f1, v1, _, n1, far1 = _evaluate(prob, gp_handle, count=True)
    f0, v0, _, n0, far0 = _evaluate(prob, gp_handle, qform=1, count=True)
    assert far1 == 0 and far0 == 0 and n1 == n0
    assert dict(zip(COUNTED, n1))["kuf_bar"] == 0               # still the Q route
    assert f1 == f0 and np.array_equal(v1, v0)


def test_frames_not_promised_ascending_keep_the_dense_product(gp_handle):
    prob = _problem(**CASES["128x1024x1_l8"])
    f1, v1, _, n1, far1 = _evaluate(prob, gp_handle, ascending=0, count=True)
    f0, v0, _, n0, far0 = _evaluate(prob, gp_handle, qform=1, ascending=0, count=True)
    assert far1 == 0 and far0 == 0 and n1 == n0
    assert f1 == f0 and np.array_equal(v1, v0)
