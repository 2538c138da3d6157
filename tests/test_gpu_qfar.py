"""The far-field form of the Q route's product (G = Q Kuf from the rows near each 256-frame group plus two tables
of rank 2 mpad) against the dense product (gemm_wave.hip role 6) in the same process: the plan's permission bit 1 — the caller's
word that the inducing inputs ascend — switches between them, and without it the path is the one GPITCH_AMD_SWITCHES=qform_far=0
selects (a child process with that switch confirms it bit for bit).  Models as in test_gpu_qform.py: MercerMatern12sm components
over fixed inducing inputs, a Matern-3/2 activation family.  Every evaluation that takes the far field also reads the device's own
range tables back (gp_debug_pdgp_far_ranges) and compares them, for every latent GP of the run, with the numpy rule at the
lengthscale the device holds: a device rule that called every row near would give the right numbers and lose the whole gain."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                    # (the child process below starts this file without conftest.py)
    sys.path.insert(0, ROOT)

import qfar_rule as qf
import qbar_rule as qb
from helpers import pdgp_from_problem, model_grad_dict

pytestmark = pytest.mark.gpu

FAR_VS_DENSE_ELBO = 1e-12   # relative (test_gpu_qform.py's bar for two float64 forms)
FAR_VS_DENSE = 1e-9         # x block scale
COUNTED = ("cond_A", "cond_LTA", "kuf_bar", "nt_gemm", "hyper")
LS_ACT = 0.002              # as test_gpu_qform.py: 8 spacings for the Matern-3/2 activations
SPACING_LS = 0.00025        # one inducing spacing, in _problem's lengthscale unit
CHILD_CASE = "128x1024x1_l8"
GAP = (3 * 256 + 5 * 32 + 11, 400)      # frame_gap: the first shifted frame (fourth group, sixth strip of it), lengthscales

# M x N x P, the components' lengthscale in inducing spacings, partials, and what the case is there for ("two": a group with
# far rows on both sides; "groups": that many column groups; "distinct": no two latent GPs share their ranges; "nonmonotone":
# the ranges are not monotone, so the widening and the running maxima change something; "full_chunk": exactly 256 groups)
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
    # three latent GPs of one run with their own inducing inputs and lengthscales: every range, reference point, table and tile
    # table differs between them, so a kernel that read item 0's for every GP cannot pass
    "per_gp_128x1024x3": dict(N=1024, M=128, P=3, ls=[8, 25, 8], z=[None, None, (5.8, [44, 42, 0, 42])], two=True, distinct=True),
    # a gap of 400 lengthscales in the frame times inside one 32-column strip (two excerpts joined): that strip spans more than
    # 300 lengthscales, its group is all near between narrower neighbours, and the ranges are not monotone
    "frame_gap_128x2048x1_l8": dict(N=2048, M=128, P=1, ls=8, z="off_grid", gap=GAP, two=True, nonmonotone=True),
    "frame_gap_128x2048x1_l2_m3": dict(N=2048, M=128, P=1, ls=2, m=3, z="off_grid", gap=GAP, two=True, nonmonotone=True),
    # the longest batch the Q route admits.  qbar_takes allows 4096 groups, but the route needs the lean contraction
    # (hyper_lean_takes, bwd.hip): at most 32 column segments of at most 2048 columns, so N <= 65536 = 256 groups — one full chunk of
    # qfar_t_kernel (QFT_CHUNK), of qbar_rec_kernel's decay tables and of qbar_assemble_kernel's decayed sums.  Their second
    # chunks (bcarry, c0 = 256, s0 += 256) cannot run in any admitted model
    "long_64x65536x1_m3": dict(N=65536, M=64, P=1, ls=2, m=3, two=True, full_chunk=True),
    # the size limits.  M = 1024 is 64 tiles (QBAR_MAX_TILES; all 64 lanes of qfar_cols_kernel's ballots, a zero shift of `am`).
    # qfar_takes allows m <= 32 (nf = 64 = QBAR_MAX_NF), but hyper_lean_takes admits three 16-feature tiles: m <= 24, nf = 48 is
    # the most an admitted model reaches — QBAR_NE = 16 and QBAR_NY = 4 are sized for a shape that never arrives (9 and 3 are used)
    "limits_1024x1024x1_m24": dict(N=1024, M=1024, P=1, ls=2, m=24, two=True),
    # one partial: nf = 8 of which three feature pairs are zero padding.  With a single cosine Kuu is worse conditioned than the
    # mixtures': at 8 spacings pdgp.py's measure is 5.5 (allowed: 3) and the model keeps the Cholesky route; 4 spacings (2.9,
    # the same ranges) is the longest admitted lengthscale on this grid
    "limits_64x512x1_m1": dict(N=512, M=64, P=1, ls=4, m=1),
}


def _problem(N, M, P, ls, m=20, z=None, seed=5, gap=None, **_):
    """ls and z: one value for every component, or a list with one per component.  z None: make_problem's uniform decimation;
    "off_grid": x[::N / M] + 0.37 frames; (step, per): clusters of per[g] inducing inputs `step` frames apart in group g, the
    lengthscale then in units of `step`; "unsorted": the uniform ones permuted.  gap = (n0, J): every frame from n0 on, and every
    inducing input (components and activations) at or after x[n0], is shifted by J lengthscales of component 0."""
    from gpitch_amd.synth import make_problem
    prob = make_problem(N, M, P, num_partials=m, seed=seed)
    fs = float(prob["fs"])
    spacing = (N / float(M)) / 4.0
    zs = z if isinstance(z, list) else [z] * P
    lss = ls if isinstance(ls, list) else [ls] * P
    assert len(zs) == P and len(lss) == P
    for p in range(P):
        unit = spacing
        if isinstance(zs[p], tuple):
            step, per = zs[p]
            zz = np.concatenate([(g * 256 + 0.37 + step * np.arange(k)) / fs for g, k in enumerate(per)])
            assert zz.shape[0] == M
            prob["zc"][p] = zz.reshape(-1, 1).copy()
            unit = step / 4.0
        elif zs[p] == "off_grid":
            zz = prob["x"][::N // M] + 0.37 / fs
            assert zz.shape[0] == M
            prob["zc"][p] = zz.copy()
        elif zs[p] == "unsorted":
            perm = np.random.RandomState(11).permutation(M)
            prob["zc"][p] = prob["zc"][p][perm].copy()
        prob["kern_com"][p]["lengthscales"] = lss[p] * SPACING_LS * unit
    for d in prob["kern_act"]:
        d["lengthscales"] = LS_ACT * spacing
    if gap is not None:
        n0, J = gap
        t0, shift = float(prob["x"][n0, 0]), J * float(prob["kern_com"][0]["lengthscales"])
        prob["x"][n0:] += shift
        for zz in list(prob["zc"]) + list(prob["za"]):
            zz[zz >= t0] += shift
    return prob


def _ranges(prob, p=0):
    return qf.ranges(np.ravel(prob["zc"][p]), np.ravel(prob["x"]), float(prob["kern_com"][p]["lengthscales"]))


def device_ranges(h, model, i, ng, nt):
    """gp_debug_pdgp_far_ranges for latent GP i of the run: (groups written, the GP's index in the plan, rng [ng][2], ref [ng][2],
    rng2 [ng][2], S0 [nt], Sa [nt]); what the call does not write keeps -1 / NaN"""
    rng, rng2 = np.full(2 * ng, -1, dtype=np.int32), np.full(2 * ng, -1, dtype=np.int32)
    ref = np.full(2 * ng, np.nan)
    s0, sa = np.full(nt, -1, dtype=np.int32), np.full(nt, -1, dtype=np.int32)
    g = C.c_int32(-1)
    n = int(h.lib.gp_debug_pdgp_far_ranges(model._plan, i, ng, C.byref(g), rng.ctypes.data, ref.ctypes.data, rng2.ctypes.data,
                                           s0.ctypes.data, sa.ctypes.data))
    return n, int(g.value), rng.reshape(-1, 2), ref.reshape(-1, 2), rng2.reshape(-1, 2), s0, sa


def assert_device_ranges(h, model, prob, far, bar):
    """After an evaluation: for every latent GP of the run the device's ranges are the numpy rule's as integers, its reference
    points the rule's bmin and bmax bit for bit, and (backward far field) its widened ranges and tile tables qbar_rule's — at the
    inducing inputs and the lengthscale of the device's own parameter vector.  Returns the range lists, one per GP."""
    P, M = int(prob["P"]), int(prob["M"])
    x = model._x_dev.cpu().numpy().reshape(-1)
    ng, nt = x.shape[0] // qf.GROUP, M // qf.TILE
    if not far:
        assert device_ranges(h, model, 0, ng, nt)[0] == 0
        return []
    params = model._params.cpu().numpy()
    assert device_ranges(h, model, P, ng, nt)[0] == 0                    # the run is the P components
    assert device_ranges(h, model, 0, ng - 1, nt)[0] == 0                # too small a buffer: nothing written
    out = []
    for i in range(P):
        n, g, rng, ref, rng2, s0, sa = device_ranges(h, model, i, ng, nt)
        assert n == ng and g == P + i, (i, n, g)
        o_th, o_z = model._layout[g][:2]
        z, ls = params[o_z:o_z + M], float(params[o_th + 1])
        assert np.array_equal(z, np.ravel(prob["zc"][i]))
        want = qf.ranges(z, x, ls)
        assert rng.tolist() == [[kb, ke] for kb, ke, _, _ in want], (i, rng.tolist())
        wref = np.array([[bmin, bmax] for _, _, bmin, bmax in want])
        assert np.array_equal(ref.view(np.int64), wref.view(np.int64)), (i, np.abs(ref - wref).max())
        if bar:
            kb, ke = qb.monotone(want)
            S0, Sa = qb.tile_tables(kb, ke, M)
            assert rng2.tolist() == [[b, e] for b, e in zip(kb, ke)], (i, rng2.tolist())
            assert s0.tolist() == S0 and sa.tolist() == Sa, (i, s0.tolist(), sa.tolist())
        else:
            assert np.all(rng2 == -1) and np.all(s0 == -1) and np.all(sa == -1)
        out.append(rng.tolist())
    return out


def _evaluate(prob, h, qform=None, overlap=None, ascending=None, count=False, flags=None):
    """(ELBO, gradient vector, gradient by name, launches per timer of COUNTED or None, far field taken).  qform None: as pdgp.py
    decides.  flags: a dict that receives "bar", whether the backward pass took the far field too."""
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
    far, bar = int(h.lib.gp_pdgp_far_field(model._plan)), int(h.lib.gp_pdgp_far_field_backward(model._plan))
    assert_device_ranges(h, model, prob, far, bar)
    if flags is not None:
        flags["bar"] = bar
    return f, model._grad.cpu().numpy().copy(), model_grad_dict(model), launches, far


def test_cases_are_admissible_and_have_their_far_fields():
    """on the host: pdgp.py allows the Q route for every case, finds its inducing inputs ascending, and the numpy range rule
    gives each case the groups it is there for (assert_device_ranges makes the same rule a statement about the device)"""
    for name, c in CASES.items():
        prob = _problem(**c)
        model = pdgp_from_problem(prob)
        assert model._qform_admissible(), name
        assert model._qform_z_ascending(), name
        rng = _ranges(prob)
        both, one, none = qf.sides(rng, c["M"])
        if len(rng) <= 16:
            print("%s: ranges %s" % (name, [(kb, ke) for kb, ke, _, _ in rng]))
        assert both + one > 0, name
        if c.get("two"):
            assert both > 0, name
        if c.get("groups"):
            assert len(rng) == c["groups"], name
        if c.get("empty"):
            assert any(kb == ke for kb, ke, _, _ in rng), name
        per_gp = [[(kb, ke) for kb, ke, _, _ in _ranges(prob, p)] for p in range(c["P"])]
        for r in per_gp:
            assert any(kb > 0 or ke < c["M"] for kb, ke in r), name
        if c.get("distinct"):
            assert all(per_gp[p] != per_gp[q] for p in range(c["P"]) for q in range(p)), name
        assert qb.is_monotone(rng) == (not c.get("nonmonotone")), name
        if c.get("nonmonotone"):
            kb, ke = qb.monotone(rng)
            assert any(k < r[0] for k, r in zip(kb, rng)) and any(e > r[1] for e, r in zip(ke, rng)), name
        if c.get("full_chunk"):
            # 256 groups fill one chunk of every chunked walk; the walks themselves (qbar_rule.tile_tables: R- down to S0 of the
            # first tile, R+ up to Sa of the last, the near x near band of a diagonal pair) stay inside it
            assert len(rng) == 256, name
            S0, Sa = qb.tile_tables(*qb.monotone(rng), c["M"])
            print("%s: S0 %s Sa %s" % (name, S0, Sa))
            assert len(rng) - S0[0] > 128 and Sa[-1] > 128 and max(s - a for s, a in zip(S0, Sa)) > 64, name


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


def _child(path):
    from gpitch_amd import _lib
    h = _lib.Handle(0)
    flags = {}
    f, v, _, n, far = _evaluate(_problem(**CASES[CHILD_CASE]), h, count=True, flags=flags)      # pdgp.py's own permission
    np.savez(path, f=f, v=v, n=np.array(n), d=np.array([far, flags["bar"]]))


def test_switch_off_is_the_library_without_the_far_field(gp_handle, tmp_path):
    """GPITCH_AMD_SWITCHES=qform_far=0 in a child process, where pdgp.py's own permission (7) then runs the dense product and the
    split-K backward pass, against permission 1 here: ELBO, gradient vector and launch counts equal, neither flag raised"""
    path = str(tmp_path / "child.npz")
    env = dict(os.environ, GPITCH_AMD_SWITCHES="qform_far=0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-1500:])
    ref = np.load(path)
    assert tuple(ref["d"]) == (0, 0)
    flags = {}
    f, v, _, n, far = _evaluate(_problem(**CASES[CHILD_CASE]), gp_handle, qform=1, count=True, flags=flags)
    assert (far, flags["bar"]) == (0, 0)
    assert f == float(ref["f"]) and np.array_equal(v, ref["v"])
    assert n == tuple(int(k) for k in ref["n"])


if __name__ == "__main__":
    _child(sys.argv[1])
