"""The operator cases of the far fields' table kernels (afar_t_kernel / afar_t_tiled_kernel of afar.hip,
qfar_t_kernel / qfar_t_lds_kernel of qfar.hip), shared by test_far_tables_cpu.py and test_gpu_far_tables.py.  A case is what
gp_debug_far_tables takes: the left factor(s), the inducing inputs, the lengthscale and the ranges with their reference points
— by the numpy rules (afar_rule.ranges, qfar_rule.ranges) for grid, off-grid and clustered inducing inputs, or made by hand
where no model produces them.  Times are in frames: x = 0, 1, ..., N - 1 unless a case shifts them."""
import numpy as np

import afar_rule as af
import qfar_rule as qf

GROUP = 256


def _z(layout, M, N, wide=False):
    """grid: every N / M frames; off_grid: the same + 0.37 frames; clustered: runs 1.9 frames apart that start in a few groups.
    wide: the inputs reach a quarter of the span beyond the frames on both sides (so that one group has far rows)."""
    lo, span = (-0.25 * N, 1.5 * N) if wide else (0.0, float(N))
    if layout == "grid":
        return lo + np.arange(M) * (span / M)
    if layout == "off_grid":
        return lo + np.arange(M) * (span / M) + 0.37
    assert layout == "clustered"
    ng = N // GROUP
    starts = sorted(set([0, ng // 3, ng - 1]))
    per = [M // len(starts)] * len(starts)
    per[-1] += M - sum(per)
    return np.sort(np.concatenate([g * GROUP + 0.37 + 1.9 * np.arange(k) for g, k in zip(starts, per)]))


def _afar(name, M, ng, z, rng, ls, nan_above=False, seed=0, **marks):
    r = np.random.RandomState(seed + 7 * M + ng)
    W = np.tril(r.randn(M, M))
    W[np.triu_indices(M, 1)] = np.nan if nan_above else 7.25     # the kernels may not use what lies above the diagonal
    return dict(name=name, M=M, ng=ng, N=ng * GROUP, z=np.asarray(z, dtype=np.float64), ls=float(ls), rng=list(rng), W=W,
                C=r.randn(M, M), nan_above=nan_above, **marks)


def _with_ref(pairs, x):
    """hand-made (kbeg, kend) per group with the groups' own xmin / xmax as reference points"""
    return [(kb, ke, float(x[S * GROUP:(S + 1) * GROUP].min()), float(x[S * GROUP:(S + 1) * GROUP].max()))
            for S, (kb, ke) in enumerate(pairs)]


def afar_cases():
    out = []
    layouts = ("grid", "off_grid", "clustered")
    k = 0
    for M in (16, 48, 272, 1024):
        for ng in (1, 2, 5, 128):
            lay = layouts[k % 3]
            k += 1
            N = ng * GROUP
            x = np.arange(N, dtype=np.float64)
            z = _z(lay, M, N, wide=(lay != "clustered"))
            out.append(_afar("%s_%dx%d" % (lay, M, ng), M, ng, z, af.ranges(z, x), 8.0 * max(N / M, 1.0), rule=True))
    # ---- by hand -------------------------------------------------------------------------------------------------------
    # every row enters at the first step of either walk: four 256-row chunks of afar_t_kernel in one step
    M, ng = 1024, 2
    x = np.arange(ng * GROUP, dtype=np.float64)
    out.append(_afar("all_at_step0_1024x2", M, ng, _z("grid", M, ng * GROUP), _with_ref([(M, M), (0, 0)], x), 400.0, chunks=4))
    # no row ever enters
    M, ng = 272, 5
    x = np.arange(ng * GROUP, dtype=np.float64)
    out.append(_afar("none_272x5", M, ng, _z("off_grid", M, ng * GROUP), _with_ref([(0, M)] * ng, x), 40.0, none=True))
    # far < done in both walks: the maximum holds (upwards 16 32 16 32 48; downwards 0 0 16 0 0)
    M, ng = 48, 5
    out.append(_afar("backwards_48x5", M, ng, _z("grid", M, ng * GROUP), _with_ref([(16, 48), (32, 48), (16, 32), (32, 48), (48, 48)], x),
                     200.0, backwards=True))
    # counts that are no multiples of 16: a step ends and the next begins inside a tile
    out.append(_afar("ragged_48x5", M, ng, _z("off_grid", M, ng * GROUP), _with_ref([(5, 40), (21, 40), (21, 47), (40, 47), (47, 48)], x),
                     200.0, ragged=True))
    # two excerpts joined: a gap in the frame times inside the fourth group, the inducing inputs behind it shifted with them
    M, ng = 272, 5
    N = ng * GROUP
    x = np.arange(N, dtype=np.float64)
    n0, shift = 3 * GROUP + 5 * 32 + 11, 4000.0
    z = _z("off_grid", M, N)
    z[z >= x[n0]] += shift
    x[n0:] += shift
    out.append(_afar("frame_gap_272x5", M, ng, z, af.ranges(z, x), 10.0, rule=True, gap=True))
    # NaN above W's diagonal: afar_t_kernel never reads those entries
    for M, ng, lay in ((272, 5, "off_grid"), (16, 2, "grid"), (1024, 2, "clustered")):
        N = ng * GROUP
        x = np.arange(N, dtype=np.float64)
        z = _z(lay, M, N)
        out.append(_afar("nan_above_%dx%d" % (M, ng), M, ng, z, af.ranges(z, x), 8.0 * max(N / M, 1.0), nan_above=True, rule=True))
    return out


def afar_counts(case, side):
    """rows entered by the end of each step of a walk (the running maximum), in walk order"""
    M, out, done = case["M"], [], 0
    for q in range(case["ng"]):
        S = case["ng"] - 1 - q if side else q
        far = M - case["rng"][S][1] if side else case["rng"][S][0]
        done = max(done, far)
        out.append(done)
    return out


def _qfar(name, M, nf, ng, z, x, ls, rng=None, seed=0, **marks):
    r = np.random.RandomState(seed + 3 * M + 5 * nf + ng)
    Q = r.randn(M, M)
    Q = 0.5 * (Q + Q.T)
    z, x = np.asarray(z, dtype=np.float64), np.asarray(x, dtype=np.float64)
    if rng is None:
        rng = qf.ranges(z, x, ls)
    return dict(name=name, M=M, nf=nf, ng=ng, N=ng * GROUP, z=z, x=x, ls=float(ls), rng=[tuple(t) for t in rng], Q=Q,
                fz=r.uniform(-1.0, 1.0, size=(nf, M)), **marks)


def qfar_cases():
    out = []
    layouts = ("grid", "off_grid", "clustered")
    # every M with every nf, ng in turn; the long walks (255 groups and more) at M = 64
    grid = [(64, 8, 1), (64, 40, 2), (64, 48, 3), (64, 64, 2), (128, 8, 3), (128, 40, 2), (128, 48, 1), (128, 64, 3),
            (1024, 8, 2), (1024, 40, 3), (1024, 48, 2), (1024, 64, 1),
            (64, 40, 255), (64, 8, 256), (64, 8, 257), (64, 8, 300)]
    for k, (M, nf, ng) in enumerate(grid):
        lay = layouts[k % 3]
        N = ng * GROUP
        x = np.arange(N, dtype=np.float64)
        z = _z(lay, M, N, wide=(lay != "clustered"))
        out.append(_qfar("%s_%dx%dx%d" % (lay, M, nf, ng), M, nf, ng, z, x, 6.0, rule=True, second_chunk=ng > 256))
    # the frame_gap layout: a gap of 400 lengthscales inside one 32-column strip; that group is all near between narrower neighbours
    M, nf, ng = 128, 40, 8
    N = ng * GROUP
    x = np.arange(N, dtype=np.float64)
    n0, ls = 3 * GROUP + 5 * 32 + 11, 6.0
    z = _z("off_grid", M, N)
    z[z >= x[n0]] += 400.0 * ls
    x[n0:] += 400.0 * ls
    out.append(_qfar("frame_gap_128x40x8", M, nf, ng, z, x, ls, rule=True, nonmonotone=True))
    # a lengthscale of the whole span: nothing is separable, every range is [0, M)
    M, nf, ng = 64, 8, 3
    x = np.arange(ng * GROUP, dtype=np.float64)
    out.append(_qfar("all_near_64x8x3", M, nf, ng, _z("grid", M, ng * GROUP), x, 4.0 * ng * GROUP, rule=True, none=True))
    # every row far from the first step: the inducing inputs all below the frames (T-), all above them (T+)
    M, nf, ng = 128, 48, 3
    x = np.arange(ng * GROUP, dtype=np.float64)
    out.append(_qfar("all_below_128x48x3", M, nf, ng, -40.0 - np.arange(M)[::-1] * 1.5, x, 6.0, rule=True, all_side=0))
    out.append(_qfar("all_above_128x48x3", M, nf, ng, ng * GROUP + 40.0 + np.arange(M) * 1.5, x, 6.0, rule=True, all_side=1))
    return out


def qfar_counts(case, side):
    M, out, done = case["M"], [], 0
    for q in range(case["ng"]):
        S = case["ng"] - 1 - q if side else q
        far = M - case["rng"][S][1] if side else case["rng"][S][0]
        done = max(done, far)
        out.append(done)
    return out


def qfar_rule_tables(case):
    """qfar_rule.tables at the case's ranges: the rule works its ranges out itself, and every case here carries the rule's own
    (rng is qfar_rule.ranges(z, x, ls)), so this is the plain call; T [ng][M][2 nf]"""
    _, T, _ = qf.tables(case["Q"], case["z"], case["x"], 1.0, case["ls"], case["fz"], np.zeros((case["nf"], case["N"])))
    return T


def afar_rule_tables(case):
    """afar_rule.tables of both factors in the device's layout T [ng][M][8]: W's four columns, then C's"""
    return np.concatenate([af.tables(case["W"], case["z"], case["rng"], case["ls"], lower=True),
                           af.tables(case["C"], case["z"], case["rng"], case["ls"])], axis=2)
