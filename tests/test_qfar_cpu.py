"""The far-field form of G = Q Kuf in numpy: Kuf by the strip builder's rule (product form on separable tiles,
sqrt(d^2 + 1e-12) elsewhere), a random symmetric Q, and G by the near rows plus the two far tables against the dense float64
product, both measured against the dense product in np.longdouble.  The bar is the project's "within 10 x the present
route": the new form's deviation over the scale of G at most ten times the dense float64 form's own."""
import numpy as np
import pytest

import qfar_rule as qf

M, N, NPART = 128, 2048, 20
FS = 16000.0
SPACING = (N // M) / FS                  # one inducing spacing on the grid: 16 frames
LS_SPACINGS = (4, 8, 25, 10000)
GAP_N0, GAP_LS = 3 * 256 + 5 * 32 + 11, 8
LAYOUTS = [(case, s) for s in LS_SPACINGS for case in ("on_grid", "off_grid", "clustered", "both_ends")] + [("frame_gap", GAP_LS)]


def _z(case):
    x = np.arange(N) / FS
    if case == "on_grid":
        z = x[::N // M].copy()
    elif case == "off_grid":
        z = x[::N // M] + 0.37 / FS
    elif case == "clustered":
        # eight clusters of 16 inducing inputs a frame and a bit apart: several z in one group, groups with none
        starts = np.array([0, 300, 330, 900, 1100, 1500, 1530, 2000]) / FS
        z = np.sort((starts[:, None] + (np.arange(16) * 1.3 / FS)[None, :]).reshape(-1))
    elif case == "both_ends":
        z = np.concatenate([x[:4 * 64:4], x[N - 4 * 64::4]])
    elif case == "frame_gap":
        # test_gpu_qfar.py's frame_gap layout (two excerpts joined): off-grid z, and every frame from GAP_N0 on — inside the sixth
        # strip of the fourth group — with every inducing input behind it shifted by 400 lengthscales of GAP_LS spacings
        z = x[::N // M] + 0.37 / FS
        t0, shift = x[GAP_N0], 400.0 * GAP_LS * SPACING
        x[GAP_N0:] += shift
        z[z >= t0] += shift
    else:
        raise ValueError(case)
    assert z.shape == (M,) and np.all(z[1:] >= z[:-1])
    return x, z


def _case(case, ls_spacings, seed=3):
    rng = np.random.RandomState(seed)
    x, z = _z(case)
    var, ls = 0.7, ls_spacings * SPACING
    energy = rng.uniform(0.2, 1.0, NPART) / NPART
    freq = 110.0 * np.arange(1, NPART + 1) * (1.0 + 0.001 * rng.standard_normal(NPART))
    fz, fx = qf.features(energy, freq, z), qf.features(energy, freq, x)
    Q = rng.standard_normal((M, M))
    Q = 0.5 * (Q + Q.T)
    K = qf.kuf_builder(z, x, var, ls, fz, fx)
    return x, z, var, ls, fz, fx, Q, K


@pytest.fixture(scope="module")
def side_counts():
    return {}


@pytest.mark.parametrize("case,ls_spacings", LAYOUTS)
def test_far_form_within_ten_times_the_dense_form(case, ls_spacings, side_counts):
    x, z, var, ls, fz, fx, Q, K = _case(case, ls_spacings)
    rng, T, Psi = qf.tables(Q, z, x, var, ls, fz, fx)
    if case == "frame_gap":
        # the strip with the gap spans more than 300 lengthscales: its group is all near between narrower neighbours, so the
        # running maxima of the T recurrence (qfar_t_kernel's) hold rows that group's own range does not call far
        assert [(kb, ke) for kb, ke, _, _ in rng] == [(0, 32), (0, 48), (16, 64), (0, 128), (48, 96), (64, 112), (80, 128), (96, 128)]
    side_counts[(case, ls_spacings)] = qf.sides(rng, M)
    g_new, g_dense = qf.g_far(Q, K, rng, T, Psi), qf.g_dense(Q, K)
    ref = Q.astype(np.longdouble) @ K.astype(np.longdouble)
    scale = float(np.abs(ref).max())
    d_new = float(np.abs(g_new - ref).max()) / scale
    d_dense = float(np.abs(g_dense - ref).max()) / scale
    print("%s l = %d spacings: far form %.3e, dense float64 %.3e of the scale of G; groups (both, one, none) %s"
          % (case, ls_spacings, d_new, d_dense, side_counts[(case, ls_spacings)]))
    if ls_spacings == 10000:
        # the lengthscale spans the window: every near range is [0, M), the second loop never runs
        assert all(kb == 0 and ke == M for kb, ke, _, _ in rng)
        assert np.array_equal(g_new, g_dense)
    assert d_new <= 10.0 * d_dense, (d_new, d_dense)


def test_the_cases_cover_every_kind_of_group():
    """from the range rule alone: groups with far rows on both sides, on one side and on neither"""
    both = one = none = 0
    for case in ("on_grid", "off_grid", "clustered", "both_ends"):
        for s in LS_SPACINGS:
            x, z = _z(case)
            b, o, n = qf.sides(qf.ranges(z, x, s * SPACING), M)
            both, one, none = both + b, one + o, none + n
    assert both > 0 and one > 0 and none > 0, (both, one, none)


def test_every_far_entry_is_one_the_builder_wrote_as_a_product():
    """the range rule calls a row far for a group only where the builder's rule separates its tile from every strip of it"""
    for case in ("on_grid", "clustered"):
        x, z = _z(case)
        ls = 8 * SPACING
        a, b = z / ls, x / ls
        for S, (kb, ke, _, _) in enumerate(qf.ranges(z, x, ls)):
            bs = b[S * qf.GROUP:(S + 1) * qf.GROUP].reshape(-1, qf.STRIP)
            for w in range(bs.shape[0]):
                if kb > 0:
                    assert bs[w].min() - a[:kb].max() >= qf.SEP
                if ke < M:
                    assert a[ke:].min() - bs[w].max() >= qf.SEP
