"""The far-field form of Qbar = Kuf D Kuf^T and v = Kuf gm in numpy: Kuf by the strip builder's rule, a column
scale d of mixed sign, and the form of qbar_rule (per-group Gram blocks, recurrences over the groups, assembly per tile pair)
against the dense float64 product, both measured against the product in np.longdouble.  The bar is the project's "within 10 x the
present route".  Shapes: M = 128, N = 2048; m = 20 at 4, 8 and 25 spacings, m = 3 at 2 spacings (nf = 8, the largest bmax - bmin in
lengthscales: an undecayed below x above sum would overflow there), 10 000 spacings (every range [0, M))."""
import numpy as np
import pytest

import qfar_rule as qf
import qbar_rule as qb

M, N = 128, 2048
FS = 16000.0
SPACING = (N // M) / FS
GAP_N0, GAP_LS = 3 * 256 + 5 * 32 + 11, 8

# layout -> (inducing inputs, one spacing of theirs in seconds)
def _z(layout):
    x = np.arange(N) / FS
    if layout == "on_grid":
        return x, x[::N // M].copy(), SPACING
    if layout == "off_grid":
        return x, x[::N // M] + 0.37 / FS, SPACING
    if layout == "frame_gap":
        # test_gpu_qfar.py's frame_gap layout (two excerpts joined): off-grid z, and every frame from GAP_N0 on — inside the sixth
        # strip of the fourth group — with every inducing input behind it shifted by 400 lengthscales of GAP_LS spacings
        z = x[::N // M] + 0.37 / FS
        t0, shift = x[GAP_N0], 400.0 * GAP_LS * SPACING
        x[GAP_N0:] += shift
        z[z >= t0] += shift
        return x, z, SPACING
    # test_gpu_qfar.py's clustered and gap layouts over eight groups: several inducing inputs per group, groups with none
    step, per = {"clustered": (5.8, [44, 42, 0, 42, 0, 0, 0, 0]), "gap": (5.2, [48, 32, 0, 0, 48, 0, 0, 0])}[layout]
    z = np.concatenate([(g * 256 + 0.37 + step * np.arange(k)) / FS for g, k in enumerate(per)])
    assert z.shape == (M,) and np.all(z[1:] >= z[:-1])
    return x, z, step / FS


CASES = [(lay, ls, 20) for lay in ("on_grid", "off_grid", "clustered", "gap") for ls in (4, 8, 25)]
CASES += [(lay, 2, 3) for lay in ("on_grid", "off_grid", "clustered", "gap")]
CASES += [("on_grid", 10000, 20), ("gap", 10000, 3)]
CASES += [("frame_gap", GAP_LS, 20)]         # ranges that are not monotone: the widening changes them


@pytest.mark.parametrize("layout,ls_spacings,m", CASES)
def test_far_form_within_ten_times_the_dense_form(layout, ls_spacings, m):
    rs = np.random.RandomState(3)
    x, z, spacing = _z(layout)
    var, ls = 0.7, ls_spacings * spacing
    energy = rs.uniform(0.2, 1.0, m) / m
    freq = 110.0 * np.arange(1, m + 1) * (1.0 + 0.001 * rs.standard_normal(m))
    fz, fx = qf.features(energy, freq, z), qf.features(energy, freq, x)
    K = qf.kuf_builder(z, x, var, ls, fz, fx)
    d, gm = rs.standard_normal(N), rs.standard_normal(N)            # mixed sign
    Q, v, rng = qb.qbar_far(K, d, gm, z, x, var, ls, fz, fx)
    if layout == "frame_gap":
        # the group with the gap is all near between narrower neighbours: widened, kb = 0 up to it and ke = M from it on
        assert not qb.is_monotone(rng), [(kb, ke) for kb, ke, _, _ in rng]
        assert qb.monotone(rng) == ([0, 0, 0, 0, 48, 64, 80, 96], [32, 48, 64, 128, 128, 128, 128, 128])
    else:
        assert qb.is_monotone(rng), [(kb, ke) for kb, ke, _, _ in rng]
    if layout == "gap":
        assert ls_spacings == 10000 or any(kb == ke for kb, ke, _, _ in rng)
    if ls_spacings == 10000:
        assert all(kb == 0 and ke == M for kb, ke, _, _ in rng)
    Kl = K.astype(np.longdouble)
    ref, vref = (Kl * d.astype(np.longdouble)) @ Kl.T, Kl @ gm.astype(np.longdouble)
    dense, vdense = (K * d) @ K.T, K @ gm
    scale, vscale = float(np.abs(ref).max()), float(np.abs(vref).max())
    d_new, d_dense = float(np.abs(Q - ref).max()) / scale, float(np.abs(dense - ref).max()) / scale
    v_new, v_dense = float(np.abs(v - vref).max()) / vscale, float(np.abs(vdense - vref).max()) / vscale
    print("%s l = %d spacings m = %d: Qbar far form %.3e, dense float64 %.3e (%.2f x); v %.3e, dense %.3e (%.2f x); groups (both, one, none) %s"
          % (layout, ls_spacings, m, d_new, d_dense, d_new / d_dense, v_new, v_dense, v_new / v_dense, qf.sides(rng, M)))
    assert np.array_equal(Q, Q.T)
    assert d_new <= 10.0 * d_dense, (d_new, d_dense)
    assert v_new <= 10.0 * v_dense, (v_new, v_dense)


def test_widening_makes_any_ranges_monotone_and_never_narrows_them():
    rng = [(32, 96, 0.0, 0.0), (0, 128, 0.0, 0.0), (48, 80, 0.0, 0.0), (64, 112, 0.0, 0.0)]
    kb, ke = qb.monotone(rng)
    assert kb == [0, 0, 48, 64] and ke == [96, 128, 128, 128]
    assert all(k <= r[0] and e >= r[1] for k, e, r in zip(kb, ke, rng))
    S0, Sa = qb.tile_tables(kb, ke, 128)
    assert S0 == [2, 2, 2, 3, 4, 4, 4, 4] and Sa == [0] * 6 + [1, 1]
