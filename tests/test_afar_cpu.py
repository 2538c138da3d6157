"""The activations' far field in numpy, in the kernels' order (afar_rule.py): A = W Kuf and C Kuf, C = tril(Lq)^T W,
from the near rows of a Matern-3/2 strip plus the exact rank-4 far field, against the dense float64 products — both measured
against the np.longdouble product of the same float64 left factor with the strip evaluated in np.longdouble (the far form
rounds the far entries of the strip another way than the builder does; neither rounding is the better one).  W is the inverse
Cholesky factor of Kuu + 1e-6 I, at 250 spacings with cond_2 ~ 4e8: the far form multiplies through it once, as the dense form does.

The bar is a ratio to the dense form's own deviation.  Measured over the cases below (printed by the test): 0.97 - 1.39 for A,
0.40 - 1.88 for the two column sums.  RATIO_MAX = 4 leaves a factor of about 2 for a BLAS that sums in another order.  Without
the kappa = 1 - 1.5e-12 term of the far entries the ratio for A is about 2000: the last test."""
import numpy as np
import pytest

import afar_rule as af

M, N = 128, 8192
FS = 16000.0
SPACING = (N // M) / FS                  # one inducing spacing on the grid: 64 frames, 4 ms
LS_SPACINGS = (8, 250)                   # the suites' LS_ACT, and the benchmark's l = 1 s
LAYOUTS = ("on_grid", "off_grid", "clustered", "frame_gap")
GAP_N0 = 3 * 256 + 5 * 32 + 11
VAR, JITTER = 3.5, 1e-6
RATIO_MAX = 4.0


def layout(case, ls):
    x = np.arange(N) / FS
    if case == "on_grid":
        z = x[::N // M].copy()
    elif case == "off_grid":
        z = x[::N // M] + 1e-7
    elif case == "clustered":
        # eight clusters of 16 inducing inputs 5.3 frames apart: several tiles in one group, most groups with none
        starts = np.array([0, 300, 530, 2000, 2100, 5000, 5090, 8000]) / FS
        z = np.sort((starts[:, None] + (np.arange(16) * 5.3 / FS)[None, :]).reshape(-1))
    elif case == "frame_gap":
        # two excerpts joined: every frame from GAP_N0 on, and every inducing input behind it, shifted by 400 lengthscales
        z = x[::N // M] + 0.37 / FS
        t0, shift = x[GAP_N0], 400.0 * ls
        x[GAP_N0:] += shift
        z[z >= t0] += shift
    else:
        raise ValueError(case)
    assert z.shape == (M,) and np.all(z[1:] >= z[:-1])
    return x, z


def factors(z, ls, seed=3):
    rs = np.random.RandomState(seed)
    d = (z[:, None] - z[None, :]) / ls
    r = np.sqrt(d * d + 1e-12)
    Kuu = VAR * (1.0 + af.SQRT3 * r) * np.exp(-af.SQRT3 * r) + JITTER * np.eye(M)
    L = np.linalg.cholesky(Kuu)
    W = np.tril(np.linalg.solve(L, np.eye(M)))
    Lq = np.tril(0.3 * rs.standard_normal((M, M)) / np.sqrt(M)) + np.eye(M)
    return W, np.triu(Lq.T) @ W


def deviations(case, s, kappa=af.KAPPA):
    """{quantity: (far form's deviation, dense float64 form's) over the reference's scale}, and the ranges"""
    ls = s * SPACING
    x, z = layout(case, ls)
    W, Cm = factors(z, ls)
    K = af.kuf(z, x, VAR, ls)
    rng = af.ranges(z, x)
    Psi = af.psi(x, rng, VAR, ls, kappa)
    Kl = af.kuf(z, x, VAR, ls, np.longdouble)           # the strip itself in long double: the far form is another rounding of it
    out = {}
    for name, X, lower in (("A", W, True), ("CK", Cm, False)):
        far = af.product_far(X, K, rng, af.tables(X, z, rng, ls, lower), Psi, lower)
        dense = X @ K
        ref = X.astype(np.longdouble) @ Kl
        cs_ref = (ref * ref).sum(axis=0)
        sc, cs_sc = float(np.abs(ref).max()), float(np.abs(cs_ref).max())
        if name == "A":
            out["A"] = (float(np.abs(far - ref).max()) / sc, float(np.abs(dense - ref).max()) / sc)
        out["colsum(%s^2)" % name] = (float(np.abs((far * far).sum(axis=0) - cs_ref).max()) / cs_sc,
                                      float(np.abs((dense * dense).sum(axis=0) - cs_ref).max()) / cs_sc)
    return out, rng


@pytest.mark.parametrize("s", LS_SPACINGS)
@pytest.mark.parametrize("case", LAYOUTS)
def test_far_form_deviates_like_the_dense_form(case, s):
    out, rng = deviations(case, s)
    assert af.is_monotone(rng)
    assert any(kb > 0 for kb, _, _, _ in rng) and any(ke < M for _, ke, _, _ in rng)
    if case == "clustered":
        assert any(kb == ke for kb, ke, _, _ in rng)                 # groups with no near row
        assert max(ke - kb for kb, ke, _, _ in rng) >= 2 * af.TILE
    else:
        assert max(ke - kb for kb, ke, _, _ in rng) <= 2 * af.TILE   # 4 inducing inputs per group: one or two tiles
    for name, (d_far, d_dense) in out.items():
        print("%s l = %d spacings, %s: far form %.3e, dense float64 %.3e of scale, ratio %.2f" % (case, s, name, d_far, d_dense, d_far / d_dense))
        assert d_far <= RATIO_MAX * d_dense, (name, d_far, d_dense)


def test_one_group_holding_every_row_is_the_dense_sum():
    """a group whose span holds every inducing input has no far row: the far tables are zero and the rows are summed in order"""
    x = np.arange(af.GROUP) / FS
    z = np.linspace(x[3], x[-3], 32)
    rng = af.ranges(z, x)
    assert [(kb, ke) for kb, ke, _, _ in rng] == [(0, 32)]
    X = np.random.RandomState(1).standard_normal((32, 32))
    assert not af.tables(X, z, rng, 0.01).any()


@pytest.mark.parametrize("s", LS_SPACINGS)
def test_without_kappa_the_far_entries_are_off(s):
    """every far entry without the 1 - 1.5e-12 term is off by 1.5e-12 var e^{-c rho}, and W multiplies that by up to ~7e2"""
    out, _ = deviations("on_grid", s, kappa=1.0)
    d_far, d_dense = out["A"]
    print("on_grid l = %d spacings, A without kappa: far form %.3e, dense float64 %.3e of scale, ratio %.1f" % (s, d_far, d_dense, d_far / d_dense))
    assert d_far > 10.0 * RATIO_MAX * d_dense
