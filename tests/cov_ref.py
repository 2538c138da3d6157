"""Plain references of the covariance builds of cov.hip (numpy only; shared by tests/test_cov_ref_cpu.py and
tests/test_gpu_cov.py).

Two references, chosen by the range of a = x / lengthscale:

* ``oracle(kern, x1, x2)``: oracle.gpflow05.K, the reference's operation order in float64 (the expanded square
  -2ab + a^2 + b^2).  The bar wherever max |a| <= ORACLE_RANGE = 256, at RTOL / ATOL = 1e-11 / 1e-12.
* ``closed_form(kern, z, x)``: var * env(sqrt((a - b)^2 + 1e-12)) * sum_p e_p cos(2 pi f_p (z - x)) in np.longdouble
  (the phases 2 pi f_p x rounded to float64 as the features round them).
  Beyond that range the expanded square cancels (|a| = 1280: a^2 ~ 1.6e6, one rounding of it is 2e-10 absolute in r^2)
  and the ORACLE is the less accurate side; the device is then compared with the closed form.  Within the range the two
  agree at the tolerance on every entry at least a lengthscale apart (``far_entries``); nearer, the same cancellation is
  divided by a small r and the oracle, being the reference's arithmetic, is the definition.

``emulate(kern, z, x)`` evaluates the DEVICE's formulas in numpy float64: entry by entry inside the band (the expanded
square, as cov_mercer_entry), the separable product per 16-row tile and 32-column wavefront outside it, by the predicate of
cov_entry.h (``tile_classes``).  Its largest deviation from the closed form, in units of the tolerance, is what a beyond-range
case records as `measured`, separately for the entries of separable tiles and for the entry-by-entry tiles (whose expanded
square cancels as the oracle's does); the device gets 4 times each (matrix-core summation order, 1-2 ulp of sincos and exp).
"""
import numpy as np

from oracle import gpflow05 as orc

LD = np.longdouble
RTOL, ATOL = 1e-11, 1e-12
ORACLE_RANGE = 256.0
CVM_SEP = 1.0            # cov_entry.h
SEP_ROWS, SEP_COLS = 16, 32
KT = {"matern12": 0, "matern32": 1, "matern52": 2, "rbf": 3, "mercer_matern12sm": 4, "matern12sm": 5, "matern32sm": 6,
      "mercer_matern52sm": 7}
MERCER = ("mercer_matern12sm", "mercer_matern52sm")
S5 = 2.23606797749979


def sm_mpad(m):
    return 0 if m <= 0 else (m + 3) // 4 * 4


def theta(k):
    return np.array([k["variance"], k["lengthscales"]] + list(k["energy"]) + list(k["frequency"]), dtype=np.float64)


def oracle(kern, x1, x2=None):
    x1 = np.asarray(x1, dtype=np.float64).reshape(-1, 1)
    return orc.K(kern, x1, None if x2 is None else np.asarray(x2, dtype=np.float64).reshape(-1, 1))


def amax(kern, *xs):
    return max(float(np.max(np.abs(x))) for x in xs) / kern["lengthscales"]


def units(got, ref, mask=None):
    """largest error in units of the tolerance RTOL |ref| + ATOL (over the entries of `mask`; 0 for none)"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    if mask is not None:
        got, ref = got[mask], ref[mask]
    if got.size == 0:
        return 0.0
    return float(np.max(np.abs(got - ref) / (ATOL + RTOL * np.abs(ref))))


def closed_form(kern, z, x):
    """the Mercer kernels in long double: no expanded square, the feature dot product summed as cosines of the phase
    difference.  The phases are the float64 arguments of cov_sm_feature, fl(fl(2 pi f) x) (the reference rounds them the
    same way, and at 2 pi f x ~ 1e6 that rounding is 1e-10 of a radian): sum_q e_q cos(A_q(z) - A_q(x)) is then exactly
    what the feature products Phi(z)^T Phi(x) stand for."""
    assert kern["type"] in MERCER
    z64, x64 = np.asarray(z, dtype=np.float64).ravel(), np.asarray(x, dtype=np.float64).ravel()
    l = LD(kern["lengthscales"])
    d = z64.astype(LD)[:, None] / l - x64.astype(LD)[None, :] / l
    r = np.sqrt(d * d + LD(1e-12))
    if kern["type"] == "mercer_matern12sm":
        env = np.exp(-r)
    else:
        s5 = np.sqrt(LD(5))
        env = (1 + s5 * r + LD(5) / LD(3) * r * r) * np.exp(-s5 * r)
    # cos(A - B) = cos A cos B + sin A sin B, every factor and the sum over partials in long double
    fz, fx = feature_table(kern, z64, len(kern["frequency"])), feature_table(kern, x64, len(kern["frequency"]))
    return LD(kern["variance"]) * env * (fz.T @ fx)


def far_entries(kern, z, x):
    """entries at least CVM_SEP lengthscales apart.  Only there do the two references agree at the tolerance: nearer, the
    oracle's expanded square -2ab + a^2 + b^2 carries a rounding of a^2 (absolute eps a^2 in r^2, so eps a^2 / (2 r) in r), which
    is the reference's own arithmetic and what the device reproduces entry by entry."""
    l = kern["lengthscales"]
    a, b = np.asarray(z, dtype=np.float64).ravel() / l, np.asarray(x, dtype=np.float64).ravel() / l
    return np.abs(a[:, None] - b[None, :]) >= CVM_SEP


def separable_entries(kern, z, x):
    """entries of the tiles the matrix-core builders write in product form"""
    cls, _ = tile_classes(kern, z, x)
    n1, n2 = np.asarray(z).size, np.asarray(x).size
    return np.repeat(np.repeat(cls != 0, SEP_ROWS, 0), SEP_COLS, 1)[:n1, :n2]


def tile_classes(kern, z, x):
    """per (16-row tile, 32-column wavefront) of the matrix-core builders: +1 separable with the rows above the columns,
    -1 below, 0 entry by entry (the predicate of cov_entry.h, in the device's float64 arithmetic); and which of the
    entry-by-entry tiles straddle the band (hold entries on both sides of |a - b| = CVM_SEP)"""
    l = kern["lengthscales"]
    s = 1.0 if kern["type"] == "mercer_matern12sm" else S5
    a = np.asarray(z, dtype=np.float64).ravel() / l
    b = np.asarray(x, dtype=np.float64).ravel() / l
    nt, nw = -(-a.size // SEP_ROWS), -(-b.size // SEP_COLS)
    # rows / columns past the end repeat the last one, as the kernels clamp them
    ap = np.concatenate([a, np.full(nt * SEP_ROWS - a.size, a[-1])]).reshape(nt, SEP_ROWS)
    bp = np.concatenate([b, np.full(nw * SEP_COLS - b.size, b[-1])]).reshape(nw, SEP_COLS)
    lo, hi = ap.min(1)[:, None], ap.max(1)[:, None]
    bmin, bmax = bp.min(1)[None, :], bp.max(1)[None, :]
    ok = s * (bmax - bmin) < 300.0
    above = ok & (lo - bmax >= CVM_SEP)
    below = ok & (bmin - hi >= CVM_SEP)
    cls = above.astype(np.int8) - below.astype(np.int8)
    # closest and farthest pair of a tile, from the two ranges
    gap = np.maximum(np.maximum(lo - bmax, bmin - hi), 0.0)
    far = np.maximum(hi - bmin, bmax - lo)
    straddle = (cls == 0) & (gap < CVM_SEP) & (far >= CVM_SEP)
    return cls, straddle


def geometry(kern, z, x):
    cls, straddle = tile_classes(kern, z, x)
    return {"tiles": int(cls.size), "separable": int(np.count_nonzero(cls)), "straddle": int(np.count_nonzero(straddle))}


def emulate(kern, z, x):
    """the matrix-core builders' formulas in numpy float64 (the feature dot product as one float64 matmul)"""
    assert kern["type"] in MERCER
    l, var = kern["lengthscales"], kern["variance"]
    env52 = kern["type"] != "mercer_matern12sm"
    s = S5 if env52 else 1.0
    z = np.asarray(z, dtype=np.float64).ravel()
    x = np.asarray(x, dtype=np.float64).ravel()
    a, b = z / l, x / l
    acc = orc.phi_features(kern, z.reshape(-1, 1)).T @ orc.phi_features(kern, x.reshape(-1, 1))
    # inside the band: ((-2 (a b)) + a a) + b b, every operation rounded on its own
    r = np.sqrt(((-2.0 * (a[:, None] * b[None, :]) + (a * a)[:, None]) + (b * b)[None, :]) + 1e-12)
    env = np.exp(-s * r)
    if env52:
        env = (1.0 + s * r + (5.0 / 3.0) * (r * r)) * env
    out = var * env * acc
    cls, _ = tile_classes(kern, z, x)
    for t, w in zip(*np.nonzero(cls)):
        rs, cs = slice(t * SEP_ROWS, min((t + 1) * SEP_ROWS, a.size)), slice(w * SEP_COLS, min((w + 1) * SEP_COLS, b.size))
        at, bw = a[rs], b[cs]
        bcl = b[w * SEP_COLS:(w + 1) * SEP_COLS]
        if cls[t, w] > 0:
            bmax = bcl.max()
            e = np.exp(-s * (at - bmax))[:, None] * (var * np.exp(-s * (bmax - bw)))[None, :]
        else:
            bmin = bcl.min()
            e = np.exp(-s * (bmin - at))[:, None] * (var * np.exp(-s * (bw - bmin)))[None, :]
        if env52:
            rr = np.abs(at[:, None] - bw[None, :])
            e = e * (1.0 + s * rr + (5.0 / 3.0) * (rr * rr))
        out[rs, cs] = e * acc[rs, cs]
    return out


def feature_table(kern, x, mpad):
    """[2 mpad][n] as sm_features_kernel writes it, in long double from the float64-rounded argument of cov_sm_feature:
    arg = fl(fl(2 pi f) x); rows q < m: sqrt(e_q) cos(arg), rows mpad + q: sqrt(e_q) sin(arg); the rest exactly zero"""
    x = np.asarray(x, dtype=np.float64).ravel()
    m = len(kern["frequency"])
    tab = np.zeros((2 * mpad, x.size), dtype=LD)
    for q in range(m):
        arg = ((6.283185307179586 * np.float64(kern["frequency"][q])) * x).astype(LD)
        se = np.sqrt(LD(kern["energy"][q]))
        tab[q], tab[mpad + q] = se * np.cos(arg), se * np.sin(arg)
    return tab
