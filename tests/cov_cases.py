"""The case list of the covariance-build operator tests: shared by tests/test_cov_ref_cpu.py (geometry, references,
the measured bars) and tests/test_gpu_cov.py (the launches).  numpy only; inputs are generated from seeds, never stored.

Frames are at 16 kHz.  The lengthscale sets the geometry of a matrix-core case: l = 0.05 a wide band, l = 0.01 mostly
separable tiles, l = 1.0 no separable tile.  A case meant to test the separable envelope (kind "envelope") must hold at
least MIN_TILES separable tiles and as many that straddle the band; kind "nosep" must hold no separable tile;
tests/test_cov_ref_cpu.py counts them.

ref "oracle": max |x / l| <= 256, the bar is oracle.gpflow05.K at 1e-11 / 1e-12.  ref "closed": beyond that range; the bar
is the long-double closed form of tests/cov_ref.py at `bar` units of that tolerance, bar = 4 * measured, where `measured`
is the largest deviation of the float64 emulation of the device's formulas from the closed form, computed on the CPU
(tests/test_cov_ref_cpu.py recomputes it and holds the recorded figure to it).
"""
import numpy as np

FS = 16000.0
MIN_TILES = 64
M12, M52 = "mercer_matern12sm", "mercer_matern52sm"


def kernel(ktype, m, l, seed=0, variance=1.3):
    """a kernel dict of the oracle; energies normalised, partials near the harmonics of 110 Hz"""
    rng = np.random.RandomState(1000 + 7 * seed + m)
    if ktype in ("matern12", "matern32", "matern52", "rbf"):
        return {"type": ktype, "variance": variance, "lengthscales": l, "energy": [], "frequency": []}
    e = rng.rand(m) + 0.2
    f = 110.0 * (np.arange(m) + 1) * (1.0 + 0.01 * rng.rand(m))
    return {"type": ktype, "variance": variance, "lengthscales": l, "energy": list(e / e.sum()), "frequency": list(f)}


def frames(n2, order="asc", seed=0):
    x = np.arange(n2) / FS
    if order == "desc":
        x = x[::-1].copy()
    elif order == "shuffled":
        x = x[np.random.RandomState(77 + seed).permutation(n2)]
    return x


def inducing(n1, xmax, order="blocks", seed=0):
    """n1 inducing inputs in [0, xmax].  "blocks": sorted, then the 16-row tiles permuted and the rows of each tile permuted
    (tight tile ranges, nothing monotone); "random": no order at all; "sorted": ascending"""
    rng = np.random.RandomState(31 + seed)
    z = np.sort(rng.rand(n1)) * xmax
    if order == "random":
        return z[rng.permutation(n1)]
    if order == "blocks":
        nt = -(-n1 // 16)
        tiles = [z[16 * t:16 * t + 16] for t in rng.permutation(nt)]
        return np.concatenate([t[rng.permutation(t.size)] for t in tiles])
    return z


def threshold_inputs():
    """l = 1 and inputs on the binary grid 1 / 16, so that a = z and b = x are exact: 4096 frames x_j = j / 16 (a wavefront w
    holds [2 w, 2 w + 31 / 16]); 16 row tiles z = base_t + q / 16 with, by t % 4,
      0: base = 2 w + 31/16 + 1          tile_lo - bmax == 1.0 exactly for wavefront w           (separable above)
      1: base = 2 w + 31/16 + 1 - 1/16   one grid step short                                      (entry by entry)
      2: base = 2 w - 15/16 - 1          bmin - tile_hi == 1.0 exactly                            (separable below)
      3: base = 2 w - 15/16 - 1 + 1/16   one grid step short                                      (entry by entry)
    with w = 8 t + 4.  Returns z, x and the (tile, wavefront, expected class) triples."""
    x = np.arange(4096) / 16.0
    z, expect = [], []
    for t in range(16):
        w = 8 * t + 4
        base = [2 * w + 31 / 16.0 + 1, 2 * w + 31 / 16.0 + 1 - 1 / 16.0, 2 * w - 15 / 16.0 - 1, 2 * w - 15 / 16.0 - 1 + 1 / 16.0][t % 4]
        expect.append((t, w, [1, 0, -1, 0][t % 4]))
        z.append(base + np.arange(16) / 16.0)
    return np.concatenate(z), x, expect


def mfma_inputs(c):
    """kernels (one per record), inducing inputs (one per record) and the shared frames of a matrix-core case"""
    if c.get("threshold"):
        z, x, _ = threshold_inputs()
        return [kernel(c["type"], c["recs"][0][1], 1.0, seed=5)], [z], x
    x = frames(c["n2"], c.get("x_order", "asc"))
    kerns = [kernel(c["type"], m, c["l"], seed=k) for k, (n1, m) in enumerate(c["recs"])]
    zs = [inducing(n1, float(x.max()), c.get("z_order", "blocks"), seed=k) for k, (n1, m) in enumerate(c["recs"])]
    return kerns, zs, x


def _mc(name, recs, n2, l, es, form, row_seg, kind="any", ref="oracle", **kw):
    d = dict(name=name, recs=recs, n2=n2, l=l, es=es, form=form, row_seg=row_seg, kind=kind, ref=ref)
    d.update(kw)
    return d


# name, records (n1, m), n2, lengthscale, engine_strips, the form and row segment the launch must report, geometry, reference.
# ld_pad: leading dimension n2 + ld_pad; misalign: the output is 8-byte but not 16-byte aligned; f32: float32 strips
_MFMA_SHAPES = [
    # ---- staged, whole tiles: two row segments ----
    _mc("staged_whole_l05", [(256, 3)], 4096, 0.05, 1, 1, 128, "envelope"),
    _mc("staged_whole_l01", [(256, 3)], 4096, 0.01, 1, 1, 128, "envelope"),
    _mc("staged_whole_l1", [(256, 3)], 4096, 1.0, 1, 1, 128, "nosep"),
    # ---- staged, ragged: last row tile of 10 rows, wavefronts wholly and partly past n2, n2 odd ----
    _mc("staged_ragged_scalar", [(250, 3)], 4199, 0.01, 0, 1, 256, "envelope"),                       # ld odd: scalar stores
    _mc("staged_ragged_vector", [(250, 3)], 4199, 0.01, 0, 1, 256, "envelope", ld_pad=1),            # vector stores, j + 1 < n2 tail
    _mc("staged_ragged_misaligned", [(250, 3)], 4199, 0.01, 0, 1, 256, "envelope", ld_pad=1, misalign=1),
    _mc("staged_ragged_f32", [(250, 3)], 4199, 0.01, 0, 1, 256, "envelope", ld_pad=1, f32=1),
    _mc("staged_ragged_two_segments", [(300, 3)], 4199, 0.01, 0, 1, 192, "envelope", ld_pad=1),     # second segment: 108 rows
    # ---- staged, one segment, although n2 % 128 == 0 (no engine strips) ----
    _mc("staged_one_segment", [(200, 3)], 5376, 0.01, 0, 1, 256, "envelope"),
    # ---- lean ----
    _mc("lean_m12_l05", [(256, 12)], 4096, 0.05, 1, 2, 128, "envelope"),
    _mc("lean_m12_l01", [(256, 12)], 4096, 0.01, 1, 2, 128, "envelope"),
    _mc("lean_m12_l1", [(256, 12)], 4096, 1.0, 1, 2, 128, "nosep"),
    _mc("lean_m20", [(256, 20)], 4096, 0.01, 1, 2, 128, "envelope"),
    _mc("lean_m32", [(256, 32)], 4096, 0.01, 1, 2, 128, "envelope"),
    _mc("lean_m12_f32", [(256, 12)], 4096, 0.01, 2, 2, 128, "envelope", f32=1),
    _mc("lean_m5_f32", [(256, 5)], 4096, 0.01, 2, 2, 128, "envelope", f32=1),                      # float32 strips: lean from mpad 8
    _mc("staged_m5_f64", [(256, 5)], 4096, 0.01, 1, 1, 128, "envelope"),                           # float64 strips: mpad 8 stays staged
    _mc("lean_z_random", [(256, 12)], 4096, 0.01, 1, 2, 128, "any", z_order="random"),
    _mc("lean_frames_desc", [(256, 12)], 4096, 0.01, 1, 2, 128, "envelope", x_order="desc"),
    _mc("lean_frames_shuffled", [(256, 12)], 4096, 0.01, 1, 2, 128, "any", x_order="shuffled"),
    _mc("lean_threshold", [(256, 12)], 4096, 1.0, 1, 2, 128, "any", threshold=1),
    # ---- lean, row segments: 1036 rows in segments of 192, the last one 76 rows = 5 tiles, the last tile 12 rows ----
    _mc("lean_segments", [(1036, 12)], 1024, 0.001, 1, 2, 192, "envelope"),
    _mc("lean_segments_two_records", [(1036, 12), (300, 9)], 1024, 0.001, 1, 2, 192, "envelope"),   # segments past 300 rows write nothing
    # ---- lean falls back: n2 % 128 != 0 ----
    _mc("lean_fallback", [(256, 12)], 4100, 0.01, 1, 1, 128, "envelope"),
    # ---- beyond the oracle's range: the long-double closed form at 4 * measured ----
    # frames shuffled, l = 5e-4 (|a| to 512): the column-range test s (bmax - bmin) < 300 refuses every tile
    _mc("lean_shuffled_l5e-4", [(256, 12)], 4096, 5e-4, 1, 2, 128, "nosep", ref="closed", x_order="shuffled"),
    # l = 2e-4: |a| reaches 1280
    _mc("lean_l2e-4", [(256, 12)], 4096, 2e-4, 1, 2, 128, "envelope", ref="closed"),
]

# measured: the largest deviation of the float64 emulation of the device's formulas from the long-double closed form, in units
# of 1e-11 |ref| + 1e-12, computed on the CPU (tests/test_cov_ref_cpu.py), as (entries of separable tiles, entries of
# entry-by-entry tiles); bar = 4 * measured, what the device is held to.  The entry-by-entry figure is the cancellation of the
# expanded square -2ab + a^2 + b^2 at |a| up to 512 / 1280, divided by the small r of near-coincident points: the reference's
# own arithmetic (the oracle deviates from the closed form by the same figure).  The Matern-5/2 profile is flat at r = 0, so
# it feels that error in second order only.
CLOSED_BARS = {
    #                               measured (separable, entry by entry)   bar (separable, entry by entry)
    ("lean_shuffled_l5e-4", M12): ((0.0, 2666.40), (0.0, 10665.6)),        # no separable tile
    ("lean_shuffled_l5e-4", M52): ((0.0, 3.602), (0.0, 14.408)),
    ("lean_l2e-4", M12): ((0.0105, 12621.9), (0.042, 50487.6)),
    ("lean_l2e-4", M52): ((0.0164, 22.483), (0.0656, 89.932)),
}

MFMA_CASES = []
for _t in (M12, M52):
    for _c in _MFMA_SHAPES:
        _d = dict(_c, type=_t, id="%s-%s" % (_c["name"], "m12" if _t == M12 else "m52"))
        if _d["ref"] == "closed":
            _d["measured"], _d["bar"] = CLOSED_BARS[(_c["name"], _t)]
        MFMA_CASES.append(_d)
LEAN_CASES = [c for c in MFMA_CASES if c["form"] == 2]

# ---- single record: every kernel type on every tier of cov_rows_for (4, 8, 32 rows per workgroup), n1 no multiple of the
# tier's rows, n2 odd
SINGLE_KERNELS = [
    kernel("matern12", 0, 0.7), kernel("matern32", 0, 0.02, variance=3.5), kernel("matern52", 0, 0.3, variance=0.8),
    kernel("rbf", 0, 0.25, variance=2.0), kernel(M12, 7, 0.01, variance=1.1), kernel("matern12sm", 2, 0.2, variance=0.9),
    kernel("matern32sm", 3, 0.7, variance=1.0), kernel(M52, 4, 0.05, variance=0.25),
]
SINGLE_SHAPES = [(37, 513, 4), (130, 1021, 8), (1030, 1025, 32), (1025, 33, 4)]     # n1, n2, rows per workgroup
DIAG_SIZES = [37, 130, 1030]          # K(X) + diag_add I; 1030: the 32-row tier with three column blocks


def rows_for(n1, n2):
    """cov_rows_for of cov.hip"""
    e = n1 * n2
    return 32 if e >= 1 << 20 else (8 if e >= 1 << 17 else 4)


def single_inputs(n1, n2):
    """x2 sorted in [0, 0.5], x1 unordered, three of its points coincident with frames (r = 1e-6 exactly as the reference)"""
    rng = np.random.RandomState(n1 * 1000 + n2)
    x2 = np.sort(rng.rand(n2)) * 0.5
    x1 = rng.rand(n1) * 0.5
    x1[[0, n1 // 2, n1 - 1]] = x2[[0, n2 // 3, n2 - 1]]
    return x1, x2


# ---- grouped generic form: three records of one family, n1 = 5, 64, 109, below 2^20 entries
GROUP_N1 = (5, 64, 109)
GROUP_N2_SHARED, GROUP_N2_OWN = 1001, 777
# family: type, partial counts of the three records, lengthscale
GROUP_FAMILIES = [("matern32", (0, 0, 0), 0.02), ("rbf", (0, 0, 0), 0.25), ("matern12sm", (2, 2, 2), 0.2), ("matern32sm", (3, 3, 3), 0.7),
                  (M12, (9, 12, 9), 0.01), (M52, (12, 9, 12), 0.05)]
# per record: frames ("shared", "own", "self" = K(Z)), accumulate, diag_add, f32out, ld padding; shared: the launch has x2_shared
GROUP_MIXES = {
    "A": dict(shared=True, recs=[("shared", 0, 0.0, 1, 2), ("self", 0, 0.37, 0, 0), ("own", 1, 0.0, 0, 0)]),
    "B": dict(shared=True, recs=[("own", 1, 0.0, 1, 0), ("shared", 0, 0.0, 0, 1), ("shared", 1, 0.0, 0, 3)]),
    "C": dict(shared=False, recs=[("own", 0, 0.0, 0, 1), ("self", 1, 1e-6, 0, 0), ("own", 0, 0.0, 1, 0)]),
}


def group_inputs(family, mix):
    ktype, ms, l = family
    rng = np.random.RandomState(4242)
    xs = np.sort(rng.rand(GROUP_N2_SHARED)) * 0.5
    recs = []
    for k, (n1, m) in enumerate(zip(GROUP_N1, ms)):
        z = rng.rand(n1) * 0.5
        z[0] = xs[17 * (k + 1)]
        recs.append(dict(kern=kernel(ktype, m, l, seed=k), z=z, x_own=np.sort(rng.rand(GROUP_N2_OWN)) * 0.5))
    return xs, recs


# ---- the sum kernel: P MercerMatern12sm kernels of one padded partial count
SUM_P = (2, 5, 8)
SUM_MPAD = (4, 8)
# name, n1, n2 (None: K(Z) + jitter), ld padding, f32out
SUM_SHAPES = [("kuu_109", 109, None, 0, 0), ("kuf_109x1001", 109, 1001, 0, 0), ("kuf_109x1001_f32", 109, 1001, 2, 1),
              ("kuf_64x16385", 64, 16385, 1, 0)]
SUM_JITTER = 1e-6


def sum_kernels(P, mpad, ktype=M12):
    """P kernels whose partial counts run through mpad - 3 .. mpad (mixed m within one padded count)"""
    return [kernel(ktype, mpad - 3 + (p % 4), 0.01 * (1 + p), seed=p, variance=0.5 + 0.1 * p) for p in range(P)]


def sum_inputs(n1, n2):
    rng = np.random.RandomState(9000 + n1 + (n2 or 0))
    z = rng.rand(n1) * 0.5
    x = None if n2 is None else np.sort(rng.rand(n2)) * 0.5
    return z, x


FEATURE_M = (1, 5, 9, 29)
