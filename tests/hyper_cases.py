"""Case tables of the kernel-gradient contraction tests (test_gpu_hyper.py on the device, test_hyper_ref_cpu.py for the
reference, the bound and the dispatch rule) and `expected_form`: bwd.hip's dispatch (hy_rows_for, hy_rows_form, hyr_geometry,
the lean_ok condition of both launchers) and the partial records each form leaves, replicated in Python.  Pure numpy."""
import numpy as np

import hyper_ref as hr

HY_THREADS, HY_ROWS, HY_ROWS_SMALL = 256, 32, 8
HYR_COLSEG_MIN, HYR_MAX_SEGS, HYR_CF_MAX, HYL_CF_MAX = 512, 32, 4096, 2048


def sm_mpad(m):
    return 0 if m <= 0 else (m + 3) // 4 * 4


def hy_rows_for(n1, n2):
    return HY_ROWS if n1 * n2 >= (1 << 20) else HY_ROWS_SMALL


def hy_rows_form(nt, lean_ok):
    if lean_ok and nt <= 3:
        return 2
    return 1 if nt <= 2 else 0


def hyr_geometry(n1, n2, count):
    rows64 = (n1 + 63) // 64
    segs = 1
    while segs < HYR_MAX_SEGS and rows64 * count * segs < 1024 and (n2 + segs * 2 - 1) // (segs * 2) >= HYR_COLSEG_MIN:
        segs *= 2
    cs = ((n2 + segs - 1) // segs + 31) // 32 * 32
    return cs, (n2 + cs - 1) // cs


def expected_form(entry, ktype, m, n1, n2, count=1, with_gz=False, use_mfma=True, lean_items=True, symmetric=False, has_alpha=True,
                  has_kvals=True, aligned=True, even_ld=True, g32=False, gscale=False):
    """What one launch runs: dict(form 0 generic / 1 rows / 2 lean, nparts, inst = the instantiation's name, wg_rows | col_seg, nseg,
    nt, sep).  entry 0: launch_hyper_contract; 1: launch_hyper_contract_items; 2: launch_hyper_contract_sum (P = count)."""
    mercer = ktype in hr.MERCER
    wg = hy_rows_for(n1, n2)
    generic = dict(form=0, nparts=-(-n2 // HY_THREADS) * -(-n1 // wg), wg_rows=wg, col_seg=0, nseg=0, nt=0, sep=False)
    if entry == 2:
        generic["inst"] = "hyper_contract_sum_kernel<%d>" % count
        return generic
    gz = bool(with_gz)
    if ktype in hr.BROADCAST:
        generic["inst"] = "hyper_m12sm_kernel<%s>" % ("true" if gz else "false")
        return generic
    if not mercer:
        generic["inst"] = "hyper_contract_kernel<1,false,%s,%d>" % ("true" if gz else "false", ktype)
        return generic
    generic["inst"] = "hyper_contract_kernel<%d,true,%s>" % (sm_mpad(m), "true" if gz else "false")
    cs, nseg = hyr_geometry(n1, n2, count)
    nt = (2 * sm_mpad(m) + 15) // 16
    shape_ok = ktype == hr.MERCER12 and n1 % 16 == 0 and n2 % 16 == 0 and cs <= HYL_CF_MAX
    if entry == 0:
        lean_ok = shape_ok and even_ld and aligned
        rows_path = has_kvals and not gz and not symmetric and has_alpha
    else:
        lean_ok = bool(lean_items) and shape_ok
        rows_path = bool(use_mfma) and not gz
    form = hy_rows_form(nt, lean_ok)
    if not rows_path or form == 0:
        return generic
    vec_ok = n2 % 2 == 0 and even_ld
    g = "true" if g32 else "false"
    if form == 2:
        inst = "hyper_sm_rows_lean_kernel<%d,false,SC>" % nt if gscale else "hyper_sm_rows_lean_kernel<%d,%s>" % (nt, g)
    else:
        inst = "hyper_sm_rows_kernel<%d,%s,%s>" % (min(nt, 2), "true" if ktype == hr.MERCER52 else "false", g)
    return dict(form=form, nparts=-(-n1 // 64) * nseg, wg_rows=0, col_seg=cs, nseg=nseg, nt=nt, inst=inst,
                sep=(form == 2) or (cs <= HYR_CF_MAX and vec_ok))


def max_records(n1, n2, count):
    """the most records any form leaves for one n1 x n2 contraction of a launch of `count`"""
    best = expected_form(1, hr.MATERN12, 0, n1, n2, count)["nparts"]
    for ktype, m in ((hr.MERCER12, 1), (hr.MERCER52, 1)):
        for lean in (0, 1):
            best = max(best, expected_form(1, ktype, m, n1, n2, count, lean_items=lean)["nparts"])
    return best


# ---- inputs -------------------------------------------------------------------------------------------------------------------
def theta_for(ktype, m, ls=0.04, seed=0):
    rng = np.random.RandomState(1000 + seed)
    th = [1.3 if ktype != hr.M32SM else 1.0, ls]
    if ktype not in hr.STATIONARY:
        th += list(0.2 + rng.rand(m)) + list(3.0 + 37.0 * rng.rand(m))
    return np.array(th, np.float64)


def inputs(c):
    """numpy inputs of a case: theta, x1, x2 and `count` records of (G, alpha, gm, gscale); kvals where the case has the strip.
    x in [0, 1] with l = 0.04: |x / l| <= 25 (hyper_ref's rule: <= 50).  Layouts: 'grid' ascending jittered frames and random
    inducing inputs; 'envelope' / 'coincide' below."""
    rng = np.random.RandomState(c.get("seed", 0))
    ktype, m, n1, n2 = c["type"], c.get("m", 0), c["n1"], c["n2"]
    ls = c.get("ls", 0.04)
    theta = theta_for(ktype, m, ls, c.get("seed", 0))
    layout = c.get("layout", "grid")
    if layout == "envelope":
        x1, x2 = envelope_layout(n1, n2, ls, rng)
    elif layout == "coincide":
        # every input near x / l = 100; inducing input i IS frame 2 i + 1, to the bit
        x2 = np.sort(ls * (100.0 + 4.0 * rng.rand(n2)))
        x1 = x2[(2 * np.arange(n1) + 1) % n2].copy()
    else:
        x2 = (np.arange(n2) + 0.3 * rng.rand(n2)) / max(n2, 1)
        x1 = np.sort(rng.rand(n1))
    if c.get("symmetric") or c.get("kuu"):
        x2 = x1
    recs = []
    onehot = c.get("onehot")
    count = len(onehot) if onehot else c.get("count", 1)
    share = c.get("share", False)
    for k in range(count):
        if share and k:
            recs.append(recs[0])
            continue
        if onehot:
            G = np.zeros((n1, n2))
            i, j = onehot[k]
            G[i % n1, j % n2] = 1.0 + 0.5 * rng.rand()
        else:
            G = rng.randn(n1, n2)
        has_alpha = c.get("alpha", True)
        if onehot and has_alpha:      # the forms that read alpha unasked: a zero vector
            alpha, gm = np.zeros(n1), rng.randn(n2)
        else:
            alpha, gm = (rng.randn(n1), rng.randn(n2)) if has_alpha else (None, None)
        gscale = (0.25 + rng.rand(n2)) if c.get("gscale") else None
        if c.get("g32"):
            G = G.astype(np.float32)
        recs.append(dict(G=G, alpha=alpha, gm=gm, gscale=gscale))
    out = dict(theta=theta, x1=x1, x2=x2, recs=recs, kvals=None)
    if c.get("kvals", ktype in hr.MERCER):
        kv = hr.kvals_ref(ktype, theta, x1, x2)
        out["kvals"] = kv.astype(np.float32) if c.get("g32") else kv.astype(np.float64)
    return out


def envelope_layout(n1, n2, ls, rng):
    """Inducing inputs over 6 lengthscales around x / l = 25; frames in 16-column blocks of every kind of the separable envelope:
    wholly below the rows by more than a lengthscale, wholly above, wholly inside the band, straddling the lower edge (A - 1),
    straddling the upper edge (B + 1), and columns on BOTH far sides (unsorted frames).  The kinds repeat along n2."""
    a = 22.0 + 6.0 * np.sort(rng.rand(n1))
    a[0], a[-1] = 22.0, 28.0
    kinds = []
    nb = -(-n2 // 16)
    for b in range(nb):
        k = b % 6
        if k == 0:
            v = 10.0 + 10.5 * rng.rand(16)                 # below 21
        elif k == 1:
            v = 29.5 + 10.0 * rng.rand(16)                 # above 29
        elif k == 2:
            v = 21.5 + 7.0 * rng.rand(16)                  # in the band
        elif k == 3:
            v = 20.5 + 1.0 * rng.rand(16)                  # across A - 1 = 21
        elif k == 4:
            v = 28.5 + 1.0 * rng.rand(16)                  # across B + 1 = 29
        else:
            v = np.where(np.arange(16) % 3 == 0, 30.0 + 5.0 * rng.rand(16), 12.0 + 8.0 * rng.rand(16))     # both far sides
        kinds.append(v)
    return a * ls, np.concatenate(kinds)[:n2] * ls


# ---- the tables -----------------------------------------------------------------------------------------------------------------
M12_MS = (1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 24, 25, 28, 29, 32)
M52_MS = (3, 8, 9, 16, 17)
GENERIC_N1 = (1, 7, 8, 9, 33)
GENERIC_N2 = (1, 255, 256, 257, 513)


def _c(name, **kw):
    kw["name"] = name
    kw.setdefault("entry", 0)
    kw.setdefault("m", 0)
    return kw


def generic_cases():
    cs = []
    tn = {hr.MATERN12: "m12", hr.MATERN32: "m32", hr.MATERN52: "m52", hr.RBF: "rbf"}
    for t, s in tn.items():
        for gz in (1, 0):
            cs.append(_c("%s-gz%d-9x257" % (s, gz), type=t, n1=9, n2=257, with_gz=gz))
        cs.append(_c("%s-gz1-33x513" % s, type=t, n1=33, n2=513, with_gz=1))
        cs.append(_c("%s-kuu-sym-33" % s, type=t, n1=33, n2=33, with_gz=1, symmetric=1, alpha=False))
        cs.append(_c("%s-noalpha-9x257" % s, type=t, n1=9, n2=257, with_gz=1, alpha=False))
        cs.append(_c("%s-g32-9x257" % s, type=t, n1=9, n2=257, with_gz=1, g32=1))
        cs.append(_c("%s-items3-9x257" % s, type=t, n1=9, n2=257, with_gz=1, entry=1, count=3, use_mfma=0))
    # every generic shape edge, for one kernel of each generic family
    for t, s, m in ((hr.MATERN32, "m32", 0), (hr.MERCER12, "mm12-m5", 5), (hr.M12SM, "b12-m2", 2)):
        for n1 in GENERIC_N1:
            for n2 in GENERIC_N2:
                if (n1, n2) != (9, 257) or t != hr.MATERN32:
                    cs.append(_c("%s-edge-%dx%d" % (s, n1, n2), type=t, m=m, n1=n1, n2=n2, with_gz=1, kvals=False))
    cs.append(_c("m32-ldg-9x257", type=hr.MATERN32, n1=9, n2=257, with_gz=1, ldg_pad=7))
    cs.append(_c("m32-items-sharedx2-9x257", type=hr.MATERN32, n1=9, n2=257, with_gz=1, entry=1, count=2, use_mfma=0, shared_x2=1))
    # the 8-row to 32-row workgroup switch at n1 n2 = 2^20
    cs.append(_c("m12-switch-256x4096", type=hr.MATERN12, n1=256, n2=4096, with_gz=1, alpha=False))
    cs.append(_c("m12-switch-256x4095", type=hr.MATERN12, n1=256, n2=4095, with_gz=1, alpha=False))
    cs.append(_c("rbf-switch-kuu-1024", type=hr.RBF, n1=1024, n2=1024, with_gz=1, symmetric=1, alpha=False))
    # every spectral-mixture padding, both sides of each step, with and without the inducing-input gradient
    for m in M12_MS:
        for gz in (1, 0):
            cs.append(_c("mm12-m%d-gz%d-generic-9x257" % (m, gz), type=hr.MERCER12, m=m, n1=9, n2=257, with_gz=gz, kvals=False))
    cs.append(_c("mm12-m5-kuu-sym-33", type=hr.MERCER12, m=5, n1=33, n2=33, with_gz=1, symmetric=1, alpha=False, kvals=False))
    cs.append(_c("mm52-m17-generic-17x33", type=hr.MERCER52, m=17, n1=17, n2=33, with_gz=0))
    cs.append(_c("mm52-m3-gz1-generic-9x257", type=hr.MERCER52, m=3, n1=9, n2=257, with_gz=1, kvals=False))
    cs.append(_c("mm12-m25-nt4-generic-64x96", type=hr.MERCER12, m=25, n1=64, n2=96, entry=1, count=2))
    cs.append(_c("mm12-m17-nt3-ragged-generic-17x33", type=hr.MERCER12, m=17, n1=17, n2=33))
    for t, s in ((hr.M12SM, "b12"), (hr.M32SM, "b32")):
        for m in (1, 32):
            for gz in (1, 0):
                cs.append(_c("%s-m%d-gz%d-9x257" % (s, m, gz), type=t, m=m, n1=9, n2=257, with_gz=gz))
        cs.append(_c("%s-m2-kuu-sym-33" % s, type=t, m=2, n1=33, n2=33, with_gz=1, symmetric=1, alpha=False))
    return cs


def rows_cases():
    cs = []
    # the lean form at every NT, both sides of each padding step (items entry, two records)
    for m in (1, 4, 5, 8, 9, 12, 13, 16, 17, 20, 24):
        cs.append(_c("mm12-m%d-lean-64x96" % m, type=hr.MERCER12, m=m, n1=64, n2=96, entry=1, count=2))
    for m in (4, 12, 20):
        cs.append(_c("mm12-m%d-lean-g32-64x96" % m, type=hr.MERCER12, m=m, n1=64, n2=96, entry=1, count=2, g32=1))
        cs.append(_c("mm12-m%d-lean-sc-64x96" % m, type=hr.MERCER12, m=m, n1=64, n2=96, entry=1, count=2, gscale=1))
    cs.append(_c("mm12-m5-lean-sharedx2-64x96", type=hr.MERCER12, m=5, n1=64, n2=96, entry=1, count=2, shared_x2=1))
    cs.append(_c("mm12-m5-lean-single-64x96", type=hr.MERCER12, m=5, n1=64, n2=96))
    cs.append(_c("mm12-m5-notlean-items-64x96", type=hr.MERCER12, m=5, n1=64, n2=96, entry=1, count=2, lean_items=0))
    # the rows form: both envelopes, NT 1 and 2, float32 strips
    for m in (1, 4, 5, 8, 9, 12, 13, 16):
        cs.append(_c("mm12-m%d-rows-17x33" % m, type=hr.MERCER12, m=m, n1=17, n2=33))
    for m in (3, 8, 9, 16):
        cs.append(_c("mm52-m%d-rows-64x96" % m, type=hr.MERCER52, m=m, n1=64, n2=96, entry=1, count=2))
    for t, s, m in ((hr.MERCER12, "mm12", 4), (hr.MERCER12, "mm12", 12), (hr.MERCER52, "mm52", 3), (hr.MERCER52, "mm52", 9)):
        cs.append(_c("%s-m%d-rows-g32-17x34" % (s, m), type=t, m=m, n1=17, n2=34, g32=1))
        cs.append(_c("%s-m%d-rows-g32-17x33" % (s, m), type=t, m=m, n1=17, n2=33, g32=1))
    # shape edges of the matrix-core forms (n2 odd, ldg odd, ldk odd: each forces the checked path)
    for n1 in (16, 17, 63, 64, 65, 72):
        cs.append(_c("mm12-m5-rowsedge-%dx32" % n1, type=hr.MERCER12, m=5, n1=n1, n2=32))
        cs.append(_c("mm52-m3-rowsedge-%dx33" % n1, type=hr.MERCER52, m=3, n1=n1, n2=33))
    for n2 in (31, 32, 33, 2004):
        cs.append(_c("mm12-m5-rowsedge-65x%d" % n2, type=hr.MERCER12, m=5, n1=65, n2=n2))
        cs.append(_c("mm52-m9-rowsedge-64x%d" % n2, type=hr.MERCER52, m=9, n1=64, n2=n2))
    cs.append(_c("mm12-m5-oddldg-64x32", type=hr.MERCER12, m=5, n1=64, n2=32, ldg_pad=1))
    cs.append(_c("mm12-m5-oddldk-64x32", type=hr.MERCER12, m=5, n1=64, n2=32, ldk_pad=3))
    cs.append(_c("mm12-m5-evenld-64x32", type=hr.MERCER12, m=5, n1=64, n2=32, ldg_pad=2, ldk_pad=4))
    cs.append(_c("mm12-m5-misaligned-64x64", type=hr.MERCER12, m=5, n1=64, n2=64, misalign=1))
    # column segments: 2, 4 and 4 (the last ragged)
    for n2 in (1024, 2048, 2064):
        cs.append(_c("mm12-m5-lean-segs-64x%d" % n2, type=hr.MERCER12, m=5, n1=64, n2=n2))
        cs.append(_c("mm52-m3-rows-segs-64x%d" % n2, type=hr.MERCER52, m=3, n1=64, n2=n2))
    # col_seg beyond the table limits: 1024 records share every read-only operand
    cs.append(_c("mm12-m5-x1024-16x2064-beyond-lean-table", type=hr.MERCER12, m=5, n1=16, n2=2064, entry=1, count=1024, share=True))
    cs.append(_c("mm12-m5-x1024-16x4112-no-envelope", type=hr.MERCER12, m=5, n1=16, n2=4112, entry=1, count=1024, share=True))
    # the separable envelope: every block kind in one launch
    cs.append(_c("mm12-m5-envelope-lean-64x192", type=hr.MERCER12, m=5, n1=64, n2=192, layout="envelope"))
    cs.append(_c("mm12-m20-envelope-lean-nt3-64x192", type=hr.MERCER12, m=20, n1=64, n2=192, layout="envelope"))
    cs.append(_c("mm12-m5-envelope-sc-64x192", type=hr.MERCER12, m=5, n1=64, n2=192, layout="envelope", entry=1, count=1, gscale=1))
    cs.append(_c("mm12-m5-envelope-rows-63x192", type=hr.MERCER12, m=5, n1=63, n2=192, layout="envelope"))
    cs.append(_c("mm52-m9-envelope-rows-64x192", type=hr.MERCER52, m=9, n1=64, n2=192, layout="envelope"))
    # an inducing input that IS a frame, 100 lengthscales out (r2 = 0 exactly)
    cs.append(_c("mm12-m5-coincide-lean-16x64", type=hr.MERCER12, m=5, n1=16, n2=64, layout="coincide", ls=0.01))
    cs.append(_c("mm12-m5-coincide-rows-17x64", type=hr.MERCER12, m=5, n1=17, n2=64, layout="coincide", ls=0.01))
    cs.append(_c("mm52-m3-coincide-rows-16x64", type=hr.MERCER52, m=3, n1=16, n2=64, layout="coincide", ls=0.01))
    cs.append(_c("mm12-m5-coincide-generic-16x64", type=hr.MERCER12, m=5, n1=16, n2=64, layout="coincide", ls=0.01, with_gz=1, kvals=False))
    cs.append(_c("m32-coincide-generic-16x64", type=hr.MATERN32, n1=16, n2=64, layout="coincide", ls=0.01, with_gz=1))
    return cs


def _rows_placements(n1, n2, cs, nseg):
    """(row, column) of the one-hot entries: first / last row and column, first / last column of every segment, both columns of a
    paired load, each of the four k-lanes (columns 0, 2, 4, 6 of a block: column 8 s + 2 kq + u)"""
    pl = [(0, 0), (n1 - 1, 0), (0, n2 - 1), (n1 - 1, n2 - 1)]
    for s in range(nseg):
        pl += [(3, s * cs), (5, min(n2, (s + 1) * cs) - 1)]
    pl += [(7, 16 + 2 * kq + u) for kq in range(4) for u in (0, 1)] + [(9, 16 + 8 + 2)]
    return pl


def onehot_cases():
    cs = []
    gen = [(0, 0), (8, 0), (0, 256), (8, 256), (7, 255), (8, 255), (3, 100)]
    cs.append(_c("onehot-m32-generic-9x257", type=hr.MATERN32, n1=9, n2=257, with_gz=1, entry=1, use_mfma=0, alpha=False, onehot=gen))
    cs.append(_c("onehot-mm12-m5-generic-9x257", type=hr.MERCER12, m=5, n1=9, n2=257, with_gz=1, entry=1, use_mfma=0, alpha=False,
                 kvals=False, onehot=gen))
    cs.append(_c("onehot-b12-m2-generic-9x257", type=hr.M12SM, m=2, n1=9, n2=257, with_gz=1, entry=1, use_mfma=0, alpha=False, onehot=gen))
    # four column segments of 544 (the last 448): 21 records, so the launch stays far below the 1024 workgroups that end the split
    n1, n2 = 64, 2080
    col_seg, nseg = hyr_geometry(n1, n2, 21)
    assert (col_seg, nseg) == (544, 4) and len(_rows_placements(n1, n2, col_seg, nseg)) == 21
    cs.append(_c("onehot-mm12-m5-lean-64x2080", type=hr.MERCER12, m=5, n1=n1, n2=n2, entry=1, onehot=_rows_placements(n1, n2, col_seg, nseg),
                 geometry=(col_seg, nseg)))
    cs.append(_c("onehot-mm52-m3-rows-64x2080", type=hr.MERCER52, m=3, n1=n1, n2=n2, entry=1, onehot=_rows_placements(n1, n2, col_seg, nseg),
                 geometry=(col_seg, nseg)))
    # a column of a straddling block and of a both-sides block of the envelope layout (blocks 3, 4, 5)
    env = [(0, 3 * 16 + 5), (63, 4 * 16 + 9), (31, 5 * 16 + 3), (31, 5 * 16 + 4), (1, 0), (2, 16 + 1)]
    cs.append(_c("onehot-mm12-m5-envelope-lean-64x192", type=hr.MERCER12, m=5, n1=64, n2=192, entry=1, layout="envelope", onehot=env))
    cs.append(_c("onehot-mm52-m3-envelope-rows-64x192", type=hr.MERCER52, m=3, n1=64, n2=192, entry=1, layout="envelope", onehot=env))
    return cs


def sum_cases():
    cs = []
    ms = (1, 4, 2, 3, 1, 4)
    for P in range(2, 7):
        cs.append(dict(name="sum-P%d-33x513" % P, P=P, ms=ms[:P], types=[hr.MERCER12] * P, n1=33, n2=513, taken=True))
    cs.append(dict(name="sum-P3-g32-noalpha-9x257", P=3, ms=(2, 1, 3), types=[hr.MERCER12] * 3, n1=9, n2=257, taken=True, g32=1, alpha=False))
    cs.append(dict(name="sum-P1-refused", P=1, ms=(2,), types=[hr.MERCER12], n1=9, n2=257, taken=False))
    cs.append(dict(name="sum-P7-refused", P=7, ms=(1,) * 7, types=[hr.MERCER12] * 7, n1=9, n2=257, taken=False))
    cs.append(dict(name="sum-m5-refused", P=3, ms=(1, 5, 2), types=[hr.MERCER12] * 3, n1=9, n2=257, taken=False))
    cs.append(dict(name="sum-nonmercer-refused", P=3, ms=(1, 0, 2), types=[hr.MERCER12, hr.MATERN32, hr.MERCER12], n1=9, n2=257, taken=False))
    return cs


def finish_cases():
    cs = []
    fam = ((hr.MATERN12, 0), (hr.MATERN32, 0), (hr.MATERN52, 0), (hr.RBF, 0), (hr.MERCER12, 3), (hr.M12SM, 2), (hr.M32SM, 2), (hr.MERCER52, 3))
    for t, m in fam:
        cs.append(dict(name="finish-kdiag-type%d" % t, entry=3, recs=[dict(type=t, m=m, np_uf=5, np_uu=0, gv=True, n1=0, cb_uf=0, cb_uu=0)]))
    for n in (0, 1, 255, 256, 257):
        cs.append(dict(name="finish-single-np%d" % n, entry=3, recs=[dict(type=hr.MERCER12, m=2, np_uf=n, np_uu=0, gv=False, n1=33, cb_uf=1, cb_uu=0)]))
        cs.append(dict(name="finish-items-np%d" % n, entry=4, recs=[dict(type=hr.MERCER12, m=2, np_uf=n, np_uu=257 - n, gv=True, n1=33, cb_uf=1, cb_uu=1),
                                                                      dict(type=hr.MERCER12, m=2, np_uf=3, np_uu=n, gv=False, n1=33, cb_uf=3, cb_uu=0)]))
    for n1 in (255, 256, 257):
        for cb in (1, 3):
            cs.append(dict(name="finish-gz-n%d-cb%d" % (n1, cb), entry=4, recs=[dict(type=hr.MATERN32, m=0, np_uf=2, np_uu=1, gv=True, n1=n1, cb_uf=cb, cb_uu=4 - cb)]))
    # mixed m in one launch: the grid is sized by the largest record
    cs.append(dict(name="finish-items-mixed-m", entry=4, recs=[dict(type=hr.MERCER12, m=1, np_uf=4, np_uu=2, gv=True, n1=300, cb_uf=2, cb_uu=1),
                                                               dict(type=hr.MERCER12, m=7, np_uf=2, np_uu=4, gv=True, n1=5, cb_uf=1, cb_uu=1),
                                                               dict(type=hr.MERCER52, m=3, np_uf=1, np_uu=1, gv=True, n1=257, cb_uf=1, cb_uu=2)]))
    return cs


def form_kwargs(c, aligned=True):
    """expected_form's arguments for a contraction case"""
    inp_count = len(c["onehot"]) if c.get("onehot") else c.get("count", 1)
    mercer = c["type"] in hr.MERCER
    return dict(entry=c["entry"], ktype=c["type"], m=c["m"], n1=c["n1"], n2=c["n2"], count=inp_count, with_gz=c.get("with_gz", 0),
                use_mfma=c.get("use_mfma", 1), lean_items=c.get("lean_items", 1), symmetric=c.get("symmetric", 0),
                has_alpha=c.get("alpha", True), has_kvals=c.get("kvals", mercer), aligned=not c.get("misalign"),
                even_ld=(c.get("ldg_pad", 0) + c["n2"]) % 2 == 0 and (c.get("ldk_pad", 0) + c["n2"]) % 2 == 0,
                g32=c.get("g32", 0), gscale=c.get("gscale", 0))


def all_contraction_cases():
    return generic_cases() + rows_cases() + onehot_cases()
