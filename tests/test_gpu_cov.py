"""The covariance builds of cov.hip as operators: one launch of a host entry on the test's own buffers (gp_kernel_build,
gp_kernel_build_f32, gp_debug_cov_build), against the plain references of tests/cov_ref.py, at every form, family and edge
of tests/cov_cases.py.

Bars.  Within max |x / l| <= 256 the reference is oracle.gpflow05.K at rtol 1e-11, atol 1e-12 (the bar the kernel tests
already hold).  On top of it only what the number formats add, derived here and never taken from a GPU run:
  * float32 output: one rounding to nearest of the float64 value, 2^-24 |K|;
  * accumulate: the device writes fl(old + K), so the sum carries one more rounding, 2^-53 |old + K| (float32: the stored
    sum is fl32(old + fl32(K)), 2^-24 |K| + 2^-24 |old + K|);
  * K + diag_add I: one rounding of the sum, 2^-53 |K + diag_add|.
Beyond that range the reference is the long-double closed form at the bars recorded beside each case in cov_cases.py
(4 * what the float64 emulation of the device's formulas measures on the CPU, tests/test_cov_ref_cpu.py).

Every output sits in a buffer with guard bands before and after it and with its ld - n2 padding columns filled with a
sentinel; all of that must come back untouched.  A float32 output is a float32 buffer.  Every matrix-core launch asserts the
form and the row segment the library reports, so no case passes on a fallback.  Nothing from the library is imported at
module level (the CPU run collects this file).
"""
import ctypes as C

import numpy as np
import pytest

import cov_cases as cc
import cov_ref as cr

pytestmark = pytest.mark.gpu

GP_OK, GP_ERR_BAD_ARG, GP_ERR_WORKSPACE, GP_ERR_UNSUPPORTED = 0, 1, 5, 6
SENT64, SENT32 = -7.0e77, np.float32(-7.0e37)
GUARD = 64                       # elements before and after a matrix (a multiple of 4: the matrix stays 16-byte aligned)
E53, E24 = 2.0 ** -53, 2.0 ** -24


class Out(object):
    """an n1 x n2 matrix with leading dimension ld inside guard bands; padding columns and guards hold a sentinel, the body
    the sentinel too or `init`.  misalign: the matrix starts 8 bytes past a 16-byte boundary (float64 only)"""

    def __init__(self, h, n1, n2, ld=None, f32=False, misalign=False, init=None):
        self.n1, self.n2, self.ld, self.f32 = n1, n2, (n2 if ld is None else ld), f32
        dt, sent = (np.float32, SENT32) if f32 else (np.float64, SENT64)
        self.front = GUARD + (1 if misalign else 0)
        host = np.full(self.front + n1 * self.ld + GUARD, sent, dtype=dt)
        if init is not None:
            body = host[self.front:self.front + n1 * self.ld].reshape(n1, self.ld)
            body[:, :n2] = init
        self.initial = host
        self.t = h.torch.as_tensor(host.copy(), device=h.device)
        self.ptr = self.t.data_ptr() + self.front * host.itemsize
        assert self.ptr % 16 == (8 if misalign else 0)

    def read(self, what):
        flat = self.t.cpu().numpy()
        f, n = self.front, self.n1 * self.ld
        assert np.array_equal(flat[:f], self.initial[:f]) and np.array_equal(flat[f + n:], self.initial[f + n:]), \
            "%s: a guard band changed" % what
        body, body0 = flat[f:f + n].reshape(self.n1, self.ld), self.initial[f:f + n].reshape(self.n1, self.ld)
        assert np.array_equal(body[:, self.n2:], body0[:, self.n2:]), "%s: the padding columns changed" % what
        return body[:, :self.n2].copy()

    def untouched(self):
        return np.array_equal(self.t.cpu().numpy(), self.initial)


def _sync(h, name, st):
    from gpitch_amd import _lib
    try:
        h.sync()
    except _lib.GpitchError as e:
        if e.status == _lib.GP_ERR_HIP:       # a device fault: nothing more may run on this GPU from this process
            pytest.exit("HIP error after %s: %s" % (name, e), returncode=3)
        raise
    if st == _lib.GP_ERR_HIP:
        pytest.exit("HIP error from %s" % name, returncode=3)


def _desc(h, kern, keep):
    from gpitch_amd import _lib
    th = h.to_device(cr.theta(kern))
    keep.append(th)
    return _lib.KernelDesc(cr.KT[kern["type"]], len(kern["frequency"]), th.data_ptr())


def _feat(h, kern, n1, n2, keep, fill=None):
    """feature workspace of a Mercer kernel as the header sizes it (None for the other families)"""
    if kern["type"] not in cr.MERCER:
        return None, None
    n = 2 * cr.sm_mpad(len(kern["frequency"])) * (n1 + n2) + 64
    t = h.torch.full((n,), fill, dtype=h.torch.float64, device=h.device) if fill is not None else h.empty(n)
    keep.append(t)
    return t, t.data_ptr()


def _item(it, desc, p_x1, p_x2, out, feat_ptr, n1, n2, accumulate=0, diag_add=0.0):
    it.kern, it.x1, it.x2, it.out, it.feat = desc, p_x1, p_x2, out.ptr, feat_ptr
    it.ld, it.diag_add, it.n1, it.n2, it.accumulate, it.f32out = out.ld, diag_add, n1, n2, accumulate, int(out.f32)


def _cov(h, name, entry, items, count, xs_ptr=None, n2s=0, es=0, ws_bytes=None):
    ws_bytes = 192 * count if ws_bytes is None else ws_bytes
    ws = h.workspace(max(ws_bytes, 16))
    form, row_seg = C.c_int32(-9), C.c_int32(-9)
    st = h.lib.gp_debug_cov_build(h.h, entry, items, count, xs_ptr, n2s, es, C.c_void_p(ws.data_ptr()), ws_bytes, C.byref(form),
                                  C.byref(row_seg))
    _sync(h, "gp_debug_cov_build (%s)" % name, st)
    return st, form.value, row_seg.value


def _bound(ref, f32=False, old=None, diag=None):
    """the bar of the module docstring, entry by entry"""
    ref = np.asarray(ref, dtype=np.float64)
    b = cr.ATOL + cr.RTOL * np.abs(ref)
    value = ref if diag is None else ref + diag * np.eye(*ref.shape)
    total = value if old is None else value + old
    if diag is not None:
        b = b + E53 * np.abs(value)
    if f32:
        b = b + E24 * np.abs(value) + (E24 * np.abs(total) if old is not None else 0.0)
    elif old is not None:
        b = b + E53 * np.abs(total)
    return total, b


def _check(what, got, ref, **kw):
    total, b = _bound(ref, **kw)
    err = np.abs(got.astype(np.float64) - total)
    worst = float(np.max(err / b))
    print("%s: worst error / bar = %.4f" % (what, worst))
    assert worst <= 1.0, "%s: worst error / bar = %.4f at %s" % (what, worst, np.unravel_index(np.argmax(err / b), err.shape))


# ---- single record ---------------------------------------------------------------------------------------------------------
_single_ref = {}


def _single(kern, n1, n2):
    key = (kern["type"], n1, n2)
    if key not in _single_ref:
        x1, x2 = cc.single_inputs(n1, n2)
        _single_ref[key] = (x1, x2, cr.oracle(kern, x1, x2))
    return _single_ref[key]


@pytest.mark.parametrize("n1,n2,rows", cc.SINGLE_SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("kern", cc.SINGLE_KERNELS, ids=lambda k: k["type"])
def test_single_record_every_type_tier_stride_and_alignment(gp_handle, kern, n1, n2, rows):
    h, keep = gp_handle, []
    x1, x2, ref = _single(kern, n1, n2)
    d = _desc(h, kern, keep)
    dx1, dx2 = h.to_device(x1), h.to_device(x2)
    rng = np.random.RandomState(5)
    old = rng.randn(n1, n2)
    old32 = old.astype(np.float32)

    def build(out, acc=0):
        fn = h.lib.gp_kernel_build_f32 if out.f32 else h.lib.gp_kernel_build
        st = fn(h.h, C.byref(d), dx1.data_ptr(), n1, dx2.data_ptr(), n2, C.c_void_p(out.ptr), out.ld, acc)
        _sync(h, "gp_kernel_build", st)
        assert st == GP_OK, st

    plain = None
    for ld, mis in ((n2, False), (n2 + 1, False), (n2 + 3, False), (n2 + 1, True), (n2, True)):
        out = Out(h, n1, n2, ld, misalign=mis)
        build(out)
        got = out.read("ld %d misalign %d" % (ld, mis))
        _check("%s %dx%d ld %d misalign %d" % (kern["type"], n1, n2, ld, mis), got, ref)
        if plain is None:
            plain = got
        assert np.array_equal(got, plain), "stride and alignment change no bit"
    for ld, mis in ((n2, False), (n2 + 1, False), (n2 + 1, True)):
        out = Out(h, n1, n2, ld, misalign=mis, init=old)
        build(out, acc=1)
        got = out.read("accumulate ld %d" % ld)
        _check("accumulate ld %d misalign %d" % (ld, mis), got, ref, old=old)
        assert np.array_equal(got, old + plain), "accumulate adds the plain build's value once"
    for ld in (n2, n2 + 2, n2 + 1):            # odd, odd, even (the 8-byte pair stores)
        out = Out(h, n1, n2, ld, f32=True)
        build(out)
        got = out.read("float32 ld %d" % ld)
        assert got.dtype == np.float32
        _check("float32 ld %d" % ld, got, ref, f32=True)
        assert np.array_equal(got, plain.astype(np.float32)), "float32 output is the float64 value rounded once"
        out = Out(h, n1, n2, ld, f32=True, init=old32)
        build(out, acc=1)
        got = out.read("float32 accumulate ld %d" % ld)
        _check("float32 accumulate ld %d" % ld, got, ref, f32=True, old=old32.astype(np.float64))
        assert np.array_equal(got, old32 + plain.astype(np.float32))


@pytest.mark.parametrize("n", cc.DIAG_SIZES)
@pytest.mark.parametrize("kern", cc.SINGLE_KERNELS, ids=lambda k: k["type"])
def test_single_record_self_covariance_with_diagonal(gp_handle, kern, n):
    from gpitch_amd import _lib
    h, keep = gp_handle, []
    x1, _ = cc.single_inputs(n, 33)
    ref = cr.oracle(kern, x1)
    d = _desc(h, kern, keep)
    dx1 = h.to_device(x1)
    _, p_feat = _feat(h, kern, n, n, keep)
    first = None
    for ld, mis in ((n, False), (n + 1, False), (n + 2, False), (n + 2, True)):
        out = Out(h, n, n, ld, misalign=mis)
        items = (_lib.DebugCovItem * 1)()
        _item(items[0], d, dx1.data_ptr(), None, out, p_feat, n, n, diag_add=0.5)
        st, form, seg = _cov(h, "diag", 0, items, 1)
        assert (st, form, seg) == (GP_OK, 0, 0)
        got = out.read("K(X) + 0.5 I, n %d ld %d" % (n, ld))
        _check("%s K(X) + 0.5 I n %d ld %d misalign %d" % (kern["type"], n, ld, mis), got, ref, diag=0.5)
        first = got if first is None else first
        assert np.array_equal(got, first)
    # the diagonal carries the term and nothing else does: against the plain build, bit for bit
    out = Out(h, n, n, n)
    items = (_lib.DebugCovItem * 1)()
    _item(items[0], d, dx1.data_ptr(), None, out, p_feat, n, n)
    assert _cov(h, "plain", 0, items, 1)[0] == GP_OK
    plain = out.read("K(X)")
    assert np.array_equal(first, plain + 0.5 * np.eye(n))


# ---- grouped generic form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", sorted(cc.GROUP_MIXES))
@pytest.mark.parametrize("family", cc.GROUP_FAMILIES, ids=lambda f: f[0])
def test_grouped_generic_records_equal_the_single_build(gp_handle, family, mix):
    from gpitch_amd import _lib
    h, keep = gp_handle, []
    spec = cc.GROUP_MIXES[mix]
    xs, recs = cc.group_inputs(family, mix)
    dxs = h.to_device(xs)
    p_xs, n2s = (dxs.data_ptr(), xs.size) if spec["shared"] else (None, 0)
    count = len(recs)
    rng = np.random.RandomState(11)
    items = (_lib.DebugCovItem * count)()
    outs, singles = [], []
    for k, (rec, (frames, acc, diag, f32, ld_pad)) in enumerate(zip(recs, spec["recs"])):
        n1 = rec["z"].size
        x2 = {"shared": xs, "own": rec["x_own"], "self": None}[frames]
        n2 = n1 if x2 is None else x2.size
        old = (rng.randn(n1, n2).astype(np.float32 if f32 else np.float64)) if acc else None
        d = _desc(h, rec["kern"], keep)
        dz = h.to_device(rec["z"])
        dx2 = None if x2 is None else (dxs if frames == "shared" else h.to_device(x2))
        keep += [dz, dx2]
        _, p_feat = _feat(h, rec["kern"], n1, n2, keep)
        out = Out(h, n1, n2, n2 + ld_pad, f32=bool(f32), init=old)
        _item(items[k], d, dz.data_ptr(), dx2.data_ptr() if frames == "own" else None, out, p_feat, n1, -1 if frames == "shared" else n2,
              accumulate=acc, diag_add=diag)
        outs.append((out, x2, old, rec, acc, diag, f32))
        # the same record through the single-record entry, on buffers of its own
        one = (_lib.DebugCovItem * 1)()
        _, p_feat1 = _feat(h, rec["kern"], n1, n2, keep)
        out1 = Out(h, n1, n2, n2 + ld_pad, f32=bool(f32), init=old)
        _item(one[0], d, dz.data_ptr(), None if x2 is None else dx2.data_ptr(), out1, p_feat1, n1, n2, accumulate=acc, diag_add=diag)
        singles.append((one, out1))
    st, form, seg = _cov(h, "group %s %s" % (family[0], mix), 1, items, count, p_xs, n2s)
    assert (st, form, seg) == (GP_OK, 0, 0)
    for k, ((out, x2, old, rec, acc, diag, f32), (one, out1)) in enumerate(zip(outs, singles)):
        what = "%s mix %s record %d" % (family[0], mix, k)
        got = out.read(what)
        assert _cov(h, what + " single", 0, one, 1)[0] == GP_OK
        assert np.array_equal(got, out1.read(what + " single")), "%s: the grouped and the single build differ" % what
        _check(what, got, cr.oracle(rec["kern"], rec["z"], x2), f32=bool(f32), old=None if old is None else old.astype(np.float64),
               diag=diag if diag else None)


# ---- matrix-core forms -------------------------------------------------------------------------------------------------------
_mfma_ref = {}


def _mfma_reference(c):
    """inputs and the reference of every record, once per distinct input set (the cases share most of them)"""
    key = (c["type"], tuple(c["recs"]), c["n2"], c["l"], c.get("x_order"), c.get("z_order"), c.get("threshold"))
    if key not in _mfma_ref:
        kerns, zs, x = cc.mfma_inputs(c)
        refs = []
        for k, z in zip(kerns, zs):
            assert (cr.amax(k, z, x) <= cr.ORACLE_RANGE) == (c["ref"] == "oracle")
            if c["ref"] == "oracle":
                refs.append((cr.oracle(k, z, x), None))
            else:
                refs.append((cr.closed_form(k, z, x), cr.separable_entries(k, z, x)))
        _mfma_ref[key] = (kerns, zs, x, refs)
    return _mfma_ref[key]


def _mfma_launch(h, c, kerns, zs, x, es, f32, name):
    from gpitch_amd import _lib
    keep = []
    dxs = h.to_device(x)
    count = len(kerns)
    items = (_lib.DebugCovItem * count)()
    outs = []
    for k, (kern, z) in enumerate(zip(kerns, zs)):
        d = _desc(h, kern, keep)
        dz = h.to_device(z)
        keep.append(dz)
        _, p_feat = _feat(h, kern, z.size, x.size, keep)
        out = Out(h, z.size, x.size, x.size + c.get("ld_pad", 0), f32=f32, misalign=bool(c.get("misalign")))
        _item(items[k], d, dz.data_ptr(), None, out, p_feat, z.size, -1)
        outs.append(out)
    st, form, seg = _cov(h, name, 1, items, count, dxs.data_ptr(), x.size, es)
    assert st == GP_OK, (name, st)
    return form, seg, [o.read("%s record %d" % (name, k)) for k, o in enumerate(outs)]


@pytest.mark.parametrize("c", cc.MFMA_CASES, ids=lambda c: c["id"])
def test_matrix_core_forms(gp_handle, c):
    h = gp_handle
    kerns, zs, x, refs = _mfma_reference(c)
    f32 = bool(c.get("f32"))
    form, seg, got = _mfma_launch(h, c, kerns, zs, x, c["es"], f32, c["id"])
    assert (form, seg) == (c["form"], c["row_seg"]), "the launch took form %d with row segment %d" % (form, seg)
    for k, (g, (ref, sep)) in enumerate(zip(got, refs)):
        what = "%s record %d" % (c["id"], k)
        if c["ref"] == "oracle":
            _check(what, g, ref, f32=f32)
        else:
            # measured on the CPU and recorded in cov_cases.py: separable tiles / entry-by-entry tiles, bar = 4 * measured
            u_sep, u_band = cr.units(g, ref, sep), cr.units(g, ref, ~sep)
            print("%s: separable tiles %.4f (measured %.4f, bar %.4f), entry-by-entry tiles %.2f (measured %.2f, bar %.2f)"
                  % (what, u_sep, c["measured"][0], c["bar"][0], u_band, c["measured"][1], c["bar"][1]))
            assert u_sep <= c["bar"][0] and u_band <= c["bar"][1]
    # float32 strips: the float64 strip of the same launch, rounded once.  (m = 5: float64 strips of 8 padded partials stay on
    # the staged form, whose entries the lean form repeats bit for bit — asserted below for every lean case)
    es64 = 1 if c["es"] == 2 else c["es"]
    if f32:
        form64, _, got64 = _mfma_launch(h, c, kerns, zs, x, es64, False, c["id"] + " float64")
        assert form64 == (c["form"] if cr.sm_mpad(c["recs"][0][1]) >= 12 or c["es"] != 2 else 1)
        for g, g64 in zip(got, got64):
            assert np.array_equal(g, g64.astype(np.float32))
    # the lean form's entries are the staged form's, bit for bit
    if c["form"] == 2:
        form_s, _, got_s = _mfma_launch(h, c, kerns, zs, x, 0, f32, c["id"] + " staged")
        assert form_s == 1
        for k, (g, gs) in enumerate(zip(got, got_s)):
            assert np.array_equal(g, gs), "%s record %d: %d entries differ between the lean and the staged form" % (
                c["id"], k, np.count_nonzero(g != gs))


# ---- the sum kernel ----------------------------------------------------------------------------------------------------------
def _sum_setup(h, kerns, n1, n2, ld_pad, f32, keep, diag):
    from gpitch_amd import _lib
    z, x = cc.sum_inputs(n1, n2)
    dz = h.to_device(z)
    dx = None if x is None else h.to_device(x)
    keep += [dz, dx]
    cols = n1 if x is None else n2
    descs = [_desc(h, k, keep) for k in kerns]
    feats = [_feat(h, k, n1, cols, keep)[1] for k in kerns]

    def items_for(out, which, acc_from_second=False):
        items = (_lib.DebugCovItem * len(which))()
        for i, p in enumerate(which):
            _item(items[i], descs[p], dz.data_ptr(), None if dx is None else dx.data_ptr(), out, feats[p], n1, cols,
                  accumulate=int(acc_from_second and p > 0), diag_add=diag)
        return items
    return z, x, cols, items_for


@pytest.mark.parametrize("name,n1,n2,ld_pad,f32", cc.SUM_SHAPES, ids=[s[0] for s in cc.SUM_SHAPES])
@pytest.mark.parametrize("mpad", cc.SUM_MPAD)
@pytest.mark.parametrize("P", cc.SUM_P)
def test_sum_kernel_equals_accumulate_launches(gp_handle, P, mpad, name, n1, n2, ld_pad, f32):
    h, keep = gp_handle, []
    kerns = cc.sum_kernels(P, mpad)
    diag = cc.SUM_JITTER if n2 is None else 0.0
    z, x, cols, items_for = _sum_setup(h, kerns, n1, n2, ld_pad, f32, keep, diag)
    out = Out(h, n1, cols, cols + ld_pad, f32=bool(f32))
    st, form, seg = _cov(h, "sum " + name, 2, items_for(out, range(P)), P)
    assert (st, form, seg) == (GP_OK, 0, 0)
    got = out.read("sum " + name)
    # the oracle's sum, each kernel at its own bar
    ref, bar = np.zeros((n1, cols)), np.zeros((n1, cols))
    for k in kerns:
        kp = cr.oracle(k, z, x)
        ref, bar = ref + kp, bar + cr.ATOL + cr.RTOL * np.abs(kp)
    if n2 is None:
        ref = ref + diag * np.eye(n1)
    bar = bar + (E24 if f32 else P * E53) * np.abs(ref)
    worst = float(np.max(np.abs(got.astype(np.float64) - ref) / bar))
    print("sum %s P %d mpad %d: worst error / bar = %.4f" % (name, P, mpad, worst))
    assert worst <= 1.0
    # P launches of the single-record entry, accumulating from the second on (float64), the diagonal term in the first
    acc = Out(h, n1, cols, cols + ld_pad)
    for p in range(P):
        one = items_for(acc, [p], acc_from_second=True)
        one[0].diag_add = diag if p == 0 else 0.0
        assert _cov(h, "sum reference", 0, one, 1)[0] == GP_OK
    want = acc.read("accumulate launches")
    if f32:
        # one rounding of the float64 sum instead of P
        assert np.array_equal(got, want.astype(np.float32))
        return
    off = ~np.eye(n1, cols, dtype=bool) if n2 is None else np.ones((n1, cols), dtype=bool)
    assert np.array_equal(got[off], want[off]), "%d entries differ from the accumulate launches" % np.count_nonzero(got[off] != want[off])
    if n2 is None:
        # on the diagonal the sum kernel adds the jitter last, the launches first: two orders of the same P + 1 positive terms,
        # each partial sum rounded once, so they differ by at most P roundings of the total
        dg, dw = np.diag(got), np.diag(want)
        assert np.all(np.abs(dg - dw) <= P * 2.0 * E53 * np.abs(dw))


@pytest.mark.parametrize("why", ["P1", "P9", "mixed_mpad", "mpad12", "matern52_envelope"])
def test_sum_kernel_declines(gp_handle, why):
    h, keep = gp_handle, []
    kerns = {"P1": cc.sum_kernels(1, 4), "P9": cc.sum_kernels(9, 4),
             "mixed_mpad": [cc.kernel(cc.M12, 3, 0.01), cc.kernel(cc.M12, 5, 0.02)],
             "mpad12": [cc.kernel(cc.M12, 9, 0.01), cc.kernel(cc.M12, 12, 0.02)],
             "matern52_envelope": [cc.kernel(cc.M12, 3, 0.01), cc.kernel(cc.M52, 3, 0.02)]}[why]
    z, x, cols, items_for = _sum_setup(h, kerns, 109, 1001, 0, 0, keep, 0.0)
    out = Out(h, 109, 1001, 1001)
    st, form, seg = _cov(h, "sum declines " + why, 2, items_for(out, range(len(kerns))), len(kerns))
    assert (st, form) == (GP_ERR_UNSUPPORTED, -1)
    assert out.untouched()


# ---- feature tables ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ktype", [cc.M12, cc.M52], ids=["m12", "m52"])
@pytest.mark.parametrize("m", cc.FEATURE_M)
def test_grouped_feature_tables(gp_handle, m, ktype):
    from gpitch_amd import _lib
    h, keep = gp_handle, []
    mp = cr.sm_mpad(m)
    rng = np.random.RandomState(m)
    xs = cc.frames(300)
    dxs = h.to_device(xs)
    specs = [(37, "shared"), (21, "self"), (50, "own")]
    items = (_lib.DebugCovItem * len(specs))()
    recs = []
    for k, (n1, frames) in enumerate(specs):
        kern = cc.kernel(ktype, m, 0.01, seed=k)
        z = rng.rand(n1) * 0.02
        x2 = {"shared": xs, "self": None, "own": rng.rand(129) * 0.02}[frames]
        n2 = n1 if x2 is None else x2.size
        dz = h.to_device(z)
        dx2 = h.to_device(x2) if frames == "own" else None
        keep += [dz, dx2]
        t_feat, p_feat = _feat(h, kern, n1, n2, keep, fill=SENT64)
        out = Out(h, n1, n2)
        _item(items[k], _desc(h, kern, keep), dz.data_ptr(), dx2.data_ptr() if dx2 is not None else None, out, p_feat, n1,
              -1 if frames == "shared" else n2)
        recs.append((kern, z, x2, t_feat, out))
    st, form, seg = _cov(h, "features m %d" % m, 1, items, len(specs), dxs.data_ptr(), xs.size)
    assert (st, form) == (GP_OK, 0)
    for k, (kern, z, x2, t_feat, out) in enumerate(recs):
        flat = t_feat.cpu().numpy()
        n1 = z.size
        blocks = [(0, z)] + ([] if x2 is None else [(-(-(2 * mp * n1) // 32) * 32, x2)])
        used = np.zeros(flat.size, dtype=bool)
        for off, pts in blocks:
            tab = flat[off:off + 2 * mp * pts.size].reshape(2 * mp, pts.size)
            used[off:off + 2 * mp * pts.size] = True
            want = cr.feature_table(kern, pts, mp)
            for q in range(mp):
                for row in (q, mp + q):
                    if q < m:
                        # 2 ulp of sqrt(e_q): |cos|, |sin| <= 1, so an ulp of the factor bounds an ulp of the product
                        tol = 2.0 * np.spacing(np.sqrt(kern["energy"][q]))
                        err = np.max(np.abs(tab[row].astype(cr.LD) - want[row]))
                        assert err <= tol, "record %d feature row %d: error %.3g, 2 ulp = %.3g" % (k, row, err, tol)
                    else:
                        assert np.all(tab[row] == 0.0) and not np.any(np.signbit(tab[row])), "record %d padding row %d" % (k, row)
        assert np.all(flat[~used] == SENT64), "record %d: written outside the two tables" % k
        _check("features m %d record %d" % (m, k), out.read("features"), cr.oracle(kern, z, x2))


# ---- what the entry refuses --------------------------------------------------------------------------------------------------
def test_debug_entry_refuses_what_no_launcher_checks(gp_handle):
    from gpitch_amd import _lib
    h, keep = gp_handle, []
    x = cc.frames(4096)
    dxs = h.to_device(x)
    z = cc.inducing(256, float(x.max()))
    dz = h.to_device(z)

    def launch(kerns, es=1, own=False, ld_pad=0, acc=0, ws_bytes=None, f32=False):
        items = (_lib.DebugCovItem * len(kerns))()
        outs = []
        for k, kern in enumerate(kerns):
            _, p_feat = _feat(h, kern, 256, 4096, keep)
            out = Out(h, 256, 4096, 4096 + ld_pad, f32=f32)
            _item(items[k], _desc(h, kern, keep), dz.data_ptr(), dxs.data_ptr() if own else None, out, p_feat, 256, 4096 if own else -1,
                  accumulate=acc)
            outs.append(out)
        st, form, seg = _cov(h, "refusal", 1, items, len(kerns), dxs.data_ptr(), 4096, es, ws_bytes)
        assert all(o.untouched() for o in outs), "a refused launch wrote"
        return st

    k12 = cc.kernel(cc.M12, 12, 0.01)
    assert launch([k12, cc.kernel(cc.M52, 12, 0.01)]) == GP_ERR_BAD_ARG            # two families
    assert launch([k12, cc.kernel(cc.M12, 8, 0.01)]) == GP_ERR_BAD_ARG             # two padded partial counts
    assert launch([k12], own=True) == GP_ERR_BAD_ARG                               # the lean form beside a record's own frames
    assert launch([k12], ld_pad=1) == GP_ERR_BAD_ARG                               # engine strips have even strides
    assert launch([k12], es=2) == GP_ERR_BAD_ARG                                   # float32 strips promised, float64 given
    assert launch([k12], es=0, acc=1) == GP_ERR_BAD_ARG                            # the matrix-core forms do not accumulate
    assert launch([k12], ws_bytes=191) == GP_ERR_WORKSPACE
