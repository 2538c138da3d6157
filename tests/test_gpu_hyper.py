"""The kernel-gradient contractions of bwd.hip as operators: one launch of a host entry through gp_debug_hyper_contract on the
test's own buffers, against the long-double reference of tests/hyper_ref.py within the bound DERIVED in its docstring (no
tolerance here comes from a GPU run), at every form, flag and edge of tests/hyper_cases.py.

Every launch runs twice and must repeat its bits.  The partial records and the gz blocks sit between sentinel guard bands more
than one record wide and hold what a plan reserves (gp_debug_hyper_records): the reported count must equal the expected form's
(which is how a test proves WHICH kernel ran), stay within that reserve, and nothing may be written behind the records.
Nothing from the library is imported at module level (the CPU run collects this file).

Wall time of this file on one MI355X: 277 tests in 14 s, most of it the long-double references on the host.
"""
import ctypes as C

import numpy as np
import pytest

import hyper_cases as hc
import hyper_ref as hr

pytestmark = pytest.mark.gpu

LD = np.longdouble
SENT = -7.0e77
GP_OK, GP_ERR_BAD_ARG, GP_ERR_WORKSPACE, GP_ERR_UNSUPPORTED = 0, 1, 5, 6


class Guarded(object):
    """n doubles between two guard bands, everything pre-filled with the sentinel (or the body with `init`)"""

    def __init__(self, h, n, guard, init=None):
        self.n, self.guard = n, guard
        host = np.full(n + 2 * guard, SENT)
        if init is not None:
            host[guard:guard + n] = init
        self.initial = host
        self.t = h.torch.as_tensor(host.copy(), device=h.device)
        self.ptr = self.t.data_ptr() + 8 * guard

    def reset(self, h):
        self.t.copy_(h.torch.as_tensor(self.initial))

    def read(self, what):
        flat = self.t.cpu().numpy()
        g = self.guard
        assert np.array_equal(flat[:g], self.initial[:g]) and np.array_equal(flat[g + self.n:], self.initial[g + self.n:]), \
            "%s: a guard band changed" % what
        return flat[g:g + self.n]


def _dev(h, a, ld=None, dtype=np.float64, misalign=0):
    """a host array on the device: (tensor, pointer); a matrix with leading dimension ld holds NaN in its padding columns;
    misalign: the pointer is 8-byte but not 16-byte aligned"""
    if a is None:
        return None, None
    a = np.asarray(a)
    if a.ndim == 2 and ld is not None and ld != a.shape[1]:
        full = np.full((a.shape[0], ld), np.nan)
        full[:, :a.shape[1]] = a
        a = full
    flat = np.ascontiguousarray(a.astype(dtype)).ravel()
    if misalign:
        flat = np.concatenate([np.zeros(1, dtype), flat, np.zeros(1, dtype)])
    t = h.torch.as_tensor(flat, device=h.device)
    return t, t.data_ptr() + (8 if misalign else 0)


def _call(h, name, entry, items, fins, count, fl):
    from gpitch_amd import _lib
    ws = h.workspace(160 * max(count, 1))
    nparts, taken = C.c_int32(-1), C.c_int32(-1)
    st = h.lib.gp_debug_hyper_contract(h.h, entry, items, fins, count, C.byref(fl), C.c_void_p(ws.data_ptr()), 160 * max(count, 1),
                                       C.byref(nparts), C.byref(taken))
    try:
        h.sync()
    except _lib.GpitchError as e:
        if e.status == _lib.GP_ERR_HIP:       # a device fault: nothing more may run on this GPU from this process
            pytest.exit("HIP error after gp_debug_hyper_contract (%s): %s" % (name, e), returncode=3)
        raise
    if st == _lib.GP_ERR_HIP:
        pytest.exit("HIP error from gp_debug_hyper_contract (%s)" % name, returncode=3)
    return st, nparts.value, taken.value


def _records_cap(h, n2, n1):
    return h.lib.gp_debug_hyper_records(n2, n1)


class Launch(object):
    """device buffers and records of one contraction case"""

    def __init__(self, h, c, inp, nparts_cap):
        from gpitch_amd import _lib
        self.c, self.inp = c, inp
        ktype, m, n1, n2 = c["type"], c["m"], c["n1"], c["n2"]
        self.ns = ns = 2 + 2 * m
        self.keep = keep = []
        g32 = bool(c.get("g32"))
        st = np.float32 if g32 else np.float64
        ldg, ldk = n2 + c.get("ldg_pad", 0), n2 + c.get("ldk_pad", 0)
        t_theta, p_theta = _dev(h, inp["theta"])
        t_x1, p_x1 = _dev(h, inp["x1"])
        t_x2, p_x2 = (t_x1, p_x1) if inp["x2"] is inp["x1"] else _dev(h, inp["x2"])
        t_kv, p_kv = _dev(h, inp["kvals"], ldk, st)
        keep += [t_theta, t_x1, t_x2, t_kv]
        count = len(inp["recs"])
        self.items = (_lib.DebugHyperItem * count)()
        self.parts, self.gz = [], []
        self.ncb = -(-n2 // 256)
        shared = {}
        mp = hc.sm_mpad(m) if ktype in hr.MERCER else 0
        for k, rec in enumerate(inp["recs"]):
            if id(rec) in shared:
                ptrs = shared[id(rec)]
            else:
                ptrs = []
                for name, ld, dt, mis in (("G", ldg, st, c.get("misalign", 0)), ("alpha", None, np.float64, 0), ("gm", None, np.float64, 0),
                                          ("gscale", None, np.float64, 0)):
                    t, p = _dev(h, rec[name], ld, dt, mis)
                    keep.append(t)
                    ptrs.append(p)
                shared[id(rec)] = ptrs
            it = self.items[k]
            it.kern = _lib.KernelDesc(ktype, m, p_theta)
            it.x1, it.x2 = p_x1, (None if c.get("shared_x2") else p_x2)
            it.G, it.alpha, it.gm, it.gscale = ptrs
            it.kvals = p_kv
            it.ldg, it.ldk = ldg, (ldk if p_kv else 0)
            it.n1, it.n2, it.symmetric, it.g32 = n1, n2, int(bool(c.get("symmetric"))), int(g32)
            self.parts.append(Guarded(h, nparts_cap * ns, 2 * ns + 64))
            it.partials = self.parts[-1].ptr
            if c.get("with_gz"):
                self.gz.append(Guarded(h, self.ncb * n1, n1 + 64))
                it.gz = self.gz[-1].ptr
            if mp and (k == 0 or (k == 1 and not c.get("share"))):
                feat = h.torch.full((2 * mp * (n1 + n2) + 64,), float("nan"), dtype=h.torch.float64, device=h.device)
                keep.append(feat)
                it.feat, it.feat_from = feat.data_ptr(), -1
            else:
                it.feat, it.feat_from = None, (0 if mp else -1)
        self.fl = _lib.DebugHyperFlags()
        self.fl.with_gz, self.fl.use_mfma = int(bool(c.get("with_gz"))), c.get("use_mfma", 1)
        self.fl.g32_items, self.fl.lean_items, self.fl.gscale_items = int(g32), c.get("lean_items", 1), int(bool(c.get("gscale")))
        if c.get("shared_x2"):
            self.fl.x2_shared, self.fl.n2_shared = p_x2, n2
        self.count = count

    def go(self, h):
        return _call(h, self.c["name"], self.c["entry"], self.items, None, self.count, self.fl)

    def read(self):
        name = self.c["name"]
        return ([p.read(name + " partials %d" % k) for k, p in enumerate(self.parts)],
                [g.read(name + " gz %d" % k) for k, g in enumerate(self.gz)])


def _check_case(h, c):
    form = hc.expected_form(**hc.form_kwargs(c))
    if c.get("geometry"):
        assert (form["col_seg"], form["nseg"]) == c["geometry"]
    inp = hc.inputs(c)
    n1, n2, ns = c["n1"], c["n2"], 2 + 2 * c["m"]
    cap = _records_cap(h, n2, n1)         # the buffers hold what a plan reserves: no form may write past it
    assert form["nparts"] <= cap
    L = Launch(h, c, inp, cap)
    st, nparts, _ = L.go(h)
    assert st == GP_OK, (c["name"], st, h.lib.gp_last_error(h.h))
    parts, gzs = L.read()
    # which kernel ran: the record count of the expected form, and nothing written behind those records
    assert nparts == form["nparts"], (c["name"], form["inst"], nparts, form["nparts"])
    assert all(np.all(p[nparts * ns:] == SENT) for p in parts), c["name"] + ": records written beyond the reported count"
    st2, nparts2, _ = L.go(h)
    parts2, gzs2 = L.read()
    assert st2 == GP_OK and nparts2 == nparts
    for a, b in zip(parts + gzs, parts2 + gzs2):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c["name"] + ": the second run differs"
    kv = inp["kvals"] if form["form"] > 0 else None
    terms = hr.kernel_terms(c["type"], inp["theta"], inp["x1"], inp["x2"], kuu=bool(c.get("symmetric")), kvals=kv)
    ref = None
    for k, rec in enumerate(inp["recs"]):
        what = "%s [%s] record %d" % (c["name"], form["inst"], k)
        if not (c.get("share") and k):
            ref = hr.contract_ref(c["type"], inp["theta"], inp["x1"], inp["x2"], rec["G"], alpha=rec["alpha"], gm=rec["gm"],
                                  symmetric=bool(c.get("symmetric")), gscale=rec["gscale"], want_gz=bool(c.get("with_gz")), terms=terms)
        else:
            assert np.array_equal(parts[k].view(np.uint8), parts[0].view(np.uint8)), what + ": differs from record 0 on the same operands"
            continue
        p = parts[k][:nparts * ns].reshape(nparts, ns)
        assert np.all(np.isfinite(p)), what + ": a record is not finite (or was never written)"
        got = p.astype(LD).sum(axis=0)
        tol = hr.bound(ref["A"], ref["C"], form["form"], form["wg_rows"], form["col_seg"])
        err = np.abs(got - ref["sums"])
        print("%s: worst error / bound %.3g" % (what, float((err / np.maximum(tol, LD(1e-300))).max())))
        assert np.all(err <= tol), "%s: sums %r, reference %r, bound %r" % (what, got.astype(float), ref["sums"].astype(float), tol.astype(float))
        if c.get("with_gz"):
            g = gzs[k].reshape(L.ncb, n1)
            assert np.all(np.isfinite(g)), what + ": gz not finite (or never written)"
            tz = hr.bound(ref["gzA"], ref["gzC"], 0, form["wg_rows"], 0)
            ez = np.abs(g.astype(LD) - ref["gz"])
            bad = ~(ez <= tz)
            assert not bad.any(), "%s: gz wrong at (column block, row) %r: %r vs %r, bound %r" % (
                what, tuple(np.argwhere(bad)[0]), g[bad][0], float(ref["gz"][bad][0]), float(tz[bad][0]))
    return form


def _ids(cs):
    return [c["name"] for c in cs]


@pytest.mark.parametrize("c", hc.generic_cases(), ids=_ids(hc.generic_cases()))
def test_generic_contractions(gp_handle, c):
    """hyper_contract_kernel at every stationary type and spectral-mixture padding, hyper_m12sm_kernel, with and without the
    inducing-input gradient; with_gz, symmetric (Kuu side), alpha / gm, float32 strips, ldg > n2, a shared x2, one at a time;
    n1 in 1, 7, 8, 9, 33 x n2 in 1, 255, 256, 257, 513; the 8-row / 32-row workgroup switch at n1 n2 = 2^20"""
    _check_case(gp_handle, c)


@pytest.mark.parametrize("c", hc.rows_cases(), ids=_ids(hc.rows_cases()))
def test_matrix_core_contractions(gp_handle, c):
    """hyper_sm_rows_lean_kernel at NT 1, 2, 3 (float64, float32, column scale) and hyper_sm_rows_kernel at NT 1, 2 x both
    envelopes x both strip types; ragged rows and columns, odd strides, a misaligned strip, 2 / 4 / 4 column segments, segments
    beyond either column table, every block kind of the separable envelope, an inducing input equal to a frame"""
    form = _check_case(gp_handle, c)
    assert form["form"] > 0 or "generic" in c["name"]


@pytest.mark.parametrize("c", hc.onehot_cases(), ids=_ids(hc.onehot_cases()))
def test_one_hot_weights(gp_handle, c):
    """G zero but for one entry (alpha null, or zero where the form reads it): the result is that single term within its own
    bound — no other entry's size to hide a dropped, doubled or misplaced one.  First / last row and column, first / last column
    of every segment, both columns of a paired load, the four k-lanes, columns of straddling and both-sides blocks."""
    _check_case(gp_handle, c)


@pytest.mark.parametrize("c", hc.sum_cases(), ids=_ids(hc.sum_cases()))
def test_sum_kernel(gp_handle, c):
    """hyper_contract_sum_kernel<P>, P = 2..6 with mixed m in 1..4: each kernel's records equal its own contraction; P = 1, P = 7,
    an m of 5 and a non-Mercer member come back not taken with the records' sentinels intact"""
    from gpitch_amd import _lib
    h = gp_handle
    rng = np.random.RandomState(7)
    n1, n2, P = c["n1"], c["n2"], c["P"]
    x1, x2 = np.sort(rng.rand(n1)), (np.arange(n2) + 0.3 * rng.rand(n2)) / n2
    g32 = bool(c.get("g32"))
    G = rng.randn(n1, n2).astype(np.float32 if g32 else np.float64)
    alpha, gm = (rng.randn(n1), rng.randn(n2)) if c.get("alpha", True) else (None, None)
    form = hc.expected_form(2, hr.MERCER12, 0, n1, n2, count=P)
    cap = _records_cap(h, n2, n1)
    keep = [_dev(h, a, None, dt) for a, dt in ((x1, np.float64), (x2, np.float64), (G, G.dtype), (alpha, np.float64), (gm, np.float64))]
    items = (_lib.DebugHyperItem * P)()
    thetas, parts = [], []
    for k in range(P):
        t, m = c["types"][k], c["ms"][k]
        thetas.append(hc.theta_for(t, m, seed=k))
        tt, pt = _dev(h, thetas[k])
        keep.append((tt, pt))
        it = items[k]
        it.kern = _lib.KernelDesc(t, m, pt)
        it.x1, it.x2, it.G, it.alpha, it.gm = [p for _, p in keep[:5]]
        it.ldg, it.n1, it.n2, it.g32, it.feat_from = n2, n1, n2, int(g32), -1
        parts.append(Guarded(h, cap * (2 + 2 * m), 2 * (2 + 2 * m) + 64))
        it.partials = parts[-1].ptr
        if t in hr.MERCER:
            feat = h.torch.full((2 * hc.sm_mpad(m) * (n1 + n2) + 64,), float("nan"), dtype=h.torch.float64, device=h.device)
            keep.append(feat)
            it.feat = feat.data_ptr()
    fl = _lib.DebugHyperFlags()
    outs = []
    for run in range(2):
        st, nparts, taken = _call(h, c["name"], 2, items, None, P, fl)
        outs.append([p.read("%s kernel %d" % (c["name"], k)) for k, p in enumerate(parts)])
        if not c["taken"]:
            assert (st, taken) == (GP_ERR_UNSUPPORTED, 0), (c["name"], st, taken)
            assert all(np.all(o == SENT) for o in outs[-1]), c["name"] + ": a refused launch wrote records"
            return
        assert (st, taken, nparts) == (GP_OK, 1, form["nparts"]), (c["name"], st, taken, nparts)
        assert nparts <= cap
    for a, b in zip(*outs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c["name"] + ": the second run differs"
    for k in range(P):
        ref = hr.contract_ref(c["types"][k], thetas[k], x1, x2, G, alpha=alpha, gm=gm)
        nsk = 2 + 2 * c["ms"][k]
        assert np.all(outs[0][k][form["nparts"] * nsk:] == SENT), c["name"] + ": records written beyond the reported count"
        got = outs[0][k][:form["nparts"] * nsk].reshape(form["nparts"], nsk).astype(LD).sum(axis=0)
        tol = hr.bound(ref["A"], ref["C"], 0, form["wg_rows"], 0)
        assert np.all(np.abs(got - ref["sums"]) <= tol), "%s kernel %d [%s]: %r vs %r" % (c["name"], k, form["inst"], got.astype(float),
                                                                                         ref["sums"].astype(float))


@pytest.mark.parametrize("c", hc.finish_cases(), ids=_ids(hc.finish_cases()))
def test_finish(gp_handle, c):
    """hyper_finish_items_kernel, single and items: np_uf / np_uu at 0, 1, 255, 256, 257; the gv_sum (Kdiag) term of every family
    — variance always, energies only where Kdiag sums them, NOT for the Matern-5/2 product; g_z over 255, 256, 257 rows and 1 or 3
    column blocks a side; mixed m in one launch.  g_theta and g_z start prefilled: the finish accumulates."""
    from gpitch_amd import _lib
    h = gp_handle
    rng = np.random.RandomState(11)
    n = len(c["recs"])
    fins = (_lib.DebugHyperFinish * n)()
    keep, host, outs_g, outs_z = [], [], [], []
    for k, r in enumerate(c["recs"]):
        t, m, n1 = r["type"], r["m"], r["n1"]
        ns = 2 + 2 * m
        theta = hc.theta_for(t, m, seed=k)
        hk = dict(theta=theta, p_uf=rng.randn(r["np_uf"], ns), p_uu=rng.randn(r["np_uu"], ns), gv=(rng.randn() if r["gv"] else None),
                  g0=rng.randn(ns), z0=rng.randn(n1), gz_uf=rng.randn(r["cb_uf"], n1), gz_uu=rng.randn(r["cb_uu"], n1))
        host.append(hk)
        f = fins[k]
        dv = {}
        for name in ("theta", "p_uf", "p_uu", "gz_uf", "gz_uu"):
            dv[name] = _dev(h, hk[name] if hk[name].size else None)
        dv["gv"] = _dev(h, None if hk["gv"] is None else np.array([hk["gv"]]))
        keep.append(dv)
        f.kern = _lib.KernelDesc(t, m, dv["theta"][1])
        f.p_uf, f.p_uu, f.gv_sum, f.gz_uf, f.gz_uu = dv["p_uf"][1], dv["p_uu"][1], dv["gv"][1], dv["gz_uf"][1], dv["gz_uu"][1]
        f.np_uf, f.np_uu, f.cb_uf, f.cb_uu, f.n1 = r["np_uf"], r["np_uu"], r["cb_uf"], r["cb_uu"], n1
        outs_g.append(Guarded(h, ns, ns + 64, init=hk["g0"]))
        f.g_theta = outs_g[-1].ptr
        if n1 and (r["cb_uf"] or r["cb_uu"]):
            outs_z.append(Guarded(h, n1, n1 + 64, init=hk["z0"]))
            f.g_z = outs_z[-1].ptr
        else:
            outs_z.append(None)
    fl = _lib.DebugHyperFlags()
    runs = []
    for run in range(2):
        for o in outs_g + [z for z in outs_z if z is not None]:
            o.reset(h)
        st, blocks, _ = _call(h, c["name"], c["entry"], None, fins, n, fl)
        assert st == GP_OK, (c["name"], st, h.lib.gp_last_error(h.h))
        runs.append([o.read(c["name"]) for o in outs_g] + [z.read(c["name"]) for z in outs_z if z is not None])
    for a, b in zip(*runs):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), c["name"] + ": the second run differs"
    for k, (r, hk) in enumerate(zip(c["recs"], host)):
        has_z = outs_z[k] is not None
        ref = hr.finish_ref(r["type"], hk["theta"], hk["g0"], hk["p_uf"], hk["p_uu"], hk["gv"], z0=hk["z0"] if has_z else None,
                            gz_uf=hk["gz_uf"], gz_uu=hk["gz_uu"])
        got = outs_g[k].read(c["name"]).astype(LD)
        tol = hr.finish_bound(ref["gA"], r["np_uf"] + r["np_uu"])
        assert np.all(np.abs(got - ref["g"]) <= tol), "%s record %d: g_theta %r vs %r" % (c["name"], k, got.astype(float), ref["g"].astype(float))
        if has_z:
            gz = outs_z[k].read(c["name"]).astype(LD)
            assert np.all(np.abs(gz - ref["z"]) <= hr.finish_bound(ref["zA"], 0)), "%s record %d: g_z" % (c["name"], k)


def _one(h, **kw):
    c = hc._c("refusal", **kw)
    form = hc.expected_form(**hc.form_kwargs(c))
    return c, Launch(h, c, hc.inputs(c), _records_cap(h, c["n2"], c["n1"]))


def test_refusals_launch_nothing(gp_handle):
    """flags a launcher does not admit, and records that break what a form reads unasked: an error, and the sentinels intact"""
    h = gp_handle
    base = dict(type=hr.MERCER12, m=5, n1=64, n2=96, entry=1, count=2)

    def refused(want, **kw):
        c, L = _one(h, **dict(base, **kw))
        mutate = kw.get("mutate")
        if mutate:
            mutate(L)
        st, _, _ = L.go(h)
        assert st == want, (kw, st, h.lib.gp_last_error(h.h))
        parts, gzs = L.read()
        assert all(np.all(p == SENT) for p in parts + gzs), "a refused launch wrote (%r)" % (kw,)

    # a column scale needs the lean form: not without lean_items, not on float32 strips, not with gz, not beside the generic
    # kernel, not on shapes the lean form declines, not in the single-record entry
    refused(GP_ERR_UNSUPPORTED, gscale=1, lean_items=0)
    refused(GP_ERR_UNSUPPORTED, gscale=1, g32=1)
    refused(GP_ERR_UNSUPPORTED, gscale=1, with_gz=1)
    refused(GP_ERR_UNSUPPORTED, gscale=1, use_mfma=0)
    refused(GP_ERR_UNSUPPORTED, gscale=1, n1=63)
    refused(GP_ERR_UNSUPPORTED, gscale=1, m=25)
    refused(GP_ERR_UNSUPPORTED, gscale=1, type=hr.MERCER52, m=3)
    refused(GP_ERR_UNSUPPORTED, gscale=1, entry=0, count=1)
    # the matrix-core forms read alpha, gm and kvals of every record; the lean form trusts alignment and even strides
    refused(GP_ERR_BAD_ARG, alpha=False)
    refused(GP_ERR_BAD_ARG, kvals=False)
    refused(GP_ERR_BAD_ARG, ldg_pad=1)
    refused(GP_ERR_BAD_ARG, ldk_pad=1)
    refused(GP_ERR_BAD_ARG, misalign=1)

    def two_families(L):
        L.items[1].kern.num_partials = 4
    refused(GP_ERR_BAD_ARG, mutate=two_families)
    # arguments
    c, L = _one(h, **base)
    from gpitch_amd import _lib
    ws = h.workspace(1024)
    nparts, taken = C.c_int32(-1), C.c_int32(-1)
    call = lambda entry, count, wsp, wsb: h.lib.gp_debug_hyper_contract(h.h, entry, L.items, None, count, C.byref(L.fl), C.c_void_p(wsp), wsb,
                                                                         C.byref(nparts), C.byref(taken))
    assert call(5, 2, ws.data_ptr(), 1024) == GP_ERR_BAD_ARG and call(1, 0, ws.data_ptr(), 1024) == GP_ERR_BAD_ARG
    assert call(1, 2, ws.data_ptr() + 8, 1000) == GP_ERR_WORKSPACE and call(1, 2, ws.data_ptr(), 319) == GP_ERR_WORKSPACE
    assert call(3, 1, ws.data_ptr(), 1024) == GP_ERR_BAD_ARG      # a finish without finish records
    h.sync()
    parts, _ = L.read()
    assert all(np.all(p == SENT) for p in parts)
