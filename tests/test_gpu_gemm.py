"""The GEMM families as operators: one launch of a host entry through gp_debug_gemm on the test's own buffers, against the
numpy reference of tests/gemm_ref.py, at every form (wave, lean strip, generic), flag and tile edge (tables: gemm_cases.py).

Every case runs twice over:
  * on small INTEGER inputs, where every partial sum is exact whatever its order (tests/test_gemm_ref_cpu.py checks the
    condition for each case): the device must equal the reference bit for bit (-0.0 counts as 0.0);
  * on standard-normal inputs (seed 0) against the long-double reference within the bounds DERIVED in gemm_ref.py's docstring —
    no tolerance here comes from a GPU run — and a second run must repeat the first bit for bit.
C and every partial-sum buffer sit inside a larger allocation filled with a sentinel: guard bands, padding columns (ldc > N),
rows outside a row-block range and partial rows the launch does not own must still hold it afterwards.  The structurally zero
triangle of a triangular operand holds 3e33 (role 1 in the wave forms: above the diagonal 64 x 64 BLOCKS only — those forms'
contract is a W with exact zeros above the diagonal).
Nothing from the library is imported at module level (the CPU run collects this file).
"""
import ctypes as C

import numpy as np
import pytest

import gemm_cases as gc
from gemm_ref import EPI_COLDOT, EPI_COLSUMSQ, EPI_STORE, LD, TRI_LOWER, effective_flags, gemm_ref, partial_rows_rule

pytestmark = pytest.mark.gpu

GUARD = 64                                 # elements of sentinel in front of and behind every output buffer
SENT = {np.dtype(np.float64): -7.0e77, np.dtype(np.float32): np.float32(-7.0e30)}
GP_OK, GP_ERR_UNSUPPORTED = 0, 6
MAX_SLICES = 64


def _ids(cs):
    return [c["name"] if isinstance(c, dict) else c[0]["name"] for c in cs]


class Out(object):
    """an output buffer rows x ld (cols used) between two guard bands, pre-filled with the sentinel (or `init` in its columns)"""

    def __init__(self, h, rows, ld, cols, dtype, init=None, guard=GUARD):
        self.rows, self.ld, self.cols, self.dtype, self.guard = rows, ld, cols, np.dtype(dtype), guard
        host = np.full(2 * guard + rows * ld, SENT[self.dtype], dtype=self.dtype)
        if init is not None:
            host[guard:guard + rows * ld].reshape(rows, ld)[:init.shape[0], :init.shape[1]] = init
        self.initial = host
        self.t = h.torch.as_tensor(host.copy(), device=h.device)
        self.ptr = self.t.data_ptr() + guard * self.dtype.itemsize

    def read(self):
        return self.t.cpu().numpy()

    def body(self, flat):
        return flat[self.guard:self.guard + self.rows * self.ld].reshape(self.rows, self.ld)


def _row_guard(n):
    """guard bands of a partial-row buffer: more than one whole row on either side (a row written one block off lands in them)"""
    return GUARD * (n // GUARD + 2)


def _dev(h, a, dtype, ld=None):
    """a host matrix (or vector) on the device with leading dimension ld; the padding columns hold garbage"""
    if a is None:
        return None
    a = np.asarray(a)
    if a.ndim == 2 and ld is not None and ld != a.shape[1]:
        full = np.full((a.shape[0], ld), gc.GARBAGE, dtype=np.float64)
        full[:, :a.shape[1]] = a
        a = full
    return h.torch.as_tensor(np.ascontiguousarray(a.astype(dtype)), device=h.device)


def _alloc(h, c, inputs):
    kind = c["kind"]
    f = effective_flags(c["flags"]) if kind in (0, 2) else c["flags"]
    bufs = []
    for p in inputs:
        M, N, K = p["M"], p["N"], p["K"]
        b = dict(p=p)
        if kind in (1, 3):
            st = np.float32 if kind == 3 else np.float64
            b["A"], b["B"] = _dev(h, p["A"], st, p["lda"]), _dev(h, p["B"], st, p["ldb"])
            b["C"] = Out(h, M, p["ldc"], M, np.float64)
            b["o0"] = Out(h, 1, M, M, np.float64)
            b["o1"] = Out(h, MAX_SLICES + 2, M, M, np.float64, guard=_row_guard(M))
            b["xa"] = Out(h, 1, M, M, np.float64, init=None if p["xa0"] is None else p["xa0"][None, :])
            b["o2"] = h.torch.full((MAX_SLICES * M * M,), float("nan"), dtype=h.torch.float64, device=h.device)
        else:
            sb = np.float32 if kind == 2 else np.float64
            b["A"], b["B"] = _dev(h, p["A"], np.float64, p["lda"]), _dev(h, p["B"], sb, p["ldb"])
            b["C"] = Out(h, M, p["ldc"], N, sb, init=p["C0"])
            b["o0"] = Out(h, M // 64 + 2, N, N, np.float64, guard=_row_guard(N))
            b["o1"] = Out(h, M // 64 + 2, N, N, np.float64, guard=_row_guard(N))
            if f["a32_ok"]:
                b["xb"] = h.torch.full((M * M,), float("nan"), dtype=h.torch.float32, device=h.device)
        for v in ("v0", "v1", "v2"):
            b[v] = _dev(h, p[v], np.float64)
        bufs.append(b)
    return bufs


def _ptr(t):
    return None if t is None else int(t.data_ptr() if hasattr(t, "data_ptr") else t.ptr)


def _launch(h, c, bufs, form=None, flags=None, nsplit=0):
    """one gp_debug_gemm call: (status, partial rows)"""
    from gpitch_amd import _lib
    probs = (_lib.DebugGemmProblem * len(bufs))()
    for r, b in zip(probs, bufs):
        p = b["p"]
        r.A, r.B, r.C = _ptr(b["A"]), _ptr(b["B"]), _ptr(b["C"])
        r.v0, r.v1, r.v2 = _ptr(b["v0"]), _ptr(b["v1"]), _ptr(b["v2"])
        r.o0, r.o1, r.o2 = _ptr(b["o0"]), _ptr(b["o1"]), _ptr(b.get("o2"))
        r.xa, r.xb = _ptr(b.get("xa")), _ptr(b.get("xb"))
        r.M, r.N, r.K = p["M"], p["N"], p["K"]
        r.lda, r.ldb, r.ldc = p["lda"], p["ldb"], p["ldc"]
    fl = _lib.DebugGemmFlags()
    for k, v in (flags or c["flags"]).items():
        setattr(fl, k, v)
    ws = h.workspace(160 * len(bufs))
    rows = C.c_int32(-1)
    st = h.lib.gp_debug_gemm(h.h, probs, len(bufs), c["maxM"], c["maxN"], C.byref(fl), c["kind"], c["form"] if form is None else form,
                             nsplit, C.c_void_p(ws.data_ptr()), 160 * len(bufs), C.byref(rows))
    try:
        h.sync()
    except _lib.GpitchError as e:
        if e.status == _lib.GP_ERR_HIP:       # a device fault: nothing more may run on this GPU from this process
            pytest.exit("HIP error after gp_debug_gemm (%s): %s" % (c["name"], e), returncode=3)
        raise
    if st == _lib.GP_ERR_HIP:
        pytest.exit("HIP error from gp_debug_gemm (%s)" % c["name"], returncode=3)
    return st, rows.value


def _read(bufs):
    return [dict((k, b[k].read()) for k in ("C", "o0", "o1", "xa") if k in b) for b in bufs]


def _same_bits(outs_a, outs_b, what):
    for i, (a, b) in enumerate(zip(outs_a, outs_b)):
        for k in a:
            assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "%s: problem %d, %s differs" % (what, i, k)


def _check_region(flat, out, written, ref, bound, exact, what):
    """`flat`: the whole allocation read back.  Outside `written` (rows x cols of the body) everything must be as it was;
    inside, equal to `ref` (exact) or within `bound`."""
    w = np.zeros((out.rows, out.ld), bool)
    w[:written.shape[0], :written.shape[1]] = written
    wflat = np.zeros(flat.shape, bool)
    wflat[out.guard:out.guard + out.rows * out.ld] = w.ravel()
    same = (flat == out.initial) | wflat
    assert same.all(), "%s: %d entries outside the written region changed, first at flat offset %d (body starts at %d, ld %d)" % (
        what, int((~same).sum()), int(np.argmax(~same)), out.guard, out.ld)
    if not written.any():
        return
    dev = out.body(flat)[:written.shape[0], :written.shape[1]]
    if exact:
        bad = written & (dev != np.where(written, ref, 0).astype(out.dtype))
    else:
        with np.errstate(invalid="ignore"):
            bad = written & ~(np.abs(dev.astype(LD) - np.where(written, ref, 0)) <= np.where(written, bound, 0))
    if bad.any():
        i, j = np.argwhere(bad)[0]
        raise AssertionError("%s: %d of %d entries wrong, first at (%d, %d): device %r, reference %r%s" % (
            what, int(bad.sum()), int(written.sum()), i, j, dev[i, j], float(ref[i, j]), "" if exact else ", bound %.3g" % float(bound[i, j])))


def _tile_edge(c):
    f = c["flags"]
    if f["role"] >= 1 or f["big_tiles"] or c["kind"] == 2:
        return 128
    t64 = len(c["shapes"]) * (-(-c["maxM"] // 64)) * (-(-c["maxN"] // 64))
    if f["epilogue"] == EPI_STORE and f["tile_m0"] == 0 and f["tile_mcount"] == 0 and c["maxM"] >= 64 and c["maxN"] >= 64 and t64 < 320:
        return 32
    return 64


_REFS = {}


def _refs(c, inputs, exact, block_rows):
    key = (c["name"], exact, tuple(sorted(c["flags"].items())), block_rows)
    if key not in _REFS:
        _REFS.clear()          # (one case at a time: the tables are walked case by case)
        _REFS[key] = [gemm_ref(c["kind"], c["flags"], p["M"], p["N"], p["K"], p["A"], p["B"], C0=p["C0"], v0=p["v0"], v1=p["v1"], v2=p["v2"],
                               xa0=p["xa0"], exact=exact, block_rows=block_rows, tile=_tile_edge(c)) for p in inputs]
    return _REFS[key]


def _verify(c, bufs, outs, exact, rows, wave):
    """kinds 0 / 2: C, the partial rows and everything around them"""
    f = effective_flags(c["flags"])
    big = f["role"] >= 1 or f["big_tiles"] or c["kind"] == 2
    assert rows == partial_rows_rule(c["maxM"], wave, big), (rows, c["maxM"], wave, big)
    block_rows = 64 if (wave or not big) else 128
    refs = _refs(c, [b["p"] for b in bufs], exact, block_rows)
    for i, (b, o, r) in enumerate(zip(bufs, outs, refs)):
        what = "%s problem %d (%s)" % (c["name"], i, "integers" if exact else "normal")
        _check_region(o["C"], b["C"], r["written"], r["C"], r["bound_C"], exact, what + " C")
        for name, bit, bnd in (("o0", EPI_COLSUMSQ, "bound_o0"), ("o1", EPI_COLDOT, "bound_o1")):
            ref = r[name]
            written = ~np.isnan(ref) if (f["epilogue"] & bit) else np.zeros(ref.shape, bool)
            _check_region(o[name], b[name], written, ref, r[bnd], exact, what + " " + name)


def _verify_nt(c, bufs, outs, exact, ns):
    refs = _refs(c, [b["p"] for b in bufs], exact, 0)
    for i, (b, o, r) in enumerate(zip(bufs, outs, refs)):
        M = b["p"]["M"]
        what = "%s nsplit %d problem %d (%s)" % (c["name"], ns, i, "integers" if exact else "normal")
        full = np.ones((M, M), bool)
        _check_region(o["C"], b["C"], full, r["C"], r["bound_C"], exact, what + " H")
        H = b["C"].body(o["C"])[:, :M]
        if c["flags"]["triC"] == TRI_LOWER:
            assert np.array_equal(H, H.T), what + ": H is not its own mirror"
        none = np.zeros((1, M), bool)
        if r["u"] is None:
            _check_region(o["o0"], b["o0"], none, None, None, exact, what + " o0")
            _check_region(o["xa"], b["xa"], none, None, None, exact, what + " xa")
            _check_region(o["o1"], b["o1"], np.zeros((ns, M), bool), None, None, exact, what + " o1")
            continue
        one = np.ones((1, M), bool)
        bu = r["bound_u"][None, :]
        _check_region(o["o0"], b["o0"], one, r["u"][None, :], bu, exact, what + " o0 = X v2")
        _check_region(o["xa"], b["xa"], one, r["xa"][None, :], bu + np.abs(r["xa"][None, :]) * LD(2.0) ** -53, exact, what + " xa += X v2")
        # the per-slice partials: rows [0, ns) written, the rest untouched; their sum is u
        part = b["o1"].body(o["o1"])
        rest = o["o1"].copy()
        b["o1"].body(rest)[:ns, :] = SENT[np.dtype(np.float64)]
        assert np.array_equal(rest, b["o1"].initial), what + ": o1 changed outside its %d slice rows" % ns
        s = part[:ns].astype(LD).sum(axis=0)
        assert np.all(np.abs(s - r["u"]) <= (0 if exact else r["bound_u"])), what + ": the slice partials do not sum to X v2"


def _is_wave(c, form=None):
    form = c["form"] if form is None else form
    return form == 1


def _run(h, c, exact, form=None, flags=None, nsplit=0):
    inputs = gc.make_inputs(c, exact)
    bufs = _alloc(h, c, inputs)
    st, rows = _launch(h, c, bufs, form=form, flags=flags, nsplit=nsplit)
    assert st == GP_OK, (c["name"], st, h.lib.gp_last_error(h.h))
    return bufs, _read(bufs), rows


def _full_check(h, c, wave=None):
    """integers exactly, normal inputs within the derived bounds, and a second run of the latter bit for bit"""
    wave = _is_wave(c) if wave is None else wave
    for exact in (True, False):
        bufs, outs, rows = _run(h, c, exact)
        _verify(c, bufs, outs, exact, rows, wave)
    _, again, _ = _run(h, c, False)
    _same_bits(outs, again, c["name"] + ": second run")


# ---- kind 0, the generic kernel --------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", gc.generic_cases(), ids=_ids(gc.generic_cases()))
def test_generic_kernel_shapes_and_transposes(gp_handle, c):
    """gemm.hip's kernel at 32, 64 and 128 tiles, all four transposes, every 16 / 32 / 64 / 128 edge and the BK = 16 tail;
    batches of problems of different sizes under one grid (a smaller problem writes nothing outside itself), flattened grids
    that are a multiple of 8 (XCD renumbering on) and not"""
    _full_check(gp_handle, c)


@pytest.mark.parametrize("c", gc.structure_cases(), ids=_ids(gc.structure_cases()))
def test_generic_kernel_structure_flags(gp_handle, c):
    """triA / triB lower and upper with and without transposes (the other triangle holds 3e33), triC lower, beta = 1 and -0.5
    onto a non-zero C, scale_mode 1 and 2, every non-empty epilogue mask (without EPI_STORE C stays untouched)"""
    _full_check(gp_handle, c)


@pytest.mark.parametrize("pair", gc.tile32_cases(), ids=_ids(gc.tile32_cases()))
def test_tile32_agrees_with_tile64(gp_handle, pair):
    """a launch the gemm_tile32 switch admits (fewer than 320 64 x 64 tiles) and the same problems in a launch of exactly 320
    (one past the last admitted count): both exact on integers, hence equal to each other"""
    small, over = pair
    bs, os_, rs = _run(gp_handle, small, True)
    _verify(small, bs, os_, True, rs, False)
    bo, oo, ro = _run(gp_handle, over, True)
    _verify(over, bo, oo, True, ro, False)
    n = len(small["shapes"])
    for a, b in zip(os_, oo[:n]):
        assert np.array_equal(a["C"], b["C"])
    for c in (small, over):
        bufs, outs, rows = _run(gp_handle, c, False)
        _verify(c, bufs, outs, False, rows, False)
        _, again, _ = _run(gp_handle, c, False)
        _same_bits(outs, again, c["name"] + ": second run")


GEN_ROLE = gc.role_generic_cases()


@pytest.mark.parametrize("c", GEN_ROLE, ids=_ids(GEN_ROLE))
def test_roles_generic_kernel(gp_handle, c):
    """roles 1, 2, 3 on gemm.hip's dedicated 128-tile instantiations, whole and ragged M, N within a batch"""
    _full_check(gp_handle, c)


LEAN = gc.role_lean_cases()


@pytest.mark.parametrize("c", LEAN, ids=_ids(LEAN))
def test_roles_lean_strip_form(gp_handle, c):
    """gemm_strip.hip, called directly: roles 1, 2, 3; role 3 with alpha 1, 2, 0.5, 4"""
    _full_check(gp_handle, c)


@pytest.mark.parametrize("kind", [0, 2])
@pytest.mark.parametrize("why", ["alpha3", "beta", "M192", "role1-alpha2"])
def test_lean_form_refuses(gp_handle, kind, why):
    """what the lean form does not take comes back as GP_ERR_UNSUPPORTED and nothing is written"""
    kw = dict(alpha3=dict(role=3, alpha=3.0), beta=dict(role=3, beta=1.0), M192=dict(role=3), **{"role1-alpha2": dict(role=1, alpha=2.0)})[why]
    role = kw.pop("role")
    M = 192 if why == "M192" else 128
    c = gc.case("lean-refuse-" + why, kind, 2, gc._role_flags(role, uniform_aligned=1, **kw), [(M, 128, M)], ld="strip")
    inputs = gc.make_inputs(c, True)
    bufs = _alloc(gp_handle, c, inputs)
    st, _ = _launch(gp_handle, c, bufs)
    assert st == GP_ERR_UNSUPPORTED
    for b, o in zip(bufs, _read(bufs)):
        for k in ("C", "o0", "o1"):
            assert np.array_equal(o[k], b[k].initial), k


WAVE = gc.role_wave_cases()


@pytest.mark.parametrize("c", WAVE, ids=_ids(WAVE))
def test_roles_wave_form(gp_handle, c):
    """gemm_wave.hip, called directly: 1, 2, 3, 4, 5 and 7 tiles of 64 rows (the self-paired middle tile, even and odd pair
    counts), one and several 256-column groups, partial rows per 64-row tile"""
    _full_check(gp_handle, c)


@pytest.mark.parametrize("epi", [EPI_STORE, EPI_COLDOT, EPI_STORE | EPI_COLSUMSQ, 7])
def test_wave_form_role2_gives_the_sum_of_squares_only(gp_handle, epi):
    """gemm_wave.hip holds the tile of Lq^T A with its rows permuted inside each 64-row tile: a store or a dot with v0 would come
    out in the wrong rows (found by this file's first run; no engine launch asks for either).  The launcher refuses them, called
    directly and dispatched, and writes nothing"""
    fl = dict(gc._role_flags(2, wave64=True, uniform_aligned=1, rows64_ok=1), epilogue=epi)
    c = gc.case("wave-role2-epi%d" % epi, 0, 1, fl, [(128, 256, 128)], ld="strip")
    bufs = _alloc(gp_handle, c, gc.make_inputs(dict(c, flags=dict(fl, epilogue=7)), True))
    for form in (1, 0):
        st, _ = _launch(gp_handle, c, bufs, form=form)
        assert st == GP_ERR_UNSUPPORTED
    for b, o in zip(bufs, _read(bufs)):
        assert all(np.array_equal(o[k], b[k].initial) for k in ("C", "o0", "o1"))


# ---- row-block ranges ------------------------------------------------------------------------------------------------
RANGE = gc.range_cases(0) + gc.range_cases(2)


@pytest.mark.parametrize("c", RANGE, ids=_ids(RANGE))
def test_row_block_ranges(gp_handle, c):
    """(tile_m0, tile_mcount) on the wave, lean and generic forms, float64 and float32: rows outside the range and their
    partial rows stay untouched, a range past the end launches nothing, and (0, 1) followed by (1, 0) on the same buffers
    equals the whole launch bit for bit (the engine's early first row-block depends on it)"""
    h = gp_handle
    wave = c["form"] == 1
    for (m0, mc) in gc.RANGES:
        cr = gc.with_range(c, m0, mc)
        bufs, outs, rows = _run(h, cr, True)
        _verify(cr, bufs, outs, True, rows, wave)
        if 128 * m0 >= c["maxM"]:
            for b, o in zip(bufs, outs):
                assert all(np.array_equal(o[k], b[k].initial) for k in ("C", "o0", "o1"))
    bufs, whole, rows = _run(h, c, False)
    _verify(c, bufs, whole, False, rows, wave)
    _, again, _ = _run(h, c, False)
    _same_bits(whole, again, c["name"] + ": second run")
    parts = _alloc(h, c, gc.make_inputs(c, False))
    for (m0, mc) in ((0, 1), (1, 0)):
        st, _ = _launch(h, c, parts, flags=dict(c["flags"], tile_m0=m0, tile_mcount=mc))
        assert st == GP_OK
    _same_bits(whole, _read(parts), c["name"] + ": ranges (0, 1) + (1, 0) against the whole launch")


# ---- dispatch --------------------------------------------------------------------------------------------------------
DISPATCH = gc.dispatch_cases()


@pytest.mark.parametrize("triple", DISPATCH, ids=_ids(DISPATCH))
def test_dispatch_takes_the_documented_form(gp_handle, triple):
    """form 0 (as the library dispatches) equals, bit for bit on normal inputs, the form the documented rules name
    (gemm_cases.expected_form), at every aligned shape of the role and split-K tables; two runs of form 0 agree too.  The shapes
    of the form tables are checked against the reference there, under the form itself; the others here"""
    c, expect, verify = triple
    h = gp_handle
    if c["kind"] in (1, 3):
        ns = c["nsplits"][0]
        b0, o0, _ = _run(h, c, False, nsplit=ns)
        _verify_nt(c, b0, o0, False, ns)
        _, o1, _ = _run(h, c, False, form=expect, nsplit=ns)
        _, again, _ = _run(h, c, False, nsplit=ns)
    else:
        takes = h.lib.gp_debug_wave_takes(c["flags"]["role"], c["maxM"], c["maxN"], 1 if c["kind"] == 2 else 0) == 1
        assert (expect == 1) <= takes
        b0, o0, rows = _run(h, c, False)
        big = True
        assert rows == partial_rows_rule(c["maxM"], expect == 1, big)
        if verify:
            _verify(c, b0, o0, False, rows, expect == 1)
        _, o1, rows1 = _run(h, c, False, form=expect)
        assert rows1 == rows
        _, again, _ = _run(h, c, False)
    _same_bits(o0, o1, "%s: form 0 against form %d" % (c["name"], expect))
    _same_bits(o0, again, c["name"] + ": second run")


# ---- split-K ---------------------------------------------------------------------------------------------------------
SPLITK = gc.splitk_cases(1) + gc.splitk_cases(3)


@pytest.mark.parametrize("c", SPLITK, ids=_ids(SPLITK))
def test_split_k_product(gp_handle, c):
    """H = alpha (X [D]) Y^T, float64 (generic and lean form) and float32 strips: sym and scale_by_k on and off, 2, 3, 5, 8 slices
    and the library's own count (the odd ones reach the slab reduction's tail loop), ldc odd and even, M * M odd (the reduction's
    single-element path), the mirror entry by entry, and the fused row dot products u = X v2 -> o1 partials, o0 = u, xa += u"""
    h = gp_handle
    for exact in (True, False):
        for ns in c["nsplits"]:
            bufs, outs, rows = _run(h, c, exact, nsplit=ns)
            assert rows == ns or (ns == 0 and 2 <= rows <= MAX_SLICES)
            _verify_nt(c, bufs, outs, exact, rows)
            if not exact:
                _, again, rows2 = _run(h, c, False, nsplit=ns)
                assert rows2 == rows
                _same_bits(outs, again, "%s nsplit %d: second run" % (c["name"], ns))


# ---- float32 strips --------------------------------------------------------------------------------------------------
F32 = gc.f32_role_cases()


@pytest.mark.parametrize("c", F32, ids=_ids(F32))
def test_f32_roles_every_form(gp_handle, c):
    """kind 2: roles 1, 2, 3 in gemm_wave_f32.hip (a32_ok), gemm_strip_f32.hip and gemm_f32.hip, leading dimensions a multiple
    of 4; the M x M operand is float64 in memory and rounded to float32 once"""
    _full_check(gp_handle, c)


@pytest.mark.parametrize("role", [1, 2, 3])
def test_f32_wave_needs_a32_scratch(gp_handle, role):
    """without a32_ok the float32 wave form is not taken: called directly it is refused, dispatched the launch takes the lean form"""
    fl = gc._role_flags(role, uniform_aligned=1, rows64_ok=1 if role != 3 else 0, a32_ok=0)
    c = gc.case("f32-noscratch-role%d" % role, 2, 1, fl, [(256, 256, 256)], ld="strip")
    bufs = _alloc(gp_handle, c, gc.make_inputs(c, True))
    st, _ = _launch(gp_handle, c, bufs)
    assert st == GP_ERR_UNSUPPORTED
    _, o0, _ = _run(gp_handle, c, False, form=0)
    _, o2, _ = _run(gp_handle, c, False, form=2)
    _same_bits(o0, o2, c["name"])


def test_debug_entry_refuses_other_roles(gp_handle):
    """roles 5, 6 and 7 (tested in test_gpu_pdgp.py, test_gpu_qfar.py, test_gpu_qbar.py) are not reachable through gp_debug_gemm"""
    plain = gc.case("refuse-roles", 0, 0, gc.flags_of(), [(128, 256, 128)], ld="strip")
    bufs = _alloc(gp_handle, plain, gc.make_inputs(plain, True))
    for role in (5, 6, 7):
        st, _ = _launch(gp_handle, plain, bufs, flags=dict(plain["flags"], role=role, uniform_aligned=1))
        assert st == GP_ERR_UNSUPPORTED
    for b, o in zip(bufs, _read(bufs)):
        assert np.array_equal(o["C"], b["C"].initial)
