"""Case tables and host inputs of tests/test_gpu_gemm.py (pure numpy: tests/test_gemm_ref_cpu.py checks the exactness
condition of every integer case here without a GPU).

A case is a dict: name, kind (0 float64 product, 1 float64 split-K, 2 / 3 the float32 twins), form (0 dispatch, 1 wave, 2 lean,
3 generic), flags (gemm_ref.flags_of), shapes [(M, N, K), ...] (one per problem; split-K: (M, M, Nlong)), maxM, maxN, ld
("odd" / "even" / "strip": how leading dimensions are padded), nsplits, rowdot.
"""
import numpy as np

from gemm_ref import (EPI_COLDOT, EPI_COLSUMSQ, EPI_STORE, TRI_LOWER, TRI_NONE, TRI_UPPER, effective_flags, flags_of)

GARBAGE = 3.0e33          # what the structurally zero triangle of a triangular operand holds (finite in float32 too)
ALPHAS = (1.0, 2.0, 0.5, 4.0)


def case(name, kind, form, flags, shapes, ld="odd", maxM=None, maxN=None, nsplits=(0,), rowdot=True):
    shapes = [tuple(s) for s in shapes]
    return dict(name=name, kind=kind, form=form, flags=flags, shapes=shapes, ld=ld,
                maxM=maxM or max(s[0] for s in shapes), maxN=maxN or max((s[2] if kind in (1, 3) else s[1]) for s in shapes),
                nsplits=tuple(nsplits), rowdot=rowdot)


def strip_ld(n, f32):
    return (n + 3) & ~3 if f32 else (n + 1) & ~1


def _ld(cols, mode, f32, which):
    """leading dimension of a buffer with `cols` columns.  odd: odd and > cols (no 16-byte path); even: even and > cols;
    strip: what the engine gives a strip (gp_strip_ld), plus one more 16-byte unit for C so that ldc > N"""
    if f32:
        base = strip_ld(cols, True)
        return base + (4 if (mode != "tight" and which == "c") else 0)
    if mode == "odd":
        return (cols | 1) + 2
    if mode == "even":
        return ((cols + 1) & ~1) + 2
    if mode == "strip":
        return strip_ld(cols, False) + (2 if which == "c" else 0)
    return cols


def wave_contract_zero(c):
    """role 1 in the wave forms reads W's diagonal 64 x 64 blocks whole: their documented contract is that W carries exact
    zeros above the diagonal (it is the library's own inverse).  Such a case gets garbage above the diagonal BLOCKS only."""
    f = c["flags"]
    return c["kind"] in (0, 2) and f["role"] == 1 and c["form"] in (0, 1) and f["uniform_aligned"] and f["rows64_ok"]


def make_inputs(c, exact, seed=0):
    """host buffers of every problem of the case: list of dicts(M, N, K, A, B, C0, v0, v1, v2, xa0, lda, ldb, ldc)"""
    rng = np.random.RandomState(seed)
    kind = c["kind"]
    f32 = kind in (2, 3)
    f = effective_flags(c["flags"]) if kind in (0, 2) else dict(c["flags"])
    lim = 2 if f32 else 8

    def vals(shape, lo=None, hi=None):
        if exact:
            return rng.randint(-lim if lo is None else lo, (lim if hi is None else hi) + 1, size=shape).astype(np.float64)
        return rng.standard_normal(shape)

    out = []
    for (M, N, K) in c["shapes"]:
        p = dict(M=M, N=N, K=K)
        if kind in (1, 3):
            A, B = vals((M, K)), vals((M, K))
            p["lda"], p["ldb"] = _ld(K, c["ld"], f32, "a"), _ld(K, c["ld"], f32, "b")
            p["ldc"] = M + (1 if c["ld"] == "odd" else 2 if c["ld"] == "even" else 0)
            p["v1"] = vals(K, 1, 3) if f["scale_mode"] == 2 else None
            p["v2"] = vals(K) if c["rowdot"] else None
            p["xa0"] = vals(M) if c["rowdot"] else None
            p["C0"], p["v0"] = None, None
        else:
            opA, opB = vals((M, K)), vals((K, N))
            i, k = np.arange(M)[:, None], np.arange(K)[None, :]
            if f["triA"] == TRI_LOWER:
                z = k > i
                if wave_contract_zero(c):
                    opA[z] = 0.0
                    z = (k // 64) > (i // 64)
                opA[z] = GARBAGE
            elif f["triA"] == TRI_UPPER:
                opA[k < i] = GARBAGE
            kk, n = np.arange(K)[:, None], np.arange(N)[None, :]
            if f["triB"] == TRI_LOWER:
                opB[n > kk] = GARBAGE
            elif f["triB"] == TRI_UPPER:
                opB[kk > n] = GARBAGE
            A = np.ascontiguousarray(opA.T) if f["transA"] else opA
            B = np.ascontiguousarray(opB.T) if f["transB"] else opB
            p["lda"] = _ld(A.shape[1], c["ld"], False, "a")          # (kind 2: A is the float64 M x M operand)
            p["ldb"] = _ld(B.shape[1], c["ld"], f32, "b")
            p["ldc"] = _ld(N, c["ld"], f32, "c")
            p["v0"] = vals(M, -4, 4) if (f["epilogue"] & EPI_COLDOT) else None
            sm = f["scale_mode"]
            p["v1"] = vals(N if sm == 1 else K, 1, 3) if sm else None
            if exact and sm and f32:
                p["v1"] = np.minimum(p["v1"], 2.0)
            p["C0"] = vals((M, N)) if f["beta"] != 0.0 else None
            p["v2"], p["xa0"] = None, None
        if f32:       # what a float32 buffer will hold: the reference sees the stored values
            B = B.astype(np.float32).astype(np.float64)
            if kind == 3:
                A = A.astype(np.float32).astype(np.float64)
            if p["C0"] is not None:
                p["C0"] = p["C0"].astype(np.float32).astype(np.float64)
        p["A"], p["B"] = A, B
        out.append(p)
    return out


# ---- the tables ------------------------------------------------------------------------------------------------------
GENERIC_SHAPES = [(1, 1, 1), (5, 7, 3), (16, 16, 4), (63, 65, 17), (64, 64, 16), (65, 129, 33), (130, 300, 130), (200, 70, 257)]
TRANS = [(0, 0), (1, 0), (0, 1), (1, 1)]
# tile variants: "small" (plain store: 32-tiles where the switch admits them, else 64), "small64" (a column-sum epilogue keeps
# the 64-tiles), "big" (128-tiles)
TILE_VARIANTS = {"small": dict(), "small64": dict(epilogue=EPI_STORE | EPI_COLSUMSQ), "big": dict(big_tiles=1)}


def generic_cases():
    cs = []
    for si, s in enumerate(GENERIC_SHAPES):
        for (ta, tb) in TRANS:
            for tv, extra in TILE_VARIANTS.items():
                ld = "odd" if (si + ta + 2 * tb) % 2 == 0 else "even"
                cs.append(case("gen-%dx%dx%d-t%d%d-%s" % (s + (ta, tb, tv)), 0, 3, flags_of(transA=ta, transB=tb, **extra), [s], ld=ld))
    # batches of 3 with different M, N, K under one maxM, maxN; grids a multiple of 8 (64-tiles: 2 x 4 x ... ) and not
    for (ta, tb) in TRANS:
        for tv, extra in TILE_VARIANTS.items():
            cs.append(case("gen-batch3-t%d%d-%s" % (ta, tb, tv), 0, 3, flags_of(transA=ta, transB=tb, **extra),
                           [(130, 300, 130), (5, 7, 3), (65, 129, 33)], ld="even"))
    # flattened grid a multiple of 8 (128 x 256 in 64-tiles: 2 x 4 = 8 workgroups; 128-tiles, batch 4: 1 x 2 x 4) and not (above)
    cs.append(case("gen-grid8-small64", 0, 3, flags_of(epilogue=3), [(128, 256, 40)], ld="even"))
    cs.append(case("gen-grid8-big-batch4", 0, 3, flags_of(big_tiles=1), [(128, 256, 40), (100, 130, 9), (128, 200, 33), (7, 256, 40)], ld="odd"))
    cs.append(case("gen-grid16-small64-batch2", 0, 3, flags_of(epilogue=3, transB=1), [(128, 256, 40), (70, 200, 24)], ld="even"))
    return cs


def structure_cases():
    cs = []
    shapes = [(130, 130, 130), (65, 129, 65), (200, 70, 200)]
    for s in shapes:
        for tri in (TRI_LOWER, TRI_UPPER):
            for ta in (0, 1):
                for big in (0, 1):
                    cs.append(case("triA%d-ta%d-big%d-%dx%d" % (tri, ta, big, s[0], s[1]), 0, 3,
                                   flags_of(triA=tri, transA=ta, big_tiles=big, epilogue=3), [s], ld="even" if ta else "odd"))
    for s in [(130, 130, 130), (129, 65, 129), (70, 200, 70)]:
        for tri in (TRI_LOWER, TRI_UPPER):
            for tb in (0, 1):
                cs.append(case("triB%d-tb%d-%dx%d" % (tri, tb, s[0], s[1]), 0, 3, flags_of(triB=tri, transB=tb, epilogue=3), [s],
                               ld="odd" if tb else "even"))
    # triC lower (plain store: the column sums of a launch with skipped tiles are nobody's contract): 32-tiles, 128-tiles, and
    # 64-tiles in a batch of 20 (320 tiles of 64 x 64, where the 32-tile switch lets go)
    for s in [(130, 130, 33), (200, 200, 17), (64, 64, 16)]:
        for big in (0, 1):
            cs.append(case("triC-big%d-%d" % (big, s[0]), 0, 3, flags_of(triC=TRI_LOWER, big_tiles=big, transB=1), [s]))
    cs.append(case("triC-tile64-batch20", 0, 3, flags_of(triC=TRI_LOWER, transB=1, alpha=0.5), [(200, 200, 17), (130, 130, 33)] * 10, ld="even"))
    for beta in (1.0, -0.5):
        for s in [(65, 129, 33), (130, 300, 130)]:
            for big in (0, 1):
                cs.append(case("beta%g-big%d-%dx%d" % (beta, big, s[0], s[1]), 0, 3, flags_of(beta=beta, alpha=2.0, big_tiles=big, epilogue=7), [s]))
    for sm in (1, 2):
        for (ta, tb) in TRANS:
            cs.append(case("scale%d-t%d%d" % (sm, ta, tb), 0, 3, flags_of(scale_mode=sm, transA=ta, transB=tb, epilogue=3, alpha=0.5), [(65, 129, 33)]))
            cs.append(case("scale%d-t%d%d-big" % (sm, ta, tb), 0, 3, flags_of(scale_mode=sm, transA=ta, transB=tb, big_tiles=1), [(130, 300, 130)], ld="even"))
    for epi in range(1, 8):
        for big in (0, 1):
            cs.append(case("epi%d-big%d" % (epi, big), 0, 3, flags_of(epilogue=epi, big_tiles=big, alpha=2.0), [(130, 300, 70), (63, 65, 17)]))
    return cs


def _role_flags(role, wave64=False, **kw):
    """the flags of a role's launch.  Epilogues: role 1 everything (the engine's A = W Kuf: store, sum A^2, A^T q_mu), role 2 store
    and sum of squares, role 3 store.  wave64: the float64 wave form, whose role 2 gives the sum of squares ONLY (its tile's rows
    are permuted: DESIGN.md; the engine asks for nothing else)"""
    epi = EPI_STORE if role == 3 else 7 if role == 1 else (EPI_COLSUMSQ if wave64 else 3)
    return flags_of(role=role, scale_mode=1 if role == 3 else 0, epilogue=epi, **kw)


def role_generic_cases():
    cs = []
    for role in (1, 2, 3):
        for (M, N) in [(128, 256), (130, 300), (320, 520)]:
            cs.append(case("role%d-gen-%dx%d" % (role, M, N), 0, 3, _role_flags(role), [(M, N, M)], ld="odd" if M == 130 else "even"))
        cs.append(case("role%d-gen-ragged" % role, 0, 3, _role_flags(role), [(64, 300, 64), (192, 300, 192), (320, 300, 320)], ld="even"))
    return cs


LEAN_SHAPES = [(128, 128), (128, 384), (256, 640), (384, 128)]


def role_lean_cases(kind=0):
    cs = []
    for role in (1, 2, 3):
        for (M, N) in LEAN_SHAPES:
            for alpha in (ALPHAS if role == 3 else (1.0,)):
                cs.append(case("role%d-lean-%dx%d-a%g-k%d" % (role, M, N, alpha, kind), kind, 2,
                               _role_flags(role, uniform_aligned=1, alpha=alpha), [(M, N, M)] * (2 if M == 128 else 1), ld="strip"))
    return cs


WAVE_M = [64, 128, 192, 256, 320, 448]
WAVE_N = [256, 512, 768]


def role_wave_cases(kind=0):
    cs = []
    for role in (1, 2, 3):
        for M in WAVE_M:
            for N in WAVE_N:
                fl = _role_flags(role, wave64=(kind == 0), uniform_aligned=1, rows64_ok=1 if role != 3 else 0, a32_ok=1 if kind == 2 else 0,
                                 alpha=ALPHAS[(M // 64 + N // 256) % 4] if role == 3 else 1.0)
                cs.append(case("role%d-wave-%dx%d-k%d" % (role, M, N, kind), kind, 1, fl, [(M, N, M)] * (2 if N == 512 else 1), ld="strip"))
    return cs


RANGES = [(0, 1), (1, 0), (1, 1), (2, 5), (3, 0)]


def range_cases(kind=0):
    """row-block ranges on the three forms; the whole launch of each is the case with range (0, 0)"""
    cs = []
    for form in (1, 2, 3):
        for role in (1, 2, 3):
            for M in (320, 448):
                if form == 2 and M % 128:
                    M += 64           # the lean form takes whole 128-row blocks: 384 and 512
                N = 256
                fl = _role_flags(role, wave64=(kind == 0 and form == 1), uniform_aligned=1, rows64_ok=1 if (form == 1 and role != 3) else 0,
                                 a32_ok=1 if (kind == 2 and form == 1) else 0)
                cs.append(case("range-form%d-role%d-M%d-k%d" % (form, role, M, kind), kind, form, fl, [(M, N, M)], ld="strip"))
    return cs


def with_range(c, m0, mcount):
    d = dict(c)
    d["flags"] = dict(c["flags"], tile_m0=m0, tile_mcount=mcount)
    return d


def tile32_cases():
    """(admitted launch, the same problems inside a launch of 320 64 x 64 tiles: one past the last count the switch admits)"""
    out = []
    for shapes in ([(200, 200, 70)], [(200, 136, 70), (64, 200, 129)], [(129, 65, 33)]):
        for (ta, tb) in ((0, 0), (1, 1)):
            fl = flags_of(transA=ta, transB=tb, alpha=2.0)
            small = case("tile32-b%d-t%d%d" % (len(shapes), ta, tb), 0, 3, fl, shapes, maxM=200, maxN=200, ld="odd")
            over = case("tile32-over-b%d-t%d%d" % (len(shapes), ta, tb), 0, 3, fl, (shapes * 20)[:20], maxM=200, maxN=200, ld="odd")
            out.append((small, over))
    return out


NT_NSPLITS = (2, 3, 5, 8, 0)


def splitk_cases(kind=1):
    cs = []
    for M in (40, 45, 128, 200):           # (45: M * M odd, the slab reduction's single-element path)
        for Nlong in (130, 512, 2304):
            for sym in (0, 1):
                for sbk in (0, 1):
                    ld = "odd" if (M + Nlong // 2 + sym) % 2 else "even"
                    if kind == 3:
                        ld = "odd" if ld == "odd" else "even"
                    fl = flags_of(triC=TRI_LOWER if sym else TRI_NONE, scale_mode=2 if sbk else 0, alpha=ALPHAS[(sym + 2 * sbk) % 4])
                    cs.append(case("nt-gen-M%d-N%d-sym%d-d%d-k%d" % (M, Nlong, sym, sbk, kind), kind, 3, fl, [(M, M, Nlong)], ld=ld,
                                   nsplits=NT_NSPLITS, rowdot=not (M == 40 and Nlong == 130)))
    if kind == 1:
        for M in (128, 256):
            for Nlong in (512, 2304):
                for sym in (0, 1):
                    for sbk in (0, 1):
                        fl = flags_of(triC=TRI_LOWER if sym else TRI_NONE, scale_mode=2 if sbk else 0, uniform_aligned=1, alpha=ALPHAS[(sym + 2 * sbk + 1) % 4])
                        cs.append(case("nt-lean-M%d-N%d-sym%d-d%d" % (M, Nlong, sym, sbk), 1, 2, fl, [(M, M, Nlong)] * (2 if M == 128 else 1),
                                       ld="strip" if sym else "even", nsplits=NT_NSPLITS))
    return cs


def f32_role_cases():
    """kind 2 on every form: the wave (a32_ok on), lean and generic shapes of the float64 tables"""
    cs = role_wave_cases(2) + role_lean_cases(2)
    for role in (1, 2, 3):
        for (M, N) in [(128, 256), (130, 300), (320, 520)]:
            cs.append(case("role%d-gen-%dx%d-k2" % (role, M, N), 2, 3, _role_flags(role, alpha=2.0 if role == 3 else 1.0), [(M, N, M)], ld="strip"))
        cs.append(case("role%d-gen-ragged-k2" % role, 2, 3, _role_flags(role), [(64, 300, 64), (192, 300, 192), (320, 300, 320)], ld="strip"))
    return cs


def expected_form(kind, role, M, N, uniform, rows64, a32, alpha=1.0, beta=0.0):
    """the form a dispatched (form 0) launch of roles 1-3 takes, by the documented rules: with uniform_aligned and beta = 0, the wave
    form when M % 64 == 0 and N % 256 == 0 (roles 1, 2: with rows64_ok; float32: with a32_ok), else the lean form when
    M % 128 == 0 and N % 128 == 0; both want alpha = 1 (role 3: a power of two in {0.5, 1, 2, 4}); else the generic kernel"""
    alpha_ok = (alpha in ALPHAS) if role == 3 else (alpha == 1.0)
    if uniform and beta == 0.0 and alpha_ok:
        if M % 64 == 0 and N % 256 == 0 and (role == 3 or rows64) and (kind == 0 or a32):
            return 1
        if M % 128 == 0 and N % 128 == 0:
            return 2
    return 3


def expected_form_nt(kind, M, Nlong, uniform):
    """split-K: float64 takes the lean form with uniform_aligned, M % 128 == 0 and Nlong % 16 == 0; float32 has the generic only"""
    return 2 if (kind == 1 and uniform and M % 128 == 0 and Nlong % 16 == 0) else 3


# every aligned (M, N) the role tables use: the wave grid, the lean shapes, the aligned generic shapes
DISPATCH_SHAPES = sorted(set([(M, N) for M in WAVE_M for N in WAVE_N] + LEAN_SHAPES + [(128, 256), (320, 520)]))


def dispatch_cases():
    """launches through form 0 as (case, the form the rules above name, verify).  Every aligned shape of the role tables, both
    precisions, as the engine passes it (rows64_ok and a32_ok on); then the switches off one at a time at shapes where that
    changes the form (these are also checked against the reference: the form tables do not hold them); then split-K."""
    out = []
    for kind in (0, 2):
        for role in (1, 2, 3):
            for (M, N) in DISPATCH_SHAPES:
                ex = expected_form(kind, role, M, N, 1, 1, 1)
                fl = _role_flags(role, wave64=(kind == 0 and ex == 1), uniform_aligned=1, rows64_ok=1 if role != 3 else 0,
                                 a32_ok=1 if kind == 2 else 0)
                out.append((case("disp-k%d-role%d-%dx%d" % (kind, role, M, N), kind, 0, fl, [(M, N, M)], ld="strip"), ex, False))
            for (M, N, r64, a32, ua) in [(192, 512, 0, 1, 1), (256, 256, 1, 0, 1), (128, 384, 0, 0, 1), (256, 512, 1, 1, 0), (384, 128, 0, 0, 0)]:
                r64 = r64 if role != 3 else 0
                a32 = a32 if kind == 2 else 0
                ex = expected_form(kind, role, M, N, ua, r64, a32)
                fl = _role_flags(role, wave64=(kind == 0 and ex == 1), uniform_aligned=ua, rows64_ok=r64, a32_ok=a32)
                out.append((case("disp-k%d-role%d-%dx%d-r%d-a%d-u%d" % (kind, role, M, N, r64, a32, ua), kind, 0, fl, [(M, N, M)], ld="strip"), ex, True))
    for M in (128, 200, 256):
        for Nlong in (512, 2304):
            for ua in (1, 0):
                sym = (M // 8 + Nlong // 512 + ua) % 2
                fl = flags_of(triC=TRI_LOWER if sym else TRI_NONE, scale_mode=2, uniform_aligned=ua)
                out.append((case("disp-nt-M%d-N%d-u%d" % (M, Nlong, ua), 1, 0, fl, [(M, M, Nlong)], ld="strip", nsplits=(3,)),
                            expected_form_nt(1, M, Nlong, ua), True))
    return out


def exact_cases():
    """every case that is run on integer inputs (all of them; the range cases as their whole launch)"""
    cs = generic_cases() + structure_cases() + role_generic_cases() + role_lean_cases() + role_wave_cases()
    cs += range_cases(0) + range_cases(2)      # (a row-block range forms a subset of the whole launch's sums)
    for a, b in tile32_cases():
        cs += [a, b]
    cs += splitk_cases(1) + splitk_cases(3) + f32_role_cases()
    cs += [d[0] for d in dispatch_cases()]
    return cs
