"""CPU checks of the GEMM reference (gemm_ref.py) and of the case tables of test_gpu_gemm.py (gemm_cases.py):
the reference against plain numpy.matmul on masked copies for every flag; the exactness condition of every integer case;
the partial-row count rule against the library's own wave-form query."""
import numpy as np
import pytest

import gemm_cases as gc
from gemm_ref import (EPI_COLDOT, EPI_COLSUMSQ, EPI_STORE, LD, TRI_LOWER, TRI_NONE, TRI_UPPER, flags_of, gemm_ref,
                      partial_rows_rule, row_range)


def _plain(M, N, K, A, B, f, v1):
    """the same product, written out the long way in float64"""
    opA = (A.T if f["transA"] else A).copy()
    opB = (B.T if f["transB"] else B).copy()
    for i in range(M):
        for k in range(K):
            if (f["triA"] == TRI_LOWER and k > i) or (f["triA"] == TRI_UPPER and k < i):
                opA[i, k] = 0.0
    for k in range(K):
        for n in range(N):
            if (f["triB"] == TRI_LOWER and n > k) or (f["triB"] == TRI_UPPER and k > n):
                opB[k, n] = 0.0
            if f["scale_mode"] == 1:
                opB[k, n] *= v1[n]
            if f["scale_mode"] == 2:
                opB[k, n] *= v1[k]
    return np.matmul(opA, opB)


@pytest.mark.parametrize("ta", [0, 1])
@pytest.mark.parametrize("tb", [0, 1])
@pytest.mark.parametrize("triA", [TRI_NONE, TRI_LOWER, TRI_UPPER])
@pytest.mark.parametrize("triB", [TRI_NONE, TRI_LOWER, TRI_UPPER])
@pytest.mark.parametrize("sm", [0, 1, 2])
def test_reference_against_matmul_on_masked_copies(ta, tb, triA, triB, sm):
    M, N, K = 9, 11, 9
    f = flags_of(transA=ta, transB=tb, triA=triA, triB=triB, scale_mode=sm, alpha=0.5, beta=-0.5, epilogue=7)
    c = gc.case("cpu", 0, 3, f, [(M, N, K)])
    for exact in (True, False):
        p = gc.make_inputs(c, exact, seed=3)[0]
        r = gemm_ref(0, f, M, N, K, p["A"], p["B"], C0=p["C0"], v0=p["v0"], v1=p["v1"], exact=exact, block_rows=64, tile=64)
        acc = _plain(M, N, K, p["A"], p["B"], f, p["v1"])
        want = 0.5 * acc - 0.5 * p["C0"]
        tol = 0 if exact else 1e-13
        assert np.abs(r["C"].astype(np.float64) - want).max() <= tol
        assert r["written"].all()
        assert np.abs(r["o0"][0].astype(np.float64) - ((0.5 * acc) ** 2).sum(axis=0)).max() <= tol * 100
        assert np.abs(r["o1"][0].astype(np.float64) - (0.5 * acc * p["v0"][:, None]).sum(axis=0)).max() <= tol * 100
        # the garbage in the structurally zero triangle never reaches the result or the bound
        assert np.isfinite(r["C"].astype(np.float64)).all() and float(r["P"].max()) < 1e6


def test_reference_roles_epilogues_ranges_and_triC():
    M, N = 256, 8
    for role, (ta, tri, sm) in {1: (0, TRI_LOWER, 0), 2: (1, TRI_UPPER, 0), 3: (0, TRI_NONE, 1)}.items():
        f = dict(gc._role_flags(role), epilogue=7, tile_m0=1)
        c = gc.case("cpu-role", 0, 3, f, [(M, N, M)])
        p = gc.make_inputs(c, True, seed=1)[0]
        r = gemm_ref(0, f, M, N, M, p["A"], p["B"], v0=p["v0"], v1=p["v1"], exact=True, block_rows=64)
        acc = _plain(M, N, M, p["A"], p["B"], flags_of(transA=ta, triA=tri, scale_mode=sm), p["v1"])
        assert not r["written"][:128].any() and r["written"][128:].all()
        assert np.array_equal(r["C"][128:].astype(np.float64), acc[128:])
        assert np.isnan(r["o0"][:2]).all() and not np.isnan(r["o0"][2:]).any()
        assert np.array_equal(r["o0"][3].astype(np.float64), (acc[192:256] ** 2).sum(axis=0))
        assert np.array_equal(r["o1"][2].astype(np.float64), (acc[128:192] * p["v0"][128:192, None]).sum(axis=0))
    # no EPI_STORE: nothing of C is written;  triC lower: zeros above the diagonal inside tiles on the band, nothing above
    f = flags_of(epilogue=EPI_COLSUMSQ)
    p = gc.make_inputs(gc.case("cpu-nostore", 0, 3, f, [(5, 6, 4)]), True)[0]
    assert not gemm_ref(0, f, 5, 6, 4, p["A"], p["B"], exact=True, block_rows=64)["written"].any()
    f = flags_of(triC=TRI_LOWER)
    p = gc.make_inputs(gc.case("cpu-triC", 0, 3, f, [(70, 70, 4)]), True)[0]
    r = gemm_ref(0, f, 70, 70, 4, p["A"], p["B"], exact=True, block_rows=64, tile=64)
    assert r["written"][:64, :64].all() and not r["written"][:64, 64:].any() and r["written"][64:, :].all()
    assert (np.triu(r["C"][:64, :64].astype(np.float64), 1) == 0).all()
    assert np.array_equal(np.tril(r["C"].astype(np.float64)), np.tril(p["A"] @ p["B"]))
    assert row_range(320, 128, 3, 0) == (0, 0) and row_range(320, 128, 2, 5) == (256, 320) and row_range(320, 128, 0, 1) == (0, 128)
    assert row_range(320, 128, 1, 1) == (128, 256) and row_range(320, 128, 1, 0) == (128, 320) and row_range(320, 128, 0, 0) == (0, 320)


@pytest.mark.parametrize("sym", [0, 1])
@pytest.mark.parametrize("sbk", [0, 1])
def test_reference_split_k(sym, sbk):
    M, K = 7, 13
    f = flags_of(triC=TRI_LOWER if sym else TRI_NONE, scale_mode=2 if sbk else 0, alpha=2.0)
    p = gc.make_inputs(gc.case("cpu-nt", 1, 3, f, [(M, M, K)]), True, seed=2)[0]
    r = gemm_ref(1, f, M, M, K, p["A"], p["B"], v1=p["v1"], v2=p["v2"], xa0=p["xa0"], exact=True)
    H = 2.0 * np.matmul(p["A"] * (p["v1"][None, :] if sbk else 1.0), p["B"].T)
    if sym:
        H = np.tril(H) + np.tril(H, -1).T
    assert np.array_equal(r["C"].astype(np.float64), H)
    assert np.array_equal(r["u"].astype(np.float64), p["A"] @ p["v2"])
    assert np.array_equal(r["xa"].astype(np.float64), p["xa0"] + p["A"] @ p["v2"])


def test_float32_kind_rounds_the_square_operand_once():
    f = gc._role_flags(3)
    p = gc.make_inputs(gc.case("cpu-f32", 2, 3, f, [(4, 5, 4)], ld="strip"), False)[0]
    r = gemm_ref(2, f, 4, 5, 4, p["A"], p["B"], v1=p["v1"], exact=False)
    want = np.matmul(p["A"].astype(np.float32).astype(np.float64), p["B"] * p["v1"][None, :])
    assert np.abs(r["C"].astype(np.float64) - want).max() < 1e-14
    assert np.array_equal(p["B"], p["B"].astype(np.float32).astype(np.float64))
    assert float(r["bound_C"].max()) < 1e-5 and float(r["bound_C"].min()) > 0


ALL_EXACT = gc.exact_cases()


def test_case_names_are_unique_per_table():
    for table in (gc.generic_cases(), gc.structure_cases(), gc.role_generic_cases(), gc.role_lean_cases(), gc.role_wave_cases(),
                  gc.range_cases(0) + gc.range_cases(2), gc.splitk_cases(1) + gc.splitk_cases(3), gc.f32_role_cases()):
        names = [c["name"] for c in table]
        assert len(set(names)) == len(names)
    # at least half of the product cases have ldc > N
    prod = [c for c in ALL_EXACT if c["kind"] in (0, 2)]
    wide = sum(1 for c in prod if gc.make_inputs(c, True)[0]["ldc"] > c["shapes"][0][1])
    assert 2 * wide >= len(prod)


@pytest.mark.parametrize("c", ALL_EXACT, ids=[c["name"] + ("-r%d.%d" % (c["flags"]["tile_m0"], c["flags"]["tile_mcount"])) for c in ALL_EXACT])
def test_integer_cases_are_exact_in_any_order(c):
    """the reference's largest intermediate (accumulator, alpha acc, its square, a column sum; the sums of ABSOLUTE values bound
    every partial sum of every order) stays below 2^53; what the float32 kernels hold in float32 — operands, the scaled operand,
    the accumulator (per K-slice at most the whole sum of absolute values), alpha acc and the stored C — below 2^24"""
    f32 = c["kind"] in (2, 3)
    for p in gc.make_inputs(c, True):
        r = gemm_ref(c["kind"], c["flags"], p["M"], p["N"], p["K"], p["A"], p["B"], C0=p["C0"], v0=p["v0"], v1=p["v1"], v2=p["v2"],
                     xa0=p["xa0"], exact=True, block_rows=128)
        # the sum of |a| |b| bounds the accumulator and every partial sum of it; with alpha^2 and 128 rows, the column sums
        alpha = abs(c["flags"]["alpha"])
        amax = float(r["P"].max())            # |alpha| sum |a| |b|: bounds alpha acc
        accmax = amax / alpha                  # sum |a| |b|: bounds the accumulator and every partial sum of it, in any order
        assert r["peak"] < 2.0 ** 53 and max(amax, accmax) < 2.0 ** 53
        if c["kind"] in (0, 2) and (c["flags"]["epilogue"] & (EPI_COLSUMSQ | EPI_COLDOT)):
            assert 128 * amax * max(amax, 4.0) < 2.0 ** 53          # a column sum of squares, or of products with |v0| <= 4
        if c["kind"] in (1, 3) and p["v2"] is not None:
            assert (2 if f32 else 8) * 8 * p["K"] + 8 < 2.0 ** 53   # u = X v2, and xa += u
        if f32:
            assert r["peak32"] < 2.0 ** 24 and max(amax, accmax) < 2.0 ** 24
        for a in (p["A"], p["B"]):
            fin = np.abs(a[np.abs(a) < 1e30])
            assert np.array_equal(fin, np.round(fin)) and fin.max(initial=0) <= (2 if f32 else 8)


def test_partial_row_rule_matches_the_library():
    """rows of o0 / o1 = one per 64-row tile where gp_debug_wave_takes says the wave form takes the launch, else ceil(M / 64 or 128)"""
    from gpitch_amd import _lib
    lib = _lib.load_library()
    for f32 in (0, 1):
        for role in (1, 2, 3):
            for M in (64, 128, 130, 192, 320, 448):
                for N in (128, 256, 300, 768):
                    takes = lib.gp_debug_wave_takes(role, M, N, f32) == 1
                    assert takes == (M % 64 == 0 and N % 256 == 0)
    # the counts written out: (M, wave form, 128-row blocks) -> rows
    table = {(64, True, True): 1, (128, True, True): 2, (192, True, True): 3, (320, True, True): 5, (448, True, True): 7,
             (64, False, True): 1, (128, False, True): 1, (130, False, True): 2, (192, False, True): 2, (256, False, True): 2,
             (320, False, True): 3, (384, False, True): 3, (448, False, True): 4, (512, False, True): 4,
             (1, False, False): 1, (63, False, False): 1, (64, False, False): 1, (65, False, False): 2, (130, False, False): 3,
             (200, False, False): 4}
    for (M, wave, big), rows in table.items():
        assert partial_rows_rule(M, wave, big) == rows, (M, wave, big)


def test_dispatch_rule_by_hand():
    """gemm_cases.expected_form at shapes worked out by hand from the launchers' conditions"""
    ef = gc.expected_form
    assert ef(0, 1, 64, 256, 1, 1, 0) == 1 and ef(0, 1, 64, 256, 1, 0, 0) == 3 and ef(0, 3, 64, 256, 1, 0, 0) == 1
    assert ef(0, 2, 128, 128, 1, 1, 0) == 2 and ef(0, 2, 128, 384, 1, 1, 0) == 2 and ef(0, 2, 128, 256, 1, 0, 0) == 2
    assert ef(0, 1, 192, 512, 1, 0, 0) == 3 and ef(0, 1, 320, 520, 1, 1, 0) == 3 and ef(0, 1, 256, 512, 0, 1, 0) == 3
    assert ef(2, 1, 256, 256, 1, 1, 0) == 2 and ef(2, 1, 256, 256, 1, 1, 1) == 1 and ef(2, 3, 448, 768, 1, 0, 1) == 1
    assert ef(0, 3, 128, 128, 1, 0, 0, alpha=3.0) == 3 and ef(0, 1, 128, 256, 1, 1, 0, alpha=2.0) == 3 and ef(0, 3, 128, 256, 1, 0, 0, beta=1.0) == 3
    assert gc.expected_form_nt(1, 128, 2304, 1) == 2 and gc.expected_form_nt(1, 200, 512, 1) == 3 and gc.expected_form_nt(1, 256, 512, 0) == 3
    assert gc.expected_form_nt(3, 128, 512, 1) == 3
    shapes = set(gc.DISPATCH_SHAPES)
    assert all((M, N) in shapes for M in gc.WAVE_M for N in gc.WAVE_N) and all(s in shapes for s in gc.LEAN_SHAPES)
    got = set((d[0]["kind"], d[0]["flags"]["role"]) + d[0]["shapes"][0][:2] for d in gc.dispatch_cases() if d[0]["kind"] in (0, 2))
    assert all((k, r, M, N) in got for k in (0, 2) for r in (1, 2, 3) for (M, N) in shapes)
