"""On the host: the operator cases of far_tables_cases.py have the property each is there for, keep the promise
gp_debug_far_tables asks of its caller, and stay inside the range where both forms of a kernel compute finite numbers (so that
"byte for byte" in test_gpu_far_tables.py compares values, not NaN patterns)."""
import numpy as np

import afar_rule as af
import far_tables_cases as fc
import qfar_rule as qf

AFAR = fc.afar_cases()
QFAR = fc.qfar_cases()


def test_names_are_unique_and_the_grids_are_covered():
    assert len({c["name"] for c in AFAR}) == len(AFAR) and len({c["name"] for c in QFAR}) == len(QFAR)
    rule = [c for c in AFAR if c.get("rule") and not c.get("gap") and not c["nan_above"]]
    assert {(c["M"], c["ng"]) for c in rule} == {(M, ng) for M in (16, 48, 272, 1024) for ng in (1, 2, 5, 128)}
    assert {c["name"].rsplit("_", 1)[0] for c in rule} == {"grid", "off_grid", "clustered"}
    assert {c["M"] for c in QFAR} == {64, 128, 1024}
    assert {c["nf"] for c in QFAR} == {8, 40, 48, 64}
    assert {c["ng"] for c in QFAR} >= {1, 2, 3, 255, 256, 257, 300}
    for M in (64, 128, 1024):
        assert {c["nf"] for c in QFAR if c["M"] == M} == {8, 40, 48, 64}, M
    assert all((c["M"], c["nf"]) == (64, 8) for c in QFAR if c["ng"] > 256)


def test_every_case_keeps_the_callers_promise():
    for c in AFAR + QFAR:
        M = c["M"]
        assert len(c["rng"]) == c["ng"] and c["N"] == 256 * c["ng"], c["name"]
        assert all(0 <= kb <= ke <= M for kb, ke, _, _ in c["rng"]), c["name"]
        assert np.all(np.diff(c["z"]) > 0), c["name"]
    for c in AFAR:
        assert c["M"] % 16 == 0 and c["M"] <= 1024
    for c in QFAR:
        assert c["M"] % 64 == 0 and c["nf"] % 8 == 0 and c["nf"] <= 64
        assert all(k % 16 == 0 for side in (0, 1) for k in fc.qfar_counts(c, side)), c["name"]   # whole tiles enter


def test_rule_cases_carry_the_rules_own_ranges():
    for c in AFAR:
        if c.get("rule"):
            x = np.arange(c["N"], dtype=np.float64)
            if c.get("gap"):
                assert not np.all(np.diff([r[2] for r in c["rng"]]) < 1000.0), c["name"]       # the gap shows in the reference points
            else:
                assert c["rng"] == af.ranges(c["z"], x), c["name"]
    for c in QFAR:
        assert [tuple(r) for r in qf.ranges(c["z"], c["x"], c["ls"])] == c["rng"], c["name"]


def test_hand_made_cases_have_their_property():
    by = {c["name"]: c for c in AFAR}
    c = by["all_at_step0_1024x2"]
    for side in (0, 1):                       # every row at the first step: ceil(1024 / 256) chunks of afar_t_kernel in one step
        counts = fc.afar_counts(c, side)
        assert counts[0] == c["M"] and -(-counts[0] // 256) == c["chunks"] == 4
    c = by["none_272x5"]
    assert all(k == 0 for side in (0, 1) for k in fc.afar_counts(c, side))
    c = by["backwards_48x5"]
    for side in (0, 1):                       # a step whose own count lies below what has entered: the running maximum holds
        far = [c["M"] - c["rng"][c["ng"] - 1 - q][1] if side else c["rng"][q][0] for q in range(c["ng"])]
        counts = fc.afar_counts(c, side)
        assert any(f < k for f, k in zip(far, counts)), side
        assert counts == sorted(counts)
    c = by["ragged_48x5"]
    assert any(k % 16 for side in (0, 1) for k in fc.afar_counts(c, side))
    assert not af.is_monotone(by["backwards_48x5"]["rng"])
    nan_cases = [c for c in AFAR if c["nan_above"]]
    assert len(nan_cases) >= 3
    for c in AFAR:
        above = c["W"][np.triu_indices(c["M"], 1)]
        assert np.all(np.isnan(above)) if c["nan_above"] else np.all(above == 7.25), c["name"]
        assert np.all(np.isfinite(np.tril(c["W"]))) and np.all(np.isfinite(c["C"]))
    # the nan cases let rows enter (else the mask is never asked)
    assert any(max(fc.afar_counts(c, 0)[-1], fc.afar_counts(c, 1)[-1]) > 16 for c in nan_cases)


def test_qfar_cases_have_their_property():
    by = {c["name"]: c for c in QFAR}
    c = by["frame_gap_128x40x8"]
    kb, ke = [r[0] for r in c["rng"]], [r[1] for r in c["rng"]]
    assert any(b < a for a, b in zip(kb, kb[1:])) and any(b < a for a, b in zip(ke, ke[1:]))   # a non-monotone step, both walks
    c = by["all_near_64x8x3"]
    assert all((r[0], r[1]) == (0, c["M"]) for r in c["rng"])
    for name, side in (("all_below_128x48x3", 0), ("all_above_128x48x3", 1)):
        c = by[name]
        assert fc.qfar_counts(c, side)[0] == c["M"] and fc.qfar_counts(c, 1 - side)[-1] == 0
    both = [c for c in QFAR if fc.qfar_counts(c, 0)[-1] > 0 and fc.qfar_counts(c, 1)[-1] > 0]
    assert len(both) >= 10                                               # both sides
    # more than 256 groups: the second chunk of steps runs, and rows still enter in it (bcarry and c0 = 256 matter)
    for c in QFAR:
        if c["ng"] > 256:
            assert c.get("second_chunk")
            up, down = fc.qfar_counts(c, 0), fc.qfar_counts(c, 1)
            assert up[-1] > up[255] or down[-1] > down[255] or up[255] > 0, c["name"]
    assert sum(1 for c in QFAR if c["ng"] > 256) >= 2
    assert any(c["ng"] == 256 for c in QFAR) and any(c["ng"] == 255 for c in QFAR)


def test_rule_tables_are_finite_everywhere():
    for c in AFAR:
        assert np.all(np.isfinite(fc.afar_rule_tables(c))), c["name"]
    for c in QFAR:
        assert np.all(np.isfinite(fc.qfar_rule_tables(c))), c["name"]
