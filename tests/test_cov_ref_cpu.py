"""CPU checks of what tests/test_gpu_cov.py leans on: the two references of tests/cov_ref.py agree where both hold, the
float64 emulation of the device's formulas (entry by entry inside the band, separable product outside it) meets the oracle's
bar wherever max |x / l| <= 256, the recorded bars of the beyond-range cases are what the emulation measures, and the case
list of tests/cov_cases.py has the tile geometry it claims.  No GPU, no library call except the host-only ABI load."""
import numpy as np
import pytest

import cov_cases as cc
import cov_ref as cr

_ids = [c["id"] for c in cc.MFMA_CASES]
_cache = {}


def _evaluated(c):
    """per distinct input set, once: inputs of record 0 (the further records repeat its geometry), the float64 emulation, the
    oracle and the long-double closed form.  Within the oracle's range the closed form is evaluated on every second row (the
    agreement of two references is an entry-wise statement); beyond it on all rows, since the bars are maxima over them."""
    key = (c["type"], tuple(c["recs"][0]), c["n2"], c["l"], c.get("x_order"), c.get("z_order"), c.get("threshold"))
    if key not in _cache:
        kerns, zs, x = cc.mfma_inputs(c)
        k, z = kerns[0], zs[0]
        rows = np.arange(z.size) if c["ref"] == "closed" else np.arange(0, z.size, 2)
        _cache[key] = dict(kern=k, z=z, x=x, rows=rows, emu=cr.emulate(k, z, x), oracle=cr.oracle(k, z, x),
                           closed=cr.closed_form(k, z[rows], x), far=cr.far_entries(k, z[rows], x),
                           sep=cr.separable_entries(k, z, x), amax=cr.amax(k, z, x))
    return _cache[key]


@pytest.mark.parametrize("c", cc.MFMA_CASES, ids=_ids)
def test_geometry_of_every_matrix_core_case(c):
    kerns, zs, x = cc.mfma_inputs(c)
    for k, z in zip(kerns[:1], zs[:1]):
        g = cr.geometry(k, z, x)
        print("%s: %d tiles, %d separable, %d straddle the band, max |a| = %.1f" % (c["id"], g["tiles"], g["separable"], g["straddle"],
                                                                                  cr.amax(k, z, x)))
        if c["kind"] == "envelope":
            assert g["separable"] >= cc.MIN_TILES and g["straddle"] >= cc.MIN_TILES, g
        elif c["kind"] == "nosep":
            assert g["separable"] == 0, g
        assert (cr.amax(k, z, x) <= cr.ORACLE_RANGE) == (c["ref"] == "oracle")
    # every record is a shape the launch is said to take: at least 2^20 entries for the largest, sizes as listed
    assert max(n1 for n1, m in c["recs"]) * x.size >= 1 << 20
    assert len({cr.sm_mpad(m) for n1, m in c["recs"]}) == 1


def test_threshold_case_sits_on_the_threshold():
    z, x, expect = cc.threshold_inputs()
    kern = cc.kernel(cc.M12, 12, 1.0, seed=5)
    for ktype in (cc.M12, cc.M52):
        cls, _ = cr.tile_classes(dict(kern, type=ktype), z, x)
        for t, w, want in expect:
            assert cls[t, w] == want, (t, w, want, cls[t, w])
            a, b = z[16 * t:16 * t + 16], x[32 * w:32 * w + 32]
            gap = (a.min() - b.max()) if t % 4 < 2 else (b.min() - a.max())
            assert gap == (1.0 if want else 1.0 - 1.0 / 16.0)                  # exactly on it, or exactly one grid step short
            # the neighbours on the far side are separable, the one on the near side is not
            far, near = (w - 1, w + 1) if t % 4 < 2 else (w + 1, w - 1)
            assert cls[t, far] == (1 if t % 4 < 2 else -1) and cls[t, near] == 0


@pytest.mark.parametrize("c", [c for c in cc.MFMA_CASES if c["ref"] == "oracle"], ids=lambda c: c["id"])
def test_emulation_and_references_agree_within_the_oracle_range(c):
    e = _evaluated(c)
    assert e["amax"] <= cr.ORACLE_RANGE
    u_emu = cr.units(e["emu"], e["oracle"])
    u_ref = cr.units(e["oracle"][e["rows"]], e["closed"], e["far"])
    u_near = cr.units(e["oracle"][e["rows"]], e["closed"], ~e["far"])
    print("%s: emulation vs oracle %.3f; oracle vs closed form %.3f at least a lengthscale apart, %.1f nearer "
          "(units of 1e-11 |ref| + 1e-12)" % (c["id"], u_emu, u_ref, u_near))
    assert u_emu <= 1.0
    assert u_ref <= 1.0


@pytest.mark.parametrize("c", [c for c in cc.MFMA_CASES if c["ref"] == "closed"], ids=lambda c: c["id"])
def test_recorded_bars_are_what_the_emulation_measures(c):
    e = _evaluated(c)
    assert e["amax"] > cr.ORACLE_RANGE
    m_sep, m_band = cr.units(e["emu"], e["closed"], e["sep"]), cr.units(e["emu"], e["closed"], ~e["sep"])
    print("%s: emulation vs closed form %.4f on separable tiles, %.4f on entry-by-entry tiles; oracle vs closed form %.4f / %.4f"
          % (c["id"], m_sep, m_band, cr.units(e["oracle"], e["closed"], e["sep"]), cr.units(e["oracle"], e["closed"], ~e["sep"])))
    # the recorded figures are this computation's, written with three digits; the bars are four times them
    for got, rec in ((m_sep, c["measured"][0]), (m_band, c["measured"][1])):
        assert abs(got - rec) <= 0.01 * rec + 5e-4
    assert c["bar"] == pytest.approx((4.0 * c["measured"][0], 4.0 * c["measured"][1]))


def test_single_and_group_shapes_sit_on_the_tiers_they_name():
    for n1, n2, rows in cc.SINGLE_SHAPES:
        assert cc.rows_for(n1, n2) == rows and n1 % rows != 0 and n2 % 2 == 1
    assert cc.rows_for(1030, 1030) == 32 and -(-1030 // 512) == 3
    assert max(cc.GROUP_N1) * max(cc.GROUP_N2_SHARED, cc.GROUP_N2_OWN) < 1 << 20
    for ktype, ms, l in cc.GROUP_FAMILIES:
        assert len({cr.sm_mpad(m) for m in ms}) == 1
    assert cc.rows_for(64, 16385) == 32 and cc.rows_for(109, 1001) == 4
    for P in cc.SUM_P:
        for mp in cc.SUM_MPAD:
            ms = [len(k["frequency"]) for k in cc.sum_kernels(P, mp)]
            assert {cr.sm_mpad(m) for m in ms} == {mp} and len(set(ms)) > 1
