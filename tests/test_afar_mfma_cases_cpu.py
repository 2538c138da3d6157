"""Host check of afar_mfma_cases.py: every case is admissible (a strip of 2^20 entries or more, ascending inducing inputs, a
lengthscale within FAR_ACT_MAX_SPACINGS median spacings), its ranges are monotone, and it reaches the near-row counts and range
starts it is listed for.  This is what keeps test_gpu_afar_mfma.py from passing on a case that no longer exercises anything."""
import numpy as np
import pytest

import afar_mfma_cases as mc
import afar_rule as af
from gpitch_amd.pdgp import Pdgp


@pytest.mark.parametrize("case", sorted(mc.CASES))
def test_case_reaches_what_it_is_listed_for(case):
    c = mc.CASES[case]
    prob = mc.problem(**c)
    assert c["P"] <= 2
    assert (1 << 20) <= c["M"] * c["N"] <= 1.2 * (1 << 20), case
    assert c["M"] % af.TILE == 0 and c["N"] % af.GROUP == 0
    x = np.ravel(prob["x"])
    assert np.all(np.diff(x) > 0)
    for p in range(c["P"]):
        z = np.ravel(prob["za"][p])
        assert np.all(np.diff(z) > 0), case
        ls = float(np.ravel(prob["kern_act"][p]["lengthscales"])[0])
        assert ls <= Pdgp.FAR_ACT_MAX_SPACINGS * float(np.median(np.diff(z))), case
        rng = mc.case_ranges(prob, p)
        assert af.is_monotone(rng), case
        nks = [ke - kb for kb, ke, _, _ in rng]
        assert all(nk % af.TILE == 0 and 0 <= nk <= c["M"] for nk in nks)
        assert c["nk"] <= set(nks), (case, sorted(set(nks)))
        if "kbeg" in c:
            assert c["kbeg"] <= {kb for kb, _, _, _ in rng}, (case, sorted({kb for kb, _, _, _ in rng}))
            assert any(kb % 64 for kb in c["kbeg"])
        if "crowd" in c:
            nk, groups = c["crowd"]
            assert nks.count(nk) == groups and len(nks) == groups + 1, (case, nks)
