"""The store of Y, its far columns, the per-group A gm and the check's flag (hfar.hip) in the plan's carve: an
activation plan of two GPs that takes the form, between guard bands at exactly gp_pdgp_workspace_bytes and one granule short
(test_gpu_workspace_bounds.py's check: results equal those of a workspace twice as large, the guard bands untouched, a
granule less refused before anything is launched)."""
import pytest

import test_gpu_afar as ta
import test_gpu_hfar as th
import test_gpu_workspace_bounds as wb

pytestmark = pytest.mark.gpu


def test_workspace_at_its_exact_size(gp_handle, monkeypatch):
    prob = ta._problem(**ta.CASES["two_gps_192x5632"])

    def run():
        m = th._model(prob, gp_handle)
        out = {"elbo": m._elbo(True), "grad": m._grad.cpu().numpy().copy()}
        assert int(gp_handle.lib.gp_pdgp_h_far(m._plan)) == 1
        return out
    wb._check(gp_handle, monkeypatch, run, exact_keys=("elbo",))
