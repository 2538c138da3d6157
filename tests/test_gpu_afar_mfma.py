"""The activations' product on the float64 matrix cores (afar.hip afar_prod_kernel) at the places where it can
go wrong and test_gpu_afar.py's layouts do not go: afar_mfma_cases.py (test_afar_mfma_cases_cpu.py checks on the host that each
case reaches what it is listed for).  Per case: the route is taken, the device's ranges are the numpy rule's, the ELBO and every
gradient block agree with the dense products on the same handle within the project's bars for two float64 forms, and a second
evaluation, overlap levels 0 and 2 and a forward-only ELBO are bit-equal to the first."""
import numpy as np
import pytest

import afar_mfma_cases as mc
import test_gpu_afar as ga

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", sorted(mc.CASES))
def test_mfma_product_against_dense_products(gp_handle, case):
    c = mc.CASES[case]
    prob = mc.problem(**c)
    model = ga._model(prob, gp_handle)
    f1, v1, g1, _, far1, rng = ga._evaluate(prob, gp_handle, model=model)          # (compares the device's ranges with the rule's)
    assert far1 == 1
    for r in rng:
        assert c["nk"] <= {ke - kb for kb, ke in r}, case
    f2, v2, _, _, far2, _ = ga._evaluate(prob, gp_handle, model=model)              # the same plan again
    assert far2 == 1 and f2 == f1 and np.array_equal(v2, v1)
    f0, _, g0, _, far0, _ = ga._evaluate(prob, gp_handle, far=0)
    assert far0 == 0
    dev = abs(f1 - f0) / abs(f0)
    print("%s ELBO: matrix-core far field vs dense %.2e relative" % (case, dev))
    worst = 0.0
    for name in g0:
        d = np.abs(g1[name] - g0[name]).max() / max(np.abs(g0[name]).max(), 1e-12)
        print("%s %s: far field vs dense %.2e of the block's scale" % (case, name, d))
        worst = max(worst, d)
    assert dev <= ga.FAR_VS_DENSE_ELBO, (f1, f0)
    assert worst <= ga.FAR_VS_DENSE, worst
    for level in (0, 2):
        f_o, v_o, _, _, far_o, _ = ga._evaluate(prob, gp_handle, overlap=level)
        assert far_o == 1 and f_o == f1 and np.array_equal(v_o, v1), level
    m = ga._model(prob, gp_handle)
    assert m._elbo(False) == f1 and int(gp_handle.lib.gp_pdgp_far_field_act(m._plan)) == 1


def test_forward_only_elbo_meets_the_guard_on_the_helper_stream(gp_handle):
    """The Q route's product now waits for Q and its tables only; the guard joins the main stream behind it.
    At 4096 frames the chain runs on the helper stream.  A forward-only ELBO, which no backward prefetch follows there, is
    the gradient evaluation's bit for bit; and with a component lengthscale that trips the guard (test_gpu_qform.py's model: the
    guard only reads L and W and raises the status word) both calls fail with the error that names the switch, and the handle
    works again afterwards."""
    import test_gpu_qform as gq
    from gpitch_amd import _lib
    from helpers import pdgp_from_problem

    def model_of(prob):
        m = pdgp_from_problem(prob, handle=gp_handle)
        m.za.fixed = True
        m.zc.fixed = True
        m._pack()
        gp_handle.check(gp_handle.lib.gp_pdgp_set_overlap(m._plan, 2))
        return m
    shape = dict(N=4096, M=64, P=1)
    good = model_of(gq._problem(**shape))
    assert good._qform_admissible()
    f = good._elbo(True)
    assert model_of(gq._problem(**shape))._elbo(False) == f
    bad = model_of(gq._problem(**dict(shape, ls_com=1.0)))
    assert not bad._qform_admissible()
    f_ok = bad._elbo(False)
    assert np.isfinite(f_ok)
    gp_handle.check(gp_handle.lib.gp_pdgp_set_qform(bad._plan, 1))
    for grad in (False, True):
        with pytest.raises(_lib.GpitchError) as err:
            bad._elbo(grad)
        assert err.value.status == _lib.GP_ERR_UNSUPPORTED and "qform" in str(err.value)
    gp_handle.check(gp_handle.lib.gp_pdgp_set_qform(bad._plan, 0))
    assert bad._elbo(False) == f_ok
