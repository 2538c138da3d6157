"""CPU checks of what tests/test_gpu_hyper.py rests on: the long-double reference of the kernel-gradient contractions against torch
autograd of the kernel definitions, its bound against a float64 evaluation in the kernels' order (for every case of the tables:
the bound is not too tight before any GPU is involved), the Python replica of the dispatch against hand-listed examples and the
library's own queries, and the sizing rule every plan's partial-record workspace rests on."""
import numpy as np
import pytest

import hyper_cases as hc
import hyper_ref as hr

LD = np.longdouble
FAMILIES = ((hr.MATERN12, 0), (hr.MATERN32, 0), (hr.MATERN52, 0), (hr.RBF, 0), (hr.MERCER12, 3), (hr.M12SM, 3), (hr.M32SM, 2),
            (hr.MERCER52, 2))


def _autograd(ktype, theta, x1, x2, w, kuu):
    import torch
    from oracle import gpflow05 as gp
    from oracle.backend import TorchBackend
    xp = TorchBackend()
    m = hr.num_partials(ktype, theta)
    t = torch.tensor(theta, dtype=torch.float64, requires_grad=True)
    X1 = torch.tensor(x1.reshape(-1, 1), dtype=torch.float64, requires_grad=True)
    X2 = None if kuu else torch.tensor(x2.reshape(-1, 1), dtype=torch.float64)
    kern = dict(type=hr.ORACLE_NAME[ktype], variance=t[0], lengthscales=t[1], energy=[t[2 + q] for q in range(m)],
                frequency=[t[2 + m + q] for q in range(m)])
    K = gp.K(kern, X1, X2, xp)
    (K * torch.tensor(w)).sum().backward()
    return t.grad.numpy(), X1.grad.numpy().reshape(-1)


@pytest.mark.parametrize("ktype,m", FAMILIES, ids=["type%d" % t for t, _ in FAMILIES])
@pytest.mark.parametrize("kuu", (False, True), ids=("kuf", "kuu"))
def test_reference_agrees_with_autograd(ktype, m, kuu):
    """sums and the inducing-input gradient against reverse-mode differentiation of the definition.  Kuu side: autograd of
    K(Z, Z) differentiates both arguments, the diagonal included (d_ii = +1e-12 both ways for the broadcast kernels, where the
    two one-sided derivatives cancel; a zero of d / r for the others)."""
    rng = np.random.RandomState(3 + ktype)
    theta = hc.theta_for(ktype, m, ls=0.3)
    n1, n2 = 6, (6 if kuu else 9)
    x1 = np.sort(rng.rand(n1))
    x2 = x1 if kuu else rng.rand(n2)
    G = rng.randn(n1, n2)
    ref = hr.contract_ref(ktype, theta, x1, x2, G, symmetric=kuu, want_gz=True)
    w, _ = hr.weights(G, None, None, kuu)
    gt, gx = _autograd(ktype, theta, x1, x2, w.astype(np.float64), kuu)
    scale = np.abs(ref["A"]).astype(np.float64)
    assert np.all(np.abs(ref["sums"].astype(np.float64) - gt) <= 1e-9 * scale + 1e-300), (ref["sums"], gt)
    gz = ref["gz"].sum(axis=0).astype(np.float64)
    assert np.all(np.abs(gz - gx) <= 1e-9 * ref["gzA"].sum(axis=0).astype(np.float64)), (gz, gx)


def test_finish_reference_kdiag_terms():
    """dKdiag/dtheta: the variance always; the energies only where Kdiag carries the energy sum (not the Matern-5/2 product)"""
    for ktype, m in FAMILIES:
        theta = hc.theta_for(ktype, m)
        ns = 2 + 2 * m
        r = hr.finish_ref(ktype, theta, np.zeros(ns), None, None, 2.0)
        want = np.zeros(ns)
        if ktype in (hr.MERCER12, hr.M12SM, hr.M32SM):
            want[0] = 2.0 * theta[2:2 + m].sum()
            want[2:2 + m] = 2.0 * theta[0]
        else:
            want[0] = 2.0
        np.testing.assert_allclose(r["g"].astype(np.float64), want, rtol=1e-15)


def _case_ref_and_replay(c, inp, k, form):
    rec = inp["recs"][k]
    kv = inp["kvals"] if form["form"] > 0 else None
    args = dict(alpha=rec["alpha"], gm=rec["gm"], symmetric=bool(c.get("symmetric")), gscale=rec["gscale"], kvals=kv,
                want_gz=bool(c.get("with_gz")))
    ref = hr.contract_ref(c["type"], inp["theta"], inp["x1"], inp["x2"], rec["G"], **args)
    rep = hr.replay64(c["type"], inp["theta"], inp["x1"], inp["x2"], rec["G"], rows_form=form["form"] > 0, **args)
    return ref, rep


@pytest.mark.parametrize("c", hc.all_contraction_cases(), ids=lambda c: c["name"])
def test_bound_holds_for_float64_replay(c):
    form = hc.expected_form(**hc.form_kwargs(c))
    inp = hc.inputs(c)
    for k in sorted(set([0, len(inp["recs"]) - 1])):
        ref, rep = _case_ref_and_replay(c, inp, k, form)
        tol = hr.bound(ref["A"], ref["C"], form["form"], form["wg_rows"], form["col_seg"])
        err = np.abs(rep["sums"].astype(LD) - ref["sums"])
        assert np.all(np.isfinite(rep["sums"])) and np.all(err <= tol), (c["name"], k, (err / np.maximum(tol, LD(1e-300))).astype(float))
        if c.get("with_gz"):
            tz = hr.bound(ref["gzA"], ref["gzC"], 0, form["wg_rows"], 0)
            ez = np.abs(rep["gz"].astype(LD) - ref["gz"])
            assert np.all(ez <= tz), (c["name"], k, float((ez / np.maximum(tz, LD(1e-300))).max()))
        # the bound is a bound, not a licence: it stays below 1e-6 of the majorant even where the inputs are ill-conditioned
        assert np.all(tol <= 1e-6 * ref["A"] + 1e-300)


def test_expected_form_hand_listed():
    f = hc.expected_form
    M12, M52 = hr.MERCER12, hr.MERCER52
    # generic: records = column blocks of 256 x row groups of 8 (32 from n1 n2 = 2^20 on)
    assert f(0, hr.MATERN32, 0, 9, 257, with_gz=True)["nparts"] == 2 * 2
    assert f(0, hr.MATERN12, 0, 256, 4096, with_gz=True)["nparts"] == 16 * 8
    assert f(0, hr.MATERN12, 0, 256, 4095, with_gz=True)["nparts"] == 16 * 32
    assert f(0, hr.RBF, 0, 1024, 1024, with_gz=True, symmetric=True)["nparts"] == 4 * 32
    assert f(0, hr.MATERN32, 0, 9, 257, with_gz=True)["inst"] == "hyper_contract_kernel<1,false,true,1>"
    assert f(0, hr.M32SM, 32, 9, 257)["inst"] == "hyper_m12sm_kernel<false>"
    # lean: whole 16-tiles, Matern-1/2, up to 24 partials
    for m, nt in ((1, 1), (8, 1), (9, 2), (16, 2), (17, 3), (24, 3)):
        e = f(1, M12, m, 64, 96, count=2)
        assert (e["form"], e["nt"], e["nparts"], e["col_seg"], e["nseg"]) == (2, nt, 1, 96, 1), (m, e)
    assert f(1, M12, 25, 64, 96, count=2)["inst"] == "hyper_contract_kernel<28,true,false>"
    assert f(1, M12, 5, 64, 96, count=2, lean_items=0)["form"] == 1
    assert f(1, M12, 5, 64, 96, count=2, use_mfma=0)["form"] == 0
    assert f(1, M12, 5, 64, 96, count=2, with_gz=1)["form"] == 0
    assert f(1, M12, 5, 64, 96, count=2, gscale=1)["inst"] == "hyper_sm_rows_lean_kernel<1,false,SC>"
    # rows: ragged shapes and the Matern-5/2 envelope, up to 16 partials
    assert f(0, M12, 5, 17, 33)["inst"] == "hyper_sm_rows_kernel<1,false,false>" and not f(0, M12, 5, 17, 33)["sep"]
    assert f(0, M52, 9, 64, 96, g32=1)["inst"] == "hyper_sm_rows_kernel<2,true,true>"
    assert f(0, M52, 17, 64, 96)["form"] == 0 and f(0, M12, 17, 17, 33)["form"] == 0
    assert f(0, M12, 5, 64, 96, has_kvals=False)["form"] == 0 and f(0, M12, 5, 64, 96, has_alpha=False)["form"] == 0
    assert f(0, M12, 5, 64, 64, aligned=False)["form"] == 1 and f(0, M12, 5, 64, 32, even_ld=False)["form"] == 1
    # segments of one 64-row record: 2, 4, 4 (the last one 432 of 544 columns)
    assert [(f(0, M12, 5, 64, n)["col_seg"], f(0, M12, 5, 64, n)["nseg"]) for n in (1024, 2048, 2064)] == [(512, 2), (512, 4), (544, 4)]
    # 1024 records: one segment, beyond the lean table at 2064 columns, beyond the rows form's envelope table at 4112
    e = f(1, M12, 5, 16, 2064, count=1024)
    assert (e["form"], e["col_seg"], e["nseg"], e["sep"]) == (1, 2080, 1, True)
    e = f(1, M12, 5, 16, 4112, count=1024)
    assert (e["form"], e["col_seg"], e["nseg"], e["sep"]) == (1, 4128, 1, False)
    assert f(2, M12, 0, 33, 513, count=4)["nparts"] == 3 * 5


def test_every_listed_instantiation_is_named_by_a_case():
    """the dispatch code's instantiations (hyper_generic_dispatch, hyper_rows_dispatch, the sum switch): each is the expected form
    of at least one case, whose GPU test asserts the form by its record count"""
    got = set(hc.expected_form(**hc.form_kwargs(c))["inst"] for c in hc.all_contraction_cases())
    got |= set("hyper_contract_sum_kernel<%d>" % c["P"] for c in hc.sum_cases() if c["taken"])
    want = set()
    for gz in ("true", "false"):
        want |= set("hyper_contract_kernel<1,false,%s,%d>" % (gz, t) for t in range(4))
        want |= set("hyper_contract_kernel<%d,true,%s>" % (mp, gz) for mp in range(4, 33, 4))
        want.add("hyper_m12sm_kernel<%s>" % gz)
    want |= set("hyper_contract_sum_kernel<%d>" % p for p in range(2, 7))
    for g in ("true", "false"):
        want |= set("hyper_sm_rows_lean_kernel<%d,%s>" % (nt, g) for nt in (1, 2, 3))
        want |= set("hyper_sm_rows_kernel<%d,%s,%s>" % (nt, m52, g) for nt in (1, 2) for m52 in ("true", "false"))
    want |= set("hyper_sm_rows_lean_kernel<%d,false,SC>" % nt for nt in (1, 2, 3))
    assert want - got == set(), sorted(want - got)


def _lib():
    from gpitch_amd import _lib
    return _lib.load_library()


def test_expected_form_agrees_with_lean_takes_query():
    lib = _lib()
    n = 0
    for ktype in (hr.MERCER12, hr.MERCER52, hr.MATERN12):
        for m in (1, 8, 9, 16, 17, 24, 25, 32):
            for n1 in (16, 17, 64, 80, 512):
                for n2 in (16, 31, 32, 2048, 2064, 4096, 4112, 65536):
                    for count in (1, 4, 64, 1024):
                        e = hc.expected_form(1, ktype, m if ktype != hr.MATERN12 else 0, n1, n2, count)
                        takes = lib.gp_debug_hyper_lean_takes(ktype, m, n1, n2, count)
                        assert takes == (1 if e["form"] == 2 else 0), (ktype, m, n1, n2, count, e)
                        n += 1
    assert n > 3000
    assert lib.gp_debug_hyper_lean_takes(hr.MERCER12, 5, 64, 96, 0) == 0 and lib.gp_debug_hyper_lean_takes(hr.MERCER12, 0, 64, 96, 1) == 0


def test_record_count_never_exceeds_the_sizing_rule():
    """hyper_kuf_records(N, M) sizes every plan's partial-record workspace for a contraction of ANY form over M x N' (N' <= N):
    no form may leave more records than it gives."""
    lib = _lib()
    assert lib.gp_debug_hyper_records(0, 4) == -1 and lib.gp_debug_hyper_records(4, 0) == -1
    worst = 0.0
    for N in (1, 255, 256, 257, 2001, 4096, 65536, 65537):
        for M in range(1, 1101):
            cap = lib.gp_debug_hyper_records(N, M)
            for count in (1, 4, 64, 1024):
                got = hc.max_records(M, N, count)
                assert got <= cap, (N, M, count, got, cap)
                worst = max(worst, got / float(cap))
    assert worst <= 1.0
    # and for a smaller batch of the same plan (the small-workgroup form only while M N' < 2^20)
    for M, N, Ns in ((256, 65536, 4095), (256, 65536, 4096), (64, 65536, 16383), (1100, 65537, 953)):
        assert hc.max_records(M, Ns, 1) <= lib.gp_debug_hyper_records(N, M)


def test_device_function_ports_accuracy():
    """the figures the bound's kappa uses (4.5 u, 1.5 u, 3.5 u; 1 ulp = 2 u), measured on the CPU against long double"""
    x = -np.concatenate([np.linspace(0, 744, 100001), 10.0 ** np.linspace(-12, 2.8, 100001)])
    got = hr.exp_neg_port(x)
    want = np.exp(x.astype(LD))
    ok = want > LD(1e-300)
    ulp = np.spacing(want[ok].astype(np.float64)).astype(LD)
    e_exp = float((np.abs(got[ok].astype(LD) - want[ok]) / ulp).max())
    xs = 10.0 ** np.linspace(-13, 4, 200001)
    s, ri = hr.sqrt_rsqrt_port(xs)
    ws, wr = np.sqrt(xs.astype(LD)), 1 / np.sqrt(xs.astype(LD))
    e_s = float((np.abs(s.astype(LD) - ws) / np.spacing(ws.astype(np.float64)).astype(LD)).max())
    e_r = float((np.abs(ri.astype(LD) - wr) / np.spacing(wr.astype(np.float64)).astype(LD)).max())
    print("gp_exp_neg port: %.3f ulp; gp_sqrt_rsqrt_pos port: s %.3f ulp, rinv %.3f ulp" % (e_exp, e_s, e_r))
    assert e_exp <= 2.25 and e_s <= 0.75 and e_r <= 1.75
