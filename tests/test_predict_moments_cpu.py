"""Host-side checks of the source / mixture / held-out-density predictions: the new C-ABI entries are exported with the
header's argument counts, the Python entries refuse bad input before any device work, and the formula the GPU tests
use as their reference (tests/test_gpu_predict_moments.py) is sound on the quadrature grid.  No GPU needed."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gp_mpd_predict_moments", "gp_pdgp_predict_moments", "gp_pdgp_predict_moments_reuse",
               "gp_pdgpb_predict_moments_workspace_bytes", "gp_pdgpb_predict_moments")


def _header_arg_counts():
    src = open(os.path.join(ROOT, "include", "gpitch_abi.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(gp_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_new_symbols_are_exported_with_the_headers_argument_counts():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    counts = _header_arg_counts()
    assert counts["gp_mpd_varexp"] == 10 == len(lib.gp_mpd_varexp.argtypes)      # the parser, on a known entry
    for name in NEW_SYMBOLS:
        assert name in _lib.ABI_SYMBOLS and name in counts, name
        assert len(getattr(lib, name).argtypes) == counts[name], name
    assert counts["gp_mpd_predict_moments"] == 13


def _no_device(monkeypatch):
    from gpitch_amd import _lib

    def refuse(*a, **k):
        raise AssertionError("a handle was asked for before the arguments were checked")
    monkeypatch.setattr(_lib, "default_handle", refuse)
    monkeypatch.setattr(_lib, "Handle", refuse)


def _model(seed=3, P=1, n=200):
    from gpitch_amd.synth import make_problem, pdgp_from_problem
    p = make_problem(n, 12, P, num_partials=2, seed=seed)
    return pdgp_from_problem(p), p


def test_predict_sources_many_checks_its_arguments_on_the_host(monkeypatch):
    import gpitch_amd
    _no_device(monkeypatch)
    (m0, p0), (m1, p1) = _model(3), _model(4, P=2)
    x = p0["x"][:50]
    with pytest.raises(ValueError, match="targets of model 1 have shape"):
        gpitch_amd.predict_sources_many([m0, m1], [x, x], [np.zeros(50), np.zeros(49)])
    with pytest.raises(ValueError, match="1 target arrays for 2 models"):
        gpitch_amd.predict_sources_many([m0, m1], [x, x], [np.zeros(50)])
    with pytest.raises(ValueError, match="targets of model 0"):
        gpitch_amd.predict_sources_many([m0, m1], x, np.zeros((50, 2)))
    with pytest.raises(ValueError, match="item 1 is not a Pdgp"):
        gpitch_amd.predict_sources_many([m0, object()], x)
    with pytest.raises(ValueError, match="the same model appears twice"):
        gpitch_amd.predict_sources_many([m0, m0], x)
    with pytest.raises(ValueError, match="needs at least one model"):
        gpitch_amd.predict_sources_many([], x)
    assert m0._plan is None and m1._plan is None


def test_pdgp_methods_check_their_arguments_on_the_host(monkeypatch):
    _no_device(monkeypatch)
    m, p = _model(5)
    x = p["x"][:40]
    with pytest.raises(ValueError, match="ynew has shape"):
        m.expected_log_density(x, np.zeros(39))
    with pytest.raises(ValueError, match="ynew has shape"):
        m.expected_log_density(x, np.zeros((40, 2)))
    with pytest.raises(ValueError, match="needs ynew"):
        m.expected_log_density(x, None)
    for call in (m.predict_sources, m.predict_y, m.predict_mixture):
        with pytest.raises(ValueError, match="xnew has shape"):
            call(np.zeros((40, 2)))
    with pytest.raises(ValueError, match="N x 2\\*num_sources"):
        m.likelihood.predict_sources(np.zeros((5, 3)), np.zeros((5, 3)))
    with pytest.raises(ValueError, match="Y has 4 values for 5 rows"):
        m.likelihood.expected_log_density(np.zeros((5, 2)), np.ones((5, 2)), np.zeros(4))
    assert m._plan is None


def test_check_predictable_messages_are_unchanged(monkeypatch):
    """predict_sources_many shares predict_many's scope check: its wording is part of what callers match on"""
    import gpitch_amd
    from gpitch_amd import pdgp_batch
    _no_device(monkeypatch)
    m, p = _model(6)
    x = p["x"][:10]
    cases = [
        (lambda: pdgp_batch.check_predictable([], x), ValueError, "predict_many needs at least one model"),
        (lambda: pdgp_batch.check_predictable([m, m], x), ValueError, "predict_many: the same model appears twice in the list"),
        (lambda: pdgp_batch.check_predictable([m, 3], x), ValueError, "predict_many: item 1 is not a Pdgp"),
        (lambda: pdgp_batch.check_predictable([m], [x, x]), ValueError, "predict_many: 2 input arrays for 1 models"),
        (lambda: pdgp_batch.check_predictable([m], np.zeros((4, 2))), ValueError,
         "predict_many: inputs of model 0 have shape (4, 2), not (n,) or (n, 1)"),
    ]
    w, _ = _model(7)
    w.whiten = False
    cases.append((lambda: pdgp_batch.check_predictable([w], x), NotImplementedError,
                  "model 0: whiten=False is not batched; predict this model on its own with Pdgp.predict_act_n_com"))
    for call, exc, text in cases:
        with pytest.raises(exc) as e:
            call()
        assert str(e.value) == text
    for call in (lambda: gpitch_amd.predict_sources_many([w], x), lambda: gpitch_amd.predict_many([w], x)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == cases[-1][2]


def test_the_reference_form_of_the_source_variance():
    """svar = V m_f^2 + E2 v_f with V = sum_h w_h (nlin(x_h) - E1)^2 (the form the kernel codes and the GPU tests compose
    from the oracle's hermgauss1d) against E2 (v_f + m_f^2) - (E1 m_f)^2 on the grid of the quadrature check (mu in
    [-6, 12], s^2 in [1e-8, 25]), for the three nonlinearities.  The two differ by E1^2 m_f^2 (sum_h w_h - 1) and by the
    rounding of 20-term sums whose terms reach E2 (v_f + m_f^2): 64 eps of that magnitude bounds both (each sum rounds at
    most 20 times by half an ulp of its total, and the weights sum to 1 within a few ulp).  The first form is >= 0."""
    from oracle import gpflow05 as orc
    rs = np.random.RandomState(20)
    mu = np.concatenate([np.linspace(-6., 12., 61), rs.uniform(-6., 12., 200)])
    s2 = np.concatenate([np.logspace(-8, np.log10(25.), 40), rs.uniform(1e-8, 25., 60)])
    MU, S2 = [a.reshape(-1, 1) for a in np.meshgrid(mu, s2)]
    mf = rs.randn(*MU.shape) * 3.
    vf = rs.rand(*MU.shape) * 2. + 1e-10
    gh_x, gh_w = np.polynomial.hermite.hermgauss(20)
    w = (gh_w / np.sqrt(np.pi)).reshape(-1, 1)
    eps = np.finfo(np.float64).eps
    for code in (0, 1, 2):
        nl = orc.nlinfun(code)
        E1, E2 = orc.hermgauss1d(MU, S2, 20, nl)
        ev = nl(gh_x.reshape(1, -1) * np.sqrt(2. * S2) + MU)
        V = np.matmul((ev - E1) ** 2, w)
        a = V * mf ** 2 + E2 * vf
        b = E2 * (vf + mf ** 2) - (E1 * mf) ** 2
        assert np.all(V >= 0.) and np.all(a >= 0.)
        assert np.all(np.abs(a - b) <= 64 * eps * E2 * (vf + mf ** 2)), code
