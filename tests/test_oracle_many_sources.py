"""What the many-source GPU tolerance rests on (tests/test_gpu_many_sources.py).  CPU only.

The likelihood kernels accumulate a frame's cross term with a running prefix, the float64 oracle as log_lik_exp's
explicit pair sum (likelihoods.py:56-65): P (P - 1) / 2 products at up to P = 128 sources, in different association.
The operator bar of tests/test_gpu_ops.py, 1e-11 relative per frame, was set at P <= 12.  It stands at large P when the
oracle itself is within 2.5e-12 relative per frame of the exact value of the same formula: two float64 evaluations in
different order may each be that far from it, with a factor two of margin.  The exact value is the mpmath composition
of oracle/mp_elbo.py (50 digits): hermgauss1d plus the log_lik_exp formula, on the very inputs the GPU test draws."""
import mpmath as mp
import numpy as np
import pytest

from oracle import gpflow05 as orc
from oracle import mp_elbo

NOISE = 0.37
LANES = 16                  # csrc/lik.hip LIK_LANES, csrc/gh_quad.h MOM_LANES
ORACLE_BUDGET = 2.5e-12     # relative per frame: a quarter of the operator bar 1e-11


def many_source_inputs(P, N, nlin):
    """Fmu, Fvar (N x 2P), Y (N x 1) drawn as tests/test_gpu_ops.py::test_mpd_varexp_matches_oracle draws them.  Every
    source differs, in every frame and in each of its four moments, from the source LANES places before it (the one the
    same lane took on its previous trip): a kernel that reuses that neighbour's value cannot agree by accident."""
    rng = np.random.RandomState(100000 + 1000 * P + 10 * N + nlin)
    Fmu = rng.randn(N, 2 * P) * 2.0 + 1.0
    Fvar = rng.rand(N, 2 * P) * 3.0 + 1e-8
    Y = rng.randn(N, 1)
    for a in (Fmu[:, :P], Fmu[:, P:], Fvar[:, :P], Fvar[:, P:]):
        assert np.all(a[:, LANES:] != a[:, :-LANES])
    return Fmu, Fvar, Y


def mp_varexp(Fmu, Fvar, Y, noise, P, nlin):
    """MpdLik.variational_expectations per frame at 50 digits: mp_elbo.hermgauss1d and the formula of log_lik_exp with
    its explicit pair sum (the per-frame term of mp_elbo.pdgp_elbo on given moments); a list of N mpf"""
    N = Fmu.shape[0]
    f = lambda a: [mp.mpf(float(v)) for v in a]
    s2 = mp.mpf(float(noise))
    E1, E2, mf, vf = [], [], [], []
    for i in range(P):
        e1, e2 = mp_elbo.hermgauss1d(f(Fmu[:, i]), f(Fvar[:, i]), nlin)
        E1.append(e1); E2.append(e2)
        mf.append(f(Fmu[:, P + i])); vf.append(f(Fvar[:, P + i]))
    ys = f(Y.reshape(-1))
    out = []
    for n in range(N):
        a = [E1[i][n] * mf[i][n] for i in range(P)]
        A = mp.fsum(a)
        B = mp.fsum(E2[i][n] * (vf[i][n] + mf[i][n] ** 2) for i in range(P))
        C = 2 * mp.fsum(a[i] * a[j] for i in range(P - 1) for j in range(i + 1, P))
        out.append(-(((ys[n] ** 2 - 2 * ys[n] * A + B + C) / s2) + mp.log(2 * mp.pi) + mp.log(s2)) / 2)
    return out


def oracle_vs_mpmath(P, N, nlin):
    """(largest relative error of a frame, relative error of the sum over frames) of the float64 oracle against mp_varexp"""
    Fmu, Fvar, Y = many_source_inputs(P, N, nlin)
    ref = orc.mpd_variational_expectations(Fmu, Fvar, Y, NOISE, P, nlin)[:, 0]
    exact = mp_varexp(Fmu, Fvar, Y, NOISE, P, nlin)
    per = max(float(abs((mp.mpf(float(r)) - e) / e)) for r, e in zip(ref, exact))
    tot = mp.fsum(exact)
    return per, float(abs((mp.mpf(float(ref.sum())) - tot) / tot))


@pytest.mark.parametrize("P,nlin", [(17, 0), (17, 1), (17, 2), (128, 0)])
def test_oracle_is_within_its_share_of_the_operator_bar_at_many_sources(P, nlin):
    per, tot = oracle_vs_mpmath(P, 8, nlin)
    print("P %d nlin %d: oracle vs mpmath %.3g relative per frame, %.3g on the sum (budget %.3g)"
          % (P, nlin, per, tot, ORACLE_BUDGET))
    assert per < ORACLE_BUDGET, (P, nlin, per)
    assert tot < ORACLE_BUDGET, (P, nlin, tot)
