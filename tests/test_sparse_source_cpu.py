"""The restatement of the sparse per-source posterior (tests/sparse_source_ref.py) against the oracle: its sources add up to
predict_f, one source IS predict_f, and with Z = X it meets the exact posterior up to the 1e-6 jitter."""
import numpy as np
import pytest

from oracle import gpflow05 as orc
from sparse_source_ref import problem, sparse_source


def test_source_means_add_up_to_predict_f():
    X, Y, Z, kl = problem(300, 24, 3, 5)
    Xs = X[::3] + 1e-5
    sm, sv = sparse_source(Xs, X, Y, Z, kl, 0.2)
    rm, _ = orc.sgpr_predict_f(Xs, X, Y, Z, kl, 0.2)
    assert np.abs(sum(sm) - rm).max() <= 1e-12 * np.abs(rm).max()


def test_one_source_is_predict_f():
    X, Y, Z, kl = problem(200, 12, 1, 3)
    Xs = X[::2] + 1e-5
    sm, sv = sparse_source(Xs, X, Y, Z, kl, 0.2)
    rm, rv = orc.sgpr_predict_f(Xs, X, Y, Z, kl, 0.2)
    assert np.abs(sm[0] - rm).max() <= 1e-12 * np.abs(rm).max()
    assert np.abs(sv[0] - rv).max() <= 1e-12 * np.abs(rv).max()


@pytest.mark.parametrize("N", [64, 96])
def test_inducing_points_at_the_frames_give_the_exact_posterior(N):
    """Z = X: q(u) is the exact posterior of f(X) (up to the jitter on Kuu), so every source's sparse posterior is its exact
    one; the exact variance is moved from the sum kernel's Kdiag (sgpr_ss.py:101) to the source's own.  Bounds 1e-5: ten
    times the gap the 1e-6 jitter leaves (means 1.4e-6 relative, variances 1.1e-6 absolute)."""
    X, Y, _, kl = problem(N, N, 3, N)
    Xs = np.linspace(X.min(), X.max(), 41).reshape(-1, 1) + 1e-5
    sm, sv = sparse_source(Xs, X, Y, X.copy(), kl, 0.2)
    em, ev = orc.sgpr_predict_source(Xs, X, Y, kl, 0.2)
    kd_sum = orc.Kdiag_sum(kl, Xs).reshape(-1, 1)
    for p in range(3):
        assert np.abs(sm[p] - em[p]).max() <= 1e-5 * np.abs(em[p]).max()
        own = ev[p] - kd_sum + orc.Kdiag(kl[p], Xs).reshape(-1, 1)
        assert np.abs(sv[p] - own).max() <= 1e-5
