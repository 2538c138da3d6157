"""The score of the exact likelihood without a device: the numpy restatement (tests/ssm_score_ref.py) against torch autograd of
the dense Gaussian on the idealised kernels at every shape the GPU tests use, the handle-free workspace function, and the
refusals of the Python entry points that come before any device work."""
import numpy as np
import pytest

import ssm_score_ref as S
import ssm_smooth_ref as R

IDS = [S.case_id(i) for i in range(len(S.CASES))]


# ---- (a) the restatement against autograd of the dense log N(y | 0, K + s2 I): a tenth of the bar the GPU is held to ----------
@pytest.mark.parametrize("i", range(len(S.CASES)), ids=IDS)
def test_restatement_matches_dense_autograd(i):
    X, Y, _, kl, nz = S.case(i)
    ll, g, sc, gres = S.score(X, Y[:, 0], kl, nz)
    dl, dg, dres = S.dense_score(X, Y[:, 0], kl, nz)
    assert g.shape == dg.shape == sc.shape == S.param_vector(nz, kl).shape
    ratio = (np.abs(g - dg) / S.bar(dg, sc)).max()
    rres = np.abs(gres - dres).max() / (1e-8 * max(np.abs(dres).max(), 1e-3))
    print("    worst |restatement - autograd| / bar: gradient %.2e (recorded %.1e), d / dy %.2e; log-likelihood %.2e relative"
          % (ratio, S.DENSE_RATIO[IDS[i]], rres, abs(ll - dl) / abs(dl)))
    assert abs(ll - dl) <= 1e-9 * max(abs(dl), 1e-3)
    assert ratio <= 0.1 and rres <= 0.1


def test_the_value_is_the_smoothers_and_sums_have_their_scale():
    X, Y, Xn, kl, nz = S.case(IDS.index("d63-N37-mixed-s0.3"))
    ll, g, sc, _ = S.score(X, Y[:, 0], kl, nz)
    assert abs(ll - R.smooth(X, Y, np.zeros(0), kl, nz)[2]) <= 1e-13 * abs(ll)
    assert np.all(sc >= np.abs(g) * (1 - 1e-12))          # a sum of absolute values bounds the sum


def test_shuffled_frames_give_the_same_score():
    """the timeline is the stable ascending order of the frames; d / dy comes back in the caller's order"""
    X, Y, _, kl, nz = S.case(IDS.index("d4-N37-dup-s0.3"))
    perm = np.random.RandomState(5).permutation(X.shape[0])
    a, b = S.score(X, Y[:, 0], kl, nz), S.score(X[perm], Y[perm, 0], kl, nz)
    assert abs(a[0] - b[0]) <= 1e-12 * abs(a[0])
    assert np.all(np.abs(a[1] - b[1]) <= 1e-10 * np.maximum(a[2], 1e-3))
    assert np.abs(a[3][perm] - b[3]).max() <= 1e-10 * max(np.abs(a[3]).max(), 1e-3)


# ---- (b) the workspace function: handle-free, monotone in every argument, 0 outside its ranges ------------------------------
def test_workspace_function():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    f = lambda d, s, p, c: int(lib.gp_ssm_score_workspace_bytes(d, s, p, c))      # noqa: E731
    base = f(60, 2001, 3, 1)
    assert base % 256 == 0 and base >= 8 * 2001 * (60 * 60 + 3 * 60)
    assert base > int(lib.gp_ssm_smooth_workspace_bytes(60, 2001, 3, 1))          # the smoother's carve and the score's terms
    assert 3.9 * base < f(60, 2001, 3, 4) < 4.1 * base
    prev = 0
    for d in (3, 4, 59, 60, 61, 64, 65, 127, 128):
        assert f(d, 300, 3, 2) > prev
        prev = f(d, 300, 3, 2)
    for lo, hi in (((60, 1, 3, 1), (60, 2, 3, 1)), ((60, 300, 3, 1), (60, 301, 3, 1)), ((60, 300, 1, 1), (60, 300, 2, 1)),
                   ((60, 300, 59, 1), (60, 300, 60, 1)), ((60, 300, 3, 1), (60, 300, 3, 2)), ((60, 300, 3, 255), (60, 300, 3, 256))):
        assert 0 < f(*lo) <= f(*hi) and f(*lo) % 256 == 0
    assert f(60, 301, 3, 1) > f(60, 300, 3, 1) and f(60, 300, 3, 2) > f(60, 300, 3, 1)
    for bad in ((0, 10, 1, 1), (129, 10, 1, 1), (4, 0, 1, 1), (4, 10, 0, 1), (4, 10, 5, 1), (4, 10, 1, 0), (-1, 10, 1, 1)):
        assert f(*bad) == 0, bad


# ---- (c) refusals before any device work (there is no device here) -------------------------------------------------------------
def _sum_model(kl, **kw):
    X, Y, _, _ = R.problem(30, 4, 2, 1)
    return R.model(X, Y, kl, 0.1, **kw)


def test_refusals_raise_without_a_device():
    from gpitch_amd.windows import fit_windows_exact
    m32 = {"type": "matern32", "variance": 1.0, "lengthscales": 0.01, "energy": [], "frequency": []}
    X, Y, _, _ = R.problem(30, 4, 2, 1)
    wins = [(X, Y), (X + 0.01, Y)]
    calls = (lambda m: m.exact_log_likelihood_and_grad(), lambda m: m.optimize(objective="exact", maxiter=1),
             lambda m: fit_windows_exact(lambda h: m, wins, maxiter=1))
    for call in calls:
        with pytest.raises(NotImplementedError, match="kernel 1 of the sum is Matern32"):
            call(_sum_model(R.kernels(4) + [m32]))
        with pytest.raises(NotImplementedError, match="d = 129"):
            call(_sum_model(R.kernels(128) + R.kernels(1)))
    for call in calls:
        with pytest.raises(NotImplementedError, match="frame-sharded"):
            call(_sum_model(R.kernels(4), shard=(0, 2)))
    for call in calls[1:]:
        with pytest.raises(NotImplementedError, match="reg=True"):
            call(_sum_model(R.kernels(4), reg=True))
    from gpitch_amd.mean_functions import Constant
    with pytest.raises(NotImplementedError, match="mean_function"):
        fit_windows_exact(lambda h: _sum_model(R.kernels(4), mean_function=Constant(0.1)), wins, maxiter=1)
    with pytest.raises(ValueError, match="same number of frames"):
        fit_windows_exact(lambda h: _sum_model(R.kernels(4)), [wins[0], (X[:-1], Y[:-1])], maxiter=1)
    with pytest.raises(ValueError, match='"bound" or "exact"'):
        _sum_model(R.kernels(4)).optimize(objective="elbo")
    assert fit_windows_exact(lambda h: None, []) == []
