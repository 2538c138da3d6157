"""The simulation smoother without a device: the numpy restatement of the map (tests/ssm_sample_ref.py) against the Kalman
smoother's restatement and the dense exact GP on the idealised kernels (its mean at zero normals, its linear part's A A^T against
the full joint posterior covariance), the shapes of the normals, the checks of the Python layer and the workspace's dry run."""
import numpy as np
import pytest

import ssm_sample_ref as SR
import ssm_smooth_ref as R

IDS = [R.case_id(i) for i in range(len(R.CASES))]
LINEAR = ["d1-N37-mixed", "d4-N37-mixed", "d4-N2-mixed", "d4-N37-dup"]


def _close(name, got, ref, rel=1e-8, floor=1e-3):
    err, bar = np.abs(np.asarray(got) - np.asarray(ref)).max(), rel * max(np.abs(ref).max(), floor)
    print("    %s: largest difference %.3e (bar %.3e)" % (name, err, bar))
    assert err <= bar, name


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_zero_normals_give_the_posterior_mean(i):
    X, Y, Xn, kl, nz = R.case(i)
    gn = SR.gains(X, Xn, kl, nz)
    got = SR.draw(gn, Y, np.zeros((1, gn["steps"], gn["d"])), np.zeros((1, gn["N"])))[:, 0]
    assert got.shape == (len(kl), Xn.shape[0])
    _close("against the smoother's mean", got, R.smooth(X, Y, Xn, kl, nz)[0])
    _close("against the dense mean", got.reshape(-1), SR.dense_joint(X, Y, Xn, kl, nz)[0])


@pytest.mark.parametrize("name", LINEAR)
def test_linear_part_has_the_joint_posterior_covariance(name):
    X, Y, Xn, kl, nz = R.case(SR.case_index(name))
    gn = SR.gains(X, Xn, kl, nz)
    A = SR.linear_part(gn, Y)
    cov = A.dot(A.T)
    _close("A A^T against the dense joint covariance", cov, SR.dense_joint(X, Y, Xn, kl, nz)[1])
    _close("its diagonal against the smoother's variances", np.diag(cov), R.smooth(X, Y, Xn, kl, nz)[1].reshape(-1))


def test_the_map_is_affine_and_repeats_repeated_frames():
    X, Y, Xn, kl, nz = R.case(SR.case_index("d4-N37-mixed"))
    gn = SR.gains(X, Xn, kl, nz)
    ex, ey = SR.random_eps(gn, 3, 5)
    a, z = SR.draw(gn, Y, ex, ey), SR.draw(gn, Y, 0 * ex[:1], 0 * ey[:1])
    b = SR.draw(gn, Y, 2 * ex, 2 * ey)
    assert np.abs((b - z) - 2 * (a - z)).max() <= 1e-12
    xs = Xn.reshape(-1)
    same = [(i, k) for i in range(xs.size) for k in range(i) if xs[i] == xs[k]]
    assert len(same) >= 3 and all(np.array_equal(a[:, :, i], a[:, :, k]) for i, k in same)


def test_eps_shapes():
    from gpitch_amd import ssm_sample_eps_shapes
    from gpitch_amd import _lib
    codes = [(_lib.KERN_MERCER_MATERN12SM, 10), (_lib.KERN_MATERN12SM, 3), (_lib.KERN_MATERN12, 0)]
    assert ssm_sample_eps_shapes(codes, 87, 37, 5) == ((5, 87, 27), (5, 37))
    assert ssm_sample_eps_shapes(codes, 40, 40) == ((1, 40, 27), (1, 40))
    kern = np.sum([R.kern_from_dict(k) for k in R.kernels(63)])
    assert ssm_sample_eps_shapes(kern, 9, 4, 2) == ((2, 9, 63), (2, 4))
    with pytest.raises(NotImplementedError, match="sample_s_ssm: kernel 1 of the sum is Matern32"):
        ssm_sample_eps_shapes([(_lib.KERN_MATERN12, 0), (_lib.KERN_MATERN32, 0)], 3, 3)


def _sum_model(kl, D=1, **kw):
    X, Y, _, _ = R.problem(30, 4, 2, 1)
    return R.model(X, np.tile(Y, (1, D)), kl, 0.1, **kw), X


def test_checks_raise_without_a_device():
    m32 = {"type": "matern32", "variance": 1.0, "lengthscales": 0.01, "energy": [], "frequency": []}
    with pytest.raises(NotImplementedError, match="sample_s_ssm: kernel 1 of the sum is Matern32"):
        _sum_model(R.kernels(4) + [m32])[0].sample_s_ssm(np.zeros(3))
    with pytest.raises(NotImplementedError, match="sample_s_ssm: the state dimension d = 130"):
        _sum_model(R.kernels(128) + R.kernels(2))[0].sample_s_ssm(np.zeros(3))
    with pytest.raises(NotImplementedError, match="frame-sharded"):
        _sum_model(R.kernels(4), shard=(0, 2))[0].sample_s_ssm(np.zeros(3))
    m, X = _sum_model(R.kernels(4))
    with pytest.raises(ValueError, match="at least one new point and one sample"):
        m.sample_s_ssm(np.zeros(0))
    with pytest.raises(ValueError, match="at least one new point and one sample"):
        m.sample_s_ssm(np.zeros(3), num_samples=0)
    xn = np.array([X[3, 0], X[3, 0] + 1e-5, -1.0, -1.0])          # 30 training frames + 2 fresh values: 32 steps
    good = (np.zeros((2, 32, 4)), np.zeros((2, 30)))
    for bad in ((np.zeros((2, 4, 32)), good[1]), (good[0], np.zeros((2, 32))), (np.zeros((2, 34, 4)), good[1]), good[:1],
                (good[0][:1], good[1][:1])):
        with pytest.raises(ValueError, match=r"eps must be \(eps_x, eps_y\) of shapes \[\(2, 32, 4\), \(2, 30\)\]"):
            m.sample_s_ssm(xn, num_samples=2, eps=bad)
    m2, _ = _sum_model(R.kernels(4), D=2)                          # two columns: a leading D axis
    with pytest.raises(ValueError, match=r"shapes \[\(2, 2, 32, 4\), \(2, 2, 30\)\]"):
        m2.sample_s_ssm(xn, num_samples=2, eps=good)


def test_workspace_dry_run_is_handle_free():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    size = lambda *a: int(lib.gp_ssm_sample_workspace_bytes(*a))
    for d, steps, P, S, count in ((0, 10, 1, 1, 1), (129, 10, 1, 1, 1), (4, 0, 1, 1, 1), (4, 10, 0, 1, 1), (4, 10, 5, 1, 1),
                                  (4, 10, 1, 0, 1), (4, 10, 1, 1, 0)):
        assert size(d, steps, P, S, count) == 0
    for args in ((1, 1, 1, 1, 1), (4, 87, 1, 3, 1), (63, 87, 4, 3, 3), (128, 350, 2, 190, 1)):
        assert size(*args) > 0 and size(*args) % 256 == 0
    by_s = [size(60, 2001, 3, S, 1) for S in (1, 2, 3, 16, 17)]
    by_count = [size(60, 2001, 3, 16, c) for c in (1, 2, 3, 256)]
    assert all(a < b for a, b in zip(by_s, by_s[1:])) and all(a < b for a, b in zip(by_count, by_count[1:]))
    # a draw costs its r history, steps * d doubles, and two [steps] vectors
    assert 8 * 2001 * 62 <= by_s[1] - by_s[0] <= 8 * 2001 * 62 + 3 * 256
    # no steps * d^2 block: about (3 d + 6 P) steps doubles of prologue and gains and steps * d per draw, against steps * d^2
    big, smooth = size(100, 65536, 5, 1, 1), int(lib.gp_ssm_smooth_workspace_bytes(100, 65536, 5, 1))
    print("    d = 100, steps = 65536, P = 5, S = 1: %.1f MB against the smoother's %.2f GB" % (big / 1e6, smooth / 1e9))
    assert 0 < big < smooth / 10
