"""Joint posterior draws of the SGPRSS sources, host side: the numpy restatement of the map (tests/sample_sparse_ref.py)
reproduces the closed-form joint posterior covariance and, at eps = 0, the sparse posterior mean; the host-only helpers of
the product (merged_order, the eps shapes, the kernel-support check) and the handle-free workspace size."""
import numpy as np
import pytest

import sample_sparse_ref as ref
from sparse_source_ref import sparse_source


def _linear_part(X, Y, Z, kl, noise, Xs):
    n, M = Xs.shape[0], Z.shape[0]
    ex, ez, eu = ref.identity_eps(kl, n, M)
    zero = [np.zeros((1,) + e.shape[1:]) for e in (ex, ez, eu)]
    base = ref.sample_sources(Xs, X, Y, Z, kl, noise, *zero)               # (P, 1, n)
    got = ref.sample_sources(Xs, X, Y, Z, kl, noise, ex, ez, eu)           # (P, S, n)
    T = (got - base).transpose(0, 2, 1).reshape(len(kl) * n, -1)           # rows (source, frame), one column per coordinate
    return T, base[:, 0, :]


def test_restatement_reproduces_the_joint_posterior_covariance():
    """T T^T against delta_pr K_p(x*, x*) - tmp1_p^T tmp1_r + tmp2_p^T tmp2_r, absolute 1e-5 max_p Kdiag_p: the difference is
    the model's r(x, x) = 1e-6 under the kernels' square root, which the OU recursion does not have (measured 2.4e-6 at
    Kdiag 1.0 - 1.1).  With eps = 0 the map is the sparse posterior mean, to 1e-12."""
    X, Y, Z, kl, noise, Xs = ref.smallest_problem()
    T, mean0 = _linear_part(X, Y, Z, kl, noise, Xs)
    assert T.shape == (2 * 40, (40 + 12) * 8 + 24)
    cov, kd = ref.joint_cov(Xs, X, Y, Z, kl, noise)
    err = np.abs(T.dot(T.T) - cov).max()
    print("T T^T against the closed form: %.3e at max Kdiag %.3f" % (err, kd))
    assert err <= 1e-5 * kd
    sm, _ = sparse_source(Xs, X, Y, Z, kl, noise)
    for p in range(2):
        assert np.abs(mean0[p] - sm[p][:, 0]).max() <= 1e-12


def test_ragged_mixed_gpu_shape_is_well_conditioned():
    """The inputs of tests/test_gpu_sample_sparse.py::test_ragged_windows_with_a_mixed_kernel_sum: two host routes of the same
    map (the restatement's triangular solves; products with the explicit W = L^-1, WB = LB^-1 the device holds) agree to a
    tenth of the 1e-8 rule in every slot, as tests/test_pdgp_sample_cpu.py asks of the Pdgp shapes."""
    from scipy.linalg import solve_triangular
    from oracle import gpflow05 as orc
    from test_gpu_sample_sparse import _ragged_mixed_windows, _random_eps
    counts, N, M, S, n = [16, 9, 1], 300, 16, 17, 70
    for i, ((X, Y, Z, kl), k) in enumerate(zip(_ragged_mixed_windows(counts, N), counts)):
        noise = 0.2 + 0.05 * i
        Xs = np.linspace(X.min(), X.max(), n).reshape(-1, 1)
        ex, ez, eu = _random_eps(kl, n, M, S, 80 + i)
        ez, eu = ez[:, :, :k], eu[:, :, :k]
        a = ref.sample_sources(Xs, X, Y, Z, kl, noise, ex, ez, eu)
        err, Kdg, L, A, AAT, LB, c = orc.sgpr_common(X, Y, Z, kl, noise)
        W, WB = solve_triangular(L, np.eye(k), lower=True), solve_triangular(LB, np.eye(k), lower=True)
        t, order = np.concatenate([Xs.ravel(), Z.ravel()]), ref.merged_order(Xs, Z)
        u0, off, prior_x = np.sqrt(ref.JITTER) * eu[:, 0, :], 0, []
        for kp in kl:
            cp = ref.components(kp)
            pr = ref.prior_paths(kp, t, order, np.concatenate([ex[:, off:off + cp], ez[:, off:off + cp]], axis=2))
            prior_x.append(pr[:, :n])
            u0 = u0 + pr[:, n:]
            off += cp
        beta = W.T.dot(WB.T.dot((c.reshape(1, k) + eu[:, 1, :]).T) - W.dot(u0.T))
        for p, kp in enumerate(kl):
            b = prior_x[p] + orc.K(kp, Z, Xs).T.dot(beta).T
            bar = 1e-8 * max(np.abs(a[p]).max(), 1e-3)
            d = np.abs(a[p] - b).max()
            print("slot %d source %d: host routes differ by %.2e, a tenth of the bar is %.2e" % (i, p, d, 0.1 * bar))
            assert d <= 0.1 * bar, (i, p, d, bar)


def test_merged_order():
    from gpitch_amd import merged_order
    z = np.array([0.1, 0.3, 0.5])
    x = np.array([0.3, 0.0, 0.5, 0.2, 0.3])                  # unsorted, with ties among the frames and against Z
    o = merged_order(x, z)
    assert o.dtype == np.int32 and sorted(o.tolist()) == list(range(8))
    t = np.concatenate([x, z])
    assert np.all(np.diff(t[o]) >= 0)
    # stable: equal points keep the caller's order, frames before the inducing input they coincide with
    assert o.tolist() == [1, 5, 3, 0, 4, 6, 2, 7]
    assert np.array_equal(o, ref.merged_order(x, z))
    # a ragged slot: k = 2 of the 3 inducing points give an (n + k)-point problem
    o2 = merged_order(x, z[:2])
    assert sorted(o2.tolist()) == list(range(7)) and o2.tolist() == [1, 5, 3, 0, 4, 6, 2]
    # column vectors as the models hold them
    assert np.array_equal(merged_order(x.reshape(-1, 1), z.reshape(-1, 1)), o)


def _mixed():
    from gpitch_amd.kernels import Matern12
    from gpitch_amd.matern12_spectral_mixture import Matern12sm, MercerMatern12sm
    e20 = np.ones(20) / 20.
    return [MercerMatern12sm(1, energy=np.array([1.0]), frequency=np.array([220.]), variance=1.1, lengthscales=0.05),
            MercerMatern12sm(1, energy=e20, frequency=110. * np.arange(1, 21), variance=0.9, lengthscales=0.07),
            Matern12sm(1, energy=[0.7, 0.3], frequency=[277., 554.], variance=0.9, lengthscales=0.05),
            Matern12(1, variance=0.4, lengthscales=0.03)]


def test_eps_shapes_of_a_mixed_sum():
    from gpitch_amd import sample_components, sample_eps_shapes
    kl = _mixed()
    assert sample_components(kl) == [2, 40, 4, 1]
    assert sample_eps_shapes(kl, 131, 70, 9) == ((9, 47, 131), (9, 47, 70), (9, 2, 70))
    assert sample_eps_shapes(np.sum(kl), 5, 3) == ((1, 47, 5), (1, 47, 3), (1, 2, 3))       # an Add, one sample
    assert sample_eps_shapes(kl, 131, 70, 9) == ref.eps_shapes([k.oracle_dict() for k in kl[:3]] +
                                                               [{"type": "matern12"}], 131, 70, 9)


def test_unsupported_kernels_are_refused_by_name():
    from gpitch_amd import kernels as K
    from gpitch_amd import sample_components
    ok = _mixed()[0]
    k52 = K.Matern52(1, variance=2.5, lengthscales=0.01)
    bad = {"Matern32": K.Matern32(1), "Matern52": K.Matern52(1), "RBF": K.RBF(1), "Matern32sm": K.Matern32sm(1, 3),
           "Matern52 * MercerCosMix": K.Prod(k52, K.MercerCosMix(1, energy=np.array([1.]), frequency=np.array([100.]),
                                                                  variance=0.2))}
    for name, k in bad.items():
        with pytest.raises(NotImplementedError) as ei:
            sample_components([ok, k])
        msg = str(ei.value)
        assert name in msg and "kernel 1" in msg
        assert "MercerMatern12sm" in msg and "Matern12sm" in msg and "Matern12" in msg


def test_workspace_bytes_without_a_device():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    f = lib.gp_sgpr_sample_source_workspace_bytes
    base = (64, 3, 12, 2001, 16, 1)                          # M, P, C, n, S, count
    b0 = f(*base)
    # at least what the operator has to hold: prior_p(Z), u0, rhs, t1 and the Xnew feature tables
    assert b0 >= 8 * (3 * 64 * 16 + 3 * 64 * 16 + 12 * 2001)
    for pos in range(6):
        prev = b0
        for step in (1, 2, 5, 64):
            a = list(base)
            a[pos] += step
            cur = f(*a)
            assert cur >= prev, (pos, step)
            prev = cur
    assert f(64, 3, 12, 2001, 16, 256) >= 256 * (b0 - (1 << 16))
    assert f(0, 3, 12, 2001, 16, 1) == 0 and f(64, 3, 12, 0, 16, 1) == 0
