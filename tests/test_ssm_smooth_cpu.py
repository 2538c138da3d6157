"""The state-space smoother without a device: the numpy restatement (tests/ssm_smooth_ref.py) against the dense exact GP on
the idealised kernels at every shape the GPU tests use, its measured gap to the oracle's kernels (the reference's 1e-12 under
the square root), the properties of the map, the timeline builder and the scope checks of the Python layer."""
import numpy as np
import pytest
from scipy.linalg import cho_solve, cholesky

import ssm_smooth_ref as R
from oracle import gpflow05 as orc

IDS = [R.case_id(i) for i in range(len(R.CASES))]


# ---- (a) the restatement against the dense idealised GP: a tenth of the 1e-8 max(|ref|, 1e-3) the GPU is held to -------------
@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_restatement_matches_dense_idealised_gp(i):
    X, Y, Xn, kl, nz = R.case(i)
    assert sum(R.components(kl)) == R.CASES[i][0] and X.shape[0] == R.CASES[i][1]
    got, ref = R.smooth(X, Y, Xn, kl, nz), R.dense_ideal(X, Y, Xn, kl, nz)
    for name, g, r in zip(("mean", "variance", "log-likelihood"), got, ref):
        err, bar = np.abs(np.asarray(g) - np.asarray(r)).max(), 1e-9 * max(np.abs(r).max(), 1e-3)
        print("    %s: largest difference %.3e (bar %.3e)" % (name, err, bar))
        assert err <= bar, name


# ---- (b) the gap to the reference's kernels, measured per case ------------------------------------------------------------------
def _oracle(X, Y, Xn, kl, nz):
    om, ov = orc.sgpr_predict_source(Xn, X, Y, kl, nz)
    shift = sum(R.kdiag(k) for k in kl)                       # sgpr_ss.py:101 starts from the sum kernel's Kdiag
    om = np.array([a[:, 0] for a in om])
    ov = np.array([a[:, 0] - (shift - R.kdiag(k)) for a, k in zip(ov, kl)])
    N = X.shape[0]
    L = cholesky(orc.K_sum(kl, X) + nz * np.eye(N), lower=True)
    y = Y[:, 0]
    return om, ov, -0.5 * y.dot(cho_solve((L, True), y)) - np.log(np.diag(L)).sum() - 0.5 * N * np.log(2 * np.pi)


@pytest.mark.parametrize("i", range(len(R.CASES)), ids=IDS)
def test_gap_to_the_oracles_kernels(i):
    """deterministic, first order in the 1e-12 and growing with 1 / noise: the recorded figure (ssm_smooth_ref.ORACLE_GAP) is
    the measured one rounded up, and ten times it is the bar of the GPU comparison with predict_s"""
    X, Y, Xn, kl, nz = R.case(i)
    m, v, ll = R.smooth(X, Y, Xn, kl, nz)
    om, ov, oll = _oracle(X, Y, Xn, kl, nz)
    measured = (np.abs(m - om).max(), np.abs(v - ov).max(), abs(ll - oll) / abs(oll))
    print("    measured mean %.3e, variance %.3e, log-likelihood (relative) %.3e" % measured)
    for got, rec in zip(measured, R.ORACLE_GAP[IDS[i]]):
        assert rec / 10 <= got <= rec


# ---- (c) properties ----------------------------------------------------------------------------------------------------------------
def test_collapsed_bound_lies_below_the_exact_likelihood():
    X, Y, _, kl, nz = R.case(IDS.index("d60-N300-same-s0.01"))
    ll = R.smooth(X, Y, np.zeros(0), kl, nz)[2]
    for M in (5, 40, 150):
        Z = X[np.linspace(0, X.shape[0] - 1, M).round().astype(int)] + 0.3 / R.FS
        bound = float(orc.sgpr_bound(X, Y, Z, kl, nz))
        print("    M = %d: bound %.6f <= log-likelihood %.6f" % (M, bound, ll))
        assert bound <= ll


def test_source_means_add_up_to_the_mixture():
    X, Y, Xn, kl, nz = R.case(IDS.index("d63-N37-mixed-s0.3"))
    m = R.smooth(X, Y, Xn, kl, nz)[0]
    x, xs = X[:, 0], Xn[:, 0]
    Ks = sum(R.k_ideal(k, x, x) for k in kl)
    mix = sum(R.k_ideal(k, xs, x) for k in kl).dot(np.linalg.solve(Ks + nz * np.eye(x.size), Y[:, 0]))
    assert np.abs(m.sum(0) - mix).max() <= 1e-9 * max(np.abs(mix).max(), 1e-3)


def test_an_unobserved_step_changes_nothing_elsewhere():
    X, Y, Xn, kl, nz = R.case(IDS.index("d4-N37-mixed-s0.03"))
    extra = np.array([[X[3, 0] + 1e-5], [X[20, 0] + 2.5e-5], [X[-1, 0] + 1e-3]])
    a = R.smooth(X, Y, Xn, kl, nz)
    b = R.smooth(X, Y, np.vstack([extra[:2], Xn, extra[2:]]), kl, nz)
    assert np.abs(a[0] - b[0][:, 2:-1]).max() <= 1e-12 and np.abs(a[1] - b[1][:, 2:-1]).max() <= 1e-12
    assert abs(a[2] - b[2]) <= 1e-12 * abs(a[2])


# ---- (d) the timeline ----------------------------------------------------------------------------------------------------------------
def _both(X, Xn):
    from gpitch_amd.sgpr_ss import ssm_timeline
    a, b = ssm_timeline(X, Xn), R.timeline(X, Xn)
    assert a[0].dtype == a[1].dtype == np.int32
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] == a[0].size
    return a


def _times(X, Xn, order):
    t = np.concatenate([np.ravel(X), np.ravel(Xn)])
    return t[order]


def test_timeline():
    rng = np.random.RandomState(3)
    X = np.sort(rng.rand(40))
    order, ostep, steps = _both(X, X)                                     # Xnew = X: N steps
    assert steps == 40 and np.array_equal(order, np.arange(40)) and np.array_equal(ostep, np.arange(40))
    perm = rng.permutation(40)                                            # shuffled training frames and a shuffled Xnew
    order, ostep, steps = _both(X[perm], X[rng.permutation(40)])
    assert steps == 40 and np.array_equal(X[perm][order], X)
    Xn = np.array([0.5, X[7], 0.25, 0.5, -1.0, X[7], 2.0, -0.5, 0.25])     # repeats, on a frame, before and beyond
    order, ostep, steps = _both(X[perm], Xn)
    assert steps == 40 + 5 and sorted(order[order < 40]) == list(range(40))
    t = _times(X[perm], Xn, order)
    assert np.all(np.diff(t) >= 0) and np.array_equal(t[ostep], Xn)
    assert ostep[0] == ostep[3] and ostep[2] == ostep[8] and ostep[1] == ostep[5]    # duplicates share a step
    assert order[ostep[1]] < 40                                           # ... the training frame's
    assert ostep[4] == 0 and ostep[7] == 1 and ostep[6] == steps - 1      # before the first, after the last observation
    assert [o for o in order if o >= 40] == [40 + 4, 40 + 7, 40 + 2, 40 + 0, 40 + 6]   # the first of each distinct value
    Xd = X.copy()                                                         # duplicate training frames: two steps, D = 0
    Xd[11] = Xd[10]
    order, ostep, steps = _both(Xd, np.array([Xd[10], 0.3]))
    assert steps == 41 and list(order[10:12]) == [10, 11] and ostep[0] == 10
    order, ostep, steps = _both(X, np.zeros(0))                           # no new frame
    assert steps == 40 and ostep.size == 0
    order, ostep, steps = _both(np.array([0.0]), np.array([-0.0, 0.0]))   # equal, not bit-equal: its own step, after the frame
    assert steps == 2 and list(order) == [0, 1] and list(ostep) == [1, 0]


# ---- (e) scope: refused before any device work (there is no device here) -------------------------------------------------------
def _sum_model(kl, **kw):
    X, Y, _, _ = R.problem(30, 4, 2, 1)
    return R.model(X, Y, kl, 0.1, **kw)


def test_scope_checks_raise_without_a_device():
    from gpitch_amd import sgpr_ss
    from gpitch_amd.windows import fit_windows_batched
    m32 = {"type": "matern32", "variance": 1.0, "lengthscales": 0.01, "energy": [], "frequency": []}
    for call in (lambda m: m.predict_s_ssm(np.zeros(3)), lambda m: m.exact_log_likelihood()):
        with pytest.raises(NotImplementedError, match="kernel 1 of the sum is Matern32"):
            call(_sum_model(R.kernels(4) + [m32]))
        with pytest.raises(NotImplementedError, match="d = 130"):
            call(_sum_model(R.kernels(128) + R.kernels(2)))
        with pytest.raises(NotImplementedError, match="frame-sharded"):
            call(_sum_model(R.kernels(4), shard=(0, 2)))
    assert sgpr_ss.ssm_state_dim([(4, 10), (5, 3), (0, 0)]) == (27, 3)
    assert sgpr_ss.sample_components([(4, 2)]) == [4]     # (the sampler's own message is unchanged)
    with pytest.raises(NotImplementedError, match="sample_s_sparse: kernel 0 of the sum is Matern32; joint draws need"):
        sgpr_ss.sample_components([(1, 0)])
    with pytest.raises(ValueError, match='False, True, "sparse" or "ssm"'):
        fit_windows_batched(lambda h: None, [], predict="exact")


def test_workspace_dry_run_is_handle_free():
    from gpitch_amd import _lib
    lib = _lib.load_library()
    one = int(lib.gp_ssm_smooth_workspace_bytes(60, 2001, 3, 1))
    assert one % 256 == 0 and one >= 8 * 2001 * 60 * 60
    four = int(lib.gp_ssm_smooth_workspace_bytes(60, 2001, 3, 4))
    assert 3.9 * one < four < 4.1 * one
    assert lib.gp_ssm_smooth_workspace_bytes(129, 10, 1, 1) == 0 and lib.gp_ssm_smooth_workspace_bytes(4, 10, 5, 1) == 0
