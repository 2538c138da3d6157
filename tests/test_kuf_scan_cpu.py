"""The algebra of gpitch_amd/csrc/kuf_scan.hip on the CPU: tests/kuf_scan_ref.py (chunk moments, prefix / suffix, far and
near part) against the dense sum  sum_ij Kbar_ij dK_ij/dtheta  with dK/dtheta by torch autograd through oracle.gpflow05.K."""
import numpy as np
import pytest

from kuf_scan_ref import frames_ascending, kuf_scan

# 1e-9 relative on each sum: two orders above what the restatement shows against the dense sum (2e-13 .. 2e-11, from the
# reference's own expanded square at scaled inputs up to 100), two below the GPU tests' bar for the same quantity.
RTOL = 1e-9


def _problem(N, M, ls, layout, seed):
    rng = np.random.RandomState(seed)
    # irregular ascending frames with repeated values
    x = np.cumsum(rng.uniform(0.2, 1.8, N)) / N
    rep = rng.choice(N - 1, N // 10, replace=False)
    x[rep + 1] = x[rep]
    x = np.sort(x)
    if layout == "mixed":
        z = np.empty(M)
        k = M // 6
        z[:k] = x[rng.choice(N, k, replace=False)]                     # on the grid / equal to a frame
        z[k:2 * k] = rng.uniform(x[0], x[-1], k)                        # off the grid
        z[2 * k:3 * k] = x[0] - rng.uniform(0.0, 3.0 * ls, k)           # below the first frame
        z[3 * k:4 * k] = x[-1] + rng.uniform(0.0, 3.0 * ls, k)          # above the last frame
        z[4 * k:5 * k] = z[k:2 * k]                                     # duplicated
        z[5 * k:] = rng.uniform(x[0], x[-1], M - 5 * k)
        z = rng.permutation(z)
    else:                                                               # every z inside one chunk
        j = N // 2
        z = rng.uniform(x[j + 3], x[j + 30], M)
    R = rng.randn(M, M)
    alpha = rng.randn(M)
    A = rng.randn(M, N)
    gv = rng.randn(N)
    gm = rng.randn(N)
    return dict(x=x, z=z, R=R, alpha=alpha, A=A, gv=gv, gm=gm, var=1.7, ls=ls)


def _dense(ktype, p):
    import torch
    from oracle import gpflow05 as orc
    from oracle.backend import TorchBackend
    v = torch.tensor(p["var"], dtype=torch.float64, requires_grad=True)
    l = torch.tensor(p["ls"], dtype=torch.float64, requires_grad=True)
    kern = {"type": ktype, "variance": v, "lengthscales": l, "energy": [], "frequency": []}
    K = orc.K(kern, torch.tensor(p["z"].reshape(-1, 1)), torch.tensor(p["x"].reshape(-1, 1)), TorchBackend())
    Kbar = p["R"] @ (p["A"] * (2.0 * p["gv"])[None, :]) + np.outer(p["alpha"], p["gm"])
    (K * torch.tensor(Kbar)).sum().backward()
    return float(v.grad), float(l.grad)


_dense_memo = {}


def _dense_once(ktype, N, M, ls, layout):
    key = (ktype, N, M, ls, layout)
    if key not in _dense_memo:
        p = _problem(N, M, ls, layout, seed=N + M)
        _dense_memo[key] = (p, _dense(ktype, p))
    return _dense_memo[key]


@pytest.mark.parametrize("Lc", [48, 64])
@pytest.mark.parametrize("N,M", [(300, 24), (1000, 40)])
@pytest.mark.parametrize("ls", [0.01, 0.2, 1.0])
@pytest.mark.parametrize("ktype", ["matern32", "matern52"])
def test_scan_matches_dense_contraction(ktype, ls, N, M, Lc):
    p, (rv, rl) = _dense_once(ktype, N, M, ls, "mixed")
    gv_, gl_ = kuf_scan(ktype, p["var"], p["ls"], p["z"], p["x"], p["R"], p["alpha"], p["A"], p["gv"], p["gm"], Lc=Lc)
    print("%s ls=%g N=%d M=%d Lc=%d: rel %.2e %.2e" % (ktype, ls, N, M, Lc, abs(gv_ - rv) / abs(rv), abs(gl_ - rl) / abs(rl)))
    assert abs(gv_ - rv) <= RTOL * abs(rv), (gv_, rv)
    assert abs(gl_ - rl) <= RTOL * abs(rl), (gl_, rl)


@pytest.mark.parametrize("Lc", [48, 64])
@pytest.mark.parametrize("ktype", ["matern32", "matern52"])
def test_all_thresholds_inside_one_chunk(ktype, Lc):
    p, (rv, rl) = _dense_once(ktype, 300, 24, 0.2, "one_chunk")
    gv_, gl_ = kuf_scan(ktype, p["var"], p["ls"], p["z"], p["x"], p["R"], p["alpha"], p["A"], p["gv"], p["gm"], Lc=Lc)
    assert abs(gv_ - rv) <= RTOL * abs(rv), (gv_, rv)
    assert abs(gl_ - rl) <= RTOL * abs(rl), (gl_, rl)


def test_descending_frames_are_detected():
    p = _problem(300, 24, 0.2, "mixed", seed=1)
    assert frames_ascending(p["x"])
    x = p["x"].copy()
    x[100], x[180] = x[180], x[100]
    assert not frames_ascending(x)
    with pytest.raises(ValueError):
        kuf_scan("matern32", p["var"], p["ls"], p["z"], x, p["R"], p["alpha"], p["A"], p["gv"], p["gm"])
