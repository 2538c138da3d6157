"""Kernel learning from training audio (samplecov / kernelfit): the host-side rules, no device needed."""
import numpy as np
import pytest

from gpitch_amd import _lib


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_start_indices_follow_the_sequential_draws(seed):
    from gpitch_amd import samplecov
    n, size, num_sam = 32000, 441, 10000
    np.random.seed(seed)
    got = samplecov.draw_starts(n, num_sam, size)
    np.random.seed(seed)
    ref = np.array([np.random.randint(0, n - size) for _ in range(num_sam)])
    assert np.array_equal(got, ref)
    assert got.max() < n - size


def test_get_samples_are_the_segments_at_the_drawn_starts():
    from gpitch_amd import samplecov
    x = np.arange(1000, dtype=np.float64).reshape(-1, 1)
    np.random.seed(3)
    segs = samplecov.get_samples(x, 7, 20)
    np.random.seed(3)
    st = [np.random.randint(0, 980) for _ in range(7)]
    assert len(segs) == 7
    for s, i in zip(segs, st):
        assert s.shape == (20, 1)
        assert np.array_equal(s, x[i:i + 20])


def test_launch_split_keeps_y_below_two_gib():
    from gpitch_amd import samplecov
    lim = samplecov.MAX_Y_BYTES
    assert lim < 2 ** 31
    big = lim // 8 // 3                     # three fit in one launch, a fourth does not
    lengths = [big] * 7 + [1000, lim // 8]
    groups = samplecov.plan_launches(lengths, 10000, 441, ws_bytes=lambda B: 0)
    assert groups[0][0] == 0 and groups[-1][1] == len(lengths)
    for (a, b), (c, _) in zip(groups, groups[1:]):
        assert b == c
    for a, b in groups:
        assert 8 * sum(lengths[a:b]) <= lim
    assert groups == [(0, 3), (3, 6), (6, 8), (8, 9)]
    with pytest.raises(ValueError):
        samplecov.plan_launches([lim // 8 + 1], 10000, 441, ws_bytes=lambda B: 0)


def test_launch_split_bounds_the_workspace():
    from gpitch_amd import samplecov
    one = samplecov.gram_workspace_bytes(1, 10000, 441)
    assert one > 0
    assert samplecov.gram_workspace_bytes(4, 10000, 441) >= 4 * (one - 512)
    groups = samplecov.plan_launches([32000] * 10, 10000, 441, max_workspace_bytes=3 * one)
    assert all(samplecov.gram_workspace_bytes(b - a, 10000, 441) <= 3 * one for a, b in groups)
    assert sum(b - a for a, b in groups) == 10


class _FakeBatch(object):
    """stands in for the device evaluation: the numpy analytic form of k, f, g"""

    def __init__(self, xs, ys, ms, handle=None):
        self.xs = [np.asarray(x, dtype=np.float64).reshape(-1) for x in xs]
        self.ys = [np.asarray(y, dtype=np.float64).reshape(-1) for y in ys]
        self.ms = list(ms)
        self.h = None

    def __call__(self, ps, want_k=False):
        fs, gs, ks = [], [], []
        for x, y, m, p in zip(self.xs, self.ys, self.ms, ps):
            p = np.asarray(p, dtype=np.float64)
            k, f, g = _np_kernfit(p[:2 + 2 * m], x, y)
            gg = np.zeros(p.size)
            gg[:2 + 2 * m] = g
            fs.append(f)
            gs.append(gg)
            ks.append(k)
        return (np.array(fs), gs, ks) if want_k else (np.array(fs), gs)


def _np_kernfit(p, x, y):
    m = (p.size - 2) // 2
    r = np.abs(x)
    l, v, fr = p[1], p[2:2 + m], p[2 + m:2 + 2 * m]
    a = np.sqrt(3.) * r / np.abs(l)
    env = (1. + a) * np.exp(-a)
    cs = np.cos(2 * np.pi * np.abs(fr)[:, None] * r[None, :])
    sn = np.sin(2 * np.pi * np.abs(fr)[:, None] * r[None, :])
    S = np.abs(v) @ cs
    k = env * S
    e = k - y
    f = np.sqrt(np.mean(e ** 2))
    c = e / (x.size * f)
    g = np.zeros(p.size)
    g[1] = np.sign(l) * np.sum(c * S * a * a * np.exp(-a) / np.abs(l))
    g[2:2 + m] = np.sign(v) * ((cs * env) @ c)
    g[2 + m:] = np.sign(fr) * ((-(sn * env * 2 * np.pi * r) * np.abs(v)[:, None]) @ c)
    return k, f, g


def _note(fs=16000., n=8000, f0=261.6255653005986, seed=0):
    rng = np.random.RandomState(seed)
    t = np.arange(n) / fs
    y = sum(np.exp(-3 * t) * (0.7 ** h) * np.sin(2 * np.pi * f0 * (h + 1) * t + h) for h in range(5))
    return (y + 1e-3 * rng.randn(n)).reshape(-1, 1)


def test_fit_parameter_split_and_layout(monkeypatch):
    from gpitch_amd import kernelfit
    monkeypatch.setattr(kernelfit, "KernfitBatch", _FakeBatch)
    fs = 16000.
    audio = _note(fs)
    xk = np.linspace(0, 440. / fs, 441)
    kern = _np_kernfit(np.array([0., 0.02, 0.5, 0.3, 261.6, 523.3]), xk, np.zeros(441))[0].reshape(-1, 1)
    params, k_init, k_approx = kernelfit.fit(kern, audio, "x_M60_train.wav", max_par=4, fs=fs, handle=object())
    l, v, f = params
    assert np.ndim(l) == 0 and l > 0
    assert v.shape == f.shape and 1 <= v.size <= 4
    assert np.all(v >= 0) and np.all(f >= 0)
    assert k_init.shape == (441, 1) and k_approx.shape == (441, 1)
    # the split of a parameter vector of odd length: m = (len - 2) // 2, the trailing entry is unused
    assert kernelfit._npartials(np.zeros(7)) == 2


def test_learn_kernels_layout(monkeypatch):
    from gpitch_amd import kernelfit, samplecov
    monkeypatch.setattr(kernelfit, "KernfitBatch", _FakeBatch)

    def fake_cov_many(xs, num_sam, size, handle=None):
        covs, kerns = [], []
        for x in xs:
            s = np.asarray(x).reshape(-1)[:size]
            cov = np.outer(s, s) + np.eye(size)
            kern = cov[0].copy().reshape(-1, 1)
            kerns.append(kern / np.max(np.abs(kern)))
            covs.append(cov)
        return covs, kerns, [np.zeros(num_sam, dtype=int) for _ in xs]
    monkeypatch.setattr(samplecov, "get_cov_many", fake_cov_many)
    ys = [_note(seed=s) for s in range(3)]
    names = ["a_M60_.wav", "b_M62_.wav", "c_M64_.wav"]
    params, kern_sampled, covs = kernelfit.learn_kernels(ys, names, 16000, covsize=64, num_sam=10, max_par=3,
                                                         handle=object())
    assert len(params) == 3 and all(len(p) == 3 for p in params)
    xkern, skern = kern_sampled
    assert len(xkern) == 3 and len(skern) == 3 and len(covs) == 3
    assert xkern[0].shape == (64, 1) and skern[0].shape == (64, 1) and covs[0].shape == (64, 64)
    assert np.allclose(xkern[1][-1, 0], 63. / 16000)
    for v, f in zip(params[1], params[2]):
        assert v.shape == f.shape


def test_get_cov_raises_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from gpitch_amd import samplecov
    np.random.seed(0)
    with pytest.raises(_lib.GpitchError):
        samplecov.get_cov(np.random.randn(5000, 1), 100, 441)
    with pytest.raises(_lib.GpitchError):
        samplecov.autocorr(np.random.randn(5000, 1), 441)


def test_new_symbols_are_declared():
    lib = _lib.load_library()
    for name in ("gp_segment_gram_workspace_bytes", "gp_segment_gram", "gp_autocorr", "gp_kernfit_eval"):
        assert name in _lib.ABI_SYMBOLS
        assert hasattr(lib, name)
