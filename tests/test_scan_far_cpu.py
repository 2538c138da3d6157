"""The scan's far-field moments on the host: scan_far_rule.py's restatement of kuf_scan_far_moments_kernel
against long double, beside the dense-A form it replaces.  The moments are linear in A, so W enters once, as in A = W Kuf
itself: the reference takes the SAME float64 W and carries everything behind it in long double.  M = 128, N = 8192, Matern-3/2,
jitter 1e-6, lengthscales of 8 and 250 inducing spacings (cond(Kuu) ~ 1e8 at the latter), four layouts of the inducing inputs.
Asserted: the activation's variance and lengthscale gradients assembled from the new moments and near sums (through the
prefix and far launches' arithmetic) lie within 1e-9 of their scale of the dense contraction, the project's bar for two float64
forms.  Printed, not asserted: the moments' and near sums' own deviations and their ratio to the dense-A form's."""
import numpy as np
import pytest

import afar_rule as af
import scan_far_rule as sf

FS = 16000.0
M, N = 128, 8192
BAR = 1e-9
LD = np.longdouble


def _layout(name, spacings):
    x = np.arange(N) / FS
    unit = (N / float(M)) / FS
    if name == "grid":
        z = x[::N // M].copy()
    elif name == "off_grid":
        z = x[::N // M] + 1e-7
    elif name == "clustered":
        per = {0: 48, 1: 16, 7: 32, 8: 16, 31: 16}
        z = np.concatenate([(g * 256 + 0.37 + 5.3 * np.arange(k)) / FS for g, k in sorted(per.items())])
        unit = 5.3 / FS
    elif name == "frame_gap":       # (on the grid, as test_gpu_afar.py's case: the reference's a^2 - 2 a b + b^2 is exact at a == b only)
        z = x[::N // M].copy()
    ls = spacings * unit
    if name == "frame_gap":
        # two excerpts joined inside a group: test_gpu_afar.py's gap of 12.8 s (400 lengthscales at its 8 spacings), the same
        # seconds at either lengthscale.  The per-entry arithmetic both scan forms share takes r^2 = a^2 - 2 a b + b^2 from
        # a = z / l, b = x / l in float64, which is good to 2^-52 a^2: 4e-14 at |a| = 13, far below the 1e-12 under the root.
        # A gap that grew with the lengthscale (400 s at 250 spacings, |a| = 400, 4e-11) would test that arithmetic, not the
        # two forms: there the dense-A form itself is 6.7e-9 off the dense contraction and the new form 6.4e-9 (measured).
        n0 = 3 * 256 + 5 * 32 + 11
        t0, shift = x[n0], 400 * 8 * unit
        x = x.copy()
        x[n0:] += shift
        z[z >= t0] += shift
    return z, x, ls


def _setup(name, spacings):
    z, x, ls = _layout(name, spacings)
    var = 3.5
    rs = np.random.RandomState(7)
    Kuu = af.kuf(z, z, var, ls) + 1e-6 * np.eye(M)
    W = np.tril(np.linalg.inv(np.linalg.cholesky(Kuu)))
    Lq = np.tril(np.eye(M) + 0.05 * rs.randn(M, M))
    R, alpha = W.T @ (Lq @ Lq.T - np.eye(M)), W.T @ (0.3 * rs.randn(M))
    gv, gm = -rs.rand(N), rs.randn(N)
    rng = af.ranges(z, x)
    if name == "clustered":
        assert any(kb == ke for kb, ke, _, _ in rng)
    K = af.kuf(z, x, var, ls)
    Psi, T = af.psi(x, rng, var, ls), af.tables(W, z, rng, ls, lower=True)
    return dict(z=z, x=x, ls=ls, var=var, W=W, R=R, alpha=alpha, gv=gv, gm=gm, rng=rng, K=K, Psi=Psi, T=T)


@pytest.mark.parametrize("spacings", [8, 250])
@pytest.mark.parametrize("name", ["grid", "off_grid", "clustered", "frame_gap"])
def test_moments_and_near_sums_against_long_double(name, spacings):
    s = _setup(name, spacings)
    z, x, ls, var, W, R, alpha, gv, gm = (s[k] for k in ("z", "x", "ls", "var", "W", "R", "alpha", "gv", "gm"))
    # the reference: the same W, everything behind it in long double
    K_ld = af.kuf(z, x, var, ls, dtype=LD)
    A_ld = W.astype(LD) @ K_ld
    mom_ref = sf.moments_dense(A_ld, gv, gm, sf.weights(x, ls, LD))
    near_ref = sf.near_dense(A_ld, gv, gm, R, alpha, z, x, var, ls)
    d_ld = (z.astype(LD)[:, None] - x.astype(LD)[None, :]) / LD(ls)
    g_ref = [float(v) for v in sf.dense_contraction(A_ld, d_ld * d_ld, gv, gm, R, alpha, var, ls)]
    # the dense-A form in float64: the stored strip as afar.hip leaves it, one pass over it
    w = sf.weights(x, ls)
    A = af.product_far(W, s["K"], s["rng"], s["T"], s["Psi"], lower=True)
    mom_d, near_d = sf.moments_dense(A, gv, gm, w), sf.near_dense(A, gv, gm, R, alpha, z, x, var, ls)
    # the new form
    mom_f = sf.moments_far(W, s["K"], s["rng"], s["T"], s["Psi"], gv, gm, w)
    near_f = sf.near_far(W, s["K"], s["rng"], s["T"], s["Psi"], gv, gm, R, alpha, z, x, var, ls)
    tag = "%s, l = %d spacings" % (name, spacings)
    msc = float(np.abs(mom_ref).max())
    dev_f, dev_d = float(np.abs(mom_f - mom_ref).max()) / msc, float(np.abs(mom_d - mom_ref).max()) / msc
    print("%s moments: far-field form %.2e, dense-A form %.2e of their scale (ratio %.1f)" % (tag, dev_f, dev_d, dev_f / max(dev_d, 1e-300)))
    nsc = float(np.abs(near_ref).max())
    nf, nd = float(np.abs(near_f - near_ref).max()) / nsc, float(np.abs(near_d - near_ref).max()) / nsc
    print("%s near sums: far-field form %.2e, dense-A form %.2e of their scale (ratio %.1f)" % (tag, nf, nd, nf / max(nd, 1e-300)))
    g_f = sf.assemble(mom_f, near_f, R, alpha, z, x, var, ls)
    g_d = sf.assemble(mom_d, near_d, R, alpha, z, x, var, ls)
    for what, gf, gd, gr in zip(("variance", "lengthscale"), g_f, g_d, g_ref):
        ef, ed = abs(gf - gr) / abs(gr), abs(gd - gr) / abs(gr)
        print("%s d %s: far-field form %.2e, dense-A form %.2e of the dense contraction %.6e" % (tag, what, ef, ed, gr))
        assert ef <= BAR, (tag, what, ef)
