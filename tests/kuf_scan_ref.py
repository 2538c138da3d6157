"""numpy float64 restatement of gpitch_amd/csrc/kuf_scan.hip: the Kuf-side contraction
    g_theta = sum_ij Kbar_ij dK(z_i, x_j)/dtheta,   Kbar = [R, alpha] [A diag(2 gv) ; gm^T],   theta = (variance, lengthscale)
of a Matern-3/2 / Matern-5/2 kernel along ascending frames x, without forming Kbar away from the diagonal band:
chunk moments, prefix / suffix over chunks, far part per threshold, near part entry by entry.  Same steps, same chunk
assignment (threshold i belongs to the last chunk whose first frame is <= z_i), `Lc` a parameter."""
import numpy as np

_C = {"matern32": np.sqrt(3.0), "matern52": np.sqrt(5.0)}
_NQ = {"matern32": 3, "matern52": 4}


def shift(m, a):
    """T(a) m: moments [..., q] about a reference point a >= 0 further away; (T m)^p = e^-a sum_q C(p, q) a^(p-q) m^q"""
    out = np.empty_like(m)
    E = np.exp(-a)
    out[..., 0] = E * m[..., 0]
    out[..., 1] = E * (a * m[..., 0] + m[..., 1])
    out[..., 2] = E * (a * a * m[..., 0] + 2 * a * m[..., 1] + m[..., 2])
    if m.shape[-1] > 3:
        out[..., 3] = E * (a ** 3 * m[..., 0] + 3 * a * a * m[..., 1] + 3 * a * m[..., 2] + m[..., 3])
    return out


def frames_ascending(x):
    x = np.asarray(x).reshape(-1)
    return bool(np.all(x[1:] >= x[:-1]))


def entry_terms(ktype, var, ls, zi, xj):
    """dK/dvariance and dK/dlengthscale of single entries with the reference's r = sqrt(r2 + 1e-12), r2 expanded"""
    a, b = zi / ls, xj / ls
    r2 = -2.0 * a * b + a * a + b * b
    r = np.sqrt(r2 + 1e-12)
    if ktype == "matern32":
        e = np.exp(-_C[ktype] * r)
        phi, dphi = (1 + _C[ktype] * r) * e, -3.0 * r * e
    else:
        s5 = _C[ktype]
        e = np.exp(-s5 * r)
        phi, dphi = (1 + s5 * r + 5.0 / 3.0 * r * r) * e, -(5.0 / 3.0) * r * (1 + s5 * r) * e
    return phi, var * dphi * (-r2 / r / ls)


def kuf_scan(ktype, var, ls, z, x, R, alpha, A, gv, gm, Lc=64):
    """(g_variance, g_lengthscale); raises ValueError when x is not ascending"""
    z, x = np.asarray(z, float).reshape(-1), np.asarray(x, float).reshape(-1)
    if not frames_ascending(x):
        raise ValueError("frames not ascending")
    M, N = A.shape
    nq, kap = _NQ[ktype], _C[ktype] / ls
    At = np.vstack([A * (2.0 * gv)[None, :], gm[None, :]])          # (M + 1) x N
    Rt = np.hstack([R, alpha.reshape(-1, 1)])                       # M x (M + 1)
    C = (N + Lc - 1) // Lc
    s = np.array([x[c * Lc] for c in range(C)])
    e = np.array([x[min((c + 1) * Lc, N) - 1] for c in range(C)])
    # 1. chunk moments
    mom = np.zeros((C, 2, M + 1, nq))
    for c in range(C):
        xs = x[c * Lc:(c + 1) * Lc]
        for side, u in enumerate((kap * (e[c] - xs), kap * (xs - s[c]))):
            w = np.exp(-u)[None, :] * u[None, :] ** np.arange(nq)[:, None]       # nq x frames
            mom[c, side] = At[:, c * Lc:(c + 1) * Lc] @ w.T
    # 2. prefix (left) and suffix (right) over chunks, in place
    for c in range(1, C):
        mom[c, 0] += shift(mom[c - 1, 0], kap * (e[c] - e[c - 1]))
    for c in range(C - 2, -1, -1):
        mom[c, 1] += shift(mom[c + 1, 1], kap * (s[c + 1] - s[c]))
    # chunk of each threshold: the last chunk with s_c <= z_i, 0 if there is none
    ci = np.maximum(np.searchsorted(s, z, side="right") - 1, 0)
    S = np.zeros(nq)
    g_var = g_ls = 0.0
    for i in range(M):
        c = ci[i]
        # 3. far part
        if c >= 1:
            S += shift(Rt[i] @ mom[c - 1, 0], kap * (z[i] - e[c - 1]))
        if c + 1 < C:
            S += shift(Rt[i] @ mom[c + 1, 1], kap * (s[c + 1] - z[i]))
        # 4. near part: the chunk's own entries with the per-entry arithmetic
        sl = slice(c * Lc, (c + 1) * Lc)
        kb = Rt[i] @ At[:, sl]
        dv, dl = entry_terms(ktype, var, ls, z[i], x[sl])
        g_var += float(kb @ dv)
        g_ls += float(kb @ dl)
    # 5. output
    if ktype == "matern32":
        return g_var + S[0] + S[1], g_ls + var * S[2] / ls
    return g_var + S[0] + S[1] + S[2] / 3.0, g_ls + var * (S[2] + S[3]) / (3.0 * ls)
