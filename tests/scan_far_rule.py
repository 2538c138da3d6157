"""numpy restatement of the scan's first launch in its far-field form (kuf_scan_far_moments_kernel in
gpitch_amd/csrc/kuf_scan.hip), in the kernel's order, beside the dense-A form it replaces and the two launches behind it.
Shared by test_scan_far_cpu.py.  Matern-3/2 only.

    A[:, S] = P_S B_S,   P_S = [T-_W(S), T+_W(S), W[:, near(S)]],   B_S = [Psi-; Psi+; Kuf[near(S), S]]     (afar_rule.py)
    mom[c][s][q][k] = sum_r P_S[k, r] y[r][c][s][q],   y[r][c][s][q] = sum_{j in c} B_S[r, j] 2 gv_j w_sq(j)
    near: rho_i = R_i P_S,   Kuf_bar_ij = 2 gv_j (rho_i . B_S[:, j]) + alpha_i gm_j over the chunk of z_i
"""
import numpy as np

import afar_rule as af

LC = 64                       # frames per chunk (KS_LC)
GC = af.GROUP // LC           # chunks per group
NQ = 3


def weights(x, ls, dtype=np.float64):
    """[chunks][2 NQ][LC]: u^q e^-u about the chunk's last frame (side 0) and its first (side 1)"""
    x = np.asarray(x, dtype=dtype)
    C = x.shape[0] // LC
    kap = dtype(af.SQRT3) / dtype(ls)
    w = np.zeros((C, 2 * NQ, LC), dtype=dtype)
    for c in range(C):
        xs = x[c * LC:(c + 1) * LC]
        uL, uR = kap * (xs[-1] - xs), kap * (xs - xs[0])
        pL, pR = np.exp(-uL), np.exp(-uR)
        for q in range(NQ):
            w[c, q], w[c, NQ + q] = pL, pR
            pL, pR = pL * uL, pR * uR
    return w


def chunk_of(z, x):
    """the chunk whose thresholds z_i belongs to: the last chunk with s_c <= z_i, chunk 0 when there is none"""
    s = np.asarray(x)[::LC]
    return np.maximum(np.searchsorted(s, z, side="right") - 1, 0)


def moments_dense(A, gv, gm, w):
    """the pass over A: mom[chunks][2 NQ][M + 1] from At = [A diag(2 gv); gm] in A's own precision"""
    M, N = A.shape
    dt = A.dtype
    At = np.concatenate([A * (dt.type(2.0) * gv.astype(dt))[None, :], gm.astype(dt)[None, :]], axis=0)
    C = N // LC
    mom = np.zeros((C, 2 * NQ, M + 1), dtype=dt)
    for c in range(C):
        mom[c] = w[c].astype(dt) @ At[:, c * LC:(c + 1) * LC].T
    return mom


def _quarter_sums(v, wc):
    """sum_j v[..., j] wc[q][j] over 64 frames as the kernel adds them: four quarters of 16 in order, then (q0 + q1) + (q2 + q3)"""
    parts = []
    for qt in range(4):
        acc = np.zeros(v.shape[:-1] + (wc.shape[0],))
        for jj in range(16):
            j = qt * 16 + jj
            acc = acc + v[..., j:j + 1] * wc[:, j]
        parts.append(acc)
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


def group_factors(W, K, rng, T, Psi, S):
    """(P_S [M][nr], B_S [nr][256]) with the far columns first, as the kernel walks them; W's upper triangle counts as zero"""
    kb, ke = rng[S][0], rng[S][1]
    sl = slice(S * af.GROUP, (S + 1) * af.GROUP)
    P = np.concatenate([T[S], np.tril(W)[:, kb:ke]], axis=1)
    B = np.concatenate([Psi[:, sl], K[kb:ke, sl]], axis=0)
    return P, B


def moments_far(W, K, rng, T, Psi, gv, gm, w):
    """mom[chunks][2 NQ][M + 1] from the factors: phase 1 (y per row of B_S), phase 2 (rows of P_S in order)"""
    M, N = K.shape
    mom = np.zeros((N // LC, 2 * NQ, M + 1))
    for S in range(N // af.GROUP):
        P, B = group_factors(W, K, rng, T, Psi, S)
        for cw in range(GC):
            c = S * GC + cw
            js = slice(c * LC, (c + 1) * LC)
            bl = B[:, cw * LC:(cw + 1) * LC] * (2.0 * gv[js])[None, :]
            y = _quarter_sums(bl, w[c])                           # [nr][2 NQ]
            acc = np.zeros((M, 2 * NQ))
            for r in range(P.shape[1]):
                acc = acc + P[:, r:r + 1] * y[r][None, :]
            mom[c, :, :M] = acc.T
            mom[c, :, M] = _quarter_sums(gm[js][None, :], w[c])[0]
    return mom


def _entry_sums(wrow, zi, xs, var, ls):
    """the chunk's own entries with the reference's r = sqrt(d^2 / l^2 + 1e-12): (d variance, d lengthscale)"""
    a, b = zi / ls, xs / ls
    r2 = (-2.0 * (a * b) + a * a) + b * b
    r = np.sqrt(r2 + 1e-12)
    e = np.exp(-af.SQRT3 * r)
    phi, dphi = (1.0 + af.SQRT3 * r) * e, -3.0 * r * e
    return float(np.sum(wrow * phi)), float(np.sum((wrow * var * dphi) * (-r2 / r / ls)))


def near_far(W, K, rng, T, Psi, gv, gm, R, alpha, z, x, var, ls):
    """near[chunks][2] from the factors: rho_i over k in four interleaved quarters, then the chunk's entries"""
    N = x.shape[0]
    near = np.zeros((N // LC, 2))
    ci = chunk_of(z, x)
    for S in range(N // af.GROUP):
        idx = [i for i in range(z.shape[0]) if ci[i] // GC == S]
        if not idx:
            continue
        P, B = group_factors(W, K, rng, T, Psi, S)
        for i in idx:
            parts = [R[i, kq::4] @ P[kq::4, :] for kq in range(4)]
            rho = (parts[0] + parts[1]) + (parts[2] + parts[3])
            c = int(ci[i])
            cw = c - S * GC
            js = slice(c * LC, (c + 1) * LC)
            kb = np.zeros(LC)
            for r in range(P.shape[1]):
                kb = kb + rho[r] * B[r, cw * LC:(cw + 1) * LC]
            wrow = 2.0 * gv[js] * kb + alpha[i] * gm[js]
            dv, dl = _entry_sums(wrow, z[i], x[js], var, ls)
            near[c, 0] += dv
            near[c, 1] += dl
    return near


def near_dense(A, gv, gm, R, alpha, z, x, var, ls):
    """near[chunks][2] by the pass over A: Kuf_bar_ij = Rt_i . At[:, j] over the chunk of z_i"""
    N = x.shape[0]
    near = np.zeros((N // LC, 2))
    ci = chunk_of(z, x)
    for i in range(z.shape[0]):
        c = int(ci[i])
        js = slice(c * LC, (c + 1) * LC)
        wrow = R[i] @ (A[:, js] * (2.0 * gv[js])[None, :]) + alpha[i] * gm[js]
        dv, dl = _entry_sums(wrow, z[i], x[js], var, ls)
        near[c, 0] += dv
        near[c, 1] += dl
    return near


def _shift(m, a):
    """m <- T(a) m (ks_shift): the moments about a reference point a >= 0 further away"""
    E = np.exp(-a)
    return np.stack([E * m[0], E * (a * m[0] + m[1]), E * (a * (a * m[0] + 2.0 * m[1]) + m[2])])


def assemble(mom, near, R, alpha, z, x, var, ls):
    """kuf_scan_prefix_kernel and kuf_scan_far_kernel on the moments, plus the near sums: (d variance, d lengthscale)"""
    C = mom.shape[0]
    kap = af.SQRT3 / ls
    PL, PR = np.zeros((C, NQ, mom.shape[2])), np.zeros((C, NQ, mom.shape[2]))
    P = np.zeros((NQ, mom.shape[2]))
    for c in range(C):
        if c > 0:
            P = _shift(P, kap * (x[(c + 1) * LC - 1] - x[c * LC - 1]))
        P = P + mom[c, :NQ]
        PL[c] = P
    P = np.zeros((NQ, mom.shape[2]))
    for c in range(C - 1, -1, -1):
        if c < C - 1:
            P = _shift(P, kap * (x[(c + 1) * LC] - x[c * LC]))
        P = P + mom[c, NQ:]
        PR[c] = P
    Rt = np.concatenate([R, alpha[:, None]], axis=1)
    ci = chunk_of(z, x)
    gvar, glen = 0.0, 0.0
    for i in range(z.shape[0]):
        c = int(ci[i])
        Ssum = np.zeros(NQ)
        if c - 1 >= 0:
            Ssum = Ssum + _shift((PL[c - 1] @ Rt[i])[:, None], kap * (z[i] - x[c * LC - 1]))[:, 0]
        if c + 1 < C:
            Ssum = Ssum + _shift((PR[c + 1] @ Rt[i])[:, None], kap * (x[(c + 1) * LC] - z[i]))[:, 0]
        gvar += Ssum[0] + Ssum[1]
        glen += var * Ssum[2] / ls
    return gvar + float(near[:, 0].sum()), glen + float(near[:, 1].sum())


def dense_contraction(A, K_r2, gv, gm, R, alpha, var, ls):
    """sum_ij Kuf_bar_ij dK_ij / d(variance, lengthscale) entry by entry in A's precision; K_r2 = (z_i - x_j)^2 / l^2"""
    dt = A.dtype.type
    Kbar = R.astype(A.dtype) @ (A * (dt(2.0) * gv.astype(A.dtype))[None, :]) + np.outer(alpha.astype(A.dtype), gm.astype(A.dtype))
    r = np.sqrt(K_r2 + dt(1e-12))
    e = np.exp(-dt(af.SQRT3) * r)
    phi, dphi = (dt(1.0) + dt(af.SQRT3) * r) * e, dt(-3.0) * r * e
    return (Kbar * phi).sum(), (Kbar * dt(var) * dphi * (-K_r2 / r / dt(ls))).sum()
