"""numpy restatement of the Q route's backward far field (gpitch_amd/csrc/qbar.hip), shared by test_qbar_cpu.py and
test_gpu_qbar.py: Qbar = Kuf D Kuf^T and v = Kuf gm from the near rows of the stored strip and the two far tables of qfar_rule,
in the order the kernels take — per-group Gram blocks, three recurrences over the groups, one assembly per pair of 16-row tiles."""
import numpy as np

import qfar_rule as qf

GROUP, TILE = qf.GROUP, qf.TILE


def psi(z, x, var, ls, fx, rng):
    """[2 nf][N]: qfar_rule.tables' Psi without the T recurrence"""
    b, nf = np.asarray(x) / ls, fx.shape[0]
    out = np.zeros((2 * nf, len(b)))
    for S, (_, _, bmin, bmax) in enumerate(rng):
        cols = slice(S * GROUP, (S + 1) * GROUP)
        out[:nf, cols] = (var * np.exp(-(b[cols] - bmin)))[None, :] * fx[:, cols]
        out[nf:, cols] = (var * np.exp(-(bmax - b[cols])))[None, :] * fx[:, cols]
    return out


def is_monotone(rng):
    kb, ke = [r[0] for r in rng], [r[1] for r in rng]
    return all(kb[s] <= kb[s + 1] and ke[s] <= ke[s + 1] for s in range(len(rng) - 1))


def monotone(rng):
    """near ranges widened until kbeg and kend never decrease (qbar_plan_kernel): a near row is always exact, so widening is
    free; with ascending z and x the rule's own ranges already are monotone and this changes nothing — unless a 32-column strip
    spans 300 lengthscales (a gap in the frame times): its group is all near between narrower neighbours"""
    kb, ke = [r[0] for r in rng], [r[1] for r in rng]
    for s in range(len(rng) - 2, -1, -1):
        kb[s] = min(kb[s], kb[s + 1])
    for s in range(1, len(rng)):
        ke[s] = max(ke[s], ke[s - 1])
    return kb, ke


def tile_tables(kb, ke, M):
    """per 16-row tile: S0 = the first group it lies below, Sa = the first group it does not lie above (len(kb) where none)"""
    ng, nt = len(kb), M // TILE
    S0 = [next((s for s in range(ng) if kb[s] > TILE * t), ng) for t in range(nt)]
    Sa = [next((s for s in range(ng) if ke[s] > TILE * t), ng) for t in range(nt)]
    return S0, Sa


def qbar_far(K, d, gm, z, x, var, ls, fz, fx):
    """(Qbar, v, ranges): K the builder's strip, d the column scale (2 gv, any sign)"""
    a = np.asarray(z) / ls
    M, N, nf = K.shape[0], K.shape[1], fz.shape[0]
    rng = qf.ranges(z, x, ls)
    ng, nt = len(rng), M // TILE
    kb, ke = monotone(rng)
    bmin, bmax = np.array([r[2] for r in rng]), np.array([r[3] for r in rng])
    Psi = psi(z, x, var, ls, fx, rng)
    S0, Sa = tile_tables(kb, ke, M)
    # stage 1: per group, the Gram blocks that are stored (near x far, far x far) and the three vectors
    CnF, CFF = np.zeros((ng, M, 2 * nf)), np.zeros((ng, 2 * nf, 2 * nf))
    cn, cF = np.zeros((ng, M)), np.zeros((ng, 2 * nf))
    for S in range(ng):
        cols = slice(S * GROUP, (S + 1) * GROUP)
        Kn, Ps = K[kb[S]:ke[S], cols], Psi[:, cols]
        CnF[S, kb[S]:ke[S]] = (Kn * d[cols]) @ Ps.T
        CFF[S] = (Ps * d[cols]) @ Ps.T
        cn[S, kb[S]:ke[S]] = Kn @ gm[cols]
        cF[S] = Ps @ gm[cols]
    rows = lambda t: slice(TILE * t, TILE * (t + 1))
    # stage 2a: the recurrences.  Um[j] = e^{-(bmin_S0 - a_j)} R-(S0(j)) Phi(z_j), Vp[i] = e^{-(a_i - bmax_S1)} R+(S1(i)) Phi(z_i)
    Um, Vp, Wv = np.zeros((M, nf)), np.zeros((M, nf)), np.zeros((nt, M, nf))
    R = np.zeros((nf, nf))
    for S in range(ng - 1, -1, -1):
        R = CFF[S, :nf, :nf] + (np.exp(-2.0 * (bmin[S + 1] - bmin[S])) * R if S + 1 < ng else 0.0)
        for t in range(nt):
            if S0[t] == S:
                Um[rows(t)] = np.exp(-(bmin[S] - a[rows(t)]))[:, None] * (R @ fz[:, rows(t)]).T
    R = np.zeros((nf, nf))
    for S in range(ng):
        R = CFF[S, nf:, nf:] + (np.exp(-2.0 * (bmax[S] - bmax[S - 1])) * R if S > 0 else 0.0)
        for t in range(nt):
            if Sa[t] - 1 == S:
                Vp[rows(t)] = np.exp(-(a[rows(t)] - bmax[S]))[:, None] * (R @ fz[:, rows(t)]).T
    for ti in range(nt):                     # below x above: one running W per row tile, from the group where the tile goes below
        W = np.zeros((nf, nf))
        for S in range(S0[ti], ng):
            W = (np.exp(-(bmax[S] - bmax[S - 1])) * W if S > S0[ti] else 0.0) + np.exp(-(bmin[S] - bmin[S0[ti]])) * CFF[S, :nf, nf:]
            for tj in range(ti + 1, nt):
                if Sa[tj] - 1 == S:
                    Wv[ti, rows(tj)] = np.exp(-(a[rows(tj)] - bmax[S]))[:, None] * (W @ fz[:, rows(tj)]).T
    # stage 2b: one 16 x 16 tile of Qbar per pair ti <= tj, and its mirror
    Qb = np.zeros((M, M))
    for ti in range(nt):
        ri, fi = rows(ti), fz[:, rows(ti)]
        for tj in range(ti, nt):
            rj, fj = rows(tj), fz[:, rows(tj)]
            blk = np.zeros((TILE, TILE))
            lo, hi = Sa[tj], S0[ti]                                   # both near: the band of the stored strip
            if lo < hi:
                cols = slice(lo * GROUP, hi * GROUP)
                blk += (K[ri, cols] * d[cols]) @ K[rj, cols].T
            if Sa[ti] > 0:                                            # both above
                blk += (Vp[ri] @ fj) * np.exp(-(a[rj] - bmax[Sa[ti] - 1]))[None, :]
            if S0[tj] < ng:                                           # both below
                blk += np.exp(-(bmin[S0[tj]] - a[ri]))[:, None] * (fi.T @ Um[rj].T)
            if S0[ti] < Sa[tj]:                                       # i below, j above
                blk += np.exp(-(bmin[S0[ti]] - a[ri]))[:, None] * (fi.T @ Wv[ti, rj].T)
            lo, hi = Sa[ti], min(Sa[tj], S0[ti])                      # i near, j above
            if lo < hi:
                Y = sum(np.exp(-(bmax[hi - 1] - bmax[S])) * CnF[S, ri, nf:] for S in range(lo, hi))
                blk += (Y @ fj) * np.exp(-(a[rj] - bmax[hi - 1]))[None, :]
            lo, hi = max(S0[ti], Sa[tj]), S0[tj]                      # i below, j near
            if lo < hi:
                Y = sum(np.exp(-(bmin[S] - bmin[lo])) * CnF[S, rj, :nf] for S in range(lo, hi))
                blk += np.exp(-(bmin[lo] - a[ri]))[:, None] * (fi.T @ Y.T)
            if tj == ti:                                              # (the kernel evaluates element (min, max) for both)
                blk = np.triu(blk) + np.triu(blk, 1).T
            Qb[ri, rj] = blk
            Qb[rj, ri] = blk.T
    v = np.zeros(M)
    for t in range(nt):
        r = rows(t)
        for S in range(ng):
            if S < Sa[t]:
                v[r] += np.exp(-(a[r] - bmax[S])) * (fz[:, r].T @ cF[S, nf:])
            elif S < S0[t]:
                v[r] += cn[S, r]
            else:
                v[r] += np.exp(-(bmin[S] - a[r])) * (fz[:, r].T @ cF[S, :nf])
    return Qb, v, rng
