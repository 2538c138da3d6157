"""numpy restatement of the activations' H = A diag(2 gv) A^T and u = A gm from the stored A once and its factors once
(gpitch_amd/csrc/hfar.hip), in the kernels' order, beside the dense form it replaces and the two-sided form
DESIGN.md 3.09 dismissed.  Built on afar_rule.py and scan_far_rule.group_factors; shared by test_hfar_cpu.py and
test_gpu_hfar.py.

    A[:, S] = P_S B_S,   P_S = [T-_W(S), T+_W(S), W[:, near(S)]],   B_S = [Psi-; Psi+; Kuf[near(S), S]]     (afar_rule.py)
    one-sided:  H = sum_S Y_S P_S^T,   Y_S = A[:, S] diag(2 gv_S) B_S^T;   u = sum_S A[:, S] gm_S       (W enters once)
    two-sided:  H = sum_S P_S (B_S diag(2 gv_S) B_S^T) P_S^T                                            (W enters twice)
"""
import numpy as np

import afar_rule as af
import scan_far_rule as sf

TILE = af.TILE


def near_pairs(rng):
    """[(tile, group)] of every 16-row tile inside a group's near range"""
    return [(t, S) for S, r in enumerate(rng) for t in range(r[0] // TILE, r[1] // TILE)]


def slot_count(M, ng):
    """slots of the store of Y's near columns: pair (t, S) lives in slot t + S"""
    return M // TILE + ng - 1


def slots_collide(rng):
    """do two near pairs share a slot (hfar_check_kernel's count per slot)?"""
    seen = set()
    for t, S in near_pairs(rng):
        if t + S in seen:
            return True
        seen.add(t + S)
    return False


def y_group(A, K, rng, Psi, gv, gm, S, scale=2.0):
    """(Y_S [M][nr], A[:, S] gm_S [M]) as hfar_y_kernel sums them: the rows of B_S scaled by 2 gv once, gm unscaled as one more
    row, then 16 frames at a time, four k-steps each, a k-step adding frames 16 ch + 4 kq + s over kq"""
    sl = slice(S * af.GROUP, (S + 1) * af.GROUP)
    B = np.concatenate([Psi[:, sl], K[rng[S][0]:rng[S][1], sl]], axis=0)          # (scan_far_rule.group_factors' B_S)
    Bs = np.concatenate([B * (scale * gv[sl])[None, :], gm[sl][None, :]], axis=0)
    As = A[:, sl]
    acc = np.zeros((A.shape[0], Bs.shape[0]))
    for ch in range(af.GROUP // 16):
        for s in range(4):
            j = 16 * ch + 4 * np.arange(4) + s
            acc = acc + As[:, j] @ Bs[:, j].T
    return acc[:, :-1], acc[:, -1]


def slab_sum(slabs, alpha=1.0):
    """slab_reduce_kernel's order: four running sums over k = q, q + 4, .., the remainder into the first, ((0 + 1) + (2 + 3))"""
    s = [np.zeros_like(slabs[0]) for _ in range(4)]
    k = 0
    while k + 4 <= len(slabs):
        for q in range(4):
            s[q] = s[q] + slabs[k + q]
        k += 4
    while k < len(slabs):
        s[0] = s[0] + slabs[k]
        k += 1
    return ((s[0] + s[1]) + (s[2] + s[3])) * alpha


def h_one_sided(A, K, W, rng, T, Psi, gv, gm, nsplit=4):
    """(tril(H), u) by hfar.hip: Y_S per group, then per slab of groups the far step and the near tiles in order, W's entries
    above the diagonal zero; the slabs summed as the reduction sums them"""
    M, ng = A.shape[0], len(rng)
    Wl = np.tril(W)
    slabs, uparts = [], []
    for k in range(nsplit):
        acc, up = np.zeros((M, M)), np.zeros(M)
        for S in range(k * ng // nsplit, (k + 1) * ng // nsplit):
            Y, ugm = y_group(A, K, rng, Psi, gv, gm, S)
            acc = acc + Y[:, :4] @ T[S].T
            for t in range(rng[S][0] // TILE, rng[S][1] // TILE):
                Yt = Y[:, 4 + TILE * t - rng[S][0]:4 + TILE * (t + 1) - rng[S][0]]
                Wt = Wl[:, TILE * t:TILE * (t + 1)]
                for s in range(4):
                    acc = acc + Yt[:, s::4] @ Wt[:, s::4].T
            up = up + ugm
        slabs.append(acc)
        uparts.append(up)
    u = np.zeros(M)
    for up in uparts:
        u = u + up
    return np.tril(slab_sum(slabs)), u


def h_two_sided(K, W, rng, T, Psi, gv):
    """tril of sum_S P_S (B_S diag(2 gv_S) B_S^T) P_S^T: the form that carries W's rounding twice"""
    M = W.shape[0]
    H = np.zeros((M, M))
    for S in range(len(rng)):
        sl = slice(S * af.GROUP, (S + 1) * af.GROUP)
        P, B = sf.group_factors(W, K, rng, T, Psi, S)
        H = H + P @ ((B * (2.0 * gv[sl])[None, :]) @ B.T) @ P.T
    return np.tril(H)


def h_dense(A, gv, gm):
    """(tril(A diag(2 gv) A^T), A gm) in A's own precision"""
    dt = A.dtype
    return np.tril((A * (dt.type(2.0) * gv.astype(dt))[None, :]) @ A.T), A @ gm.astype(dt)
