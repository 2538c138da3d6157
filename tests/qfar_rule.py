"""numpy restatement of the Q route's far field (gpitch_amd/csrc/qfar.hip, gemm_wave.hip role 7), shared by
test_qfar_cpu.py and test_gpu_qfar.py: the strip builder's rule for which entries of Kuf are written in product form, the
range rule that follows from it, and G = Q Kuf by the near rows plus the two far tables."""
import numpy as np

GROUP = 256         # frames per column group: the wave product's workgroup (QFAR_GROUP)
STRIP = 32          # columns of one builder wavefront (CVM_SEP_COLS)
TILE = 16           # rows of one builder tile
SEP = 1.0           # CVM_SEP


def sm_mpad(m):
    return ((m + 3) // 4) * 4


def features(energy, freq, x):
    """[2 mpad][len(x)]: sqrt(e_q) cos(2 pi f_q x), then the sines; zero rows up to mpad (sm_features_kernel)"""
    m, mp = len(energy), sm_mpad(len(energy))
    out = np.zeros((2 * mp, len(x)))
    arg = (2.0 * np.pi * np.asarray(freq))[:, None] * np.asarray(x)[None, :]
    out[:m] = np.sqrt(energy)[:, None] * np.cos(arg)
    out[mp:mp + m] = np.sqrt(energy)[:, None] * np.sin(arg)
    return out


def _tiles(a):
    t = a.reshape(-1, TILE)
    return t.min(axis=1), t.max(axis=1)


def ranges(z, x, ls):
    """per 256-frame group: kbeg, kend (the near rows, whole 16-row tiles), bmin, bmax — the builder's predicate over the
    builder's wavefronts: a tile is far for the group when it is separable for every 32-column strip of it"""
    a, b = np.asarray(z) / ls, np.asarray(x) / ls
    M, N = len(a), len(b)
    assert M % TILE == 0 and N % GROUP == 0
    tlo, thi = _tiles(a)
    nt = M // TILE
    out = []
    for S in range(N // GROUP):
        bs = b[S * GROUP:(S + 1) * GROUP].reshape(-1, STRIP)
        ok = bool(np.all(bs.max(axis=1) - bs.min(axis=1) < 300.0))
        bmin, bmax = bs.min(), bs.max()
        below = ok & (bmin - thi >= SEP)
        above = ok & (tlo - bmax >= SEP)
        nb = 0
        while nb < nt and below[nb]:
            nb += 1
        na = 0
        while na < nt and above[nt - 1 - na]:
            na += 1
        out.append((TILE * nb, M - TILE * na, bmin, bmax))
    return out


def kuf_builder(z, x, var, ls, fz, fx):
    """Kuf as the Mercer strip builder writes it (cov.hip): var exp(-r) Phi(z)^T Phi(x) with r = sqrt(d^2 + 1e-12) of the expanded
    square, except on (16-row tile, 32-column strip) pairs at least a lengthscale apart, where the envelope is the product of a
    row factor and a column factor about the strip's nearer end"""
    a, b = np.asarray(z) / ls, np.asarray(x) / ls
    acc = fz.T @ fx
    r2 = ((-2.0 * (a[:, None] * b[None, :])) + (a * a)[:, None]) + (b * b)[None, :]
    K = var * np.exp(-np.sqrt(r2 + 1e-12)) * acc
    tlo, thi = _tiles(a)
    for w in range(len(b) // STRIP):
        cols = slice(w * STRIP, (w + 1) * STRIP)
        bw = b[cols]
        bmin, bmax = bw.min(), bw.max()
        if not (bmax - bmin < 300.0):
            continue
        for t in range(len(a) // TILE):
            rows = slice(t * TILE, (t + 1) * TILE)
            if tlo[t] - bmax >= SEP:
                env = np.exp(-(a[rows] - bmax))[:, None] * (var * np.exp(-(bmax - bw)))[None, :]
            elif bmin - thi[t] >= SEP:
                env = np.exp(-(bmin - a[rows]))[:, None] * (var * np.exp(-(bw - bmin)))[None, :]
            else:
                continue
            K[rows, cols] = env * acc[rows, cols]
    return K


def tables(Q, z, x, var, ls, fz, fx):
    """ranges, T [group][M][2 nf] by the recurrence over the groups, Psi [2 nf][N]"""
    a, b = np.asarray(z) / ls, np.asarray(x) / ls
    M, N, nf = len(a), len(b), fz.shape[0]
    rng = ranges(z, x, ls)
    ng = len(rng)
    T = np.zeros((ng, M, 2 * nf))
    Psi = np.zeros((2 * nf, N))
    for S, (_, _, bmin, bmax) in enumerate(rng):
        cols = slice(S * GROUP, (S + 1) * GROUP)
        Psi[:nf, cols] = (var * np.exp(-(b[cols] - bmin)))[None, :] * fx[:, cols]
        Psi[nf:, cols] = (var * np.exp(-(bmax - b[cols])))[None, :] * fx[:, cols]
    t, kprev, bprev = np.zeros((M, nf)), 0, 0.0
    for S in range(ng):                                    # rows below: upwards
        kb, bref = max(kprev, rng[S][0]), rng[S][2]
        if S > 0:
            t = t * np.exp(-(bref - bprev))
        for i in range(kprev, kb):
            t = t + Q[:, i:i + 1] * (np.exp(-(bref - a[i])) * fz[:, i])[None, :]
        T[S, :, :nf] = t
        kprev, bprev = kb, bref
    t, kprev = np.zeros((M, nf)), M
    for s, S in enumerate(range(ng - 1, -1, -1)):          # rows above: downwards
        ke, bref = min(kprev, rng[S][1]), rng[S][3]
        if s > 0:
            t = t * np.exp(-(bprev - bref))
        for i in range(ke, kprev):
            t = t + Q[:, i:i + 1] * (np.exp(-(a[i] - bref)) * fz[:, i])[None, :]
        T[S, :, nf:] = t
        kprev, bprev = ke, bref
    return rng, T, Psi


def g_far(Q, K, rng, T, Psi):
    """G = Q K group by group: the near rows of the stored strip, then the far sides that have rows"""
    M, nf = Q.shape[0], T.shape[2] // 2
    G = np.empty_like(K)
    for S, (kbeg, kend, _, _) in enumerate(rng):
        cols = slice(S * GROUP, (S + 1) * GROUP)
        g = Q[:, kbeg:kend] @ K[kbeg:kend, cols]
        f0, f1 = (0 if kbeg > 0 else nf), (2 * nf if kend < M else nf)
        if f1 > f0:
            g = g + T[S][:, f0:f1] @ Psi[f0:f1, cols]
        G[:, cols] = g
    return G


def g_dense(Q, K):
    """the dense product with the same calls per group (so that full near ranges reproduce it bit for bit)"""
    return np.concatenate([Q @ K[:, S * GROUP:(S + 1) * GROUP] for S in range(K.shape[1] // GROUP)], axis=1)


def sides(rng, M):
    """how many groups have far rows on both sides, on one, on neither"""
    both = sum(1 for kb, ke, _, _ in rng if kb > 0 and ke < M)
    none = sum(1 for kb, ke, _, _ in rng if kb == 0 and ke == M)
    return both, len(rng) - both - none, none
