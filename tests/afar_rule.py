"""numpy restatement of the activations' far field (gpitch_amd/csrc/afar.hip), shared by test_afar_cpu.py and
test_gpu_afar.py: the range rule (which 16-row tiles lie below or above a 256-frame group), the tables Psi and T in the
kernels' order, and X Kuf for a left factor X from the near rows plus the far field.  A Matern-3/2 Kuf is exactly
semiseparable along sorted inputs, so the far form carries no truncation: only rounding, and the constant KAPPA."""
import numpy as np

GROUP = 256                    # frames per column group (AFAR_GROUP)
TILE = 16                      # rows per tile
SQRT3 = 1.7320508075688772
KAPPA = 1.0 - 1.5e-12          # the reference's sqrt(d^2 / l^2 + 1e-12): K(r) = 1 - 3 r^2 / 2 + O(r^3) shifts a far entry by -1.5e-12 var e^{-c rho}


def kuf(z, x, var, ls, dtype=np.float64):
    """the reference's Matern-3/2 Kuf [M][N]: r = sqrt(d^2 / l^2 + 1e-12)"""
    z, x = np.asarray(z, dtype=dtype), np.asarray(x, dtype=dtype)
    d = (z[:, None] - x[None, :]) / dtype(ls)
    r = np.sqrt(d * d + dtype(1e-12))
    c = dtype(SQRT3)
    return dtype(var) * (dtype(1.0) + c * r) * np.exp(-c * r)


def ranges(z, x):
    """[(kbeg, kend, xmin, xmax)] per group: the near rows are the whole tiles that are neither in the leading run of tiles below
    the group (largest z < xmin) nor in the trailing run of tiles above it (smallest z > xmax)"""
    M, N = z.shape[0], x.shape[0]
    assert M % TILE == 0 and N % GROUP == 0
    nt = M // TILE
    tlo, thi = z.reshape(nt, TILE).min(axis=1), z.reshape(nt, TILE).max(axis=1)
    out = []
    for S in range(N // GROUP):
        xs = x[S * GROUP:(S + 1) * GROUP]
        xmin, xmax = float(xs.min()), float(xs.max())
        nb = 0
        while nb < nt and thi[nb] < xmin:
            nb += 1
        na = 0
        while na < nt and tlo[nt - 1 - na] > xmax:
            na += 1
        out.append((TILE * nb, M - TILE * na, xmin, xmax))
    return out


def psi(x, rng, var, ls, kappa=KAPPA):
    """[4][N]: Psi-[0], Psi-[1], Psi+[0], Psi+[1] (afar_cols_kernel)"""
    c = SQRT3 / ls
    out = np.zeros((4, x.shape[0]))
    for S, (_, _, xmin, xmax) in enumerate(rng):
        sl = slice(S * GROUP, (S + 1) * GROUP)
        bn, bp = c * (x[sl] - xmin), c * (xmax - x[sl])
        pn, pp = var * np.exp(-bn), var * np.exp(-bp)
        out[0, sl], out[1, sl], out[2, sl], out[3, sl] = pn * (kappa + bn), pn, pp * (kappa + bp), pp
    return out


def tables(X, z, rng, ls, lower=False):
    """T [groups][M][4]: (T-[0], T-[1], T+[0], T+[1]) of the left factor X by afar_t_kernel's recurrences — the reference point
    moves by a = c (ref' - ref) >= 0 as m0' = e^{-a} m0, m1' = e^{-a} (m1 + a m0), then the rows that became far enter one by
    one.  lower: X is lower triangular (entries above the diagonal count as zero)."""
    M, ng = z.shape[0], len(rng)
    c = SQRT3 / ls
    Xm = np.tril(X) if lower else X
    T = np.zeros((ng, M, 4))
    for side in (0, 1):
        m0, m1 = np.zeros(M), np.zeros(M)
        done, refprev = 0, 0.0
        for q in range(ng):
            S = ng - 1 - q if side else q
            far = M - rng[S][1] if side else rng[S][0]
            cnt = max(far, done)
            ref = rng[S][2 + side]
            if q > 0:
                a = c * (refprev - ref) if side else c * (ref - refprev)
                e = np.exp(-a)
                m1 = e * (a * m0 + m1)
                m0 = e * m0
            refprev = ref
            for r in range(done, cnt):
                i = M - 1 - r if side else r
                a = c * (z[i] - ref) if side else c * (ref - z[i])
                e = np.exp(-a)
                m0 = Xm[:, i] * e + m0
                m1 = Xm[:, i] * (e * a) + m1
            done = cnt
            T[S, :, 2 * side], T[S, :, 2 * side + 1] = m0, m1
    return T


def product_far(X, K, rng, T, Psi, lower=False):
    """X Kuf [M][N] from the near rows of the stored strip K plus the far field (afar_prod_kernel): the far terms first, then
    the near rows in order"""
    M, N = K.shape
    Xm = np.tril(X) if lower else X
    out = np.zeros((M, N))
    for S, (kb, ke, _, _) in enumerate(rng):
        sl = slice(S * GROUP, (S + 1) * GROUP)
        acc = T[S][:, 0:1] * Psi[0:1, sl]
        for f in (1, 2, 3):
            acc = acc + T[S][:, f:f + 1] * Psi[f:f + 1, sl]
        for k in range(kb, ke):
            acc = acc + Xm[:, k:k + 1] * K[k:k + 1, sl]
        out[:, sl] = acc
    return out


def is_monotone(rng):
    return all(rng[s + 1][0] >= rng[s][0] and rng[s + 1][1] >= rng[s][1] for s in range(len(rng) - 1))
