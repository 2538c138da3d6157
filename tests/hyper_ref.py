"""Reference of the kernel-gradient contractions (bwd.hip: hyper_contract_kernel, hyper_m12sm_kernel, hyper_contract_sum_kernel,
hyper_sm_rows_kernel, hyper_sm_rows_lean_kernel, hyper_finish_items_kernel), stated once, in numpy.longdouble:

    sums[s] = sum_ij Gw_ij dK_ij/dtheta_s          theta = [variance, lengthscale, energy_0.., frequency_0..]
    gz[c][i] = sum_{j in column block c} Gw_ij dK_ij/dx1_i            (column blocks of 256)
    Gw = G + alpha gm^T;  G -> (G + G^T) / 2 when `symmetric` (then gz is the TOTAL derivative of sum_ij Gw_ij K(z_i, z_j) by z_i);
    G's columns scaled by 2 gscale[j] first where a column scale is given (the Q route).

The kernels, from the definitions (oracle/gpflow05.py K, the transcription of gpitch_amd/kernels.py and
matern12_spectral_mixture.py that the model tests differentiate):
  stationary   r = sqrt(d^2 / l^2 + 1e-12), d = x1 - x2:  K = var phi(r), phi = exp(-r) | (1 + s3 r) exp(-s3 r) |
               (1 + s5 r + 5/3 r^2) exp(-s5 r);  RBF: K = var exp(-d^2 / (2 l^2)), no nugget
  Mercer       K = var phi(r) S, S = sum_q e_q cos(p1_q - p2_q), p_q = fl(fl(2 pi f_q) x) — the float64 phase of the feature
               sqrt(e_q) [cos, sin](2 pi f_q x) as the definition forms it (left to right); phi Matern-1/2 or Matern-5/2
  broadcast    d = fl(fl(x1 - x2) + 1e-12), r = fl(sqrt(fl(d d))) (float64, as the definition), K = var E(r; l) sum_q e_q cos(fl(fl(2 pi f_q) r)),
               E = exp(-r / l) | (1 + r1) exp(-r1), r1 = sqrt(3) r / l
With dr/dl = -r2 / (l r), dr/dx1 = d / (l^2 r), r2 = d^2 / l^2:
  dK/dvar = phi S                 dK/dl = -var phi'(r) r2 / (l r) S           dK/de_q = var phi cos_q
  dK/df_q = -2 pi var phi e_q d sin_q            dK/dx1 = var phi' d / (l^2 r) S - var phi sum_q e_q w_q sin_q,  w_q = 2 pi f_q
  broadcast: dK/dl = var dE/dl S, dK/df_q = -2 pi var E e_q r sin_q, dK/dx1 = sign(d) (var dE/dr S - var E sum e_q w_q sin_q).
  Kuu side of a broadcast kernel: z_i is x1 of K_ij and x2 of K_ji (d_ji = z_j - z_i + 1e-12), so the total derivative is
  sum_j Gw_ij [sign(d_ij) K'(r_ij) - sign(d_ji) K'(r_ji)]: the two cancel on the diagonal, where d_ii = +1e-12 both ways.
Where the covariance strip `kvals` is an operand (the matrix-core forms) the variance and lengthscale sums are contractions OF
that strip: dK/dvar = kvals / var, dK/dl = kvals (-phi'/phi) r2 / (l r).  Float32 strips enter as their float32-rounded
values, converted exactly: their rounding is an input, not an error.
Finish: g_theta[s] += sum of the records (+ gv_sum dKdiag/dtheta_s: Kdiag = var, or var sum_q e_q for MercerMatern12sm and the
broadcast kernels; the Matern-5/2 product's Kdiag is var alone);  g_z[i] += sum over the column blocks.

THE BOUND.  u = 2^-53.  Beside each sum the reference returns its majorant
    A_s = sum_ij (|G_ij| + |alpha_i| |gm_j|) |dK_ij/dtheta_s|_termwise ,
the cosine sums taken as sum_q e_q (a feature product cos cos + sin sin rounds at the size of e_q, not of e_q |cos|), and a
conditioning sum C_s.  A device sum must lie within   (kappa u + eps_form) A_s + C_s.
  kappa = 64 + depth.  Per entry every path is a product of at most: the weight (fma: 1 rounding), var, phi (gp_exp_neg, 4.5 u
    measured below, times a polynomial of <= 4 roundings), r and rinv from gp_sqrt_rsqrt_pos (1.5 u and 3.5 u, measured below),
    <= 6 further multiplies, and per partial two feature products (sqrt(e): 1, sincos: 2 u, product: 1, each side; fma + mul:
    2) — under 40 u in all; 64 leaves room for the second-order terms.  depth = the longest chain of additions a term joins: rows per
    workgroup (8 or 32) + 6 shuffle steps + 2 for the generic kernels; col_seg / 4 (the columns one lane adds one after the
    other) + 4 + 6 + 2 for the matrix-core forms; the records are added here in long double.
  C_s: the expanded square r2 = -2 a b + a a + b b (a = x1 / l, b = x2 / l) carries absolute roundings <= 5 u (a^2 + b^2), the
    scaled inputs 2 u each and r itself 3 u, so r is off by  dr = u (3 (a^2 + b^2) / max(r, 1e-6) + 4 (|a| + |b|) + 3 r)  and
    C_s = sum_ij |Gw_ij| |d term_s / d r| dr  (the r-derivatives below, termwise absolute).  It is NOT small next to u A_s: at
    |x / l| = 50 and r = 0.01, dr / r = 1.5e-10.  The random cases keep |x / l| <= 50 (dr < 1.7e-12 / max(r, 1e-6)); the coinciding
    case (|x / l| ~ 100, r2 = 0 exactly by construction of the kernels' arithmetic, see bwd.hip) gets the same formula with its own a, b.
    RBF has no root: dr2 = u (5 (a^2 + b^2) + 8 sqrt(r2) (|a| + |b|)) on r2 itself.
    Broadcast kernels take r as the definition's float64 value: no conditioning term, except on the Kuu-side gz, where the
    kernel evaluates the mirrored entry at r_ij instead of r_ji = r_ij -+ 2e-12: |d^2K/dr^2| 2e-12 per entry.
  eps_form = 5e-13 for the two matrix-core forms: the separable envelope replaces sqrt((a - b)^2 + 1e-12) by |a - b| at r >= 1,
    a relative deviation of 1e-12 / (2 r^2) <= 5e-13 (the comment at HYR_SEP in bwd.hip); 0 elsewhere.
No figure here comes from a GPU run.  The device functions' accuracy (numpy ports below, against long double, on this CPU):
  gp_exp_neg          2.005 ulp = 4.01 u over [-744, 0]   (2e5 arguments; multiply-adds through a 64-bit significand, near-fused)
  gp_sqrt_rsqrt_pos   s 0.500 ulp = 1.0 u, rinv 1.480 ulp = 2.96 u over [1e-13, 1e4] (2e5 arguments) from a seed 2^-24 off
                      (an assumption about v_rsq_f64 on the safe side: two Goldschmidt steps square a seed error of 2^-24 away)
(tests/test_hyper_ref_cpu.py re-measures both and asserts them under the 4.5 u, 1.5 u and 3.5 u the count above uses.)
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
MATERN12, MATERN32, MATERN52, RBF, MERCER12, M12SM, M32SM, MERCER52 = range(8)
STATIONARY = (MATERN12, MATERN32, MATERN52, RBF)
MERCER = (MERCER12, MERCER52)
BROADCAST = (M12SM, M32SM)
EPS_FORM_ROWS = 5e-13
TWO_PI = 6.283185307179586          # the float64 the definition and the library multiply by
ORACLE_NAME = {MATERN12: "matern12", MATERN32: "matern32", MATERN52: "matern52", RBF: "rbf", MERCER12: "mercer_matern12sm",
               M12SM: "matern12sm", M32SM: "matern32sm", MERCER52: "mercer_matern52sm"}


def num_partials(ktype, theta):
    return 0 if ktype in STATIONARY else (len(theta) - 2) // 2


def kdiag_energy(ktype):
    return ktype in (MERCER12, M12SM, M32SM)


def _env(kind, r):
    """phi, phi', phi'' of the Matern envelopes at r (long double)"""
    if kind == 12:
        e = np.exp(-r)
        return e, -e, e
    if kind == 32:
        s = np.sqrt(LD(3))
        e = np.exp(-s * r)
        return (1 + s * r) * e, -3 * r * e, 3 * e * (s * r - 1)
    s = np.sqrt(LD(5))
    e = np.exp(-s * r)
    return (1 + s * r + LD(5) / 3 * r * r) * e, -LD(5) / 3 * r * (1 + s * r) * e, -LD(5) / 3 * e * (1 + s * r - 5 * r * r)


_ENV_OF = {MATERN12: 12, MATERN32: 32, MATERN52: 52, MERCER12: 12, MERCER52: 52}


def kernel_terms(ktype, theta, x1, x2, kuu=False, kvals=None):
    """Every entry's derivatives.  Returns dict: T [ns, n1, n2] (dK/dtheta_s), Ta (termwise absolute), Tr (|dT/dr| dr, the
    conditioning weight), Z / Za / Zr the same for dK/dx1 (the total derivative by z_i when kuu).  x1, x2: float64 vectors."""
    theta = np.asarray(theta, np.float64)
    m = num_partials(ktype, theta)
    ns = 2 + 2 * m
    var, ls = LD(theta[0]), LD(theta[1])
    en = theta[2:2 + m].astype(LD)
    fr = theta[2 + m:2 + 2 * m]
    x1 = np.asarray(x1, np.float64)
    x2 = np.asarray(x2, np.float64)
    n1, n2 = len(x1), len(x2)
    T = np.zeros((ns, n1, n2), LD)
    Ta = np.zeros((ns, n1, n2), LD)
    Tr = np.zeros((ns, n1, n2), LD)
    d = x1.astype(LD)[:, None] - x2.astype(LD)[None, :]
    a, b = np.abs(x1.astype(LD) / ls)[:, None], np.abs(x2.astype(LD) / ls)[None, :]
    if ktype in BROADCAST:
        d64 = (x1[:, None] - x2[None, :]) + 1e-12
        r64 = np.sqrt(d64 * d64)
        r = r64.astype(LD)
        sg = np.where(d64 < 0, LD(-1), LD(1))
        if ktype == M12SM:
            E = np.exp(-r / ls)
            Er, El, Err = -E / ls, E * r / (ls * ls), E / (ls * ls)
        else:
            s3 = np.sqrt(LD(3))
            r1 = s3 * r / ls
            e1 = np.exp(-r1)
            E, Er, El = (1 + r1) * e1, -r1 * e1 * s3 / ls, r1 * r1 * e1 / ls
            Err = -3 / (ls * ls) * e1 * (1 - r1)
        S = np.zeros((n1, n2), LD)
        Sw = np.zeros((n1, n2), LD)
        esum, ew, eww = LD(0), LD(0), LD(0)
        for q in range(m):
            om = np.float64(TWO_PI * fr[q])
            ph = (om * r64).astype(LD)
            c, s = np.cos(ph), np.sin(ph)
            S += en[q] * c
            Sw += en[q] * LD(om) * s
            T[2 + q] = var * E * c
            Ta[2 + q] = var * E
            T[2 + m + q] = -LD(TWO_PI) * var * E * en[q] * r * s
            Ta[2 + m + q] = LD(TWO_PI) * var * E * en[q] * r
            esum += en[q]
            ew += en[q] * LD(om)
            eww += en[q] * LD(om) ** 2
        T[0], Ta[0] = E * S, E * esum
        T[1], Ta[1] = var * El * S, var * np.abs(El) * esum
        Kp = var * Er * S - var * E * Sw                       # dK/dr
        Z = sg * Kp
        Za = var * np.abs(Er) * esum + var * E * ew
        Zr = np.zeros((n1, n2), LD)
        if kuu:
            # the mirrored entry K_ji: d_ji = z_j - z_i + 1e-12, derivative by its SECOND argument
            Zm = kernel_terms(ktype, theta, x2, x1)["Z"].T     # sign(d_ji) K'(r_ji), indexed [i, j]
            Z = Z - Zm
            Za = 2 * Za
            Zr = (var * np.abs(Err) * esum + 2 * var * np.abs(Er) * ew + var * E * eww) * LD(2e-12)
        return dict(T=T, Ta=Ta, Tr=Tr, Z=Z, Za=Za, Zr=Zr, m=m)
    r2 = (d / ls) ** 2
    if ktype == RBF:
        e = np.exp(-r2 / 2)
        dr2 = U * (5 * (a * a + b * b) + 8 * np.sqrt(r2) * (a + b))
        T[0], Ta[0], Tr[0] = e, e, e / 2 * dr2
        T[1] = var * e * r2 / ls
        Ta[1], Tr[1] = T[1], var / ls * np.abs(e * (1 - r2 / 2)) * dr2
        Z = -var * e * d / (ls * ls)
        return dict(T=T, Ta=Ta, Tr=Tr, Z=Z * (2 if kuu else 1), Za=np.abs(Z) * (2 if kuu else 1),
                    Zr=var * e * np.abs(d) / (2 * ls * ls) * dr2 * (2 if kuu else 1), m=m)
    r = np.sqrt(r2 + LD(1e-12))
    p, p1, p2 = _env(_ENV_OF[ktype], r)
    dr = U * (3 * (a * a + b * b) / np.maximum(r, LD(1e-6)) + 4 * (a + b) + 3 * r)
    drl = r2 / (ls * r)                                        # -dr/dl
    if ktype in STATIONARY:
        S, Sw, esum, ew = LD(1), LD(0), LD(1), LD(0)
    else:
        S = np.zeros((n1, n2), LD)
        Sw = np.zeros((n1, n2), LD)
        esum, ew = LD(0), LD(0)
        for q in range(m):
            om = np.float64(TWO_PI * fr[q])
            ph = (om * x1).astype(LD)[:, None] - (om * x2).astype(LD)[None, :]
            c, s = np.cos(ph), np.sin(ph)
            S += en[q] * c
            Sw += en[q] * LD(om) * s
            T[2 + q] = var * p * c
            Ta[2 + q] = var * p
            Tr[2 + q] = var * np.abs(p1) * dr
            T[2 + m + q] = -LD(TWO_PI) * var * p * en[q] * d * s
            Ta[2 + m + q] = LD(TWO_PI) * var * p * en[q] * np.abs(d)
            Tr[2 + m + q] = LD(TWO_PI) * var * np.abs(p1) * en[q] * np.abs(d) * dr
            esum += en[q]
            ew += en[q] * LD(om)
    if kvals is None:
        T[0], T[1] = p * S, -var * p1 * drl * S
    else:
        kv = np.asarray(kvals).astype(LD)
        T[0], T[1] = kv / var, kv * (-p1 / p) * drl
    Ta[0], Tr[0] = p * esum, np.abs(p1) * esum * dr
    Ta[1] = var * np.abs(p1) * drl * esum
    Tr[1] = var / ls * (np.abs(p2) * r + 2 * np.abs(p1)) * esum * dr
    Z = var * p1 * d / (ls * ls * r) * S - var * p * Sw
    Za = var * np.abs(p1) * np.abs(d) / (ls * ls * r) * esum + var * p * ew
    Zr = (var * (np.abs(p2) + np.abs(p1) / r) * np.abs(d) / (ls * ls * r) * esum + var * np.abs(p1) * ew) * dr
    f = 2 if kuu else 1
    return dict(T=T, Ta=Ta, Tr=Tr, Z=Z * f, Za=Za * f, Zr=Zr * f, m=m)


def weights(G, alpha, gm, symmetric, gscale=None):
    """Gw and its termwise majorant.  G: float64 or float32 array (n1, n2) — float32 converts exactly."""
    g = np.asarray(G).astype(LD)
    if gscale is not None:
        g = g * (2 * np.asarray(gscale, np.float64).astype(LD))[None, :]
    if symmetric:
        g = (g + g.T) / 2
    ga = np.abs(g)
    if alpha is not None:
        al, gg = np.asarray(alpha, np.float64).astype(LD), np.asarray(gm, np.float64).astype(LD)
        g = g + al[:, None] * gg[None, :]
        ga = ga + np.abs(al)[:, None] * np.abs(gg)[None, :]
    return g, ga


def contract_ref(ktype, theta, x1, x2, G, alpha=None, gm=None, symmetric=False, gscale=None, kvals=None, want_gz=False, terms=None):
    """sums / A / C [ns] and, when want_gz, gz / gzA / gzC [column blocks of 256][n1]"""
    t = terms if terms is not None else kernel_terms(ktype, theta, x1, x2, kuu=bool(symmetric), kvals=kvals)
    w, wa = weights(G, alpha, gm, symmetric, gscale)
    out = dict(sums=(t["T"] * w[None]).sum(axis=(1, 2)), A=(t["Ta"] * wa[None]).sum(axis=(1, 2)),
               C=(t["Tr"] * wa[None]).sum(axis=(1, 2)), m=t["m"])
    if want_gz:
        n2 = w.shape[1]
        blocks = [slice(c, min(c + 256, n2)) for c in range(0, n2, 256)]
        out["gz"] = np.stack([(t["Z"][:, s] * w[:, s]).sum(axis=1) for s in blocks])
        out["gzA"] = np.stack([(t["Za"][:, s] * wa[:, s]).sum(axis=1) for s in blocks])
        out["gzC"] = np.stack([(t["Zr"][:, s] * wa[:, s]).sum(axis=1) for s in blocks])
    return out


def kappa(form, wg_rows=32, col_seg=0):
    """roundings per entry + reduction depth (module docstring); form 0 generic / broadcast / sum kernel, 1 rows, 2 lean"""
    depth = (wg_rows + 8) if form == 0 else (col_seg // 4 + 12)
    return 64 + depth


def bound(A, C, form, wg_rows=32, col_seg=0):
    eps = EPS_FORM_ROWS if form in (1, 2) else 0.0
    return (kappa(form, wg_rows, col_seg) * U + LD(eps)) * A + C


def kvals_ref(ktype, theta, x1, x2):
    """the covariance strip itself, long double"""
    theta = np.asarray(theta, np.float64)
    return kernel_terms(ktype, theta, x1, x2)["T"][0] * LD(theta[0])


def finish_ref(ktype, theta, g0, p_uf, p_uu, gv_sum, z0=None, gz_uf=None, gz_uu=None):
    """g_theta and g_z after the finish, with majorants (for the bound: depth of the 256-strided sums + the tree)"""
    theta = np.asarray(theta, np.float64)
    m = num_partials(ktype, theta)
    ns = 2 + 2 * m
    parts = [np.asarray(p, np.float64).reshape(-1, ns).astype(LD) for p in (p_uf, p_uu) if p is not None and len(p)]
    s = sum((p.sum(axis=0) for p in parts), np.zeros(ns, LD))
    sa = sum((np.abs(p).sum(axis=0) for p in parts), np.zeros(ns, LD))
    if gv_sum is not None:
        gs = LD(gv_sum)
        kd = np.zeros(ns, LD)
        if kdiag_energy(ktype):
            kd[0] = theta[2:2 + m].astype(LD).sum()
            kd[2:2 + m] = LD(theta[0])
        else:
            kd[0] = 1
        s = s + gs * kd
        sa = sa + np.abs(gs * kd)
    g = np.asarray(g0, np.float64).astype(LD) + s
    ga = np.abs(np.asarray(g0, np.float64).astype(LD)) + sa
    out = dict(g=g, gA=ga)
    if z0 is not None:
        zs = [np.asarray(p, np.float64).astype(LD) for p in (gz_uf, gz_uu) if p is not None and len(p)]
        z = np.asarray(z0, np.float64).astype(LD) + sum((p.sum(axis=0) for p in zs), 0)
        za = np.abs(np.asarray(z0, np.float64).astype(LD)) + sum((np.abs(p).sum(axis=0) for p in zs), 0)
        out.update(z=z, zA=za)
    return out


def finish_bound(A, n_records):
    """a thread adds ceil(n / 256) records one after the other (twice: both sides), a tree of 8 levels, the Kdiag term and the
    accumulate: depth n / 256 + 12"""
    return (n_records // 256 + 14) * U * A


# ---- the kernel's order in plain float64 (tests/test_hyper_ref_cpu.py: the bound is not too tight) --------------------------
def replay64(ktype, theta, x1, x2, G, alpha=None, gm=None, symmetric=False, gscale=None, kvals=None, want_gz=False, rows_form=False):
    """float64 numpy evaluation in the kernels' arithmetic order: expanded square on the scaled inputs, feature products, and for
    the matrix-core forms the K / (var phi) identity; numpy's own exp / sqrt / pairwise sums stand in for the device's."""
    theta = np.asarray(theta, np.float64)
    m = num_partials(ktype, theta)
    ns = 2 + 2 * m
    var, ls = theta[0], theta[1]
    x1 = np.asarray(x1, np.float64)
    x2 = np.asarray(x2, np.float64)
    g = np.asarray(G).astype(np.float64)
    if gscale is not None:
        g = g * (2.0 * np.asarray(gscale, np.float64))[None, :]
    if symmetric:
        g = 0.5 * (g + g.T)
    w = g + (np.asarray(alpha)[:, None] * np.asarray(gm)[None, :] if alpha is not None else 0.0)
    sums = np.zeros(ns)
    d = x1[:, None] - x2[None, :]
    if ktype in BROADCAST:
        dd = d + 1e-12
        r = np.sqrt(dd * dd)
        sg = np.where(dd < 0, -1.0, 1.0)
        if symmetric:
            dji = (x2[None, :] - x1[:, None]) + 1e-12
            sg = 0.5 * (sg - np.where(dji < 0, -1.0, 1.0))
        if ktype == M12SM:
            E = np.exp(-(r / ls)); dEr = -E / ls; dEl = E * r / (ls * ls)
        else:
            s3 = 1.7320508075688772
            r1 = s3 * (r / ls); e1 = np.exp(-r1)
            E = (1.0 + r1) * e1; dEr = -r1 * e1 * s3 / ls; dEl = r1 * r1 * e1 / ls
        S = np.zeros_like(r); Sf = np.zeros_like(r)
        for q in range(m):
            om = TWO_PI * theta[2 + m + q]
            cs, sn = np.cos(om * r), np.sin(om * r)
            S += theta[2 + q] * cs
            Sf += theta[2 + q] * om * sn
            sums[2 + q] = (w * var * E * cs).sum()
            sums[2 + m + q] = -TWO_PI * (w * var * E * theta[2 + q] * r * sn).sum()
        sums[0] = (w * E * S).sum()
        sums[1] = (w * var * dEl * S).sum()
        z = sg * (w * var * dEr * S - w * var * E * Sf)
        f = 2.0 if symmetric else 1.0
    else:
        inv_ls = 1.0 / ls
        a = (x1 * inv_ls if rows_form else x1 / ls)[:, None]
        b = (x2 * inv_ls if rows_form else x2 / ls)[None, :]
        r2 = (-2.0 * (a * b) + a * a) + b * b
        if ktype == RBF:
            e = np.exp(-0.5 * r2)
            sums[0] = (w * e).sum()
            sums[1] = (w * (var * e * r2 * inv_ls)).sum()
            z = -w * var * e * d * (inv_ls * inv_ls)
        else:
            r = np.sqrt(r2 + 1e-12)
            rinv = 1.0 / r
            kind = _ENV_OF[ktype]
            if kind == 12:
                phi = np.exp(-r); dphi = -phi
            elif kind == 32:
                s3 = 1.7320508075688772; e = np.exp(-s3 * r)
                phi = (1.0 + s3 * r) * e; dphi = -3.0 * r * e
            else:
                s5 = 2.23606797749979; e = np.exp(-s5 * r)
                phi = (1.0 + s5 * r + (5.0 / 3.0) * r * r) * e; dphi = -(5.0 / 3.0) * r * (1.0 + s5 * r) * e
            if ktype in STATIONARY:
                sums[0] = (w * phi).sum()
                sums[1] = (w * var * dphi * (-r2 * rinv * inv_ls)).sum()
                z = w * var * dphi * d * (inv_ls * inv_ls) * rinv
            else:
                S = np.zeros_like(r); Ssin = np.zeros_like(r)
                for q in range(m):
                    om = TWO_PI * theta[2 + m + q]
                    se = np.sqrt(theta[2 + q])
                    zc, zs = (np.cos(om * x1) * se)[:, None], (np.sin(om * x1) * se)[:, None]
                    fc, fs = (np.cos(om * x2) * se)[None, :], (np.sin(om * x2) * se)[None, :]
                    cc = zc * fc + zs * fs
                    ss = zs * fc - zc * fs
                    S += cc
                    Ssin += ss * om
                    sums[2 + q] = (w * var * phi * cc).sum() / theta[2 + q]
                    sums[2 + m + q] = -TWO_PI * (w * var * phi * d * ss).sum()
                if rows_form:
                    kv = np.asarray(kvals).astype(np.float64)
                    wk = w * kv
                    sums[0] = wk.sum() / var
                    sums[1] = (wk * (-dphi / phi) * ((r2 * inv_ls) * rinv)).sum()
                else:
                    sums[0] = (w * phi * S).sum()
                    sums[1] = (-(w * var * dphi) * S * (r2 * rinv * inv_ls)).sum()
                z = w * var * dphi * S * d * (inv_ls * inv_ls) * rinv - w * var * phi * Ssin
        f = 2.0 if symmetric else 1.0
    out = dict(sums=sums)
    if want_gz:
        n2 = len(x2)
        out["gz"] = np.stack([f * z[:, c:c + 256].sum(axis=1) for c in range(0, n2, 256)])
    return out


# ---- numpy ports of the two device functions (common.h), for the measured accuracy figures ----------------------------------
def _fma(a, b, c):
    return (a.astype(LD) * b.astype(LD) + np.asarray(c).astype(LD)).astype(np.float64)     # (64-bit significand: near-fused)


def exp_neg_port(x):
    x = np.maximum(np.asarray(x, np.float64), -744.0)
    n = np.rint(x * 92.33248261689366)
    r = _fma(n, np.full_like(n, -float.fromhex("0x1.62e42fe000000p-7")), x)
    r = _fma(n, np.full_like(n, -float.fromhex("0x1.f473de6af278fp-36")), r)
    ni = n.astype(np.int64)
    p = _fma(r, np.full_like(r, 1.0 / 120.0), np.float64(1.0 / 24.0))
    p = _fma(p, r, np.float64(1.0 / 6.0))
    p = _fma(p, r, np.float64(0.5))
    p = _fma(p, r, np.float64(1.0))
    p = _fma(p, r, np.float64(1.0))
    tab = np.exp2(np.arange(64) / 64.0)
    return np.ldexp(tab[ni & 63] * p, (ni >> 6).astype(np.int32))


def sqrt_rsqrt_port(x, seed_rel=2.0 ** -24):
    x = np.asarray(x, np.float64)
    y = (1.0 / np.sqrt(x)) * (1.0 + seed_rel * np.cos(np.arange(x.size).reshape(x.shape)))
    g, h = x * y, 0.5 * y
    e = _fma(-h, g, np.float64(0.5))
    g, h = _fma(g, e, g), _fma(h, e, h)
    d = _fma(-g, g, x)
    g = _fma(d, h, g)
    r = h + h
    r = _fma(_fma(-g, r, np.float64(1.0)), r, r)
    return g, r
