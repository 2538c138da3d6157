"""Host reference of the GEMM host entries that gp_debug_gemm reaches (gemm*.hip), in plain numpy.

One function, `gemm_ref`, takes one problem's HOST buffers and the launch's flags and states the contracts once:

  op(A), op(B)   A is stored K x M when transA (else M x K), B is stored N x K when transB (else K x N).  triA / triB name
                 the structure of op(A) (M x K) / op(B) (K x N): lower keeps k <= i (n <= k), upper keeps k >= i (n >= k);
                 the other triangle is taken as ZERO WHATEVER THE BUFFER HOLDS.
  roles          role 1: op(A) = A lower triangular (A = W Kuf); role 2: op(A) = A^T upper triangular, i.e. A stored
                 lower (Lq^T A); role 3: dense A, columns of B scaled by v1[n] (Kuf_bar).  They fix transA / triA /
                 scale_mode whatever the flags say.
  scale_mode     1: op(B)(k, n) *= v1[n];  2: op(B)(k, n) *= v1[k]
  alpha, beta    C = alpha op(A) op(B) + beta C  (EPI_STORE); without EPI_STORE C is not touched
  triC lower     entries above the diagonal read 0 inside every B x B output tile that touches the diagonal band (tile
                 column <= tile row); tiles wholly above are not written at all.  For the split-K kinds triC lower means
                 `sym`: the lower triangle is computed and MIRRORED.
  epilogues      EPI_COLSUMSQ: o0[blk][n] = sum over the block's rows of (alpha acc)^2; EPI_COLDOT: o1[blk][n] = sum of
                 alpha acc * v0[row] — of alpha acc, never of the stored value (beta does not enter).
  row ranges     (tile_m0, tile_mcount), in row blocks of 128: rows outside [128 m0, 128 (m0 + mcount)) are left untouched
                 (mcount = 0, or a range that passes the end: to the last row; m0 past the end: nothing at all).
  split-K        H = alpha (X diag(d)) Y^T with X = A, Y = B (both M x Nlong), d = v1 when scale_mode == 2; with v2 given,
                 u = X v2 (NOT scaled): o1[slice][i] partials that sum to u, o0 = u, xa += u.
  float32 kinds  kind 2: A float64 in memory and ROUNDED TO FLOAT32 ONCE, B / C float32; kind 3: A, B float32, H float64.

Exact mode (`exact=True`): the inputs are small integers; products are formed in int64 and everything after (alpha, squares,
column sums) in numpy.longdouble (64-bit significand), so the result is exact, and `peak` reports the largest intermediate
(accumulator, alpha acc, its square, a column sum, beta C) — the caller asserts it below 2^53 (float64) or, for what the float32
kernels hold in float32 (operands, scaled operand, accumulator, alpha acc, the stored C: `peak32`), below 2^24.  Then every
partial sum of ANY summation order is an integer below the significand and the device must agree bit for bit.

Real-valued mode: everything in numpy.longdouble, and `bound` fields give the entrywise error bounds, DERIVED, not measured.
With u = 2^-53 (float64 kinds) or 2^-24 (float32 kinds), P = |alpha| |op A| |op B (scaled)| entrywise:

  C:     |C_dev - C_ref| <= (K + c) u P + |beta C0| u,   c = 4 (float64), 6 (float32: operand rounding and the stored result).
         (A K-term dot product in any order, fused or not, errs by at most K u sum|a b| to first order; scale, alpha, beta
         and the final store add one rounding each.)
  sums:  with e_ij = (K + c) u P_ij the error of one entry c_ij = alpha acc_ij (stored-value rounding included for float32),
           o0_j = sum_i c_ij^2:     |c^2 - c_ref^2| <= 2 |c_ij| e_ij  to first order, and the float64 sum of R squares (each an
                                    fma) adds at most (R + 2) 2^-53 sum_i c_ij^2:
                                    bound0_j = sum_i 2 |c_ij| e_ij + (R + 2) 2^-53 sum_i c_ij^2
           o1_j = sum_i c_ij v0_i:  bound1_j = sum_i |v0_i| e_ij + (R + 2) 2^-53 sum_i |c_ij v0_i|
         (R = rows of the block; the sums themselves are float64 in every kind, hence 2^-53 there.)
  u = X v2:  (K + 4) 2^-53 |X| |v2|  (float64 fma chain over K, plus the sum over slices).
"""
import numpy as np

EPI_STORE, EPI_COLSUMSQ, EPI_COLDOT = 1, 2, 4
TRI_NONE, TRI_LOWER, TRI_UPPER = 0, 1, 2
LD = np.longdouble

FLAG_DEFAULTS = dict(transA=0, transB=0, triA=0, triB=0, triC=0, big_tiles=0, epilogue=1, scale_mode=0, role=0, tile_m0=0,
                     tile_mcount=0, uniform_aligned=0, a32_ok=0, rows64_ok=0, alpha=1.0, beta=0.0)


def flags_of(**kw):
    f = dict(FLAG_DEFAULTS)
    for k in kw:
        assert k in f, k
    f.update(kw)
    return f


def effective_flags(f):
    """the structure a role fixes at compile time, whatever the run-time flags say"""
    f = dict(f)
    if f["role"] == 1:
        f.update(transA=0, transB=0, triA=TRI_LOWER, triB=TRI_NONE, scale_mode=0)
    elif f["role"] == 2:
        f.update(transA=1, transB=0, triA=TRI_UPPER, triB=TRI_NONE, scale_mode=0)
    elif f["role"] == 3:
        f.update(transA=0, transB=0, triA=TRI_NONE, triB=TRI_NONE, scale_mode=1)
    return f


def row_range(M, bm, m0, mcount):
    """rows [r0, r1) a launch with that row-block range writes (blocks of bm rows)"""
    allb = -(-M // bm)
    if m0 == 0 and mcount == 0:
        return 0, M
    if m0 >= allb:
        return 0, 0
    nb = mcount if (mcount > 0 and m0 + mcount < allb) else allb - m0
    return m0 * bm, min(M, (m0 + nb) * bm)


def partial_rows_rule(M, wave, big):
    """rows of o0 / o1: one per 64-row tile in the wave form, else one per row block of 64 (small tiles) or 128"""
    return M // 64 if wave else -(-M // (128 if big else 64))


def _masked_ops(A, B, f, K, M, N, v1, dt):
    opA = np.asarray(A).T if f["transA"] else np.asarray(A)
    opB = np.asarray(B).T if f["transB"] else np.asarray(B)
    opA, opB = opA[:M, :K], opB[:K, :N]
    i, k = np.arange(M)[:, None], np.arange(K)[None, :]
    if f["triA"] == TRI_LOWER:
        opA = np.where(k > i, 0, opA)
    elif f["triA"] == TRI_UPPER:
        opA = np.where(k < i, 0, opA)
    kk, n = np.arange(K)[:, None], np.arange(N)[None, :]
    if f["triB"] == TRI_LOWER:
        opB = np.where(n > kk, 0, opB)
    elif f["triB"] == TRI_UPPER:
        opB = np.where(kk > n, 0, opB)
    opA, opB = opA.astype(dt), opB.astype(dt)      # (masked first: the other triangle may hold anything)
    if f["scale_mode"] == 1:
        opB = opB * np.asarray(v1)[:N].astype(dt)[None, :]
    elif f["scale_mode"] == 2:
        opB = opB * np.asarray(v1)[:K].astype(dt)[:, None]
    return opA, opB


def _absprod(a, b):
    """|a| |b| for the bounds: float64 (BLAS) and inflated by 1e-9, which covers its own rounding (K 2^-53 relative, all terms
    non-negative); exact for the integer inputs, whose sums stay below 2^53"""
    p = np.abs(np.asarray(a, dtype=np.float64)) @ np.abs(np.asarray(b, dtype=np.float64))
    if np.asarray(a).dtype == np.int64:
        return p.astype(LD)
    return p.astype(LD) * (1 + LD(1e-9))


def _amax(*xs):
    m = 0.0
    for x in xs:
        x = np.asarray(x)
        if x.size:
            m = max(m, float(np.max(np.abs(x.astype(LD)))))
    return m


def gemm_ref(kind, flags, M, N, K, A, B, C0=None, v0=None, v1=None, v2=None, xa0=None, exact=False, block_rows=128, tile=128):
    """One problem.  kind 0 / 2: returns dict(C, written (bool M x N), o0, o1 ([blocks][N], NaN rows unwritten), peak, peak32,
    P, bound_C, bound_o0, bound_o1).  kind 1 / 3: dict(C = H, u, xa, P, bound_C, bound_u, peak, peak32).
    block_rows: rows per partial row (64: wave form or small tiles; 128); tile: output tile edge (triC's zeroing)."""
    f32 = kind in (2, 3)
    f = effective_flags(flags) if kind in (0, 2) else dict(flags)
    dt = np.int64 if exact else LD
    u_round = LD(2.0) ** (-24 if f32 else -53)
    c_extra = 6 if f32 else 4
    alpha, beta = LD(f["alpha"]), LD(f["beta"])
    if kind == 2 and not exact:
        A = np.asarray(A, dtype=np.float64).astype(np.float32)        # the M x M operand, rounded once
    if kind in (1, 3):
        g = dict(FLAG_DEFAULTS, transA=0, transB=1, scale_mode=2 if f["scale_mode"] == 2 else 0)
        X, Yt = _masked_ops(A, B, g, K, M, M, v1, dt)
        acc = X @ Yt
        P = np.abs(alpha) * _absprod(X, Yt)
        H = alpha * acc.astype(LD)
        if f["triC"] == TRI_LOWER:
            H = np.tril(H) + np.tril(H, -1).T
            P = np.tril(P) + np.tril(P, -1).T
        out = dict(C=H, P=P, bound_C=(K + c_extra) * u_round * P, peak=_amax(acc, H), peak32=_amax(X, Yt, acc), u=None)
        if v2 is not None:
            Xr = np.asarray(A)[:M, :K].astype(dt)
            g2 = np.asarray(v2)[:K].astype(dt)
            uu = (Xr @ g2).astype(LD)
            out["u"] = uu
            out["xa"] = uu + (np.asarray(xa0).astype(LD) if xa0 is not None else 0)
            out["bound_u"] = (K + 4) * LD(2.0) ** -53 * (np.abs(Xr).astype(LD) @ np.abs(g2).astype(LD))
            out["peak"] = max(out["peak"], _amax(uu, out["xa"]))
        return out

    assert not (f["triC"] and (f["epilogue"] & (EPI_COLSUMSQ | EPI_COLDOT))), "triC with column sums: no contract (skipped tiles write none)"
    opA, opB = _masked_ops(A, B, f, K, M, N, v1, dt)
    acc = opA @ opB
    P = np.abs(alpha) * _absprod(opA, opB)
    c = alpha * acc.astype(LD)                        # alpha acc: what the column sums see
    C0 = np.zeros((M, N), LD) if C0 is None else np.asarray(C0)[:M, :N].astype(LD)
    bm = 128 if (f["role"] >= 1 or f["big_tiles"] or f32) else 64
    r0, r1 = row_range(M, bm, f["tile_m0"], f["tile_mcount"])
    rows = np.zeros(M, bool)
    rows[r0:r1] = True
    Cn = c + beta * C0
    written = np.zeros((M, N), bool)
    if f["epilogue"] & EPI_STORE:
        written[rows, :] = True
        if f["triC"] == TRI_LOWER:
            i, j = np.arange(M)[:, None], np.arange(N)[None, :]
            Cn = np.where(j > i, LD(0), Cn)
            written &= (j // tile) <= (i // tile)
    Cout = np.where(written, Cn, C0)
    e = (K + c_extra) * u_round * P
    nblk = -(-M // block_rows)
    o0 = np.full((nblk, N), np.nan, LD)
    o1 = np.full((nblk, N), np.nan, LD)
    b0 = np.zeros((nblk, N), LD)
    b1 = np.zeros((nblk, N), LD)
    peak_sum = 0.0
    v0l = None if v0 is None else np.asarray(v0)[:M].astype(LD)
    for b in range(nblk):
        s, t = b * block_rows, min(M, (b + 1) * block_rows)
        if not rows[s:t].any():
            continue
        assert rows[s:t].all()                        # ranges are whole 128-row blocks, partial rows 64 or 128 rows
        cb, eb, R = c[s:t], e[s:t], t - s
        u53 = LD(2.0) ** -53
        if f["epilogue"] & EPI_COLSUMSQ:
            o0[b] = np.sum(cb * cb, axis=0)
            b0[b] = np.sum(2 * np.abs(cb) * eb, axis=0) + (R + 2) * u53 * o0[b]
            peak_sum = max(peak_sum, _amax(cb * cb, o0[b]))
        if f["epilogue"] & EPI_COLDOT:
            o1[b] = np.sum(cb * v0l[s:t, None], axis=0)
            absd = np.sum(np.abs(cb * v0l[s:t, None]), axis=0)
            b1[b] = np.sum(np.abs(v0l[s:t, None]) * eb, axis=0) + (R + 2) * u53 * absd
            peak_sum = max(peak_sum, _amax(absd))
    return dict(C=Cout, written=written, o0=o0, o1=o1, P=P, bound_C=e + np.abs(beta * C0) * u_round, bound_o0=b0, bound_o1=b1,
                peak=max(_amax(acc, c, Cn, beta * C0), peak_sum), peak32=_amax(opA, opB, acc, c, Cn))
