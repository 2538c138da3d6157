// qbar.hip — the Q route's backward products from the far field: Qbar = Kuf D Kuf^T (D = diag(2 gv)) and
// v = Kuf gm for a MercerMatern12sm family whose product G = Q Kuf took qfar.hip's tables, without the dense split-K product.
// With qfar.hip's notation (group S of 256 frames, near(S) = [kb_S, ke_S), a = z / l, bmin_S / bmax_S, Phi, Psi- / Psi+):
//     Kuf[:, S] = P_S B_S,   B_S = [ Kuf[near(S), S] ; Psi-[:, S] ; Psi+[:, S] ]
//     P_S[i, :] = unit row (i near), exp(-(bmin_S - a_i)) Phi(z_i)^T on the Psi- block (i < kb_S), exp(-(a_i - bmax_S)) Phi(z_i)^T
//                 on the Psi+ block (i >= ke_S)
// so Qbar = sum_S P_S (B_S D_S B_S^T) P_S^T.  Near ranges are whole 16-row tiles and, once widened so that kb and ke never
// decrease (free: a near row is exact), every tile t lies above the groups S < Sa(t), near Sa(t) <= S < S0(t), below S >= S0(t).
// For a pair of tiles ti <= tj the groups fall into six runs, one per pair of sides, and every run but the near x near one is
// a decayed sum of nf-vectors or nf x nf blocks: every factor is at most 1 (times var^2), nothing is divided, no prefix sum
// is subtracted from another.
//
// Four launches per step over the Q run, a fixed order everywhere, no atomics (two runs agree bit for bit):
//   qbar_plan_kernel      the widened ranges and, per 16-row tile, S0 and Sa
//   qbar_gram_kernel      one workgroup per (group, GP), the only pass over the strip's near rows: the near x far and far x far
//                         blocks of B_S D_S B_S^T on the float64 matrix cores, and B_S gm
//   qbar_rec_kernel       the recurrences over the groups: R-(S) = C--_S + e^{-2 (bmin_{S+1} - bmin_S)} R-(S+1) downwards, R+ upwards,
//                         and per row tile ti the running below x above block W from S0(ti) on; each is applied to the features
//                         of the 16 rows whose run ends at S, so what is stored is nf-vectors per row (Um, Vp, Wv)
//   qbar_assemble_kernel  one workgroup per tile pair ti <= tj: the near x near band of the stored strip on the matrix cores
//                         (four wavefronts, four contiguous parts of the run, summed in order), the five far runs as dot
//                         products of length nf, the tile and its mirror stored once; diagonal pairs also form their rows of v
#include "engine.h"

typedef double qb_d2 __attribute__((ext_vector_type(2)));
typedef double qb_d4 __attribute__((ext_vector_type(4)));

QbarSizes qbar_sizes(int M, int N, int m) {
  const size_t ng = ((size_t)N + QFAR_GROUP - 1) / QFAR_GROUP, nf = 2 * (size_t)sm_mpad(m);
  QbarSizes s;
  s.rng2 = gp_align_up(ng, 32);                      // two ints per group
  s.tS = QBAR_MAX_TILES;                             // two ints per tile
  s.CnF = gp_align_up(ng * (size_t)M * 2 * nf, 32);
  s.CFF = gp_align_up(ng * 4 * nf * nf, 32);
  s.cn = gp_align_up(ng * (size_t)M, 32);
  s.cF = gp_align_up(ng * 2 * nf, 32);
  s.Um = gp_align_up((size_t)M * nf, 32);
  s.Wv = gp_align_up((size_t)(M / 16) * M * nf, 32);
  return s;
}

// the far-field tables' shapes; few enough groups that one thread may walk them (qbar_plan_kernel); and more than one group:
// a batch of one group has nothing to recur over and a band as long as the strip, so the split-K product keeps it (and its
// bits, which tests/test_gpu_qfar.py compares with the dense route's at such a batch)
bool qbar_takes(int M, int N, int m) {
  return qfar_takes(M, N, m) && M / 16 <= QBAR_MAX_TILES && N / QFAR_GROUP >= 2 && N / QFAR_GROUP <= 4096;
}

__global__ void __launch_bounds__(64) qbar_plan_kernel(const QbarItem* __restrict__ items, int ng) {
  const QbarItem it = items[blockIdx.x];
  const int tid = threadIdx.x, M = it.M;
  if (tid == 0) {
    int k = M;
    for (int S = ng - 1; S >= 0; S--) { k = min(k, it.rng[2 * S]); it.rng2[2 * S] = k; }
    k = 0;
    for (int S = 0; S < ng; S++) { k = max(k, it.rng[2 * S + 1]); it.rng2[2 * S + 1] = k; }
  }
  __syncthreads();
  if (tid < M / 16) {       // the first group with kb > 16 t / with ke > 16 t (ng: none), by bisection over the monotone ranges
    for (int side = 0; side < 2; side++) {
      int lo = 0, hi = ng;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (it.rng2[2 * mid + side] > 16 * tid) hi = mid; else lo = mid + 1; }
      it.tS[side * QBAR_MAX_TILES + tid] = lo;
    }
  }
}

// rows of B_S in order: the near rows, Psi-, Psi+ (all whole 16-row tiles); a wavefront owns 32 x 32 of the lower triangle of
// B_S D_S B_S^T at a time and skips what lies wholly in near x near (the assembly takes that from the strip itself, summed
// over groups in registers — stored per group it would be N / 256 matrices of M x M when every range is [0, M)).
// v_mfma_f64_16x16x4_f64: A lane (kq, lc) = rows[lc][k], B lane (kq, lc) = cols[lc][k], the same k in both — here
// k = 16 step + 4 kq + u for the u-th of four instructions, so a lane loads 32 contiguous bytes per row and step.
__global__ void __launch_bounds__(256) qbar_gram_kernel(const QbarItem* __restrict__ items, int N, int nf) {
  const QbarItem it = items[blockIdx.y];
  const int S = blockIdx.x, M = it.M, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, lc = lane & 15, kq = lane >> 4;
  const int kb = it.rng2[2 * S], ke = it.rng2[2 * S + 1], nn = ke - kb, nr = nn + 2 * nf;
  const int nt16 = nr / 16, ns = (nt16 + 1) / 2, nnear16 = nn / 16;
  const size_t c0 = (size_t)S * QFAR_GROUP;
  const double* __restrict__ gv = it.gv + c0;
  auto row_ptr = [&](int r) -> const double* {      // r < nr
    return r < nn ? it.Kuf + (size_t)(kb + r) * it.ldk + c0 : it.Psi + (size_t)(r - nn) * N + c0;
  };
  for (int p = wave; p < ns * (ns + 1) / 2; p += 4) {
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= p) I++;
    const int J = p - I * (I + 1) / 2;
    if (2 * I + 1 < nnear16) continue;              // wholly near x near
    const double* ra[2]; const double* rb[2];
    bool va[2], vb[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      va[q] = 2 * I + q < nt16; vb[q] = 2 * J + q < nt16;
      ra[q] = row_ptr(va[q] ? 16 * (2 * I + q) + lc : 0) + 4 * kq;
      rb[q] = row_ptr(vb[q] ? 16 * (2 * J + q) + lc : 0) + 4 * kq;
    }
    qb_d4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) acc[a][b] = qb_d4{0.0, 0.0, 0.0, 0.0};
    for (int k0 = 0; k0 < QFAR_GROUP; k0 += 16) {
      const qb_d2 d0 = *(const qb_d2*)(gv + k0 + 4 * kq), d1 = *(const qb_d2*)(gv + k0 + 4 * kq + 2);
      const double dv[4] = {2.0 * d0.x, 2.0 * d0.y, 2.0 * d1.x, 2.0 * d1.y};
      double av[2][4], bv[2][4];
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const qb_d2 a0 = *(const qb_d2*)(ra[q] + k0), a1 = *(const qb_d2*)(ra[q] + k0 + 2);
        const qb_d2 b0 = *(const qb_d2*)(rb[q] + k0), b1 = *(const qb_d2*)(rb[q] + k0 + 2);
        av[q][0] = a0.x * dv[0]; av[q][1] = a0.y * dv[1]; av[q][2] = a1.x * dv[2]; av[q][3] = a1.y * dv[3];
        bv[q][0] = b0.x; bv[q][1] = b0.y; bv[q][2] = b1.x; bv[q][3] = b1.y;
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
          for (int b = 0; b < 2; b++) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a][u], bv[b][u], acc[a][b], 0, 0, 0);
    }
    // C/D map: column lc, row kq + 4 reg.  Tile (ta, tb) with ta >= tb: far x near goes to CnF[S][near row][feature], far x far
    // to CFF[S] and its mirror (a diagonal tile: from its lower half)
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++) {
        const int ta = 2 * I + a, tb = 2 * J + b;
        if (!va[a] || !vb[b] || tb > ta || ta < nnear16) continue;
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int f = 16 * ta + kq + 4 * r - nn, cc = 16 * tb + lc;
          const double val = acc[a][b][r];
          if (tb < nnear16) {
            it.CnF[((size_t)S * M + kb + cc) * (2 * nf) + f] = val;
          } else if (ta > tb || f >= cc - nn) {
            const int f2 = cc - nn;
            double* C = it.CFF + (size_t)S * (4 * nf * nf);
            C[f * (2 * nf) + f2] = val;
            C[f2 * (2 * nf) + f] = val;
          }
        }
      }
  }
  // B_S gm: a row per wavefront at a time, four frames per lane, one butterfly
  const double* __restrict__ gm = it.gm + c0;
  const qb_d2 g0 = *(const qb_d2*)(gm + 4 * lane), g1 = *(const qb_d2*)(gm + 4 * lane + 2);
  for (int r = wave; r < nr; r += 4) {
    const double* row = row_ptr(r) + 4 * lane;
    const qb_d2 x0 = *(const qb_d2*)row, x1 = *(const qb_d2*)(row + 2);
    double s = fma(x1.y, g1.y, fma(x1.x, g1.x, fma(x0.y, g0.y, x0.x * g0.x)));
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) {
      if (r < nn) it.cn[(size_t)S * M + kb + r] = s;
      else it.cF[(size_t)S * (2 * nf) + r - nn] = s;
    }
  }
}

// blockIdx.x = 0: R- downwards; 1: R+ upwards; 2 + ti: W of row tile ti upwards from S0(ti).  A thread keeps elements
// e = tid + 256 q of the nf x nf block in registers.  The walk is a chain of dependent steps, so nothing in a step may wait
// for memory: the decays of 256 steps are worked out at once into LDS (one exp per thread), the blocks of QBAR_RB groups
// are requested together, and where a tile's run ends at S the block and the tile's features go through LDS into 16
// matrix-vector products.
#define QBAR_NE ((QBAR_MAX_NF * QBAR_MAX_NF + 255) / 256)
#define QBAR_RB 4
__global__ void __launch_bounds__(256) qbar_rec_kernel(const QbarItem* __restrict__ items, int ng, int nf) {
  const QbarItem it = items[blockIdx.y];
  const int role = blockIdx.x, tid = threadIdx.x, M = it.M, nt = M / 16, n2 = nf * nf, ld = 2 * nf;
  const double ls = it.theta[1];
  __shared__ double Rs[QBAR_MAX_NF * QBAR_MAX_NF], Ps[16 * QBAR_MAX_NF], wrs[256], wcs[256];
  __shared__ int tS0[QBAR_MAX_TILES], tSa[QBAR_MAX_TILES];
  if (tid < nt) { tS0[tid] = it.tS[tid]; tSa[tid] = it.tS[QBAR_MAX_TILES + tid]; }
  __syncthreads();
  const int ti = role - 2;
  // the walk: first group, last group, direction; the block's corner in CFF[S]
  int Sbeg, Send, dir, corner;
  if (role == 0) { Sbeg = ng - 1; Send = tS0[0]; dir = -1; corner = 0; }
  else if (role == 1) { Sbeg = 0; Send = tSa[nt - 1] - 1; dir = 1; corner = nf * ld + nf; }
  else { Sbeg = tS0[ti]; Send = tSa[nt - 1] - 1; dir = 1; corner = nf; }
  const int nsteps = dir * (Send - Sbeg) + 1;
  if (nsteps <= 0) return;                          // (uniform) nothing ends in this walk
  int off[QBAR_NE];
  double R[QBAR_NE], buf[QBAR_RB][QBAR_NE];
#pragma unroll
  for (int q = 0; q < QBAR_NE; q++) {
    const int e = tid + 256 * q;
    off[q] = e < n2 ? corner + (e / nf) * ld + (e % nf) : -1;
    R[q] = 0.0;
  }
  // the tiles whose run ends at S, in the walk's order (S0 and Sa never decrease with the tile)
  int tp = (role == 0) ? nt - 1 : (role == 1 ? 0 : ti + 1);
  double* out = role == 0 ? it.Um : (role == 1 ? it.Vp : it.Wv + (size_t)ti * M * nf);
  const double bmin0 = it.ref[2 * Sbeg];
  for (int c0 = 0; c0 < nsteps; c0 += 256) {
    const int cend = min(c0 + 256, nsteps);
    __syncthreads();
    if (c0 + tid < cend) {      // step k: wr scales what the walk has so far, wc the group's own block
      const int k = c0 + tid, S = Sbeg + dir * k;
      double wr = 0.0;
      if (k > 0) {
        if (role == 0) wr = exp(-2.0 * (it.ref[2 * (S + 1)] - it.ref[2 * S]));
        else if (role == 1) wr = exp(-2.0 * (it.ref[2 * S + 1] - it.ref[2 * (S - 1) + 1]));
        else wr = exp(-(it.ref[2 * S + 1] - it.ref[2 * (S - 1) + 1]));
      }
      wrs[tid] = wr;
      wcs[tid] = role >= 2 ? exp(-(it.ref[2 * S] - bmin0)) : 1.0;
    }
    __syncthreads();
    for (int b0 = c0; b0 < cend; b0 += QBAR_RB) {
#pragma unroll
      for (int r = 0; r < QBAR_RB; r++) {
        if (b0 + r < cend) {
          const double* C = it.CFF + (size_t)(Sbeg + dir * (b0 + r)) * (4 * n2);
#pragma unroll
          for (int q = 0; q < QBAR_NE; q++) buf[r][q] = off[q] >= 0 ? C[off[q]] : 0.0;
        }
      }
#pragma unroll
      for (int r = 0; r < QBAR_RB; r++) {
        if (b0 + r >= cend) break;
        const int S = Sbeg + dir * (b0 + r);
        const double wr = wrs[b0 + r - c0], wc = wcs[b0 + r - c0];
#pragma unroll
        for (int q = 0; q < QBAR_NE; q++) R[q] = fma(wr, R[q], wc * buf[r][q]);
        // (uniform) skip the tiles whose run ended outside the walk, then serve those that end here
        if (role == 0) { while (tp >= 0 && tS0[tp] > S) tp--; }
        else { while (tp < nt && tSa[tp] - 1 < S) tp++; }
        bool staged = false;
        while (role == 0 ? (tp >= 0 && tS0[tp] == S) : (tp < nt && tSa[tp] - 1 == S)) {
          __syncthreads();
          if (!staged) {
#pragma unroll
            for (int q = 0; q < QBAR_NE; q++) if (off[q] >= 0) Rs[tid + 256 * q] = R[q];
            staged = true;
          }
          for (int o = tid; o < 16 * nf; o += 256) Ps[o] = it.fz[(size_t)(o / 16) * M + 16 * tp + (o % 16)];
          __syncthreads();
          const double bref = it.ref[2 * S + (role == 0 ? 0 : 1)];
          for (int o = tid; o < 16 * nf; o += 256) {
            const int f = o / 16, c = o % 16, j = 16 * tp + c;
            double s = 0.0;
            for (int f2 = 0; f2 < nf; f2++) s = fma(Rs[f * nf + f2], Ps[f2 * 16 + c], s);
            const double a = it.z[j] / ls;
            out[(size_t)j * nf + f] = exp(role == 0 ? -(bref - a) : -(a - bref)) * s;
          }
          tp += (role == 0) ? -1 : 1;
        }
      }
    }
  }
}

// acc + sum_s w[s] src[s stride], in order; eight loads in flight
__device__ __forceinline__ double qbar_decayed_sum(const double* w, const double* __restrict__ src, size_t stride, int len, double acc) {
  int s = 0;
  for (; s + 8 <= len; s += 8) {
    double x[8];
#pragma unroll
    for (int u = 0; u < 8; u++) x[u] = src[(size_t)(s + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; u++) acc = fma(w[s + u], x[u], acc);
  }
  for (; s < len; s++) acc = fma(w[s], src[(size_t)s * stride], acc);
  return acc;
}

#define QBAR_NY (16 * QBAR_MAX_NF / 256)
__global__ void __launch_bounds__(256) qbar_assemble_kernel(const QbarItem* __restrict__ items, int ng, int nf) {
  const QbarItem it = items[blockIdx.y];
  const int tid = threadIdx.x, M = it.M, lane = tid & 63, wave = tid >> 6, lc = lane & 15, kq = lane >> 4;
  int tj = 0;
  while ((tj + 1) * (tj + 2) / 2 <= (int)blockIdx.x) tj++;
  const int ti = blockIdx.x - tj * (tj + 1) / 2;    // ti <= tj
  if (16 * tj >= M) return;
  const double ls = it.theta[1];
  const int S0i = it.tS[ti], Sai = it.tS[QBAR_MAX_TILES + ti], S0j = it.tS[tj], Saj = it.tS[QBAR_MAX_TILES + tj];
  __shared__ double part[4][256];
  __shared__ double PI[16 * QBAR_MAX_NF], PJ[16 * QBAR_MAX_NF], YR[16 * QBAR_MAX_NF], YC[16 * QBAR_MAX_NF];
  // ---- both near: groups [Saj, S0i) of the stored strip, four contiguous parts
  {
    const int lo = Saj, cnt = max(S0i - Saj, 0);
    const int g0 = lo + (cnt * wave) / 4, g1 = lo + (cnt * (wave + 1)) / 4;
    const double* __restrict__ ra = it.Kuf + (size_t)(16 * ti + lc) * it.ldk + 4 * kq;
    const double* __restrict__ rb = it.Kuf + (size_t)(16 * tj + lc) * it.ldk + 4 * kq;
    const double* __restrict__ gv = it.gv + 4 * kq;
    // 64 frames a trip (a group is four trips): every load of the trip first, then four independent chains of four
    // instructions, one per 16 frames, summed in a fixed order at the end
    qb_d4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; u++) acc[u] = qb_d4{0.0, 0.0, 0.0, 0.0};
    for (size_t k0 = (size_t)g0 * QFAR_GROUP; k0 < (size_t)g1 * QFAR_GROUP; k0 += 64) {
      qb_d2 d[4][2], a[4][2], b[4][2];
#pragma unroll
      for (int u = 0; u < 4; u++)
#pragma unroll
        for (int w = 0; w < 2; w++) {
          d[u][w] = *(const qb_d2*)(gv + k0 + 16 * u + 2 * w);
          a[u][w] = *(const qb_d2*)(ra + k0 + 16 * u + 2 * w);
          b[u][w] = *(const qb_d2*)(rb + k0 + 16 * u + 2 * w);
        }
#pragma unroll
      for (int w = 0; w < 2; w++) {
#pragma unroll
        for (int u = 0; u < 4; u++) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][w].x * (2.0 * d[u][w].x), b[u][w].x, acc[u], 0, 0, 0);
#pragma unroll
        for (int u = 0; u < 4; u++) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u][w].y * (2.0 * d[u][w].y), b[u][w].y, acc[u], 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) part[wave][(kq + 4 * r) * 16 + lc] = (acc[0][r] + acc[1][r]) + (acc[2][r] + acc[3][r]);
  }
  // ---- features of the two tiles; the vectors that meet Phi(z_j) (rows above: Vp, near rows against rows above: Cn+) about
  // the latest bmax among them, and those that meet Phi(z_i) (Wv, Cn-, Um) about the earliest bmin
  const int bl = Sai, bh = min(Saj, S0i);           // i near, j above
  const int el = max(S0i, Saj), eh = S0j;           // i below, j near
  const bool hasA = Sai > 0, hasB = bl < bh, hasD = S0i < Saj, hasE = el < eh, hasF = S0j < ng;
  const double refR = hasB ? it.ref[2 * (bh - 1) + 1] : (hasA ? it.ref[2 * (Sai - 1) + 1] : 0.0);
  const double refC = S0i < ng ? it.ref[2 * S0i] : 0.0;
  __shared__ double wts[256];                       // the decays of up to 256 groups of a run, one exp per thread
  double yr[QBAR_NY], yc[QBAR_NY];
#pragma unroll
  for (int k = 0; k < QBAR_NY; k++) {
    const int o = tid + 256 * k;
    yr[k] = yc[k] = 0.0;
    if (o < 16 * nf) {
      const int q = o / nf, f = o % nf, i = 16 * ti + q, j = 16 * tj + q;
      PI[o] = it.fz[(size_t)f * M + i];
      PJ[o] = it.fz[(size_t)f * M + j];
      if (hasA) yr[k] = exp(-(refR - it.ref[2 * (Sai - 1) + 1])) * it.Vp[(size_t)i * nf + f];
      if (hasD) yc[k] = it.Wv[((size_t)ti * M + j) * nf + f];
    }
  }
  for (int s0 = bl; s0 < bh; s0 += 256) {
    const int len = min(256, bh - s0);
    __syncthreads();
    if (tid < len) wts[tid] = exp(-(refR - it.ref[2 * (s0 + tid) + 1]));
    __syncthreads();
#pragma unroll
    for (int k = 0; k < QBAR_NY; k++) {
      const int o = tid + 256 * k;
      if (o >= 16 * nf) continue;
      const double* src = it.CnF + ((size_t)s0 * M + 16 * ti + o / nf) * (2 * nf) + nf + o % nf;
      yr[k] = qbar_decayed_sum(wts, src, (size_t)M * (2 * nf), len, yr[k]);
    }
  }
  for (int s0 = el; s0 < eh; s0 += 256) {
    const int len = min(256, eh - s0);
    __syncthreads();
    if (tid < len) wts[tid] = exp(-(it.ref[2 * (s0 + tid)] - refC));
    __syncthreads();
#pragma unroll
    for (int k = 0; k < QBAR_NY; k++) {
      const int o = tid + 256 * k;
      if (o >= 16 * nf) continue;
      const double* src = it.CnF + ((size_t)s0 * M + 16 * tj + o / nf) * (2 * nf) + o % nf;
      yc[k] = qbar_decayed_sum(wts, src, (size_t)M * (2 * nf), len, yc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < QBAR_NY; k++) {
    const int o = tid + 256 * k;
    if (o >= 16 * nf) continue;
    if (hasF) yc[k] = fma(exp(-(it.ref[2 * S0j] - refC)), it.Um[(size_t)(16 * tj + o / nf) * nf + o % nf], yc[k]);
    YR[o] = yr[k]; YC[o] = yc[k];
  }
  __syncthreads();
  // ---- the element: a diagonal pair evaluates (min, max) for both halves, so Qbar is symmetric to the bit
  {
    int r = tid >> 4, c = tid & 15;
    if (ti == tj && r > c) { const int t = r; r = c; c = t; }
    const int i = 16 * ti + r, j = 16 * tj + c;
    double val = (part[0][r * 16 + c] + part[1][r * 16 + c]) + (part[2][r * 16 + c] + part[3][r * 16 + c]);
    if (hasA || hasB) {
      double s = 0.0;
      for (int f = 0; f < nf; f++) s = fma(YR[r * nf + f], PJ[c * nf + f], s);
      val = fma(exp(-(it.z[j] / ls - refR)), s, val);
    }
    if (hasD || hasE || hasF) {
      double s = 0.0;
      for (int f = 0; f < nf; f++) s = fma(PI[r * nf + f], YC[c * nf + f], s);
      val = fma(exp(-(refC - it.z[i] / ls)), s, val);
    }
    const int r0 = tid >> 4, c0 = tid & 15;
    it.Qbar[(size_t)(16 * ti + r0) * M + 16 * tj + c0] = val;
    if (ti != tj) it.Qbar[(size_t)(16 * tj + c0) * M + 16 * ti + r0] = val;
  }
  // ---- v (diagonal pairs): row r, the groups S = c, c + 16, ... per thread, then the 16 sums in order
  if (ti == tj) {
    const int r = tid >> 4, c = tid & 15, i = 16 * ti + r;
    const double a = it.z[i] / ls;
    double s = 0.0;
    for (int S = c; S < ng; S += 16) {
      if (S >= Sai && S < S0i) { s += it.cn[(size_t)S * M + i]; continue; }
      const bool below = S >= S0i;
      const double* cf = it.cF + (size_t)S * (2 * nf) + (below ? 0 : nf);
      double t = 0.0;
      for (int f = 0; f < nf; f += 8) {           // (nf is a multiple of 8) the eight loads first
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = cf[f + u];
#pragma unroll
        for (int u = 0; u < 8; u++) t = fma(PI[r * nf + f + u], x[u], t);
      }
      s = fma(exp(below ? -(it.ref[2 * S] - a) : -(a - it.ref[2 * S + 1])), t, s);
    }
    __syncthreads();
    part[0][tid] = s;
    __syncthreads();
    if (c == 0) {
      double v = 0.0;
      for (int q = 0; q < 16; q++) v += part[0][r * 16 + q];
      it.v[i] = v;
    }
  }
}

gp_status launch_qbar(gp_handle h, const QbarItem* d_items, int count, int M, int m, int n) {
  if (count <= 0) return GP_OK;
  if (!qbar_takes(M, n, m)) return gp_fail(h, GP_ERR_UNSUPPORTED, "far-field Qbar: the far-field tables' shapes, at most 4096 groups of 256 frames");
  const int nf = 2 * sm_mpad(m), ng = n / QFAR_GROUP, nt = M / 16;
  hipLaunchKernelGGL(qbar_plan_kernel, dim3(count), dim3(64), 0, h->stream, d_items, ng);
  hipLaunchKernelGGL(qbar_gram_kernel, dim3(ng, count), dim3(256), 0, h->stream, d_items, n, nf);
  hipLaunchKernelGGL(qbar_rec_kernel, dim3(2 + nt, count), dim3(256), 0, h->stream, d_items, ng, nf);
  hipLaunchKernelGGL(qbar_assemble_kernel, dim3(nt * (nt + 1) / 2, count), dim3(256), 0, h->stream, d_items, ng, nf);
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}
