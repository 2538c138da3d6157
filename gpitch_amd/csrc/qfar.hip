// qfar.hip — the tables of the Q route's far field: for a MercerMatern12sm family whose inducing inputs z
// and frames x are both ascending, G = Q Kuf is formed per 256-frame group S (the wave product's workgroup) as
//     G[:, S] = Q[:, near(S)] Kuf[near(S), S]  +  T-(S) Psi-[:, S]  +  T+(S) Psi+[:, S]
// where near(S) = [kbeg, kend) are the rows some entry of which is NOT written in product form by the strip builder, and
//     T-(S)[j, f] = sum_{i < kbeg(S)}  Q[j, i] exp(-(bmin_S - a_i)) Phi_f(z_i)        Psi-[f, n] = var exp(-(b_n - bmin_S)) Phi_f(x_n)
//     T+(S)[j, f] = sum_{i >= kend(S)} Q[j, i] exp(-(a_i - bmax_S)) Phi_f(z_i)        Psi+[f, n] = var exp(-(bmax_S - b_n)) Phi_f(x_n)
// with a = z / l, b = x / l, bmin_S / bmax_S the smallest / largest b of the group and Phi the nf = 2 sm_mpad(m) cos / sin
// features of sm_features_kernel (cov.hip).  Every factor is at most 1 (times var) and nothing is divided or subtracted.
//
// Two launches per step over the Q run:
//   qfar_cols_kernel  one workgroup per (group, GP): the group's reference points and near range from the CURRENT lengthscale
//                     (it is trained on the device), by the builder's own predicate (cov_entry.h) over the builder's own
//                     wavefront columns and 16-row tiles; then the group's 256 columns of Psi- and Psi+.
//   qfar_t_kernel     T- upwards and T+ downwards over the groups, one independent scalar recurrence per element (j, f):
//                     T-(S + 1) = exp(-(bmin_{S+1} - bmin_S)) T-(S) + (the rows that became far, tile by tile).
//                     A fixed order, no atomics: two runs agree bit for bit.
#include "engine.h"
#include "cov_entry.h"

QfarSizes qfar_sizes(int M, int N, int m) {
  const size_t ng = ((size_t)N + QFAR_GROUP - 1) / QFAR_GROUP, nf = 2 * (size_t)sm_mpad(m);
  QfarSizes s;
  s.rng = gp_align_up(ng, 32);                       // two ints per group
  s.ref = gp_align_up(2 * ng, 32);
  s.T = gp_align_up(ng * (size_t)M * 2 * nf, 32);
  s.Psi = gp_align_up(2 * nf * (size_t)N, 32);
  return s;
}

// whole groups, whole 16-row tiles that one 64-bit mask holds, tables the wave product's 32-bit byte offsets reach
bool qfar_takes(int M, int N, int m) {
  if (M <= 0 || N <= 0 || m < 1 || m > 32 || (M % 64) != 0 || M > 1024 || (N % QFAR_GROUP) != 0) return false;
  const QfarSizes s = qfar_sizes(M, N, m);
  return s.T * 8 < ((size_t)1 << 31) && s.Psi * 8 < ((size_t)1 << 31);
}

__global__ void __launch_bounds__(QFAR_GROUP) qfar_cols_kernel(const QfarItem* __restrict__ items, const double* __restrict__ x,
                                                               int N, int nf) {
  const QfarItem it = items[blockIdx.y];
  const int S = blockIdx.x, tid = threadIdx.x, n = S * QFAR_GROUP + tid, M = it.M;
  const double var = it.theta[0], ls = it.theta[1];
  const double b = x[n] / ls;                        // (the builder's quotient)
  // the builder's wavefronts: CVM_SEP_COLS columns each
  double lo = b, hi = b;
#pragma unroll
  for (int o = 1; o < CVM_SEP_COLS; o <<= 1) { lo = fmin(lo, __shfl_xor(lo, o, 64)); hi = fmax(hi, __shfl_xor(hi, o, 64)); }
  const bool ok_w = cov_sep_cols_ok(1.0, lo, hi);
  __shared__ double r_lo[QFAR_GROUP / CVM_SEP_COLS], r_hi[QFAR_GROUP / CVM_SEP_COLS];
  __shared__ int r_ok[QFAR_GROUP / CVM_SEP_COLS];
  if ((tid % CVM_SEP_COLS) == 0) { r_lo[tid / CVM_SEP_COLS] = lo; r_hi[tid / CVM_SEP_COLS] = hi; r_ok[tid / CVM_SEP_COLS] = ok_w ? 1 : 0; }
  __syncthreads();
  // a tile is far for the group when it is separable for every wavefront of it: the smallest bmin / the largest bmax decide
  double bmin = r_lo[0], bmax = r_hi[0];
  bool ok = r_ok[0] != 0;
#pragma unroll
  for (int w = 1; w < QFAR_GROUP / CVM_SEP_COLS; w++) { bmin = fmin(bmin, r_lo[w]); bmax = fmax(bmax, r_hi[w]); ok = ok && (r_ok[w] != 0); }
  if (tid < 64) {                                    // one 16-row tile per lane (M <= 1024)
    const int ntile = M / 16, t = min(tid, ntile - 1);
    double tlo = it.z[t * 16] / ls, thi = tlo;
    for (int q = 1; q < 16; q++) { const double v = it.z[t * 16 + q] / ls; tlo = fmin(tlo, v); thi = fmax(thi, v); }
    const unsigned long long bm = __ballot(tid < ntile && cov_sep_below(ok, bmin, thi));
    const unsigned long long am = __ballot(tid < ntile && cov_sep_above(ok, tlo, bmax));
    // far rows below: the leading run of separable tiles; above: the trailing run (ascending z: all of them)
    const unsigned long long nb = ~bm, na = ~(am << (64 - ntile));
    const int nbelow = nb ? __ffsll(nb) - 1 : 64;
    const int nabove = na ? __clzll(na) : 64;
    if (tid == 0) {
      it.rng[2 * S] = 16 * min(nbelow, ntile);
      it.rng[2 * S + 1] = M - 16 * min(nabove, ntile);
      it.ref[2 * S] = bmin; it.ref[2 * S + 1] = bmax;
    }
  }
  const double cn = var * exp(-(b - bmin)), cp = var * exp(-(bmax - b));
  for (int f = 0; f < nf; f++) {
    const double v = it.fx[(size_t)f * N + n];
    it.Psi[(size_t)f * N + n] = cn * v;
    it.Psi[(size_t)(nf + f) * N + n] = cp * v;
  }
}

// blockIdx.y = side (0: T-, the rows below, groups walked upwards; 1: T+, the rows above, groups walked downwards),
// blockIdx.z = GP; thread = one element (j, f).  Rows become far in row order (whole 16-row tiles), so a thread walks row j of
// Q and row f of the z features once, one tile ahead of its need, whatever the groups do; what the groups decide — how many
// rows have entered by each step, the step's reference point and decay, and each entering row's factor — is worked out per
// chunk of QFT_CHUNK steps into LDS, so the step loop itself reads LDS, multiplies and stores.
#define QFT_CHUNK 256
__global__ void __launch_bounds__(256) qfar_t_kernel(const QfarItem* __restrict__ items, int N, int nf) {
  const QfarItem it = items[blockIdx.z];
  const int side = blockIdx.y, tid = threadIdx.x, M = it.M, ng = N / QFAR_GROUP;
  const int e = blockIdx.x * 256 + tid;
  const bool act = e < M * nf;
  const int j = act ? e / nf : 0, f = act ? e % nf : 0;
  const double ls = it.theta[1];
  const double* __restrict__ qrow = it.Q + (size_t)j * M;       // (Q is symmetric: row j is column j)
  const double* __restrict__ fz = it.fz + (size_t)f * M;
  __shared__ int cnt[QFT_CHUNK];                     // rows that have entered by the end of each step (a running maximum)
  __shared__ double sref[QFT_CHUNK], dec[QFT_CHUNK]; // the step's reference point; the decay from the step before
  __shared__ double ew[1024];                        // entering order r -> exp(-(distance of row r from its step's reference point))
  // entering order r -> row: upwards from row 0, or tile by tile downwards from row M (ascending inside a tile)
  auto row_of = [&](int r) { return side ? M - 16 * (r / 16 + 1) + (r % 16) : r; };
  double qn[16], fn[16];                             // the next tile to enter
  auto fetch = [&](int done) {
    const int i0 = row_of(done);
#pragma unroll
    for (int q = 0; q < 16; q++) { qn[q] = qrow[i0 + q]; fn[q] = fz[i0 + q]; }
  };
  double t = 0.0, bcarry = 0.0;
  int done = 0;                                      // rows entered so far (uniform, a multiple of 16)
  fetch(0);
  for (int c0 = 0; c0 < ng; c0 += QFT_CHUNK) {
    const int nc = min(QFT_CHUNK, ng - c0);
    __syncthreads();
    if (tid < nc) {
      const int S = side ? ng - 1 - (c0 + tid) : c0 + tid;
      cnt[tid] = side ? M - it.rng[2 * S + 1] : it.rng[2 * S];
      sref[tid] = it.ref[2 * S + side];
    }
    __syncthreads();
    int mine = done;
    double d = 1.0;
    if (tid < nc) {
      for (int q = 0; q <= tid; q++) mine = max(mine, cnt[q]);
      const double bprev = tid > 0 ? sref[tid - 1] : bcarry, bref = sref[tid];
      d = exp(side ? -(bprev - bref) : -(bref - bprev));
    }
    __syncthreads();
    if (tid < nc) { cnt[tid] = mine; dec[tid] = d; }
    __syncthreads();
    const int cend = cnt[nc - 1];
    for (int r = done + tid; r < cend; r += 256) {   // the rows that enter in this chunk: at the first step whose count passes r
      int lo = 0, hi = nc - 1;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (cnt[mid] > r) hi = mid; else lo = mid + 1; }
      const double a = it.z[row_of(r)] / ls, bref = sref[lo];
      ew[r] = exp(side ? -(a - bref) : -(bref - a));
    }
    __syncthreads();
    for (int q = 0; q < nc; q++) {
      if (c0 + q > 0) t *= dec[q];
      const int k1 = cnt[q];
      while (done < k1) {                            // (uniform) whole tiles, in entering order
#pragma unroll
        for (int r = 0; r < 16; r++) t = fma(qn[r], ew[done + r] * fn[r], t);
        done += 16;
        if (done < M) fetch(done);
      }
      const int S = side ? ng - 1 - (c0 + q) : c0 + q;
      if (act) it.T[((size_t)S * M + j) * (2 * nf) + side * nf + f] = t;
    }
    bcarry = sref[nc - 1];
  }
}

gp_status launch_qfar_tables(gp_handle h, const QfarItem* d_items, int count, int M, int m, const double* x, int n) {
  if (count <= 0) return GP_OK;
  if (!qfar_takes(M, n, m)) return gp_fail(h, GP_ERR_UNSUPPORTED, "far-field tables: whole 256-frame groups, M a multiple of 64 up to 1024");
  const int nf = 2 * sm_mpad(m);
  hipLaunchKernelGGL(qfar_cols_kernel, dim3(n / QFAR_GROUP, count), dim3(QFAR_GROUP), 0, h->stream, d_items, x, n, nf);
  hipLaunchKernelGGL(qfar_t_kernel, dim3((M * nf + 255) / 256, 2, count), dim3(256), 0, h->stream, d_items, n, nf);
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}
