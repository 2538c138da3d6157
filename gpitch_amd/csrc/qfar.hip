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
//                     (switches.h far_tables = 1, the default: qfar_t_lds_kernel below — the same recurrences and bits, each
//                     entering tile staged in LDS once per workgroup)
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

// The same tables, one scalar recurrence per element (j, f) with the same operations in the same order — T is byte-identical
// to qfar_t_kernel's — but an entering tile reaches the workgroup ONCE instead of once per thread (switch
// far_tables).  A workgroup owns QFL_ROWS = 32 rows j times all nf features of one side and GP (M a multiple of 64, nf of 8:
// 32 nf elements, nf / 8 <= 8 per thread: thread (j, fg) holds the features fg + 8 k of row j, so it reads ONE entry of Q per
// entering row, and eight adjacent lanes store 64 contiguous, 64-byte aligned bytes of T).  Per entering tile it stages, double-buffered in LDS:
//   qs[16][32]   the block's rows x the tile's 16 entries of Q, each row's 128 bytes loaded by eight adjacent lanes;
//   ps[16][64]   the products ew[r] * fz[f][i_r], rounded once per workgroup as every thread of qfar_t_kernel rounds them.
// The tile behind the one being walked is requested into registers (one 16-byte load of Q and nf / 16 <= 4 loads of the z
// features per thread) ahead of the walk and multiplied into the other buffer when the walk reaches it: its ew are then known,
// also when it enters in a later chunk of steps.  The step loop reads LDS only.  The counts, bcarry and the chunks of
// QFT_CHUNK steps are qfar_t_kernel's.
#define QFL_ROWS 32
#define QFL_LDP 65           // doubles between two entries of a tile in ps (nf <= 64): a constant, so the walk's offsets are immediates
#define QFL_LD 33            // doubles between two entries of a tile in qs: the eight parts of a row land on eight banks
typedef double qfl_d2 __attribute__((ext_vector_type(2)));
template <int QFL_EPT>      // elements per thread: nf / 8
__global__ void __launch_bounds__(256, 4) qfar_t_lds_kernel(const QfarItem* __restrict__ items, int N, int nf) {
  const QfarItem it = items[blockIdx.z];
  const int side = blockIdx.y, tid = threadIdx.x, M = it.M, ng = N / QFAR_GROUP;
  const int j0 = blockIdx.x * QFL_ROWS, npr = nf / 16 + ((nf & 15) ? 1 : 0);   // elements, feature loads per thread
  const double ls = it.theta[1];
  __shared__ int cnt[QFT_CHUNK];
  __shared__ double sref[QFT_CHUNK], dec[QFT_CHUNK];
  __shared__ double ew[1024];
  __shared__ double qs[2][16 * QFL_LD], ps[2][16 * QFL_LDP];
  auto row_of = [&](int r) { return side ? M - 16 * (r / 16 + 1) + (r % 16) : r; };
  const int jl = tid >> 3, fg = tid & 7;            // the thread's row of the block; its features are fg + 8 k
  qfl_d2 qn;                                         // the next tile to enter: Q, lane -> (row tid / 8, entries 2 (tid % 8), + 1)
  double fn[4];                                      //                         z features, lane -> (f = tid / 16 + 16 k, entry tid % 16)
  auto request = [&](int done) {
    const int i0 = row_of(done);
    qn = *(const qfl_d2*)(it.Q + (size_t)(j0 + (tid >> 3)) * M + i0 + 2 * (tid & 7));
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int f = (tid >> 4) + 16 * k;
      fn[k] = (k < npr && f < nf) ? it.fz[(size_t)f * M + i0 + (tid & 15)] : 0.0;
    }
  };
  auto deposit = [&](int done) {
    const int b = (done >> 4) & 1;
    qs[b][(2 * (tid & 7)) * QFL_LD + (tid >> 3)] = qn.x;
    qs[b][(2 * (tid & 7) + 1) * QFL_LD + (tid >> 3)] = qn.y;
    const double w = ew[done + (tid & 15)];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int f = (tid >> 4) + 16 * k;
      if (k < npr && f < nf) ps[b][(tid & 15) * QFL_LDP + f] = w * fn[k];
    }
  };
  double t[QFL_EPT];
#pragma unroll
  for (int k = 0; k < QFL_EPT; k++) t[k] = 0.0;
  double bcarry = 0.0;
  int done = 0;                                      // rows entered so far (uniform, a multiple of 16)
  request(0);
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
      if (c0 + q > 0) {
        const double dq = dec[q];
#pragma unroll
        for (int k = 0; k < QFL_EPT; k++) t[k] *= dq;
      }
      const int k1 = cnt[q];
      while (done < k1) {                            // (uniform) whole tiles, in entering order
        deposit(done);
        if (done + 16 < M) request(done + 16);
        __syncthreads();
        const double* qb = qs[(done >> 4) & 1];
        const double* pb = ps[(done >> 4) & 1];
#pragma unroll
        for (int r = 0; r < 16; r++) {
          const double qv = qb[r * QFL_LD + jl];
#pragma unroll
          for (int k = 0; k < QFL_EPT; k++) t[k] = fma(qv, pb[r * QFL_LDP + fg + 8 * k], t[k]);
        }
        done += 16;
      }
      const int S = side ? ng - 1 - (c0 + q) : c0 + q;
#pragma unroll
      for (int k = 0; k < QFL_EPT; k++) it.T[((size_t)S * M + j0 + jl) * (2 * nf) + side * nf + fg + 8 * k] = t[k];
    }
    bcarry = sref[nc - 1];
  }
}

// the tables' one launch (form 0: qfar_t_kernel, 1: qfar_t_lds_kernel); launch_qfar_tables and gp_debug_far_tables (far_debug.hip)
void launch_qfar_t(gp_handle h, const QfarItem* d_items, int count, int M, int nf, int n, bool lds) {
#define QFL_CASE(E) case E: hipLaunchKernelGGL(qfar_t_lds_kernel<E>, dim3(M / QFL_ROWS, 2, count), dim3(256), 0, h->stream, d_items, n, nf); break;
  if (lds) switch (nf / 8) { QFL_CASE(1) QFL_CASE(2) QFL_CASE(3) QFL_CASE(4) QFL_CASE(5) QFL_CASE(6) QFL_CASE(7) QFL_CASE(8) }
  else hipLaunchKernelGGL(qfar_t_kernel, dim3((M * nf + 255) / 256, 2, count), dim3(256), 0, h->stream, d_items, n, nf);
}

gp_status launch_qfar_tables(gp_handle h, const QfarItem* d_items, int count, int M, int m, const double* x, int n) {
  if (count <= 0) return GP_OK;
  if (!qfar_takes(M, n, m)) return gp_fail(h, GP_ERR_UNSUPPORTED, "far-field tables: whole 256-frame groups, M a multiple of 64 up to 1024");
  const int nf = 2 * sm_mpad(m);
  hipLaunchKernelGGL(qfar_cols_kernel, dim3(n / QFAR_GROUP, count), dim3(QFAR_GROUP), 0, h->stream, d_items, x, n, nf);
  launch_qfar_t(h, d_items, count, M, nf, n, gp_switches().far_tables != 0);
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}
