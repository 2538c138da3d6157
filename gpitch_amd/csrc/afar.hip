// afar.hip — the activations' forward strip work from near rows plus an exact rank-4 far field.
// A Matern-3/2 Kuf is semiseparable along sorted inputs: with c = sqrt(3) / l, a row i whose z_i lies below every frame of a
// 256-frame group S factors exactly around ref = xmin_S,
//     K(z_i, x_n) = var e^{-c (ref - z_i)} e^{-c (x_n - ref)} (kappa + c (x_n - ref) + c (ref - z_i)),   kappa = 1 - 1.5e-12
// (kappa: the reference's r = sqrt(d^2 / l^2 + 1e-12) shifts a far entry by -1.5e-12 var e^{-c rho}, uniformly in rho), and a row
// above every frame of S mirrors it around ref = xmax_S.  So for any M x M left factor X
//     (X Kuf)[:, S] = X[:, near(S)] Kuf[near(S), S]  +  T-_X(S) Psi-[:, S]  +  T+_X(S) Psi+[:, S]          T: M x 2, Psi: 2 x 256
//     T-_X(S)[j, 0] = sum_{i < kbeg(S)} X[j, i] u_i          u_i = e^{-a_i},  a_i = c (xmin_S - z_i)
//     T-_X(S)[j, 1] = sum_{i < kbeg(S)} X[j, i] u_i a_i
//     Psi-[0, n] = p_n (kappa + b_n),  Psi-[1, n] = p_n      p_n = var e^{-b_n},  b_n = c (x_n - xmin_S)
// where near(S) = [kbeg, kend) are the whole 16-row tiles that are neither below nor above the group.  Every exponent is <= 0 and
// nothing is divided.  X = W gives the stored strip A = W Kuf; X = C := tril(Lq)^T W gives Lq^T A, of which only the column sums
// of squares are kept.  Three launches per step over the run of activation GPs:
//   afar_cols_kernel  one workgroup per (group, GP): xmin / xmax of the group, its near range from the CURRENT lengthscale-free
//                     rule (a tile is below when its largest z is less than xmin, above when its smallest exceeds xmax), Psi
//   afar_t_kernel     T-_X upwards and T+_X downwards over the groups, one thread per row j, side and factor: moving the reference
//                     point by a = c (ref' - ref) >= 0 is m0' = e^{-a} m0, m1' = e^{-a} (m1 + a m0) (kuf_scan_prefix_kernel's
//                     shift), then the rows that became far enter.  A fixed order, no atomics: two runs agree bit for bit.
//                     (switches.h far_tables = 1, the default: afar_t_tiled_kernel below — the same chains and bits, 64 rows per
//                     one-wavefront workgroup, the entering tiles staged in LDS)
//   afar_prod_kernel  a wavefront per 32 frames and GP on v_mfma_f64_16x16x4_f64: Kuf[near, S] and Psi in its
//                     registers as the B operand, tiles of W, C and T as the A operand, all M / 16 row tiles walked; stores A and
//                     leaves the complete column sums colsum(A^2), colsum((C Kuf)^2) and A^T q_mu as ONE partial row each for
//                     cond_finish_kernel.
#include "engine.h"

#define AF_KAPPA (1.0 - 1.5e-12)
#define AF_SQRT3 1.7320508075688772

AfarSizes afar_sizes(int M, int N) {
  const size_t ng = ((size_t)N + AFAR_GROUP - 1) / AFAR_GROUP;
  AfarSizes s;
  s.rng = gp_align_up(ng, 32);                       // two ints per group
  s.ref = gp_align_up(2 * ng, 32);
  s.T = gp_align_up(ng * (size_t)M * 8, 32);
  s.Psi = gp_align_up(4 * (size_t)N, 32);
  s.C = gp_align_up((size_t)M * M, 32);
  return s;
}

// whole groups, whole 16-row tiles that one 64-bit mask holds, and strips of at least 2^20 entries: below that the strip is
// built by cov_build_kernel, the dense products are short, and the route gains nothing
bool afar_takes(int M, int N) {
  if (M <= 0 || N <= 0 || (M % 16) != 0 || M > 1024 || (N % AFAR_GROUP) != 0) return false;
  if ((int64_t)M * N < ((int64_t)1 << 20)) return false;
  return afar_sizes(M, N).T * 8 < ((size_t)1 << 31);
}

__global__ void __launch_bounds__(AFAR_GROUP) afar_cols_kernel(const AfarItem* __restrict__ items, const double* __restrict__ x, int N) {
  const AfarItem it = items[blockIdx.y];
  const int S = blockIdx.x, tid = threadIdx.x, n = S * AFAR_GROUP + tid, M = it.M;
  const double var = it.theta[0], c = AF_SQRT3 / it.theta[1];
  const double xn = x[n];
  double lo = xn, hi = xn;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { lo = fmin(lo, __shfl_xor(lo, o, 64)); hi = fmax(hi, __shfl_xor(hi, o, 64)); }
  __shared__ double r_lo[AFAR_GROUP / 64], r_hi[AFAR_GROUP / 64];
  if ((tid & 63) == 0) { r_lo[tid >> 6] = lo; r_hi[tid >> 6] = hi; }
  __syncthreads();
  double xmin = r_lo[0], xmax = r_hi[0];
#pragma unroll
  for (int w = 1; w < AFAR_GROUP / 64; w++) { xmin = fmin(xmin, r_lo[w]); xmax = fmax(xmax, r_hi[w]); }
  if (tid < 64) {                                    // one 16-row tile per lane (M <= 1024)
    const int ntile = M / 16, t = min(tid, ntile - 1);
    double tlo = it.z[t * 16], thi = tlo;
    for (int q = 1; q < 16; q++) { const double v = it.z[t * 16 + q]; tlo = fmin(tlo, v); thi = fmax(thi, v); }
    const unsigned long long bm = __ballot(tid < ntile && thi < xmin);
    const unsigned long long am = __ballot(tid < ntile && tlo > xmax);
    // far rows below: the leading run of tiles below the group; above: the trailing run of tiles above it
    const unsigned long long nb = ~bm, na = ~(am << (64 - ntile));
    const int nbelow = nb ? __ffsll(nb) - 1 : 64;
    const int nabove = na ? __clzll(na) : 64;
    if (tid == 0) {
      it.rng[2 * S] = 16 * min(nbelow, ntile);
      it.rng[2 * S + 1] = M - 16 * min(nabove, ntile);
      it.ref[2 * S] = xmin; it.ref[2 * S + 1] = xmax;
    }
  }
  const double bn = c * (xn - xmin), bp = c * (xmax - xn);
  const double pn = var * exp(-bn), pp = var * exp(-bp);
  it.Psi[n] = pn * (AF_KAPPA + bn);
  it.Psi[(size_t)N + n] = pn;
  it.Psi[2 * (size_t)N + n] = pp * (AF_KAPPA + bp);
  it.Psi[3 * (size_t)N + n] = pp;
}

// blockIdx.y = side + 2 * factor (side 0: T-, groups walked upwards, rows entering from row 0; side 1: T+, groups walked
// downwards, rows entering from row M - 1.  factor 0: X = W, lower triangular — entries above the diagonal count as zero
// whatever the buffer holds; factor 1: X = C), blockIdx.z = GP, thread = row j.  What the groups decide — the shift of the
// reference point and each entering row's two weights — is the same for every row: the workgroup works the weights out
// together, 256 entering rows at a time.
__global__ void __launch_bounds__(256) afar_t_kernel(const AfarItem* __restrict__ items, int N) {
  const AfarItem it = items[blockIdx.z];
  const int side = blockIdx.y & 1, fac = blockIdx.y >> 1, tid = threadIdx.x, M = it.M, ng = N / AFAR_GROUP;
  const int j = blockIdx.x * 256 + tid;
  const bool act = j < M;
  const double c = AF_SQRT3 / it.theta[1];
  const double* __restrict__ xrow = (fac ? it.C : it.W) + (size_t)(act ? j : 0) * M;
  __shared__ double ew[256], ea[256];
  double m0 = 0.0, m1 = 0.0, refprev = 0.0;
  int done = 0;                                      // rows entered so far (uniform)
  for (int q = 0; q < ng; q++) {
    const int S = side ? ng - 1 - q : q;
    const int far = side ? M - it.rng[2 * S + 1] : it.rng[2 * S];
    // (frames promised ascending: xmin and xmax ascend with S, so a tile once below stays below, whatever z does, and the ranges
    // are monotone by the rule itself — far >= done always.  The maximum only keeps `done` from running backwards under a broken
    // promise; it does not make such a batch right: the product would then count rows [far, done) twice)
    const int cnt = max(far, done);
    const double ref = it.ref[2 * S + side];
    if (q > 0) {
      const double a = side ? c * (refprev - ref) : c * (ref - refprev);
      const double e = exp(-a);
      m1 = e * fma(a, m0, m1);
      m0 = e * m0;
    }
    refprev = ref;
    while (done < cnt) {
      const int nn = min(256, cnt - done);
      __syncthreads();
      if (tid < nn) {
        const int i = side ? M - 1 - (done + tid) : done + tid;
        const double a = side ? c * (it.z[i] - ref) : c * (ref - it.z[i]);
        const double e = exp(-a);
        ew[tid] = e; ea[tid] = e * a;
      }
      __syncthreads();
      if (act) {
        for (int r = 0; r < nn; r++) {
          const int i = side ? M - 1 - (done + r) : done + r;
          const double xv = (fac == 0 && i > j) ? 0.0 : xrow[i];
          m0 = fma(xv, ew[r], m0);
          m1 = fma(xv, ea[r], m1);
        }
      }
      done += nn;
    }
    if (act) {
      double* t = it.T + ((size_t)S * M + j) * 8 + fac * 4 + side * 2;
      t[0] = m0; t[1] = m1;
    }
  }
}

// The same tables, the same chain per (row j, side, factor) and the same operations in the same order — T is byte-identical to
// afar_t_kernel's — with the operands brought to the thread another way (switch far_tables):
//   a workgroup is ONE wavefront on AFT_ROWS = 64 rows of one (side, factor, GP): M / 64 x 4 x GPs workgroups instead of 4 x GPs;
//   what the groups decide is worked out once per workgroup, AFT_CHUNK steps at a time, into LDS: the running maximum of the
//   entered rows, the shift a and exp(-a) of the reference point, and for every row that enters in the chunk e and e a around
//   the reference point of the step it enters at (found by bisection over the chunk's counts, as qfar_t_kernel does);
//   the entering rows' 16 entries of X per row of the workgroup pass through LDS tile by tile: each row's 128 bytes are loaded by
//   eight adjacent lanes, tile t + 1 is requested into registers ahead of the walk over tile t and written to the other buffer
//   behind it (one barrier per tile), and a thread reads its own row back (row stride 17 doubles: no bank is hit twice).
// factor 0 masks i > j in the registers, whatever the buffer or the tile holds: a NaN above W's diagonal reaches no sum.
typedef double aft_d2 __attribute__((ext_vector_type(2)));
#define AFT_ROWS 64
#define AFT_CHUNK 64
#define AFT_LD 17
__global__ void __launch_bounds__(AFT_ROWS) afar_t_tiled_kernel(const AfarItem* __restrict__ items, int N) {
  const AfarItem it = items[blockIdx.z];
  const int side = blockIdx.y & 1, fac = blockIdx.y >> 1, tid = threadIdx.x, M = it.M, ng = N / AFAR_GROUP;
  const int j0 = blockIdx.x * AFT_ROWS, j = j0 + tid;
  const bool act = j < M;
  const double c = AF_SQRT3 / it.theta[1];
  const double* __restrict__ X = fac ? it.C : it.W;
  __shared__ int cnt[AFT_CHUNK];                     // rows that have entered by the end of each step (a running maximum)
  __shared__ double sref[AFT_CHUNK], sa[AFT_CHUNK], se[AFT_CHUNK];   // the step's reference point; its shift from the step before
  __shared__ double ew[1024], ea[1024];              // entering order r -> e, e a around the reference point of r's step
  __shared__ double xs[2][AFT_ROWS * AFT_LD];        // entering tile (r >> 4) & 1: [row][column of the tile, ascending i]
  // tile t of the entering order holds the columns [i0, i0 + 16): from column 0 upwards, or from column M downwards
  const int nt = M / 16;
  auto tile_i0 = [&](int t) { return side ? M - 16 * (t + 1) : 16 * t; };
  // lane -> (row, 16-byte part) of the eight loads of a tile: eight adjacent lanes take a row's 128 bytes
  aft_d2 xn[8];
  auto request = [&](int t) {
    const int i0 = tile_i0(t);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int row = min(j0 + 8 * k + (tid >> 3), M - 1);
      xn[k] = *(const aft_d2*)(X + (size_t)row * M + i0 + 2 * (tid & 7));
    }
  };
  auto deposit = [&](int t) {
    double* b = xs[t & 1];
#pragma unroll
    for (int k = 0; k < 8; k++) {
      double* d = b + (8 * k + (tid >> 3)) * AFT_LD + 2 * (tid & 7);
      d[0] = xn[k].x; d[1] = xn[k].y;
    }
  };
  request(0);
  deposit(0);
  if (nt > 1) request(1);
  __syncthreads();
  int have = 0;                                      // the tile in LDS that the walk reads
  double m0 = 0.0, m1 = 0.0, rcarry = 0.0;
  int done = 0;                                      // rows entered so far (uniform)
  for (int c0 = 0; c0 < ng; c0 += AFT_CHUNK) {
    const int nc = min(AFT_CHUNK, ng - c0);
    __syncthreads();
    if (tid < nc) {
      const int S = side ? ng - 1 - (c0 + tid) : c0 + tid;
      cnt[tid] = side ? M - it.rng[2 * S + 1] : it.rng[2 * S];
      sref[tid] = it.ref[2 * S + side];
    }
    __syncthreads();
    int mine = done;
    double a = 0.0, e = 1.0;
    if (tid < nc) {
      for (int q = 0; q <= tid; q++) mine = max(mine, cnt[q]);
      const double refprev = tid > 0 ? sref[tid - 1] : rcarry, ref = sref[tid];
      a = side ? c * (refprev - ref) : c * (ref - refprev);
      e = exp(-a);
    }
    __syncthreads();
    if (tid < nc) { cnt[tid] = mine; sa[tid] = a; se[tid] = e; }
    __syncthreads();
    const int cend = min(cnt[nc - 1], M);
    for (int r = done + tid; r < cend; r += AFT_ROWS) {   // the rows that enter in this chunk: at the first step whose count passes r
      int lo = 0, hi = nc - 1;
      while (lo < hi) { const int mid = (lo + hi) >> 1; if (cnt[mid] > r) hi = mid; else lo = mid + 1; }
      const int i = side ? M - 1 - r : r;
      const double ref = sref[lo];
      const double ai = side ? c * (it.z[i] - ref) : c * (ref - it.z[i]);
      const double ei = exp(-ai);
      ew[r] = ei; ea[r] = ei * ai;
    }
    __syncthreads();
    for (int q = 0; q < nc; q++) {
      if (c0 + q > 0) {
        const double aq = sa[q], eq = se[q];
        m1 = eq * fma(aq, m0, m1);
        m0 = eq * m0;
      }
      const int k1 = min(cnt[q], M);
      while (done < k1) {                            // (uniform) the part of one tile that enters at this step
        const int t = done >> 4, r1 = min(k1, 16 * (t + 1));
        if (t != have) {                             // the walk reaches the next tile: its entries were requested a tile ago
          deposit(t);
          if (t + 1 < nt) request(t + 1);
          __syncthreads();
          have = t;
        }
        const double* xr = xs[t & 1] + tid * AFT_LD;
        for (int r = done; r < r1; r++) {
          const int q16 = r & 15, i = side ? M - 1 - r : r;
          const double xl = xr[side ? 15 - q16 : q16];
          const double xv = (fac == 0 && i > j) ? 0.0 : xl;
          m0 = fma(xv, ew[r], m0);
          m1 = fma(xv, ea[r], m1);
        }
        done = r1;
      }
      if (act) {
        const int S = side ? ng - 1 - (c0 + q) : c0 + q;
        double* t = it.T + ((size_t)S * M + j) * 8 + fac * 4 + side * 2;
        t[0] = m0; t[1] = m1;
      }
    }
    rcarry = sref[nc - 1];
  }
}

// ---- the product on v_mfma_f64_16x16x4_f64 ---------------------------------------------------------
// A wavefront owns AF_COLS = 32 frames of one group and walks all M / 16 row tiles; a workgroup is four wavefronts on
// adjacent column blocks (they read the same tiles of W, C and T at the same time), eight wavefronts cover a group.  Per row
// tile and factor X (W, C) one contraction over the far field's four columns and the near rows:
//   A operand, lane (kq, lc):  far step  T[S][16 a + lc][fac * 4 + kq]              (k = Psi-0, Psi-1, Psi+0, Psi+1)
//                              near      X[16 a + lc][k0 + 2 kq], [k0 + 2 kq + 1]   one 16-byte load = k-steps s = 0, 1
//   B operand, lane (kq, lc):  far step  Psi[kq][n0 + 2 lc], [n0 + 2 lc + 1]         one 16-byte load = column tiles p = 0, 1
//                              near      Kuf[k0 + 2 kq + s][n0 + 2 lc], [+ 1]        (gemm_wave.hip's fragment order)
// so the accumulator of column tile p holds column n0 + 2 lc + p, rows 16 a + kq + 4 r: a store of A is 16 bytes per lane, 256
// bytes per row.  The B operand does not depend on the row tile: the first AF_CT = 2 near tiles (32 rows: every group of the
// usual layouts) and Psi stay in registers for the whole walk, further near tiles are read again per row tile from the strip,
// which the caches hold.  Any near-row count: nothing depends on what fits on chip.
// W is lower triangular: a 16 x 16 tile of W[:, near] wholly above the diagonal is skipped (wave-uniform), and in the tile on
// the diagonal the entries above it are MASKED in the registers — like afar_t_kernel, the product does not rely on what the
// buffer holds there.
// Column sums: a lane keeps running s1, s2 and dot for its two columns over its rows (ascending); the four lane quarters are
// added once at the end as ((q0 + q1) + q2) + q3.  A fixed order: two runs agree bit for bit.
// W, C and T go through buffer loads (scalar base and offset, one constant lane offset); the strips, which may pass 2 GiB,
// through 64-bit addresses; q_mu is copied to LDS once (8 KB at most, the kernel's only barrier).  The operands of row tile
// a + 1 are requested behind the MFMAs of row tile a and ahead of its stores.
typedef double af_d4 __attribute__((ext_vector_type(4)));
typedef double af_d2 __attribute__((ext_vector_type(2)));
typedef const af_d2 __attribute__((address_space(1))) * af_gc2;
typedef af_d2 __attribute__((address_space(1))) * af_g2;

#define AF_COLS 32           // frames per wavefront
#define AF_CT 2              // near 16-row tiles of the B operand a wavefront keeps in registers
#define AF_SB __builtin_amdgcn_sched_barrier(0)

struct AfFrag {              // the A operands of one row tile: near tiles t < AF_CT (two 8-deep chunks each), the far step
  af_d2 w[AF_CT][2], c[AF_CT][2];
  double tw, tc;
};

// the entries above the diagonal of the tile on it: lane (kq, lc) holds row lc, columns 8 h + 2 kq and the next one
static __device__ __forceinline__ void af_mask_diag(af_d2 (&w)[2], int lc, int kq) {
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int d = 8 * h + 2 * kq - lc;
    if (d > 0) w[h].x = 0.0;
    if (d + 1 > 0) w[h].y = 0.0;
  }
}

// one near tile (four k-steps) into both factors' accumulators; WF: the tile of W has entries on or below the diagonal
template <bool WF>
static __device__ __forceinline__ void af_tile(const af_d2 (&w)[2], const af_d2 (&c)[2], const af_d2 (&b)[2][2], af_d4 (&aw)[2], af_d4 (&ac)[2]) {
#pragma unroll
  for (int h = 0; h < 2; h++)
#pragma unroll
    for (int s = 0; s < 2; s++) {
      const double cf = s ? c[h].y : c[h].x, wf = s ? w[h].y : w[h].x;
      ac[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(cf, b[h][s].x, ac[0], 0, 0, 0);
      ac[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(cf, b[h][s].y, ac[1], 0, 0, 0);
      if (WF) {
        aw[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf, b[h][s].x, aw[0], 0, 0, 0);
        aw[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(wf, b[h][s].y, aw[1], 0, 0, 0);
      }
    }
}

__global__ void __launch_bounds__(256, 3) afar_prod_kernel(const AfarItem* __restrict__ items, int N) {
  const AfarItem it = items[blockIdx.y];
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lc = lane & 15, kq = lane >> 4;
  const int n0 = (blockIdx.x * 4 + wave) * AF_COLS, S = n0 / AFAR_GROUP, M = it.M, nt = M / 16;
  // (the range is the same for the whole wavefront: said so, the loop counters and the operand offsets stay in scalar registers)
  const int kbeg = __builtin_amdgcn_readfirstlane(it.rng[2 * S]), kend = __builtin_amdgcn_readfirstlane(it.rng[2 * S + 1]);
  const int ntile = (kend - kbeg) / 16, tb = kbeg / 16;
  const size_t ld = (size_t)it.ld;

  const __amdgpu_buffer_rsrc_t rW = __builtin_amdgcn_make_buffer_rsrc((void*)it.W, 0, M * M * 8, 0x00020000);
  const __amdgpu_buffer_rsrc_t rC = __builtin_amdgcn_make_buffer_rsrc((void*)it.C, 0, M * M * 8, 0x00020000);
  const __amdgpu_buffer_rsrc_t rT = __builtin_amdgcn_make_buffer_rsrc((void*)(it.T + (size_t)S * M * 8), 0, M * 64, 0x00020000);
  const int voffX = (lc * M + 2 * kq) * 8, voffT = (lc * 8 + kq) * 8;
  __shared__ double qs[1024];                                                      // q_mu (M <= 1024), read back in every epilogue
  for (int j = threadIdx.x; j < M; j += 256) qs[j] = it.q_mu[j];
  __syncthreads();

  // the B operand: Psi and the first AF_CT near tiles, for the whole walk
  const af_d2 Pf = *(af_gc2)(it.Psi + (size_t)kq * N + n0 + 2 * lc);
  const double* kp = it.Kuf + ((size_t)kbeg + 2 * kq) * ld + n0 + 2 * lc;          // row kbeg + 2 kq of the lane's two columns
  af_d2 Bc[AF_CT][2][2];
#pragma unroll
  for (int t = 0; t < AF_CT; t++)
#pragma unroll
    for (int h = 0; h < 2; h++)
#pragma unroll
      for (int s = 0; s < 2; s++) {
        Bc[t][h][s] = af_d2{0.0, 0.0};
        if (t < ntile) Bc[t][h][s] = *(af_gc2)(kp + (size_t)(16 * t + 8 * h + s) * ld);
      }

  // requests only: nothing here consumes a loaded value
  auto load_frag = [&](AfFrag& f, const int a) {
    const int so = (a * 16 * M + kbeg) * 8, ntw = min(a - tb + 1, ntile);
#pragma unroll
    for (int t = 0; t < AF_CT; t++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        f.c[t][h] = f.w[t][h] = af_d2{0.0, 0.0};
        if (t < ntile) f.c[t][h] = __builtin_bit_cast(af_d2, __builtin_amdgcn_raw_buffer_load_b128(rC, voffX + (16 * t + 8 * h) * 8, so, 0));
        if (t < ntw) f.w[t][h] = __builtin_bit_cast(af_d2, __builtin_amdgcn_raw_buffer_load_b128(rW, voffX + (16 * t + 8 * h) * 8, so, 0));
      }
    f.tw = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rT, voffT, a * 16 * 64, 0));
    f.tc = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rT, voffT + 32, a * 16 * 64, 0));
  };

  AfFrag f;
  load_frag(f, 0);

  af_g2 pA = (af_g2)(it.A + (size_t)kq * ld + n0 + 2 * lc);
  const af_d4 zero4 = {0.0, 0.0, 0.0, 0.0};
  double s1[2] = {0.0, 0.0}, s2[2] = {0.0, 0.0}, dot[2] = {0.0, 0.0};
  for (int a = 0; a < nt; a++) {
    const int ntw = min(a - tb + 1, ntile), tdiag = a - tb;       // tiles of W[16 a .. 16 a + 15, near] with anything in them
    af_d4 aw[2], ac[2];
    aw[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.tw, Pf.x, zero4, 0, 0, 0);
    aw[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.tw, Pf.y, zero4, 0, 0, 0);
    ac[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.tc, Pf.x, zero4, 0, 0, 0);
    ac[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(f.tc, Pf.y, zero4, 0, 0, 0);
#pragma unroll
    for (int t = 0; t < AF_CT; t++) {
      if (t < ntw) {
        if (t == tdiag) af_mask_diag(f.w[t], lc, kq);
        af_tile<true>(f.w[t], f.c[t], Bc[t], aw, ac);
      } else if (t < ntile) {
        af_tile<false>(f.w[t], f.c[t], Bc[t], aw, ac);
      }
    }
    for (int t = AF_CT; t < ntile; t++) {                          // more than 32 near rows: the strip again
      af_d2 b[2][2], w[2], c[2];
      const int so = (a * 16 * M + kbeg + 16 * t) * 8;
#pragma unroll
      for (int h = 0; h < 2; h++) {
#pragma unroll
        for (int s = 0; s < 2; s++) b[h][s] = *(af_gc2)(kp + ((size_t)16 * t + 8 * h + s) * ld);
        c[h] = __builtin_bit_cast(af_d2, __builtin_amdgcn_raw_buffer_load_b128(rC, voffX + 8 * h * 8, so, 0));
        w[h] = af_d2{0.0, 0.0};
        if (t < ntw) w[h] = __builtin_bit_cast(af_d2, __builtin_amdgcn_raw_buffer_load_b128(rW, voffX + 8 * h * 8, so, 0));
      }
      if (t < ntw) {
        if (t == tdiag) af_mask_diag(w, lc, kq);
        af_tile<true>(w, c, b, aw, ac);
      } else {
        af_tile<false>(w, c, b, aw, ac);
      }
    }
    AF_SB;
    load_frag(f, min(a + 1, nt - 1));                               // (behind the last row tile: that tile again, from the cache)
    AF_SB;
#pragma unroll
    for (int r = 0; r < 4; r++) {                                   // rows 16 a + kq + 4 r
      const double v0 = aw[0][r], v1 = aw[1][r];
      *pA = af_d2{v0, v1};
      pA += 2 * ld;
      s1[0] = fma(v0, v0, s1[0]); s1[1] = fma(v1, v1, s1[1]);
      const double q = qs[16 * a + kq + 4 * r];
      dot[0] = fma(v0, q, dot[0]); dot[1] = fma(v1, q, dot[1]);
      s2[0] = fma(ac[0][r], ac[0][r], s2[0]); s2[1] = fma(ac[1][r], ac[1][r], s2[1]);
    }
  }
  // the four lane quarters hold rows = 0, 1, 2, 3 (mod 4) of the same columns
#pragma unroll
  for (int p = 0; p < 2; p++) {
    double t1 = 0.0, t2 = 0.0, td = 0.0;
#pragma unroll
    for (int qq = 0; qq < 4; qq++) {
      const double u1 = __shfl(s1[p], lc + 16 * qq, 64), u2 = __shfl(s2[p], lc + 16 * qq, 64), ud = __shfl(dot[p], lc + 16 * qq, 64);
      t1 = qq ? t1 + u1 : u1; t2 = qq ? t2 + u2 : u2; td = qq ? td + ud : ud;
    }
    if (kq == 0) { const int n = n0 + 2 * lc + p; it.s1[n] = t1; it.s2[n] = t2; it.dot[n] = td; }
  }
}

// the tables' one launch (form 0: afar_t_kernel, 1: afar_t_tiled_kernel); launch_afar and gp_debug_far_tables (far_debug.hip)
void launch_afar_t(gp_handle h, const AfarItem* d_items, int count, int M, int n, bool tiled) {
  if (tiled) hipLaunchKernelGGL(afar_t_tiled_kernel, dim3((M + AFT_ROWS - 1) / AFT_ROWS, 4, count), dim3(AFT_ROWS), 0, h->stream, d_items, n);
  else hipLaunchKernelGGL(afar_t_kernel, dim3((M + 255) / 256, 4, count), dim3(256), 0, h->stream, d_items, n);
}

gp_status launch_afar(gp_handle h, const AfarItem* d_items, int count, int M, const double* x, int n) {
  if (count <= 0) return GP_OK;
  if (!afar_takes(M, n)) return gp_fail(h, GP_ERR_UNSUPPORTED, "activation far field: whole 256-frame groups, M a multiple of 16 up to 1024, strips of 2^20 entries or more");
  hipLaunchKernelGGL(afar_cols_kernel, dim3(n / AFAR_GROUP, count), dim3(AFAR_GROUP), 0, h->stream, d_items, x, n);
  launch_afar_t(h, d_items, count, M, n, gp_switches().far_tables != 0);
  GP_HIP_CHECK(h, hipGetLastError());
  {
    GpTimerScope ts(h, GP_TIMER_COND_A);
    hipLaunchKernelGGL(afar_prod_kernel, dim3(n / (4 * AF_COLS), count), dim3(256), 0, h->stream, d_items, n);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  return GP_OK;
}
