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
//   afar_prod_kernel  one workgroup per (group, GP), a thread per frame: Kuf[near, n] on chip, the rows walked eight at a time with
//                     W, C and T as wave-uniform operands; stores A and leaves the complete column sums colsum(A^2),
//                     colsum((C Kuf)^2) and A^T q_mu as ONE partial row each for cond_finish_kernel.
#include "engine.h"
#include <type_traits>

#define AF_KAPPA (1.0 - 1.5e-12)
#define AF_SQRT3 1.7320508075688772
#define AF_NKL 32            // near rows a workgroup keeps in LDS (two tiles: what the benchmark's groups have); more are re-read
#define AF_JB 8              // rows per register block of the product

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

// (pointers read out of an item are generic to the compiler.  AfG / AfGW say "global memory": plain global loads and stores.
// AfK says "global memory that no one writes while this kernel runs" — W, C, T and q_mu, which earlier launches of the stream
// left: their wave-uniform reads then take the scalar path, eight rows' operands per load, instead of one vector load per lane)
typedef __attribute__((address_space(1))) const double AfG;
typedef __attribute__((address_space(1))) double AfGW;
typedef __attribute__((address_space(4))) const double AfK;

// Eight rows j0 .. j0 + 7 of both products for the thread's frame.  kv: the thread's column of Kuf[near, S] — its own slots of the
// workgroup's LDS array (stride 256) or, beyond AF_NKL near rows, the stored strip itself (stride ld).  W, C, T are read at
// wave-uniform addresses.  The restrict qualifiers tell the compiler that the A stores leave them alone.
template <bool LDS>
static __device__ __forceinline__ void afar_rows(AfK* __restrict__ W, AfK* __restrict__ C, AfK* __restrict__ T8,
                                                 typename std::conditional<LDS, const double, AfG>::type* kv, size_t kstride, AfK* __restrict__ q_mu,
                                                 AfGW* __restrict__ Acol, size_t ld, int M, int kbeg, int kend,
                                                 const double psi[4], double& s1, double& s2, double& dot) {
  for (int j0 = 0; j0 < M; j0 += AF_JB) {
    double aw[AF_JB], ac[AF_JB];
#pragma unroll
    for (int r = 0; r < AF_JB; r++) {
      AfK* t = T8 + (size_t)(j0 + r) * 8;
      aw[r] = fma(t[3], psi[3], fma(t[2], psi[2], fma(t[1], psi[1], t[0] * psi[0])));
      ac[r] = fma(t[7], psi[3], fma(t[6], psi[2], fma(t[5], psi[1], t[4] * psi[0])));
    }
    for (int k = kbeg; k < kend; k += 2) {
      const double k0 = kv[(size_t)(k - kbeg) * kstride], k1 = kv[(size_t)(k - kbeg + 1) * kstride];
#pragma unroll
      for (int r = 0; r < AF_JB; r++) {
        AfK* cr = C + (size_t)(j0 + r) * M + k;
        ac[r] = fma(cr[1], k1, fma(cr[0], k0, ac[r]));
      }
    }
    // W is lower triangular: row j takes the rows k <= j only
    const int kf = min(kend, j0), kw = min(kend, j0 + AF_JB);
    for (int k = kbeg; k < kf; k += 2) {               // whole columns: k < j0
      const double k0 = kv[(size_t)(k - kbeg) * kstride], k1 = kv[(size_t)(k - kbeg + 1) * kstride];
#pragma unroll
      for (int r = 0; r < AF_JB; r++) {
        AfK* wr = W + (size_t)(j0 + r) * M + k;
        aw[r] = fma(wr[1], k1, fma(wr[0], k0, aw[r]));
      }
    }
    for (int k = max(kbeg, j0); k < kw; k += 2) {      // the diagonal block
      const double k0 = kv[(size_t)(k - kbeg) * kstride], k1 = kv[(size_t)(k - kbeg + 1) * kstride];
#pragma unroll
      for (int r = 0; r < AF_JB; r++) {
        AfK* wr = W + (size_t)(j0 + r) * M + k;
        const double w0 = (k <= j0 + r) ? wr[0] : 0.0, w1 = (k + 1 <= j0 + r) ? wr[1] : 0.0;
        aw[r] = fma(w1, k1, fma(w0, k0, aw[r]));
      }
    }
#pragma unroll
    for (int r = 0; r < AF_JB; r++) {
      Acol[(size_t)(j0 + r) * ld] = aw[r];
      s1 = fma(aw[r], aw[r], s1);
      s2 = fma(ac[r], ac[r], s2);
      dot = fma(aw[r], q_mu[j0 + r], dot);
    }
  }
}

__global__ void __launch_bounds__(AFAR_GROUP) afar_prod_kernel(const AfarItem* __restrict__ items, int N) {
  const AfarItem it = items[blockIdx.y];
  const int S = blockIdx.x, tid = threadIdx.x, n = S * AFAR_GROUP + tid, M = it.M;
  // (the range is the same for the whole workgroup: said so, the loop counters and the operand addresses stay in scalar registers)
  const int kbeg = __builtin_amdgcn_readfirstlane(it.rng[2 * S]), kend = __builtin_amdgcn_readfirstlane(it.rng[2 * S + 1]), nk = kend - kbeg;
  const size_t ld = (size_t)it.ld;
  __shared__ double kl[AF_NKL * AFAR_GROUP];         // [near row][frame]: a thread reads back only what it wrote itself — no barrier
  const double psi[4] = {it.Psi[n], it.Psi[(size_t)N + n], it.Psi[2 * (size_t)N + n], it.Psi[3 * (size_t)N + n]};
  const double* T8 = it.T + (size_t)S * M * 8;
  double s1 = 0.0, s2 = 0.0, dot = 0.0;
  if (nk <= AF_NKL) {
    for (int k = 0; k < nk; k++) kl[k * AFAR_GROUP + tid] = it.Kuf[(size_t)(kbeg + k) * ld + n];
    afar_rows<true>((AfK*)it.W, (AfK*)it.C, (AfK*)T8, kl + tid, AFAR_GROUP, (AfK*)it.q_mu, (AfGW*)(it.A + n), ld, M, kbeg, kend, psi, s1, s2, dot);
  } else {
    afar_rows<false>((AfK*)it.W, (AfK*)it.C, (AfK*)T8, (AfG*)(it.Kuf + (size_t)kbeg * ld + n), ld, (AfK*)it.q_mu, (AfGW*)(it.A + n), ld, M, kbeg, kend, psi, s1, s2, dot);
  }
  it.s1[n] = s1; it.s2[n] = s2; it.dot[n] = dot;
}

gp_status launch_afar(gp_handle h, const AfarItem* d_items, int count, int M, const double* x, int n) {
  if (count <= 0) return GP_OK;
  if (!afar_takes(M, n)) return gp_fail(h, GP_ERR_UNSUPPORTED, "activation far field: whole 256-frame groups, M a multiple of 16 up to 1024, strips of 2^20 entries or more");
  hipLaunchKernelGGL(afar_cols_kernel, dim3(n / AFAR_GROUP, count), dim3(AFAR_GROUP), 0, h->stream, d_items, x, n);
  hipLaunchKernelGGL(afar_t_kernel, dim3((M + 255) / 256, 4, count), dim3(256), 0, h->stream, d_items, n);
  GP_HIP_CHECK(h, hipGetLastError());
  {
    GpTimerScope ts(h, GP_TIMER_COND_A);
    hipLaunchKernelGGL(afar_prod_kernel, dim3(n / AFAR_GROUP, count), dim3(AFAR_GROUP), 0, h->stream, d_items, n);
    GP_HIP_CHECK(h, hipGetLastError());
  }
  return GP_OK;
}
