// kernfit.hip — learning a pitch's component kernel from its isolated-note recording (gpitch/samplecov.py,
// gpitch/kernelfit.py; the drivers' `init_kernel(train=True)` branch, transcription.py:176-195).
//
//   gp_segment_gram   C_b = (1/K) sum_k s_k s_k^T, s_k = y[start_{b,k} : start_{b,k} + L]    samplecov.py:5-53
//   gp_autocorr       r[j] = sum_{i < n-L} y[i] y[i+j]                                        samplecov.py:56-74
//   gp_kernfit_eval   RMSE of the Matern-3/2 x cosine-mixture fit and its analytic gradient   kernelfit.py:28-51
//
// Segment Gram.  C = S^T S with S the K x L matrix of segments; S is never built: lane (kq, lc) of a
// v_mfma_f64_16x16x4_f64 takes A[row lc][k kq] = y[start_k + row0 + lc] and B[k kq][col lc] = y[start_k + col0 + lc]
// straight from y (one buffer resource over the whole batch, L2-resident) through its segment's start.  A wavefront owns
// one 64 x 64 lower-triangle output tile (4 x 4 MFMA tiles, 128 accumulator registers) of one k-chunk of one recording,
// as in gemm_wave.hip; the four wavefronts of a workgroup are four tiles of the same (recording, chunk) and read the same
// segments at the same time (one fetch into the CU's L1).  A k-step of four segments costs one 16-byte load of four
// starts (per lane: k = k0 + 4 kq + u, u = 0..3 — any k order works as long as A and B agree), one address add, 8
// 8-byte loads and 16 MFMAs.  Rows and columns past L read whatever follows the segment in y (or 0 past the end of the
// buffer: buffer loads out of range return 0) and land only in accumulator rows / columns that are never read; the
// diagonal tile skips its 6 MFMA tiles above the diagonal.  k past K (the last group of 16) is masked to 0.
// Determinism: the chunk length is the constant SG_KC, so the chunk count ceil(K / SG_KC) depends on K alone (never on
// the device); partial tiles go to the caller's workspace with plain 8-byte global stores (not the buffer_store-with-
// scalar-offset form whose data registers can be read late: DESIGN.md section 3.00) and segment_gram_reduce_kernel sums
// them in chunk order, scales by 1/K and writes C[i][j] and C[j][i] from the same sum: C is exactly symmetric.
// 32-bit buffer offsets: y may hold at most GP_SEGMENT_GRAM_MAX_Y_BYTES (gpitch_abi.h); every offset stays below y's size + 512 bytes.
#include "common.h"
#include <type_traits>

typedef double d4 __attribute__((ext_vector_type(4)));
typedef int i4 __attribute__((ext_vector_type(4)));

#define SG_T 64                  // rows / columns of a wavefront's output tile
#define SG_KC 512                // segments per k-chunk (multiple of 16)
#define KF_MAX_PARTIALS 64

static inline int64_t sg_round_up(int64_t a, int64_t b) { return (a + b - 1) / b * b; }
static inline int sg_tiles(int L) { const int T = (L + SG_T - 1) / SG_T; return T * (T + 1) / 2; }
static inline int sg_chunks(int K) { return (K + SG_KC - 1) / SG_KC; }

__global__ __launch_bounds__(256) void segment_gram_kernel(const double* __restrict__ y, int64_t ny, const int* __restrict__ start,
                                                           int Kp, int K, int ntiles, int ntg, int nch, double* __restrict__ part) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x / (ntg * nch);
  const int c = (blockIdx.x / ntg) % nch;
  const int t = (blockIdx.x % ntg) * 4 + wave;
  if (t >= ntiles) return;                                 // wave-uniform; no barrier in this kernel
  int I = 0;
  while ((I + 1) * (I + 2) / 2 <= t) I++;
  const int J = t - I * (I + 1) / 2;
  const int lc = lane & 15, kq = lane >> 4;
  const int kbeg = c * SG_KC, kend = min(kbeg + SG_KC, K);

  const __amdgpu_buffer_rsrc_t ry = __builtin_amdgcn_make_buffer_rsrc((void*)y, 0, (int)(ny * 8), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((void*)(start + (int64_t)b * Kp), 0, Kp * 4, 0x00020000);
  const int soI = I * SG_T * 8, soJ = J * SG_T * 8;
  const int vs = 4 * kq * 4;                               // this lane's four starts: k0 + 4 kq + u

  d4 acc[4][4];
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int q = 0; q < 4; q++) acc[a][q] = d4{0.0, 0.0, 0.0, 0.0};

  // one group of 16 segments; MASK: the last group of a chunk, k >= kend contributes 0.  DIAG: skip MFMA tiles q > a.
  auto group = [&](int k0, auto mask_tag, auto diag_tag) {
    constexpr bool MASK = decltype(mask_tag)::value, DIAG = decltype(diag_tag)::value;
    const i4 s4 = __builtin_bit_cast(i4, __builtin_amdgcn_raw_buffer_load_b128(rs, vs, k0 * 4, 0));
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int vo = (s4[u] + lc) * 8;
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; a++) {
        av[a] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(ry, vo + a * 128, soI, 0));
        bv[a] = __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(ry, vo + a * 128, soJ, 0));
      }
      if (MASK) {
        const bool ok = k0 + 4 * kq + u < kend;
#pragma unroll
        for (int a = 0; a < 4; a++) av[a] = ok ? av[a] : 0.0;
      }
#pragma unroll
      for (int a = 0; a < 4; a++)
#pragma unroll
        for (int q = 0; q < 4; q++)
          if (!DIAG || q <= a) acc[a][q] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[q], acc[a][q], 0, 0, 0);
    }
  };
  using T_ = std::true_type;
  using F_ = std::false_type;
  int k0 = kbeg;
  if (I == J) {
    for (; k0 + 16 <= kend; k0 += 16) group(k0, F_{}, T_{});
    if (k0 < kend) group(k0, T_{}, T_{});
  } else {
    for (; k0 + 16 <= kend; k0 += 16) group(k0, F_{}, F_{});
    if (k0 < kend) group(k0, T_{}, F_{});
  }

  // C/D map of the f64 MFMA: column lane & 15, row (lane >> 4) + 4 reg
  double* pt = part + (((int64_t)b * nch + c) * ntiles + t) * (SG_T * SG_T);
#pragma unroll
  for (int a = 0; a < 4; a++)
#pragma unroll
    for (int q = 0; q < 4; q++)
#pragma unroll
      for (int r = 0; r < 4; r++) pt[(16 * a + kq + 4 * r) * SG_T + 16 * q + lc] = acc[a][q][r];
}

__global__ __launch_bounds__(256) void segment_gram_reduce_kernel(const double* __restrict__ part, int L, int K, int ntiles, int nch,
                                                                  int64_t total, double* __restrict__ C) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int64_t LL = (int64_t)L * L;
  const int64_t b = e / LL;
  const int i = (int)((e % LL) / L), j = (int)(e % L);
  const int ii = max(i, j), jj = min(i, j);
  const int It = ii / SG_T, Jt = jj / SG_T;
  const int t = It * (It + 1) / 2 + Jt;
  const double* p = part + ((b * nch) * ntiles + t) * (SG_T * SG_T) + (ii % SG_T) * SG_T + (jj % SG_T);
  double s = 0.0;
  for (int c = 0; c < nch; c++) s += p[(int64_t)c * ntiles * (SG_T * SG_T)];
  C[e] = (1.0 / K) * s;
}

// r[j] = sum_{i < n - L} y[i] y[i + j]: one workgroup per lag, a fixed stride per thread and a fixed tree
__global__ __launch_bounds__(256) void autocorr_kernel(const double* __restrict__ y, int64_t n, int L, double* __restrict__ r) {
  __shared__ double red[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  const int64_t N = n - L;
  double s = 0.0;
  for (int64_t i = tid; i < N; i += 256) s += y[i] * y[i + j];
  red[tid] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  if (tid == 0) r[j] = red[0];
}

__device__ __forceinline__ double kf_sign(double v) { return v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0); }

__device__ __forceinline__ double kf_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One wavefront per problem.  p and g rows (stride P = 2 + 2 m_max): [bias, lengthscale, v_1..v_m, f_1..f_m, padding]
// with m = npar[w] (the problem's own parameter vector first; the gradient's padding is written as 0).
//   k(x) = 0 |bias| + (1 + a) e^-a sum_i |v_i| cos(2 pi |f_i| |x|),  a = sqrt(3) |x| / |l|
//   f    = sqrt(mean((k - y)^2)),  df/dp = sign(p) sum_j (k_j - y_j) dk_j/d|p| / (n f);  df/dbias = 0
// Per-lane sums over the points j = lane + 64 t in order, per-partial sums in LDS slots [2 m_max][64], then one fixed
// butterfly per sum: a problem's result depends on nothing but its own row.
__global__ __launch_bounds__(64) void kernfit_eval_kernel(const double* __restrict__ x, const double* __restrict__ y, int64_t ld,
                                                          const int* __restrict__ npts, const int* __restrict__ npar, int m_max,
                                                          const double* __restrict__ p, double* __restrict__ f,
                                                          double* __restrict__ g, double* __restrict__ kout) {
  extern __shared__ double kf_acc[];                       // [2 m_max][64]: sum e env cos, sum e env |v| (-sin) 2 pi r
  const int w = blockIdx.x, lane = threadIdx.x;
  const int P = 2 + 2 * m_max;
  const int n = (int)min((int64_t)max(npts[w], 0), ld);
  const int m = min(max(npar[w], 0), m_max);
  const double* pw = p + (int64_t)w * P;
  const double* xw = x + (int64_t)w * ld;
  const double* yw = y + (int64_t)w * ld;
  const double bias = fabs(pw[0]), al = fabs(pw[1]);
  const double twopi = 2.0 * M_PI;
  for (int i = 0; i < 2 * m; i++) kf_acc[i * 64 + lane] = 0.0;
  double q = 0.0, gl = 0.0;
  for (int j = lane; j < n; j += 64) {
    const double r = fabs(xw[j]);
    const double a = sqrt(3.0) * r / al;
    const double ea = exp(-a);
    const double env = (1.0 + a) * ea;
    double S = 0.0;
    for (int i = 0; i < m; i++) S += fabs(pw[2 + i]) * cos(twopi * fabs(pw[2 + m + i]) * r);
    const double k = 0.0 * bias + env * S;
    if (kout) kout[(int64_t)w * ld + j] = k;
    const double e = k - yw[j];
    q += e * e;
    gl += e * S * (a * a * ea / al);
    const double ee = e * env, er = ee * twopi * r;
    for (int i = 0; i < m; i++) {
      double sn, cs;
      sincos(twopi * fabs(pw[2 + m + i]) * r, &sn, &cs);
      kf_acc[i * 64 + lane] += ee * cs;
      kf_acc[(m + i) * 64 + lane] -= er * fabs(pw[2 + i]) * sn;
    }
  }
  q = kf_wave_sum(q);
  gl = kf_wave_sum(gl);
  const double fv = n > 0 ? sqrt(q / n) : 0.0;
  const double sc = fv > 0.0 ? 1.0 / (n * fv) : 0.0;
  double* gw = g + (int64_t)w * P;
  for (int i = 0; i < 2 * m; i++) {
    const double s = kf_wave_sum(kf_acc[i * 64 + lane]);
    if (lane == 0) gw[2 + i] = kf_sign(pw[2 + i]) * s * sc;
  }
  if (lane == 0) {
    f[w] = fv;
    gw[0] = 0.0;
    gw[1] = kf_sign(pw[1]) * gl * sc;
    for (int i = 2 + 2 * m; i < P; i++) gw[i] = 0.0;
  }
}

extern "C" {

// gp_segment_gram's workspace: the tile partials of every (recording, chunk), the start table padded to 16 per recording
static double* segment_gram_carve(GpArena& ar, int B, int K, int L, int** st) {
  double* part = ar.take<double>((size_t)B * sg_chunks(K) * sg_tiles(L) * SG_T * SG_T);
  *st = ar.take<int>((size_t)B * sg_round_up(K, 16));
  return part;
}
size_t gp_segment_gram_workspace_bytes(int32_t B, int32_t K, int32_t L) {
  if (B < 1 || K < 1 || L < 1) return 0;
  int* st;
  return gp_measure([&](GpArena& ar) { segment_gram_carve(ar, B, K, L, &st); });
}

gp_status gp_segment_gram(gp_handle h, const double* y, int64_t ny, const int64_t* rec_off_host, const int64_t* rec_len_host,
                          int32_t B, const int32_t* start_host, int32_t K, int32_t L, double* C, void* workspace,
                          size_t workspace_bytes) {
  if (!h) return GP_ERR_BAD_ARG;
  if (!y || !rec_off_host || !rec_len_host || !start_host || !C || !workspace)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_segment_gram: null pointer");
  if (L < 1) return gp_fail(h, GP_ERR_BAD_ARG, "gp_segment_gram: L must be >= 1");
  if (K < 1) return gp_fail(h, GP_ERR_BAD_ARG, "gp_segment_gram: K must be >= 1");
  if (B < 1) return gp_fail(h, GP_ERR_BAD_ARG, "gp_segment_gram: B must be >= 1");
  if (ny < 1 || ny * 8 > GP_SEGMENT_GRAM_MAX_Y_BYTES)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_segment_gram: y must hold 1 .. (2^31 - 4096) / 8 doubles (32-bit buffer offsets); split the batch");
  if (workspace_bytes < gp_segment_gram_workspace_bytes(B, K, L))
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_segment_gram: workspace too small (gp_segment_gram_workspace_bytes)");
  for (int b = 0; b < B; b++) {
    const int64_t o = rec_off_host[b], n = rec_len_host[b];
    if (o < 0 || n < L || o + n > ny)
      return gp_fail(h, GP_ERR_BAD_ARG, "gp_segment_gram: recording outside y or shorter than L");
    const int32_t* s = start_host + (int64_t)b * K;
    for (int k = 0; k < K; k++)
      if (s[k] < o || (int64_t)s[k] + L > o + n)
        return gp_fail(h, GP_ERR_BAD_ARG, "gp_segment_gram: a segment lies outside its recording");
  }
  const int ntiles = sg_tiles(L), nch = sg_chunks(K), ntg = (ntiles + 3) / 4;
  const int Kp = (int)sg_round_up(K, 16);
  GpArena ar(workspace, workspace_bytes);
  int* st;
  double* part = segment_gram_carve(ar, B, K, L, &st);
  GP_HIP_CHECK(h, hipMemsetAsync(st, 0, (size_t)B * Kp * 4, h->stream));
  GP_HIP_CHECK(h, hipMemcpy2DAsync(st, (size_t)Kp * 4, start_host, (size_t)K * 4, (size_t)K * 4, B, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(segment_gram_kernel, dim3(B * nch * ntg), dim3(256), 0, h->stream, y, ny, st, Kp, K, ntiles, ntg, nch, part);
  GP_HIP_CHECK(h, hipGetLastError());
  const int64_t total = (int64_t)B * L * L;
  hipLaunchKernelGGL(segment_gram_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, h->stream, part, L, K, ntiles,
                     nch, total, C);
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}

gp_status gp_autocorr(gp_handle h, const double* y, int64_t n, int32_t L, double* r) {
  if (!h) return GP_ERR_BAD_ARG;
  if (!y || !r) return gp_fail(h, GP_ERR_BAD_ARG, "gp_autocorr: null pointer");
  if (L < 1) return gp_fail(h, GP_ERR_BAD_ARG, "gp_autocorr: L must be >= 1");
  if (n <= L) return gp_fail(h, GP_ERR_BAD_ARG, "gp_autocorr: the recording must be longer than L");
  hipLaunchKernelGGL(autocorr_kernel, dim3(L), dim3(256), 0, h->stream, y, n, L, r);
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}

gp_status gp_kernfit_eval(gp_handle h, int32_t W, const double* x, const double* y, int64_t ld, const int32_t* npts,
                          const int32_t* npar, int32_t m_max, const double* p, double* f, double* g, double* k) {
  if (!h) return GP_ERR_BAD_ARG;
  if (!x || !y || !npts || !npar || !p || !f || !g) return gp_fail(h, GP_ERR_BAD_ARG, "gp_kernfit_eval: null pointer");
  if (W < 1 || ld < 1) return gp_fail(h, GP_ERR_BAD_ARG, "gp_kernfit_eval: need W >= 1 and ld >= 1");
  if (m_max < 0 || m_max > KF_MAX_PARTIALS) return gp_fail(h, GP_ERR_BAD_ARG, "gp_kernfit_eval: m_max must be in [0, 64]");
  const size_t lds = (size_t)max(2 * m_max, 1) * 64 * sizeof(double);
  hipLaunchKernelGGL(kernfit_eval_kernel, dim3(W), dim3(64), lds, h->stream, x, y, ld, npts, npar, m_max, p, f, g, k);
  GP_HIP_CHECK(h, hipGetLastError());
  return GP_OK;
}

}  // extern "C"
