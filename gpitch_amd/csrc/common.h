// common.h — shared host/device declarations for libgpitch_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "../../include/gpitch_abi.h"
#include "switches.h"

#define GP_WAVE 64

// gpflow.transforms.Logistic(a, b) bounds registered on a handle (transform code = 3 + index)
#define GP_MAX_LOGISTIC 8
struct GpLogisticTable { double a[GP_MAX_LOGISTIC]; double b[GP_MAX_LOGISTIC]; };

struct gp_handle_s {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  std::string last_error;
  int32_t not_pd_index = -1;
  int32_t* d_status = nullptr;   // device int[4]: {flag (1 not PD, 2 cluster stalled, 3 frames not ascending, 4 qform guard, 5 hfar store), pivot / frame index, gp_index, spare}
  int num_cus = 256;
  GpLogisticTable logistic = {}; int num_logistic = 0;
  // helper stream for work that can overlap the main stream (the latency-bound Kuu factorisation runs on ~24 CUs
  // while the Kuf builds stream over the rest): created on first use, joined through events
  hipStream_t aux_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_mid = nullptr, ev_era = nullptr, ev_kuu = nullptr, ev_diag = nullptr, ev_q = nullptr, ev_guard = nullptr, ev_feat = nullptr;
  hipStream_t main_stream_saved = nullptr; bool aux_active = false, aux_pending = false, guard_pending = false;   // guard_pending: ev_guard is recorded and h->stream has not waited for it yet
  // second helper stream ("side"): one more independent piece of a step (the spectral-mixture Kuf-side contractions
  // underneath the second half of the Kuf_bar product); gp_side_begin / _end / _join
  hipStream_t side_stream = nullptr; hipEvent_t ev_side_fork = nullptr, ev_side_join = nullptr;
  hipStream_t side_saved = nullptr; bool side_active = false, side_pending = false;
  // gp_poll_not_pd: pinned landing zone of the status word, event behind its copy
  int32_t* poll_host = nullptr; hipEvent_t ev_poll = nullptr; bool poll_inflight = false;
  // timers
  bool timers_on = false;
  struct TimerRec { hipEvent_t e0, e1; int which; };
  std::vector<TimerRec> pending;
  std::vector<hipEvent_t> event_pool;
  double timer_ms[GP_TIMER_COUNT] = {0};
  int64_t timer_n[GP_TIMER_COUNT] = {0};
};

#define GP_HIP_CHECK(h, expr)                                                                  \
  do {                                                                                         \
    hipError_t _e = (expr);                                                                    \
    if (_e != hipSuccess) {                                                                    \
      char _b[512];                                                                            \
      snprintf(_b, sizeof(_b), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
               __LINE__);                                                                      \
      (h)->last_error = _b;                                                                    \
      return GP_ERR_HIP;                                                                       \
    }                                                                                          \
  } while (0)

#define GP_CHECK(expr)                   \
  do {                                   \
    gp_status _s = (expr);               \
    if (_s != GP_OK) return _s;          \
  } while (0)

static inline gp_status gp_fail(gp_handle h, gp_status s, const char* msg) {
  if (h) h->last_error = msg;
  return s;
}

// scoped timer for a kernel class; records HIP events on the handle's stream when enabled
// ---- lean device math for the covariance kernels -------------------------------------------------------------
// The M x N covariance builds and their gradient contraction are bound by float64 VALU issue, not by HBM (about 57
// instructions per entry with the library sqrt / exp).  Both functions below drop the range handling the arguments
// cannot need and stay within 1.5 ulp, far inside the 1e-9 parity bar.
// sqrt(x) for 1e-13 <= x <= 1e300 (a squared distance + 1e-12): v_rsq_f64, one Goldschmidt step and ONE residual
// correction, without the library's input scaling and class checks.  The library's second correction changes nothing
// here: 4.2 M arguments spread over [1e-12, 1e4] all come out correctly rounded after the first (tools/probe_f64_ops.hip
// has the instruction costs: v_rsq_f64 and v_max_f64 are quarter-rate, 17 and 14 cycles per wavefront against 4.75 for
// v_fma_f64).
__device__ __forceinline__ double gp_sqrt_pos(double x) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double e = fma(-h, g, 0.5);
  g = fma(g, e, g); h = fma(h, e, h);
  const double d = fma(-g, g, x);
  return fma(d, h, g);
}
// sqrt(x) and 1/sqrt(x) together (same argument range): the reciprocal costs one more correction step instead of a
// float64 division (~20 instructions) wherever a kernel needs both r and something / r.
__device__ __forceinline__ void gp_sqrt_rsqrt_pos(double x, double& s, double& rinv) {
  const double y = __builtin_amdgcn_rsq(x);
  double g = x * y, h = 0.5 * y;
  const double e = fma(-h, g, 0.5);
  g = fma(g, e, g); h = fma(h, e, h);
  const double d = fma(-g, g, x);
  g = fma(d, h, g);
  double r = h + h;
  r = fma(fma(-g, r, 1.0), r, r);
  s = g; rinv = r;
}
// table for gp_exp_neg: tab[j] = 2^(j/64), j < 64 (filled per workgroup into LDS by gp_exp_tab_init)
#define GP_EXP_TAB 64
__device__ __forceinline__ void gp_exp_tab_init(double* tab) {
  if (threadIdx.x < GP_EXP_TAB) tab[threadIdx.x] = exp2((double)threadIdx.x * (1.0 / 64.0));
}
// exp(x) for x <= 0: x = (64 q + j) ln2/64 + r, |r| <= ln2/128 -> 2^q * tab[j] * P5(r); x < -744 returns 0.
__device__ __forceinline__ double gp_exp_neg(double x, const double* __restrict__ tab) {
  x = fmax(x, -744.0);
  const double n = __builtin_rint(x * 92.33248261689366);             // 64 / ln2
  double r = fma(n, -0x1.62e42fe000000p-7, x);                         // ln2/64, high 29 bits (n * hi is exact)
  r = fma(n, -0x1.f473de6af278fp-36, r);                               // ln2/64, low part
  const int ni = (int)n;
  double p = fma(r, 1.0 / 120.0, 1.0 / 24.0);
  p = fma(p, r, 1.0 / 6.0);
  p = fma(p, r, 0.5);
  p = fma(p, r, 1.0);
  p = fma(p, r, 1.0);
  return ldexp(tab[ni & 63] * p, ni >> 6);
}

// kernel families (include/gpitch_abi.h gp_kernel_type)
#define GP_KERN_LAST GP_KERN_MERCER_MATERN52SM
static inline __host__ __device__ bool gp_kern_has_partials(int t) { return t >= GP_KERN_MERCER_MATERN12SM && t <= GP_KERN_LAST; }
// feature ("Mercer") form: K = var * env(r) * Phi(x)^T Phi(x'), r = euclid_dist
static inline __host__ __device__ bool gp_kern_is_mercer(int t) { return t == GP_KERN_MERCER_MATERN12SM || t == GP_KERN_MERCER_MATERN52SM; }
// broadcast form: r = |x - x' + 1e-12|, m cosines per entry
static inline __host__ __device__ bool gp_kern_is_broadcast(int t) { return t == GP_KERN_MATERN12SM || t == GP_KERN_MATERN32SM; }
// Kdiag = variance * sum_k energy_k (true) or just variance (false)
static inline __host__ __device__ bool gp_kern_kdiag_energy(int t) { return gp_kern_has_partials(t) && t != GP_KERN_MERCER_MATERN52SM; }

// Fork / join of the handle's helper stream (see gp_handle_s::aux_stream).  Between gp_aux_fork and gp_aux_end the
// launchers (which enqueue on h->stream) target the helper stream; gp_aux_join makes the main stream wait for it.
// gp_aux_fork returns false (and changes nothing) when no helper stream can be had: the work then stays in line.
bool gp_aux_fork(gp_handle h);
// after gp_aux_end and before gp_aux_join: hand the helper stream more work that depends on what the main stream has
// enqueued so far (returns false when there is no pending fork)
bool gp_aux_resume(gp_handle h);
gp_status gp_aux_end(gp_handle h);
gp_status gp_aux_join(gp_handle h);
// the same for the second helper stream: between gp_side_begin (true on success) and gp_side_end the launchers target it;
// the work there starts after everything enqueued on the current stream so far; gp_side_join makes the current stream wait
bool gp_side_begin(gp_handle h);
gp_status gp_side_end(gp_handle h);
gp_status gp_side_join(gp_handle h);
// body() with the launchers on the side stream, when `want` and the stream is to be had: *taken says whether it ran there.
// Where it did not, nothing was enqueued and the caller runs the work in line, there or later.  Returns body's status,
// or else gp_side_end's.
template <typename Body>
static inline gp_status gp_on_side(gp_handle h, bool want, bool* taken, Body body) {
  *taken = want && gp_side_begin(h);
  if (!*taken) return GP_OK;
  const gp_status st = body();
  const gp_status se = gp_side_end(h);
  return st != GP_OK ? st : se;
}
// The launchers target `s` (null: where they are) while this object lives, and h->stream is restored on every path out.  For
// work handed to the helper stream by an event of the caller's own, outside a gp_aux_fork / gp_aux_end pair.
struct GpStreamScope {
  gp_handle h;
  hipStream_t saved;
  GpStreamScope(gp_handle h_, hipStream_t s) : h(h_), saved(h_->stream) { if (s) h->stream = s; }
  ~GpStreamScope() { h->stream = saved; }
  GpStreamScope(const GpStreamScope&) = delete;
  GpStreamScope& operator=(const GpStreamScope&) = delete;
};

struct GpTimerScope {
  gp_handle h;
  int which;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  GpTimerScope(gp_handle h_, int which_);
  ~GpTimerScope();
};

static inline size_t gp_align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// simple bump allocator over a caller-provided workspace
struct GpArena {
  char* base = nullptr;
  size_t size = 0, off = 0;
  bool ok = true;
  GpArena(void* p, size_t n) : base((char*)p), size(n) {}
  template <typename T>
  T* take(size_t count) {
    size_t bytes = gp_align_up(count * sizeof(T), 256);
    if (off + bytes > size) { ok = false; return nullptr; }
    T* r = base ? (T*)(base + off) : nullptr;     // no base: the arena only measures (`off` = bytes asked for)
    off += bytes;
    return r;
  }
};
// Every caller-allocated workspace is laid out by ONE carve function (a list of take() calls); its *_workspace_bytes is
// that same function run on an arena without memory (gp_measure), plus a trailing margin.
template <typename Carve>
static inline size_t gp_measure(Carve carve) { GpArena ar(nullptr, SIZE_MAX); carve(ar); return ar.off; }
// (a descriptor block's layout function walks its regions with this: region(bytes) -> offset, `off` = total so far)
struct GpRegions {
  size_t off = 0;
  size_t operator()(size_t bytes) { const size_t o = off; off += gp_align_up(bytes, 256); return o; }
};
// Trailing margins behind the measured carve: nobody has shown that no kernel reads a few bytes past its last buffer
// (padded vector loads at a strip's end), so each family keeps the slack it always had.
static const size_t GP_WS_TAIL_BATCH = 256;    // pdgp_batch.hip plans
static const size_t GP_WS_TAIL_CHOL = 512;     // chol.hip's blocked factorisations
static const size_t GP_WS_TAIL_OP = 4096;      // one-shot operators, the SGPR plan
static const size_t GP_WS_TAIL_PLAN = 8192;    // Pdgp plan, window-batched SGPR plan and its source prediction

// ---------------------------------------------------------------------------------------------
// device-side kernel descriptor (passed by value in kernel args)
struct DevKern {
  int type;
  int m;
  const double* theta;  // [variance, lengthscales, e_0.., f_0..]
};
static inline DevKern dev_kern(const gp_kernel_desc* k) { return DevKern{k->type, k->num_partials, k->theta}; }
// The record a kernel works on: `one` by value for a single problem, or entry `idx` of a device array for a family.
// (A copy under a branch, not `items ? items[idx] : one`: with the select between the kernel-argument segment and global
// memory, cov_build_kernel compiled to 5-30 more VGPRs and lost a wavefront of occupancy at most partial counts; this form
// compiles to the register counts the kernels had with every field as an argument of its own.)
template <typename T>
__device__ __forceinline__ T gp_item(const T& one, const T* __restrict__ items, unsigned idx) {
  T it = one;
  if (items) it = items[idx];
  return it;
}

// ---------------------------------------------------------------------------------------------
// launchers implemented across the .hip files (all enqueue on h->stream)

// cov.hip
// f32out != 0: `out` is a float32 matrix (ld in floats) — the strips of a float32 plan; the arithmetic stays float64
gp_status launch_kernel_build(gp_handle h, DevKern k, const double* x1, int n1, const double* x2, int n2,
                              double* out, int64_t ld, int accumulate, double diag_add, double* feat_ws, int feat_ready = 0,
                              int f32out = 0);
size_t kernel_build_feat_ws_doubles(int m, int n1, int n2);
int sm_mpad(int m);  // spectral-mixture partial count padded to a multiple of 4 (feature tables are zero-padded)
gp_status launch_kernel_diag(gp_handle h, DevKern k, int n, double* out, int accumulate);
gp_status launch_sm_features(gp_handle h, DevKern k, const double* x1, int n1, const double* x2, int n2, double* feat_ws);

// chol.hip
gp_status launch_cholesky_batched(gp_handle h, double* const* d_mats, const int* d_M, const int* d_ld, int batch,
                                  int maxM, int pivot_base = 0);
gp_status launch_cholesky_single(gp_handle h, double* A, int M, int64_t ld, int pivot_base = 0);
// one large matrix, blocked over the GEMM kernels: A -> L in place (lower), W = L^-1 (upper part zero); ld even
size_t cholesky_large_workspace_bytes(int N);
size_t cholesky_large_batched_workspace_bytes(int N, int count);
// one M x M matrix, 128 < M <= 1024: factor from one one-workgroup launch, inverse blocked over 128-column panels
// (descriptors prepared once for fixed buffers; run = launches only)
size_t chol_inverse_blocked_workspace_bytes(int M);
gp_status chol_inverse_blocked_prepare(gp_handle h, double* A, double* W, int M, int64_t ld, void* ws, size_t ws_bytes);
gp_status chol_inverse_blocked_run(gp_handle h, int M, int64_t ld, void* ws, size_t ws_bytes);
// host arrays of `count` device pointers: every launch of the blocked factorisation + inverse runs over all matrices
gp_status launch_cholesky_large_batched(gp_handle h, double* const* A, double* const* W, int count, int N, int64_t ld,
                                        void* ws, size_t ws_bytes);
gp_status launch_cholesky_large(gp_handle h, double* A, double* W, int N, int64_t ld, void* ws, size_t ws_bytes);
gp_status launch_tri_inverse_single(gp_handle h, const double* L, double* Linv, int M, int64_t ld);
// Cholesky factor (in place) and its inverse in one launch, one resident workgroup per matrix
gp_status launch_cholesky_inverse_batched(gp_handle h, double* const* d_mats, double* const* d_W, const int* d_M,
                                          const int* d_ld, int batch, int maxM);
// ... with d_outcome[b] = 0 or 1 + first bad pivot per matrix instead of the handle's status word; slots of size 0 are skipped
gp_status launch_cholesky_inverse_batched_outcome(gp_handle h, double* const* d_mats, double* const* d_W, const int* d_M,
                                                  const int* d_ld, int batch, int maxM, int32_t* d_outcome);
gp_status launch_cholesky_inverse_single(gp_handle h, double* A, double* W, int M, int64_t ld);
gp_status launch_zero_upper_blocks_batched(gp_handle h, double* const* d_mats, const int* d_M, const int* d_ld, int batch,
                                           int maxM, int nb);
gp_status check_not_pd(gp_handle h);  // syncs; turns the device flag into GP_ERR_NOT_PD
// chol_cluster.hip: one matrix by a cluster of workgroups (factor in place, W = L^-1 when W is given), one launch; false =
// not a launch the cluster takes (shape, switch, exchange area not allocatable inside a stream capture)
bool cholesky_cluster_takes(int M, int count);
bool launch_cholesky_cluster_single(gp_handle h, double* A, double* W, int M, int64_t ld, int pivot_base, gp_status* st);
bool launch_cholesky_cluster_batched(gp_handle h, double* const* d_mats, double* const* d_W, const int* d_M, const int* d_ld,
                                     int count, int minM, int maxM, gp_status* st);
void cholesky_cluster_release(gp_handle h);

// gemm.hip
struct GemmProblem {
  const double* A; const double* B; double* C;
  int M, N, K;
  int64_t lda, ldb, ldc;
  // epilogue / prologue extras (meaning depends on the launch variant)
  const double* v0; const double* v1; const double* v2;
  double* o0; double* o1; double* o2;
  DevKern kern;           // for epilogues that re-evaluate the covariance (hyper-gradient)
  const double* xa; const double* xb;  // kernel inputs (z, x) for those epilogues
  int a_f32;              // small vector kernels (rowdot): A is a float32 strip (lda in floats)
  int pad_;
};
enum GemmTri { TRI_NONE = 0, TRI_LOWER = 1, TRI_UPPER = 2 };
struct GemmFlags {
  int transA = 0, transB = 0;
  int triA = TRI_NONE;   // structure of op(A) (M x K)
  int triB = TRI_NONE;   // structure of op(B) (K x N)
  int triC = TRI_NONE;   // TRI_LOWER: tiles strictly above the diagonal are skipped, upper part zeroed
  double alpha = 1.0, beta = 0.0;
  int big_tiles = 0;     // 128x128 tiles (strip GEMMs) instead of 64x64
  int epilogue = 1;      // bitmask of GemmEpi
  int scale_mode = 0;    // 0 none; 1: opB(B)(k,n) *= v1[n]; 2: opB(B)(k,n) *= v1[k]
  int timer = GP_TIMER_SMALL_GEMM;
  int role = 0;          // 1 cond_A, 2 cond_LTA (needs transA), 3 kuf_bar: dedicated 128x128 instantiations; 6 G = Q Kuf, 7 the same from near rows + far field (gemm_wave.hip only)
  int tile_m0 = 0, tile_mcount = 0;   // strip products (big tiles, no split-K): only row-blocks [m0, m0 + mcount) (0 = all)
  const double* aux_x = nullptr;      // role 5 (gemm_strip.hip): the frames x of the batch; aux_ktype: the stationary kernel type
  int aux_ktype = -1;
  int aux_nf = 0;                     // role 7 (gemm_wave.hip): features per point of the far field, 2 sm_mpad(m)
  int uniform_aligned = 0;            // the caller vouches: every problem has M = maxM (= K structure), N = maxN, 16-byte
                                      // aligned operands with even leading dimensions (gemm_strip.hip's lean form)
  int a32_ok = 0;                     // float32 strips (gemm_wave_f32.hip): every problem's xb = M * M floats of scratch for the M x M operand
  int rows64_ok = 0;                  // roles 1, 2: the caller has sized o0 / o1 for one partial row per 64-ROW tile and asked
                                      // gemm_wave_takes() how many rows the launch will write (gemm_wave.hip)
};
// gemm_wave.hip: the strip products without LDS or barriers, a 64 x 64 tile per wavefront (true = taken, status in *st)
bool launch_gemm_wave(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int maxN, const GemmFlags& f, gp_status* st);
bool gemm_wave_takes(int role, int maxM, int maxN, int uniform_aligned);
int gemm_fused_contraction_records(int maxM, int maxN, int ktype);
// gemm_wave_f32.hip: the same for float32 strips
bool launch_gemm_wave_f32(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int maxN, const GemmFlags& f, gp_status* st);
bool gemm_wave_f32_takes(int role, int maxM, int maxN, int uniform_aligned);
bool launch_gemm_strip_lean(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int maxN, const GemmFlags& f,
                            gp_status* st);
bool gemm_strip_fused_contraction_ok(int maxM, int maxN, int ktype);
bool gemm_f32_fused_contraction_ok(int maxM, int maxN, int ktype);     // gemm_f32.hip: the same for float32 strips
enum GemmEpi {
  EPI_STORE = 1,     // C = alpha*acc + beta*C
  EPI_COLSUMSQ = 2,  // o0[rowblk*N + n] = sum over the tile's rows of (alpha*acc)^2
  EPI_COLDOT = 4     // o1[rowblk*N + n] = sum over the tile's rows of alpha*acc * v0[row]
};
// Batched: d_probs is a device array of `batch` problems; maxM/maxN bound the grid.
gp_status launch_gemm_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int maxN,
                              const GemmFlags& f);
// H = (X * diag(d)) * Y^T over the long dimension with split-K partial slabs + reduction (deterministic).
//   prob.A = X (M x Nlong, lda), prob.B = Y (M x Nlong, ldb), prob.v1 = d (Nlong, when scale_by_k), prob.C = H (M x M, ldc)
//   prob.M = prob.N = M, prob.K = Nlong; prob.o2 = slab workspace (nsplit * M * M doubles).  Only the lower triangle is computed when sym != 0
//   (upper mirrored).
// uniform_aligned != 0: every problem has M = maxM, K = maxNlong, 16-byte aligned rows (gemm_strip.hip's lean form)
gp_status launch_gemm_nt_reduce_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int maxNlong,
                                        int nsplit, int sym, int scale_by_k, double alpha, int uniform_aligned = 0);
bool launch_gemm_strip_f32_lean(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int maxN, const GemmFlags& f,
                                gp_status* st);
bool gemm_strip_nt_lean_takes(int M, int Nlong, int nsplit);     // would launch_gemm_strip_nt_lean take the shape?
bool launch_gemm_strip_nt_lean(gp_handle h, const GemmProblem* d_probs, int batch, int M, int Nlong, int nsplit, int sym,
                               int scale_by_k, gp_status* st);
gp_status launch_tri_inverse_batched(gp_handle h, const double* const* d_L, double* const* d_W, const int* d_M,
                                     const int* d_ld, int batch);
// scopes launch_gemm_nt_reduce_batched opens under the split-K product's timer for this shape: one for the lean form it tries
// first and, where that does not take the shape, one more for the form it falls back to
int gemm_nt_reduce_charges(int maxM, int maxNlong, int nsplit, int uniform_aligned);
int gemm_nt_nsplit(int M, int Nlong, int batch);
gp_status launch_slab_reduce(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int nsplit, int sym, double alpha);
// gemm_f32.hip: the strip products on float32 strips (roles 1-3: A float64 M x M, B / C float32 strips; nt: float32
// strips, float64 slabs).  Same descriptor struct; ldb / ldc (and lda for nt) count floats.
gp_status launch_gemm_f32_role(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int maxN, const GemmFlags& f);
gp_status launch_gemm_f32_nt_reduce_batched(gp_handle h, const GemmProblem* d_probs, int batch, int maxM, int maxNlong,
                                            int nsplit, int sym, int scale_by_k, double alpha, int uniform_aligned = 0);
// leading dimension (in elements) of an M x N strip: even for float64, a multiple of 4 for float32 (16-byte rows)
static inline int64_t gp_strip_ld(int N, bool f32) { return f32 ? (((int64_t)N + 3) & ~(int64_t)3) : (((int64_t)N + 1) & ~(int64_t)1); }
// the wave forms (gemm_wave.hip, gemm_wave_f32.hip) address their strips through buffer resources: 32-bit byte offsets
// and num_records = 2^31 - 1.  An M x ld strip of 2^31 bytes or more would be read as zeros and stored partly nowhere, so
// such a strip takes the strip forms (64-bit addresses).
static inline bool gp_strip_below_2gib(int M, int N, bool f32) {
  return (int64_t)M * gp_strip_ld(N, f32) * (f32 ? 4 : 8) < ((int64_t)1 << 31);
}
// doubles that hold an M x ld strip of either type
static inline size_t gp_strip_doubles(size_t M, int N, bool f32) {
  const size_t e = M * (size_t)gp_strip_ld(N, f32);
  return f32 ? (e + 1) / 2 : e;
}
int gemm_rowblocks(int M, int big_tiles);

// grouped covariance builds (cov.hip): one launch for all matrices of a kernel family
struct CovItem {
  DevKern k; const double* x1; const double* x2; double* out; const double* f1; const double* f2;
  int64_t ld; double diag_add; int n1, n2, accumulate, vec_ok;
  int f32out, pad_;     // out is float32 (ld in floats)
};
struct FeatItem { DevKern k; const double* x; double* f; int n; int pad; };
// one pass for K = sum of P MercerMatern12sm kernels (cov.hip; true = taken, status in *st)
bool launch_kernel_build_sum(gp_handle h, const DevKern* kernels, double* const* feats, int P, const double* x1, int n1,
                             const double* x2, int n2, double* out, int64_t ld, double diag_add, int f32out, gp_status* st);
void cov_item_fill(CovItem* it, DevKern k, const double* x1, int n1, const double* x2, int n2, double* out, int64_t ld,
                   int accumulate, double diag_add, double* feat_ws, int f32out = 0);
gp_status launch_sm_features_items(gp_handle h, const FeatItem* d_items, int count, int max_n, int mpad,
                                   const double* x_shared, int n_shared);
// engine_strips != 0: the caller vouches that every item writes an engine strip of the shared frames (item.n2 < 0, 256-byte
// aligned output, leading dimension gp_strip_ld) — what the lean Mercer form needs to know on the host
gp_status launch_kernel_build_items(gp_handle h, int type, int m, const CovItem* d_items, int count, int max_n1,
                                    int max_n2, const double* x2_shared, int n2_shared, int engine_strips = 0);
// the kernel that launch takes (host only, no device work): form 0 generic, 1 staged matrix-core, 2 lean matrix-core; forms 1
// and 2 split every record's rows into segments of row_seg rows (nseg: the doubling count behind row_seg)
struct CovItemsForm { int form, nseg, row_seg; };
CovItemsForm cov_items_form(int type, int m, int count, int max_n1, int max_n2, bool x2_shared, int n2_shared, int engine_strips);
// predict_sparse.hip: the sparse per-source posterior (gp_sgpr_predict_source_sparse), one fused launch over
// (frame tile, source, window).  One item per (source, window), kernel-major [P][nwin]: the window's forward state
// (W = chol(Kuu)^-1 and WB = chol(B)^-1 with leading dimension ldw, c), its kz inducing points z with the kernel's feature
// table fz ([2 sm_mpad(m)][kz], Mercer kernels only), the window's n new frames and the source's two output rows.
#define SPS_MAX_M 1024
struct SrcSparseItem {
  DevKern k; const double* z; const double* fz; const double* W; const double* WB; const double* c;
  const double* xnew; double* mean; double* var; int kz, ldw;
};
gp_status launch_sgpr_source_sparse(gp_handle h, const SrcSparseItem* d_items, int P, int nwin, int M, int n, int max_mpad);
// sample.hip, core: the state-space sampler of a list of independent processes (prior walk along the merged points, update
// draw(x*) = prior(x*) + K(x*, z) beta), shared by the operators below and by pdgp_batch.hip's gp_pdgpb_sample.  One record per
// sampled process: everything the prior and update kernels read.
struct SsmProc {
  DevKern k;
  const double* z; const double* xnew;
  const double* fz; const double* fx;     // sqrt(e) cos / sin tables of z ([2 mp][kz]) and of xnew ([2 mp][n]); SM kernels only
  const int* order;                       // the process's merged order, n + kz entries (validated on the host)
  const double* eps_x; const double* eps_z;   // draw 0 of this process's component block: [S][cs][n] and [S][cs][ezs]
  const double* beta;                     // [kz][S]
  double* out;                            // [S][n]
  double* pz;                             // prior(z): [kz][S]
  int n;                                  // the process's own frame count
  int kz, mp;                             // mp: sm_mpad(m) of an SM kernel, else 0
  int cs, ezs;                            // components between two draws; points between two components of eps_z
};
// the owner of entry b of a work list: the last g with start[g] <= b (start ascending, count + 1 items, the last the total)
__device__ __forceinline__ int gp_entry_owner(const int64_t* __restrict__ start, int count, int64_t b) {
  int lo = 0, hi = count;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (start[mid] <= b) lo = mid; else hi = mid;
  }
  return lo;
}
int ssm_components(int type, int m);      // standard normals per point: 1 Matern12, 2 Matern32, 2 m a Matern-1/2 spectral mixture
int ssm_mpad(DevKern k);                  // sm_mpad(m) of a spectral-mixture kernel, else 0
// A call's descriptor block: procs | the operator's own records | feature items (at most two per process) | GEMM problems |
// the update's tile list (nproc + 1 items)
struct SsmDesc { size_t procs, recs, feat, probs, tiles, bytes; };
SsmDesc ssm_desc_layout(size_t nproc, size_t rec_bytes, size_t nprob);
// fills the tile list of the host block hd from the processes' n and kz (T = the update's frames per tile at maxM); returns the entries
int64_t ssm_fill_tiles(const SsmDesc& lay, std::vector<char>& hd, int count, int maxM);
struct SsmSpan { size_t off; int len; };  // `order` becomes device addresses: every span's entries must be a permutation of 0..len-1
gp_status ssm_check_orders(gp_handle h, const int32_t* order_host, const std::vector<SsmSpan>& spans, const char* not_a_permutation);
// Uploads the block (hd: its host copy, the first nfeat feature items filled in any order) and `order`, then builds the feature tables
gp_status ssm_upload(gp_handle h, const SsmDesc& lay, std::vector<char>& hd, char* d_desc, int nfeat, const int32_t* order_host,
                     int* d_order, size_t norder, int max_n);
// d_procs: count <= 32767 processes, none with more than maxM inducing inputs; max_mpad: the largest mp among them
gp_status ssm_launch_prior(gp_handle h, const SsmProc* d_procs, int count, int S, int max_mpad, const char* unsupported);
gp_status ssm_launch_update(gp_handle h, const SsmDesc& lay, const char* d_desc, int count, int64_t entries, int maxM, int S,
                            int max_mpad, const char* unsupported);
// sample.hip, SGPRSS section: joint posterior draws of every source under the sparse posterior's q(u) (gp_sgpr_sample_source_sparse,
// gp_sgprb_sample_source_sparse).  The two entries describe their windows on the host — a window's forward state and inputs,
// and per (window, source) the kernel and the plan's Z feature table (nullptr: the plan keeps none for this kernel) — check
// every argument with sgpr_sample_check BEFORE anything is enqueued, run their forward pass, then call sgpr_sample_run.
struct SmpWindow { const double* z; const double* W; const double* WB; const double* c; const double* xnew; int kz; };
struct SmpSource { DevKern k; const double* fz; };
size_t sgpr_sample_workspace_bytes(int M, int P, int C, int n, int S, int count);
// kw: inducing points per window (nullptr: M each); order_host: [count][n + M], a slot's first n + k entries checked to be a
// permutation of 0..n+k-1 (a bad index must never become a device address)
gp_status sgpr_sample_check(gp_handle h, const int* ktype, const int* km, int P, int M, const int* kw, int count, int n, int S,
                            const int32_t* order_host, const void* ws, size_t ws_bytes, int* C_out);
gp_status sgpr_sample_run(gp_handle h, const SmpWindow* win, const SmpSource* src, int count, int P, int M, int ldw, int n, int S,
                          double jitter, const int32_t* order_host, const double* eps_x, const double* eps_z, const double* eps_u,
                          double* out, void* ws, size_t ws_bytes);
// sample.hip, Pdgp section: joint posterior draws of every latent GP and source of a Pdgp plan (gp_pdgp_sample, gp_pdgp_sample_reuse).
// The entry describes the plan's latent GPs on the host (engine order [g_0..g_{P-1}, f_0..f_{P-1}]; z, W, q_mu, q_sqrt are
// device pointers), checks every argument with pdgp_sample_check BEFORE anything is enqueued, factorises, then runs.
struct PsmGP { DevKern k; const double* z; const double* W; const double* q_mu; const double* q_sqrt; int M; };
size_t pdgp_sample_workspace_bytes(int G, int maxM, int C, int n, int S);
// order_host: the GPs' merges back to back, GP r's n + M_r entries checked to be a permutation of 0..n+M_r-1
gp_status pdgp_sample_check(gp_handle h, const PsmGP* gps, int G, int n, int S, const int32_t* order_host, const void* ws,
                            size_t ws_bytes);
gp_status pdgp_sample_run(gp_handle h, const PsmGP* gps, int P, bool whiten, int nlin, double jitter, const double* xnew, int n,
                          int S, const int32_t* order_host, const double* eps_x, const double* eps_z, const double* eps_u,
                          double* latents, double* sources, void* ws, size_t ws_bytes);
// ssm_smooth.hip: the exact per-source posterior of SGPRSS windows by a Kalman filter and a Bryson-Frazier backward pass
// (gp_sgpr_predict_source_ssm, gp_sgprb_predict_source_ssm).  Every argument is checked before anything is enqueued.  Window
// w < count: params + w * param_stride, X / Y + w * N, Xnew + w * n, order_host + w * (N + n) (its first steps_host[w] entries),
// out_step_host + w * n, mean / var + w * P * n, loglik + w.  Synchronises.
size_t ssm_smooth_workspace_bytes(int d, int steps, int P, int count);
size_t ssm_score_workspace_bytes(int d, int steps, int P, int count);
gp_status ssm_score_run(gp_handle h, const int* ktype, const int* km, const int64_t* off_theta, int P, int64_t param_stride,
                        const double* params, const double* X, const double* Y, int N, int count, const int32_t* order_host,
                        double* loglik, double* grad, double* resid_grad, void* ws, size_t ws_bytes);
gp_status ssm_smooth_run(gp_handle h, const int* ktype, const int* km, const int64_t* off_theta, int P, int64_t param_stride,
                         const double* params, const double* X, const double* Y, int N, const double* Xnew, int n, int count,
                         const int32_t* order_host, const int32_t* out_step_host, const int32_t* steps_host, double* mean,
                         double* var, double* loglik, void* ws, size_t ws_bytes);
// joint draws from the same posterior by the simulation smoother (gp_sgpr_sample_source_ssm, gp_sgprb_sample_source_ssm): window w's
// eps_x + w * S * steps * d ([S][steps][d], `steps` the call's longest timeline), eps_y + w * S * N, out + w * P * S * n ([P][S][n])
size_t ssm_sample_workspace_bytes(int d, int steps, int P, int S, int count);
gp_status ssm_sample_run(gp_handle h, const int* ktype, const int* km, const int64_t* off_theta, int P, int64_t param_stride,
                         const double* params, const double* X, const double* Y, int N, const double* Xnew, int n, int count,
                         const int32_t* order_host, const int32_t* out_step_host, const int32_t* steps_host, int S,
                         const double* eps_x, const double* eps_y, double* out, void* ws, size_t ws_bytes);
gp_status launch_overlap_merge(gp_handle h, const double* y, int nw, int ws, int64_t ldy, int n, int square, double* out);
// lik.hip
// whitened KL: each item writes GP_KL_BLOCKS partial sums to out[0..GP_KL_BLOCKS)
#define GP_KL_BLOCKS 16
int mpd_lik_blocks(int N);   // block partials (2 doubles each) one launch over N frames leaves
// lik.hip: posterior moments of the sources / mixture and the expected log density (gp_mpd_predict_moments); Fmu/Fvar element
// (frame n, column c) at [n * f_rs + c * f_cs]; smean / svar P x N row-major; any output may be NULL; yvar takes the noise variance when add_noise
gp_status launch_mpd_moments(gp_handle h, const double* Fmu, const double* Fvar, int64_t f_rs, int64_t f_cs, const double* y,
                             int N, int P, int nlin, const double* noise_var, int add_noise, double* smean, double* svar,
                             double* ymean, double* yvar, double* logp);
gp_status launch_mpd_lik(gp_handle h, const double* Fmu, const double* Fvar, int64_t f_rs, int64_t f_cs,
                         const double* y, int N, int P, int nlin, const double* noise_var, double scale,
                         double* per_frame, double* partial_sums, int* num_partials_out,
                         double* gFmu, double* gFvar, double* psum = nullptr, const double* gsum = nullptr);
gp_status launch_finish_sum(gp_handle h, const double* partials, int count, int stride, int nsums, double* out,
                            double mul, int accumulate);

// opt.hip
gp_status launch_transform_forward(gp_handle h, const double* free_state, const uint8_t* tcode, int64_t n,
                                   double* params);
gp_status launch_transform_backward(gp_handle h, const double* params, const uint8_t* tcode, int64_t n,
                                    double* free_state);
gp_status launch_adam(gp_handle h, double* free_state, double* params, const double* grad, const uint8_t* tcode,
                      double* m, double* v, int64_t n, int64_t t, double lr, double b1, double b2, double eps);
