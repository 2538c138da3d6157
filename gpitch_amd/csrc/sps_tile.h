// sps_tile.h — the K_p(Z, x*) tile of the sparse per-source kernels, built straight into LDS: shared by predict_sparse.hip
// (posterior mean and variance of each source) and sample.hip (joint posterior draws), so both see the entries the
// sparse predictor always built.  A workgroup of 4 T threads takes T new frames; the tile is frame-major, sps_stride(M)
// doubles per frame (M rounded up to 16, plus 4: 4 x odd, so the 16 frames a wavefront reads sit on different LDS banks).
// Tails: rows in [kz, Mp) are zero and never read from Z; frames past n repeat the last one.  Device-only apart from the
// host-side size functions and the MPAD dispatch; include after common.h.
#pragma once
#include <type_traits>

#include "common.h"
#include "cov_entry.h"

#define SPS_CHUNK 32      // rows of Z staged per pass of the tile build

// frames per workgroup, from the plan's M: the M x T tile (plus 4 pad doubles per frame) stays inside the 160 KiB of LDS
static constexpr int sps_tile_frames(int M) { return M <= 256 ? 64 : (M <= 512 ? 32 : 16); }
static inline int sps_stride(int M) { return ((M + 15) & ~15) + 4; }       // doubles per frame of the tile (4 x odd: see the reads)
static inline size_t sps_lds_bytes(int M, int mpad) {
  const int T = sps_tile_frames(M), S = sps_stride(M);
  const size_t buf = (size_t)T * (S > 2 * mpad ? S : 2 * mpad);
  return (GP_EXP_TAB + 2 * SPS_CHUNK + (size_t)SPS_CHUNK * 2 * mpad + buf) * sizeof(double);
}

// The kernels on this tile are templates over MPAD, the largest sm_mpad() of a launch (0: no spectral-mixture kernel, served
// by MPAD = 4).  Calls f(std::integral_constant<int, MPAD>()) and returns its status, or fails with the caller's message.
template <typename F>
static inline gp_status sps_dispatch_mpad(gp_handle h, int max_mpad, const char* unsupported, F f) {
  switch (max_mpad <= 4 ? 4 : max_mpad) {
    case 4: return f(std::integral_constant<int, 4>());
    case 8: return f(std::integral_constant<int, 8>());
    case 12: return f(std::integral_constant<int, 12>());
    case 16: return f(std::integral_constant<int, 16>());
    case 20: return f(std::integral_constant<int, 20>());
    case 24: return f(std::integral_constant<int, 24>());
    case 28: return f(std::integral_constant<int, 28>());
    case 32: return f(std::integral_constant<int, 32>());
    default: return gp_fail(h, GP_ERR_UNSUPPORTED, unsupported);
  }
}

// LDS (doubles): etab[64] | rowa[32] | rowx[32] | zf[32][2 MPAD] | buf[T][S]  (buf first holds the frames' features [2 MPAD][T])
struct SpsLds { double *etab, *rowa, *rowx, *zf, *buf; };
template <int MPAD>
__device__ __forceinline__ SpsLds sps_lds_carve(double* lds) {
  SpsLds l;
  l.etab = lds;
  l.rowa = l.etab + GP_EXP_TAB;
  l.rowx = l.rowa + SPS_CHUNK;
  l.zf = l.rowx + SPS_CHUNK;
  l.buf = l.zf + SPS_CHUNK * 2 * MPAD;
  return l;
}

// buf[jj * S + i] = K_p(z_i, x*_{j0 + jj}) for i < kz (zero up to Mp), with the entry arithmetic of cov.hip (cov_entry.h).
// k: the source's kernel; z, fz: the window's kz inducing points and, for a Mercer kernel, the plan's feature table of them
// ([2 sm_mpad(m)][kz]); xnew: the window's n new frames.  Called by all 4 T threads; ends on a barrier (the tile is whole).
template <int MPAD>
__device__ __forceinline__ void sps_build_tile(const SpsLds& l, DevKern k, const double* __restrict__ z,
                                               const double* __restrict__ fz, int kz, const double* __restrict__ xnew, int n,
                                               int j0, int T, int S) {
  double* etab = l.etab;
  double* rowa = l.rowa;
  double* rowx = l.rowx;
  double* zf = l.zf;
  double* buf = l.buf;
  const int tid = threadIdx.x, NT = blockDim.x;           // NT = 4 T
  const int Mp = (kz + 15) & ~15;
  const int type = k.type, m = k.m;
  const double* __restrict__ th = k.theta;
  const double var = th[0], ls = th[1];
  const bool mercer = gp_kern_is_mercer(type), bcast = gp_kern_is_broadcast(type);
  const int mp = mercer ? ((m + 3) / 4) * 4 : 0;          // the feature table's own padding (sm_mpad)
  const int env = (type == GP_KERN_MERCER_MATERN12SM) ? 0 : 2;
  gp_exp_tab_init(etab);

  const int jj = tid % T, rg = tid / T;                   // this thread's frame of the tile and its row group (0..3)
  const double xb = xnew[min(j0 + jj, n - 1)];
  const double b = xb / ls, bb = __dmul_rn(b, b);
  double fx[2 * MPAD];
  if (mercer) {
    for (int t = tid; t < MPAD * T; t += NT) {
      const int q = t / T, fj = t % T;
      double c = 0.0, s = 0.0;
      if (q < m) cov_sm_feature(th, m, q, xnew[min(j0 + fj, n - 1)], &c, &s);
      buf[q * T + fj] = c;
      buf[(q + MPAD) * T + fj] = s;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 2 * MPAD; q++) fx[q] = buf[q * T + jj];
  } else {
#pragma unroll
    for (int q = 0; q < 2 * MPAD; q++) fx[q] = 0.0;
  }
  for (int r0 = 0; r0 < Mp; r0 += SPS_CHUNK) {
    __syncthreads();                                      // the frames' features / the previous chunk's rows are read
    if (tid < SPS_CHUNK) {
      const int i = r0 + tid;
      const double zi = (i < kz) ? z[i] : 0.0;
      rowx[tid] = zi;
      rowa[tid] = zi / ls;
    }
    if (mercer)
      for (int t = tid; t < SPS_CHUNK * MPAD; t += NT) {
        const int q = t / SPS_CHUNK, ii = t % SPS_CHUNK, i = r0 + ii;
        const bool on = (q < mp) && (i < kz);
        zf[ii * 2 * MPAD + q] = on ? fz[(size_t)q * kz + i] : 0.0;
        zf[ii * 2 * MPAD + MPAD + q] = on ? fz[(size_t)(mp + q) * kz + i] : 0.0;
      }
    __syncthreads();
    for (int ii = rg; ii < SPS_CHUNK; ii += 4) {
      const int i = r0 + ii;
      if (i >= Mp) break;
      double res = 0.0;
      if (i < kz) {
        const double a = rowa[ii], aa = __dmul_rn(a, a);
        if (mercer) {
          const double* fzr = &zf[ii * 2 * MPAD];
          double acc = 0.0;
#pragma unroll
          for (int q = 0; q < 2 * MPAD; q++) acc = fma(fzr[q], fx[q], acc);
          res = cov_mercer_entry(env, var, a, aa, b, bb, acc, etab);
        } else if (bcast) {
          res = cov_broadcast_entry(type, th, m, var, ls, rowx[ii], xb);
        } else {
          res = stat_profile(type, r2_expand(a, aa, b, bb), var, etab);
        }
      }
      buf[jj * S + i] = res;
    }
  }
  __syncthreads();
}
