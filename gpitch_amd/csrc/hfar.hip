// hfar.hip — the activations' H = A diag(2 gv) A^T and u = A gm from the stored A once and its factors once.
// For every 256-frame group S afar.hip holds A[:, S] = P_S B_S exactly, P_S = [T-_W(S), T+_W(S), W[:, near(S)]] (M x nr),
// B_S = [Psi-; Psi+; Kuf[near(S), S]] (nr x 256).  The stored, already rounded A stays one factor and only the other is factored:
//     H = sum_S (A[:, S] D_S B_S^T) P_S^T = sum_S Y_S P_S^T,        Y_S = A[:, S] diag(2 gv_S) B_S^T        (M x nr)
// so W enters once, as in A = W Kuf itself (the two-sided form sum_S P_S (B_S D_S B_S^T) P_S^T carries W's rounding twice).
// Three launches per step over the run of activation GPs, all on v_mfma_f64_16x16x4_f64 but the first:
//   hfar_check_kernel  one workgroup per GP: every (near tile t, group S) pair keeps its 16 columns of Y_S in slot t + S of a
//                      store of M / 16 + N / 256 - 1 slots.  With ascending z and strictly ascending frames no two pairs share a
//                      slot (two pairs on one anti-diagonal need a tie of frames across a group boundary AND of z across a tile
//                      boundary).  The kernel counts the pairs of every slot from the device's own ranges; where a slot has two,
//                      or a range is not whole tiles inside [0, M], it raises the handle's status word (code 5) and the GP's
//                      flag, and the two launches behind it write nothing for that GP.
//   hfar_y_kernel      one workgroup per (group, GP), the only pass over A[:, S].  The rows of B_S, scaled by 2 gv, and gm_S,
//                      unscaled, as one more row — so A[:, S] gm_S comes out as one more column — are staged in LDS as column
//                      tiles: tile q < ntile the near rows kbeg + 16 q .., tile ntile the four rows of Psi and gm.  A wavefront
//                      owns whole 16-row tiles of A, read straight from memory, and contracts the group's 256 frames for two
//                      column tiles at a time; groups with more than 16 near rows take further column blocks and read their
//                      slab of A again.  A group without near rows has the far columns and the gm column only.
//   hfar_h_kernel      H's lower 16 x 16 tiles (row tile >= column tile; Y supplies the rows), split-K over the groups into
//                      the plan's slabs: per group the four columns of T (afar's W half) and W[j, kbeg:kend), entries above
//                      the diagonal masked in the registers; a near tile t reaches only the column tiles tj >= t.  The
//                      per-group partials of u are folded into the slab's row of upart in ascending group order.
// launch_slab_reduce (gemm.hip) then sums the slabs, mirrors, and finishes u.  Fixed orders, no atomics: two runs agree bit for bit.
#include "engine.h"

typedef double hf_d4 __attribute__((ext_vector_type(4)));
typedef double hf_d2 __attribute__((ext_vector_type(2)));

#define HF_TILE 16
#define HF_BLK 2             // column tiles per column block of the Y launch

HfarSizes hfar_sizes(int M, int N) {
  const size_t ng = ((size_t)N + AFAR_GROUP - 1) / AFAR_GROUP, nt = ((size_t)M + HF_TILE - 1) / HF_TILE;
  HfarSizes s;
  s.Yn = gp_align_up((nt + ng - 1) * (size_t)M * HF_TILE, 32);       // at most M (M + N / 16) doubles
  s.Yf = gp_align_up(ng * (size_t)M * 4, 32);
  s.up = gp_align_up(ng * (size_t)M, 32);
  s.flag = 32;
  return s;
}

bool hfar_takes(int M, int N) { return afar_takes(M, N); }

__global__ void __launch_bounds__(256) hfar_check_kernel(const HfarItem* __restrict__ items, int N, int32_t* status) {
  const HfarItem it = items[blockIdx.x];
  const int M = it.M, nt = M / HF_TILE, ng = N / AFAR_GROUP, nslot = nt + ng - 1;
  // what a thread found wrong: 1 + the group of a range that is not whole tiles inside [0, M], ng + 1 + the slot two pairs share
  int bad = 0;
  for (int S = threadIdx.x; S < ng; S += 256) {
    const int kb = it.rng[2 * S], ke = it.rng[2 * S + 1];
    if (kb < 0 || ke < kb || ke > M || (kb % HF_TILE) != 0 || (ke % HF_TILE) != 0) bad = 1 + S;
  }
  if (!__syncthreads_or(bad)) {
    for (int s = threadIdx.x; s < nslot; s += 256) {
      int pairs = 0;
      for (int S = max(0, s - (nt - 1)); S <= min(ng - 1, s); S++) {
        const int t = s - S;
        if (HF_TILE * t >= it.rng[2 * S] && HF_TILE * t < it.rng[2 * S + 1]) pairs++;
      }
      if (pairs > 1) bad = ng + 1 + s;
    }
  }
  __shared__ int worst;
  if (threadIdx.x == 0) worst = 0;
  __syncthreads();
  if (bad) atomicMax(&worst, bad);                   // (LDS; the largest is as good as any: the result is the same every run)
  __syncthreads();
  if (threadIdx.x == 0) {
    it.flag[0] = worst ? 1 : 0;
    if (worst) { status[0] = 5; status[1] = worst > ng ? worst - ng - 1 : worst - 1; status[2] = it.gp; status[3] = worst > ng ? 1 : 0; }
  }
}

// lane (kq, lc) of the A operand holds A[16 a + lc][n0 + 16 ch + 4 kq + s], s = 0 .. 3, as two 16-byte loads per 16 frames (a
// row's 128 bytes in four lanes); k-step (ch, s) of the MFMA therefore sums frames 16 ch + 4 kq + s over kq, and the B operand
// is Bs[16 p + lc][16 ch + 4 kq + s] from LDS.  A row of Bs is 256 doubles; its 16-byte pairs are stored at (n / 2) ^ (row & 15)
// so that the sixteen lanes of a quarter, which read one pair each from sixteen rows, fall on sixteen different bank groups.
__global__ void __launch_bounds__(256) hfar_y_kernel(const HfarItem* __restrict__ items, int N) {
  const HfarItem it = items[blockIdx.y];
  if (it.flag[0]) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int lc = lane & 15, kq = lane >> 4;
  const int S = blockIdx.x, M = it.M, nt = M / HF_TILE;
  const size_t n0 = (size_t)S * AFAR_GROUP, ld = (size_t)it.ld;
  const int kbeg = __builtin_amdgcn_readfirstlane(it.rng[2 * S]), kend = __builtin_amdgcn_readfirstlane(it.rng[2 * S + 1]);
  const int ntile = (kend - kbeg) / HF_TILE, tb = kbeg / HF_TILE, nct = ntile + 1;
  __shared__ double Bs[HF_BLK * HF_TILE][AFAR_GROUP];

  const double gv2 = 2.0 * it.gv[n0 + tid], gmn = it.gm[n0 + tid];
  const int wpair = tid >> 1, wodd = tid & 1;
  for (int blk = 0; blk * HF_BLK < nct; blk++) {
    __syncthreads();                                   // (the block before this one has been read)
#pragma unroll 4
    for (int c = 0; c < HF_BLK * HF_TILE; c++) {
      const int q = blk * HF_BLK + (c >> 4), r = c & 15;
      double v = 0.0;
      if (q < ntile) v = gv2 * it.Kuf[(size_t)(kbeg + HF_TILE * q + r) * ld + n0 + tid];
      else if (q == ntile && r < 4) v = gv2 * it.Psi[(size_t)r * N + n0 + tid];
      else if (q == ntile && r == 4) v = gmn;
      Bs[c][((wpair ^ r) << 1) | wodd] = v;
    }
    __syncthreads();
    const int np = min(HF_BLK, nct - blk * HF_BLK);   // column tiles of this block with anything in them
    for (int a = wave; a < nt; a += 4) {
      const double* ap = it.A + (size_t)(HF_TILE * a + lc) * ld + n0 + 4 * kq;
      hf_d2 fa[16][2];
#pragma unroll
      for (int ch = 0; ch < 16; ch++) {
        fa[ch][0] = *(const hf_d2*)(ap + 16 * ch);
        fa[ch][1] = *(const hf_d2*)(ap + 16 * ch + 2);
      }
      hf_d4 acc[HF_BLK];
#pragma unroll
      for (int p = 0; p < HF_BLK; p++) acc[p] = hf_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ch = 0; ch < 16; ch++) {
#pragma unroll
        for (int p = 0; p < HF_BLK; p++) {
          if (p < np) {
            const double* bp = &Bs[HF_TILE * p + lc][0];
            const hf_d2 b0 = *(const hf_d2*)(bp + (((8 * ch + 2 * kq) ^ lc) << 1));
            const hf_d2 b1 = *(const hf_d2*)(bp + (((8 * ch + 2 * kq + 1) ^ lc) << 1));
            acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ch][0].x, b0.x, acc[p], 0, 0, 0);
            acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ch][0].y, b0.y, acc[p], 0, 0, 0);
            acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ch][1].x, b1.x, acc[p], 0, 0, 0);
            acc[p] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[ch][1].y, b1.y, acc[p], 0, 0, 0);
          }
        }
      }
      // the accumulator of column tile p: column lc, rows 16 a + kq + 4 r
#pragma unroll
      for (int p = 0; p < HF_BLK; p++) {
        const int q = blk * HF_BLK + p;
        if (q < ntile) {
          double* yn = it.Yn + ((size_t)(tb + q + S) * M + HF_TILE * a + kq) * HF_TILE + lc;
#pragma unroll
          for (int r = 0; r < 4; r++) yn[(size_t)4 * r * HF_TILE] = acc[p][r];
        } else if (q == ntile) {
          const size_t row = (size_t)S * M + HF_TILE * a + kq;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            if (lc < 4) it.Yf[(row + 4 * r) * 4 + lc] = acc[p][r];
            else if (lc == 4) it.up[row + 4 * r] = acc[p][r];
          }
        }
      }
    }
  }
}

// blockIdx.x: a 64 x 64 block (Q, cb), cb <= Q, of H's lower triangle; wavefront w owns row tile ti = 4 Q + w and the column
// tiles tj = 4 cb + j <= ti.  blockIdx.y: the slab, groups [k ng / nsplit, (k + 1) ng / nsplit); blockIdx.z: the GP.
//   A operand, lane (kq, lc):  far   Yf[S][16 ti + lc][kq]                       near   Yn[t + S][16 ti + lc][4 kq + s]
//   B operand, lane (kq, lc):  far   T[S][16 tj + lc][kq]  (the W half)          near   W[16 tj + lc][16 t + 4 kq + s]
__global__ void __launch_bounds__(256) hfar_h_kernel(const HfarItem* __restrict__ items, int N, int nsplit) {
  const HfarItem it = items[blockIdx.z];
  if (it.flag[0]) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int lc = lane & 15, kq = lane >> 4;
  const int M = it.M, nt = M / HF_TILE, ng = N / AFAR_GROUP, k = blockIdx.y;
  int Q = 0, cb = blockIdx.x;
  while (cb > Q) { cb -= Q + 1; Q++; }
  const int ti = 4 * Q + wave;
  if (ti >= nt) return;
  const int tj0 = 4 * cb, ntj = min(4, ti - tj0 + 1);                 // >= 1: cb <= Q
  const int S0 = (int)((int64_t)k * ng / nsplit), S1 = (int)((int64_t)(k + 1) * ng / nsplit);
  hf_d4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = hf_d4{0.0, 0.0, 0.0, 0.0};
  const size_t rowY = (size_t)HF_TILE * ti + lc;
  for (int S = S0; S < S1; S++) {
    const int kbeg = __builtin_amdgcn_readfirstlane(it.rng[2 * S]), kend = __builtin_amdgcn_readfirstlane(it.rng[2 * S + 1]);
    const int tb = kbeg / HF_TILE, te = min(kend / HF_TILE, tj0 + ntj);     // near tile t reaches the column tiles tj >= t only
    const double yf = it.Yf[((size_t)S * M + rowY) * 4 + kq];
    const double* tp = it.T + ((size_t)S * M + HF_TILE * tj0 + lc) * 8 + kq;
#pragma unroll
    for (int j = 0; j < 4; j++)
      if (j < ntj) acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(yf, tp[(size_t)j * HF_TILE * 8], acc[j], 0, 0, 0);
    for (int t = tb; t < te; t++) {
      const double* yp = it.Yn + ((size_t)(t + S) * M + rowY) * HF_TILE + 4 * kq;
      const hf_d2 y0 = *(const hf_d2*)yp, y1 = *(const hf_d2*)(yp + 2);
      const double* wp = it.W + ((size_t)HF_TILE * tj0 + lc) * M + HF_TILE * t + 4 * kq;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int tj = tj0 + j;
        if (j < ntj && tj >= t) {
          hf_d2 w0 = *(const hf_d2*)(wp + (size_t)j * HF_TILE * M), w1 = *(const hf_d2*)(wp + (size_t)j * HF_TILE * M + 2);
          if (tj == t) {                                               // the tile on the diagonal: column 4 kq + s above row lc
            const int d = 4 * kq - lc;
            if (d > 0) w0.x = 0.0;
            if (d + 1 > 0) w0.y = 0.0;
            if (d + 2 > 0) w1.x = 0.0;
            if (d + 3 > 0) w1.y = 0.0;
          }
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(y0.x, w0.x, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(y0.y, w0.y, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(y1.x, w1.x, acc[j], 0, 0, 0);
          acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(y1.y, w1.y, acc[j], 0, 0, 0);
        }
      }
    }
  }
  double* slab = it.slabs + (size_t)k * M * M + ((size_t)HF_TILE * ti + kq) * M + HF_TILE * tj0 + lc;
#pragma unroll
  for (int j = 0; j < 4; j++)
    if (j < ntj) {
#pragma unroll
      for (int r = 0; r < 4; r++) slab[(size_t)4 * r * M + j * HF_TILE] = acc[j][r];
    }
  if (cb == 0 && lane < HF_TILE) {                                     // u's partial of this slab, rows of the row tile
    const size_t row = (size_t)HF_TILE * ti + lane;
    double s = 0.0;
    for (int S = S0; S < S1; S++) s += it.up[(size_t)S * M + row];
    it.upart[(size_t)k * M + row] = s;
  }
}

gp_status launch_hfar(gp_handle h, const HfarItem* d_items, int count, int M, int n, int nsplit, int charges) {
  if (count <= 0) return GP_OK;
  if (!hfar_takes(M, n) || nsplit < 1) return gp_fail(h, GP_ERR_UNSUPPORTED, "activations' H from the factors: whole 256-frame groups, M a multiple of 16 up to 1024, strips of 2^20 entries or more");
  const int nt = M / HF_TILE, nQ = (nt + 3) / 4;
  auto run = [&]() -> gp_status {
    hipLaunchKernelGGL(hfar_check_kernel, dim3(count), dim3(256), 0, h->stream, d_items, n, h->d_status);
    hipLaunchKernelGGL(hfar_y_kernel, dim3(n / AFAR_GROUP, count), dim3(256), 0, h->stream, d_items, n);
    hipLaunchKernelGGL(hfar_h_kernel, dim3(nQ * (nQ + 1) / 2, nsplit, count), dim3(256), 0, h->stream, d_items, n, nsplit);
    GP_HIP_CHECK(h, hipGetLastError());
    return GP_OK;
  };
  // (the tests compare the launches charged to the split-K product's timer between forms: where these launches are that
  // product, they open as many scopes as its launcher would — gemm_nt_reduce_charges — the further ones empty, as there)
  if (charges <= 0) return run();
  for (int q = 1; q < charges; q++) { GpTimerScope empty(h, GP_TIMER_NT_GEMM); }
  GpTimerScope ts(h, GP_TIMER_NT_GEMM);
  return run();
}
