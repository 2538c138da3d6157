// gemm_debug.hip — gp_debug_gemm: ONE launch of a GEMM host entry on the caller's buffers, for the operator tests
// (tests/test_gpu_gemm.py).  No arithmetic of its own and no kernel: the plain records are copied into GemmProblems (every
// other field zero), uploaded into the caller's device workspace on the handle's stream, and handed to the launcher that
// `kind` and `form` select.  Nothing is synchronised.
#include "common.h"
#include <string.h>
#include <vector>

// the header and the tests size the workspace at 160 bytes per problem
static_assert(sizeof(GemmProblem) <= 160, "gp_debug_gemm: include/gpitch_abi.h promises 160 bytes of workspace per problem");

extern "C" gp_status gp_debug_gemm(gp_handle h, const gp_debug_gemm_problem* probs, int32_t batch, int32_t maxM, int32_t maxN,
                                   const gp_debug_gemm_flags* fl, int32_t kind, int32_t form, int32_t nsplit,
                                   void* workspace, size_t workspace_bytes, int32_t* partial_rows) {
  if (!h) return GP_ERR_BAD_ARG;
  if (!probs || !fl || batch <= 0 || batch > 4096 || maxM <= 0 || maxN <= 0 || kind < 0 || kind > 3 || form < 0 || form > 3 || nsplit < 0)
    return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_gemm: bad argument");
  if (fl->role == 5 || fl->role == 6 || fl->role == 7)
    return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_gemm: roles 5, 6 and 7 have their own tests");
  if (fl->role < 0 || fl->role > 3) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_gemm: unknown role");
  if (!workspace || (((uintptr_t)workspace) & 15) != 0 || workspace_bytes < (size_t)batch * sizeof(GemmProblem))
    return gp_fail(h, GP_ERR_WORKSPACE, "gp_debug_gemm: workspace too small or not 16-byte aligned");

  std::vector<GemmProblem> hp((size_t)batch);
  memset((void*)hp.data(), 0, hp.size() * sizeof(GemmProblem));
  for (int b = 0; b < batch; b++) {
    const gp_debug_gemm_problem& s = probs[b];
    GemmProblem& d = hp[(size_t)b];
    d.A = (const double*)s.A; d.B = (const double*)s.B; d.C = (double*)s.C;
    d.v0 = s.v0; d.v1 = s.v1; d.v2 = s.v2; d.o0 = s.o0; d.o1 = s.o1; d.o2 = s.o2;
    d.xa = (const double*)s.xa; d.xb = (const double*)s.xb;
    d.M = s.M; d.N = s.N; d.K = s.K; d.lda = s.lda; d.ldb = s.ldb; d.ldc = s.ldc;
  }
  GemmProblem* d_probs = (GemmProblem*)workspace;
  GP_HIP_CHECK(h, hipMemcpyAsync(d_probs, hp.data(), hp.size() * sizeof(GemmProblem), hipMemcpyHostToDevice, h->stream));

  GemmFlags f;
  f.transA = fl->transA; f.transB = fl->transB; f.triA = fl->triA; f.triB = fl->triB; f.triC = fl->triC;
  f.alpha = fl->alpha; f.beta = fl->beta; f.big_tiles = fl->big_tiles; f.epilogue = fl->epilogue; f.scale_mode = fl->scale_mode;
  f.role = fl->role; f.tile_m0 = fl->tile_m0; f.tile_mcount = fl->tile_mcount;
  f.uniform_aligned = fl->uniform_aligned; f.a32_ok = fl->a32_ok; f.rows64_ok = fl->rows64_ok;
  if (form == 3) { f.uniform_aligned = 0; f.rows64_ok = 0; }       // neither the wave nor the lean form takes such a launch
  const bool f32 = (kind == 2 || kind == 3);
  const int sym = (fl->triC == TRI_LOWER) ? 1 : 0, scale_by_k = (fl->scale_mode == 2) ? 1 : 0;
  int rows = 0;
  gp_status st = GP_OK;

  if (kind == 0 || kind == 2) {
    if (f32 && (f.role < 1)) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_gemm: the float32 strip products are roles 1, 2 and 3");
    // the wave form as the dispatchers reach it: role 3 always, roles 1 / 2 when the caller sized the partial rows per 64-row tile
    const bool wave_asked = f.role == 3 || (f.role >= 1 && f.rows64_ok);
    const bool wave_shape = f32 ? (f.a32_ok && gemm_wave_f32_takes(f.role, maxM, maxN, f.uniform_aligned))
                                : gemm_wave_takes(f.role, maxM, maxN, f.uniform_aligned);
    const int blocks = gemm_rowblocks(maxM, (f.role >= 1 || f.big_tiles || f32) ? 1 : 0);
    const int tiles64 = gemm_rowblocks(maxM, 0);      // the wave forms: one partial row per 64-row tile (maxM is a multiple of 64 there)
    if (form == 1) {
      if (!wave_asked) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_gemm: the wave form needs rows64_ok for roles 1 and 2");
      const bool taken = f32 ? launch_gemm_wave_f32(h, d_probs, batch, maxM, maxN, f, &st) : launch_gemm_wave(h, d_probs, batch, maxM, maxN, f, &st);
      if (!taken) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_gemm: the wave form does not take this launch");
      rows = tiles64;
    } else if (form == 2) {
      const bool taken = f32 ? launch_gemm_strip_f32_lean(h, d_probs, batch, maxM, maxN, f, &st) : launch_gemm_strip_lean(h, d_probs, batch, maxM, maxN, f, &st);
      if (!taken) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_gemm: the lean strip form does not take this launch");
      rows = blocks;
    } else {
      st = f32 ? launch_gemm_f32_role(h, d_probs, batch, maxM, maxN, f) : launch_gemm_batched(h, d_probs, batch, maxM, maxN, f);
      // as the engine sizes them: by role and shape alone.  A launch the wave form then declines for its flags (alpha, beta,
      // triC) writes the fewer rows of the form that runs instead, so this is an upper bound
      rows = (wave_asked && wave_shape) ? tiles64 : blocks;
    }
  } else {
    const int ns = nsplit > 0 ? nsplit : gemm_nt_nsplit(maxM, maxN, batch);
    if (ns < 2) return gp_fail(h, GP_ERR_BAD_ARG, "gp_debug_gemm: split-K needs at least two slices");
    if (form == 1) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_gemm: the split-K product has no wave form");
    if (form == 2) {
      if (f32) return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_gemm: the float32 split-K product has no lean form");
      // the lean branch of launch_gemm_nt_reduce_batched (gemm.hip), spelt out so that "not taken" can be told from "taken":
      // whoever changes that function changes this too (the dispatch test compares form 0 with this bit for bit)
      if (!launch_gemm_strip_nt_lean(h, d_probs, batch, maxM, maxN, ns, sym, scale_by_k, &st))
        return gp_fail(h, GP_ERR_UNSUPPORTED, "gp_debug_gemm: the lean split-K form does not take this launch");
      if (st == GP_OK) st = launch_slab_reduce(h, d_probs, batch, maxM, ns, sym, f.alpha);
    } else if (f32) {
      st = launch_gemm_f32_nt_reduce_batched(h, d_probs, batch, maxM, maxN, ns, sym, scale_by_k, f.alpha, f.uniform_aligned);
    } else {
      st = launch_gemm_nt_reduce_batched(h, d_probs, batch, maxM, maxN, ns, sym, scale_by_k, f.alpha, f.uniform_aligned);
    }
    rows = ns;      // one row of M row-dot partials per K-slice (o1), when v2 is given
  }
  if (partial_rows) *partial_rows = rows;
  return st;
}
