// struct mmr_index: the gallery index behind the C ABI's opaque handle (include/mmr.h).  Private to the
// library: knn.hip owns its lifetime and the search; rank_eval.hip reads the rows and norms of a const index.
#pragma once
#include <mutex>

#include "common.h"

struct mmr_index {
  int device = 0;
  int64_t n = 0, Np = 0, idx_base = 0;
  int d = 0, Dp = 0;
  int dtype = 0;              // MMR_F32 (f32 rows in gal) | MMR_F16 (native fp16: raw rows in gh, no gal)
  float* gal = nullptr;       // [Np][Dp] f32 rows (MMR_F32 index)
  float* inv_norm = nullptr;  // [Np]
  double* norm64 = nullptr;   // [Np]
  uint16_t* gs = nullptr;     // [Np][2Dp] bf16 hi/lo split (mode x3)
  float* gt = nullptr;        // [Np][Dp] f32 in the tile16 layout (skinny scan)
  // [Np][Dp] fp16 in the tile32h layout, the operand of every fp16 scan (lq / gmax / tile / p8): the unit
  // rows g/|g| of an MMR_F32 index in mode f16 (built on first use), or the raw rows of an MMR_F16 index
  // (its only copy of the gallery: 2 B per element; scans scale by inv_norm per row)
  uint16_t* gh = nullptr;
  int mode = 1;               // 0: f32 MFMA scores, 1: bf16x3 split scores, 2: fp16 scan
  // Workspace: one set per index, sized by what the mode needs (grown on demand).  `mu` serialises
  // the enqueue of searches; across streams the workspace follows the stream: a search on another
  // stream records ws_event on ws_stream (the last user's) and waits for it, so two streams never race
  // on it (and a realloc waits for the last user the same way).  Recorded at the switch, not after
  // every search: an event record per search cost 3-5 us of device time (16-query search 50.3 ->
  // 47.2 us back to back).
  std::mutex mu;
  int64_t ws_qrows = 0;       // query rows in qn / qnorm64
  int64_t ws_vals = 0;        // floats in vals
  int64_t ws_qsrows = 0;      // query rows in qs
  float* qn = nullptr;        // [rows][Dp] f32 (or fp16 / tile layouts, same bytes or fewer)
  double* qnorm64 = nullptr;  // [rows]
  float* vals = nullptr;      // scores (f32 mode) or per-(query, unit) maxima
  int64_t ws_bvals = 0;       // floats in bvals
  float* bvals = nullptr;     // mode f16: per-(query, 64-row block) maxima [256][Np/64]
  uint16_t* qs = nullptr;     // [rows][3Dp] bf16 split queries (x3 GEMM)
  int n_cu = 256;             // compute units of `device` (persistent grids)
  hipEvent_t ws_event = nullptr;
  hipStream_t ws_stream = nullptr;
  bool ws_used = false;
};
