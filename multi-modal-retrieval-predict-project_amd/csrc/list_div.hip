// Retrieval diversity of whole batches of retrieved lists (compute_embedding_diversity and
// compute_label_diversity_from_labels, src/Evaluate/retrieval_diversity_compute.py:171-194) on device:
// mmr_index_list_diversity (include/mmr.h holds the semantics, the cosine expression, the validity rule and the
// limits).
//
// A list of k global indices is cut into nt = ceil(k / 16) tiles of 16 list POSITIONS; the Gram matrix of the
// list is computed per tile pair (ti <= tj) on v_mfma_f64_16x16x4_f64, A = the rows of tile ti, B = the rows of
// tile tj, both gathered straight from the index: lane l = 16 h + r holds row r of its tile and, in step p, its
// elements k = 32 p + 8 h .. + 7 (two f32x4 of an MMR_F32 row, or the one 16-B tile32h piece of an MMR_F16 row,
// converted to f64 exactly in registers).  An entry that is not a row of the index is masked by POSITION, never by
// score: its lane reads row 0 of the (padded, never empty) device image instead, so that every load is
// unconditional and independent of the others, and each cosine of that position is written as 0.0 whatever its
// accumulator holds.
//   k <= 16  (ld_small, the workload's K = 5 / 10): one wavefront per list, one tile, A = B (one load feeds both
//            operands), every output written by that wave: no workspace, no second launch.
//   k > 16   (ld_tiles + ld_finish): one workgroup of 4 waves per (list, ti); wave w takes the tile pairs
//            (ti, ti + 4 w + u), u = 0 .. 3, tj < nt (A loaded once for up to 4 B tiles; the number of B tiles is
//            a template parameter chosen by a wave-uniform switch, so the MFMA loop holds no branch) and writes
//            one partial sum per tile pair to the caller's workspace [list][pair], pair = the row-major number
//            of (ti, tj) in the upper triangle.  ld_finish, one wave per list, adds them up.
// Summation order (the same in both regimes, a function of the list's contents and k only — never of nq, the
// batch slot or neighbouring lists):
//   <g_i, g_j>   one accumulator per tile pair: steps p ascending, in a step MFMA j = 0 .. 7, MFMA j adding
//                k = 32 p + 8 h' + j over h' = 0 .. 3 (rank_eval.hip's k-permutation).
//   c(i, j)      acc / (max(|g_i|, 1e-8) * max(|g_j|, 1e-8)), |g| = the index's norm64.  A lane holds
//                (i = h + 4 reg, j = r) of a tile pair; (j, i) is never computed: out_sim gets the one value at
//                both places, so it is symmetric bit for bit.
//   tile pair    a lane adds its valid i < j cosines in reg order 0 .. 3, the 64 lanes go through wave_sum's
//                xor 32, 16, 8, 4, 2, 1 tree.
//   list         k <= 16: that one sum.  k > 16: lane l of ld_finish adds the partials of pairs l, l + 64,
//                l + 128 in this order, then wave_sum's tree.
//   out_emb = 1 - sum / (m (m - 1) / 2); the label counts are integers.  No atomics: two runs give identical bytes.
// Measured: profiles/list_diversity.txt.
#include "knn_index.h"

namespace {

using mmr::aligned16;
using mmr::DeviceGuard;
using mmr::f16x8;
using mmr::f32x4;
typedef double f64x4 __attribute__((ext_vector_type(4)));

constexpr int LD_MAX_K = 256;              // = mmr_max_k(): 16 tiles, 136 tile pairs
constexpr int64_t LD_CHUNK = 1 << 20;      // lists per pass (bounds the grid and the workspace)
constexpr double LD_CLIP = 1e-8;           // the reference's norms.clip(min=1e-8)

inline int ld_pairs(int k) {
  const int nt = (k + 15) / 16;
  return nt * (nt + 1) / 2;
}

// a lane's 8 consecutive elements of a row, as stored
template <bool F16>
struct LdFrag;
template <>
struct LdFrag<false> {
  f32x4 lo, hi;
  __device__ __forceinline__ double at(int j) const { return (double)(j < 4 ? lo[j & 3] : hi[j & 3]); }
};
template <>
struct LdFrag<true> {
  f16x8 v;
  __device__ __forceinline__ double at(int j) const { return (double)(float)v[j]; }
};

// address of elements 8 h .. 8 h + 7 of `row` (step 0); a step advances 32 floats / one 512-half tile32h piece
template <bool F16>
__device__ __forceinline__ const void* ld_row_ptr(const float* gal, const uint16_t* gh, int64_t row, int Dp, int h) {
  if constexpr (F16) return gh + (row >> 4) * (int64_t)(Dp >> 5) * 512 + (h * 16 + (int)(row & 15)) * 8;
  else return gal + row * Dp + 8 * h;
}
template <bool F16>
__device__ __forceinline__ void ld_load(LdFrag<F16>& f, const void* p, int kb) {
  if constexpr (F16) {
    f.v = *(const f16x8*)((const uint16_t*)p + (kb >> 5) * 512);
  } else {
    f.lo = *(const f32x4*)((const float*)p + kb);
    f.hi = *(const f32x4*)((const float*)p + kb + 4);
  }
}

// local row of list entry g, -1 when it is not a row of the index
__device__ __forceinline__ int64_t ld_local(int64_t g, int64_t idx_base, int64_t n) {
  return (g >= idx_base && g < idx_base + n) ? g - idx_base : -1;
}

// Gram accumulators of tile ti (A, row pa) against NB tiles (B, rows pb[u]; SELF: B = A).  Dp % 64 == 0: an even
// number of 32-k steps, the next step's loads in flight under each step's MFMAs.
template <bool F16, int NB, bool SELF>
__device__ __forceinline__ void ld_gram(const void* pa, const void* (&pb)[NB], int Dp, f64x4 (&acc)[NB]) {
  LdFrag<F16> a0, a1, b0[NB], b1[NB];
  auto load = [&](LdFrag<F16>& a, LdFrag<F16>(&b)[NB], int kb) {
    ld_load<F16>(a, pa, kb);
    if constexpr (!SELF) {
#pragma unroll
      for (int u = 0; u < NB; ++u) ld_load<F16>(b[u], pb[u], kb);
    }
  };
  auto mac = [&](const LdFrag<F16>& a, const LdFrag<F16>(&b)[NB]) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const double av = a.at(j);
#pragma unroll
      for (int u = 0; u < NB; ++u) {
        if constexpr (SELF) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, av, acc[u], 0, 0, 0);
        else acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[u].at(j), acc[u], 0, 0, 0);
      }
    }
  };
#pragma unroll
  for (int u = 0; u < NB; ++u) acc[u] = (f64x4){0.0, 0.0, 0.0, 0.0};
  load(a0, b0, 0);
  for (int kb = 0; kb < Dp; kb += 64) {
    load(a1, b1, kb + 32);
    mac(a0, b0);
    if (kb + 64 < Dp) load(a0, b0, kb + 64);
    mac(a1, b1);
  }
}

// The cosines of one tile pair from its accumulator: the lane holds (i = h + 4 reg of tile ti, j = r of tile tj).
// ni / vi: clipped norm and validity of the lane's OWN A row (lane i < 16 holds row i of tile ti), nj / vj those of
// its B row.  Writes out_sim (both places) and returns the lane's sum of the valid pairs with list position i < j.
__device__ __forceinline__ double ld_tile_cos(const f64x4& acc, int lane, int ti, int tj, int k, double ni_own,
                                              bool vi_own, double nj, bool vj, double* __restrict__ sim) {
  const int r = lane & 15, h = lane >> 4;
  const int pj = 16 * tj + r;
  double s = 0.0;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) {
    const int i = h + 4 * reg;
    const int pi = 16 * ti + i;
    const double ni = __shfl(ni_own, i, 64);
    const bool vi = __shfl((int)vi_own, i, 64) != 0;
    const double c = (vi && vj) ? acc[reg] / (ni * nj) : 0.0;
    if (pi < pj) s += c;  // an invalid pair adds 0.0
    if (sim && pi <= pj && pj < k) {
      sim[(int64_t)pi * k + pj] = c;
      sim[(int64_t)pj * k + pi] = c;
    }
  }
  return s;
}

// m, the label counts and the three per-list outputs, by one wave (every lane passes the same `total`)
__device__ __forceinline__ void ld_outputs(const int64_t* __restrict__ list, int k, int64_t n, int64_t idx_base,
                                           const uint64_t* __restrict__ glab, double total, int lane,
                                           double* __restrict__ out_emb, double* __restrict__ out_lab,
                                           int32_t* __restrict__ out_valid) {
#pragma clang fp contract(off)
  int m = 0, s = 0, c = 0;
  uint64_t all = 0;
  for (int p = lane; p < k; p += 64) {
    const int64_t row = ld_local(list[p], idx_base, n);
    if (row >= 0) {
      ++m;
      if (glab) {
        const uint64_t b = glab[row];
        all |= b;
        s += __popcll(b);
        c += b != 0 ? 1 : 0;
      }
    }
  }
#pragma unroll
  for (int x = 32; x >= 1; x >>= 1) {
    m += __shfl_xor(m, x, 64);
    s += __shfl_xor(s, x, 64);
    c += __shfl_xor(c, x, 64);
    all |= (uint64_t)__shfl_xor((long long)all, x, 64);
  }
  if (lane == 0) {
    const double pairs = 0.5 * (double)m * (double)(m - 1);  // exact: m <= 256
    *out_emb = m < 2 ? 0.0 : 1.0 - total / pairs;
    if (out_lab) *out_lab = c == 0 ? 0.0 : (double)__popcll(all) / ((double)s / (double)c);
    if (out_valid) *out_valid = m;
  }
}

// k <= 16: one wave per list
template <bool F16>
__global__ __launch_bounds__(64) void ld_small(const float* __restrict__ gal, const uint16_t* __restrict__ gh, int Dp,
                                               const double* __restrict__ gnorm, int64_t n, int64_t idx_base,
                                               const int64_t* __restrict__ idx, int k,
                                               const uint64_t* __restrict__ glab, double* __restrict__ out_emb,
                                               double* __restrict__ out_lab, int32_t* __restrict__ out_valid,
                                               double* __restrict__ out_sim) {
  const int lane = threadIdx.x, r = lane & 15, h = lane >> 4;
  const int64_t q = blockIdx.x;
  const int64_t* list = idx + q * k;
  const int64_t row = r < k ? ld_local(list[r], idx_base, n) : -1;
  const bool ok = row >= 0;
  const double nrm = ok ? fmax(gnorm[row], LD_CLIP) : 1.0;  // in flight under the row loads
  const void* const pa = ld_row_ptr<F16>(gal, gh, ok ? row : 0, Dp, h);
  const void* pb[1] = {pa};
  f64x4 acc[1];
  ld_gram<F16, 1, true>(pa, pb, Dp, acc);
  const double s = ld_tile_cos(acc[0], lane, 0, 0, k, nrm, ok, nrm, ok, out_sim ? out_sim + q * k * k : nullptr);
  const double total = mmr::wave_sum(s);
  ld_outputs(list, k, n, idx_base, glab, total, lane, out_emb + q, out_lab ? out_lab + q : nullptr,
             out_valid ? out_valid + q : nullptr);
}

// k > 16: the tile pairs (ti, tj0 + u), u < NB, of one wave
template <bool F16, int NB>
__device__ __forceinline__ void ld_tile_row(const float* __restrict__ gal, const uint16_t* __restrict__ gh, int Dp,
                                            const double* __restrict__ gnorm, int64_t n, int64_t idx_base,
                                            const int64_t* __restrict__ list, int k, int nt, int ti, int tj0, int lane,
                                            double* __restrict__ part, double* __restrict__ sim) {
  const int r = lane & 15, h = lane >> 4;
  const int pa_pos = 16 * ti + r;
  const int64_t arow = pa_pos < k ? ld_local(list[pa_pos], idx_base, n) : -1;
  const bool a_ok = arow >= 0;
  const double an = a_ok ? fmax(gnorm[arow], LD_CLIP) : 1.0;
  const void* const pa = ld_row_ptr<F16>(gal, gh, a_ok ? arow : 0, Dp, h);
  const void* pb[NB];
  bool b_ok[NB];
  double bn[NB];
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int pos = 16 * (tj0 + u) + r;
    const int64_t brow = pos < k ? ld_local(list[pos], idx_base, n) : -1;
    b_ok[u] = brow >= 0;
    bn[u] = b_ok[u] ? fmax(gnorm[brow], LD_CLIP) : 1.0;
    pb[u] = ld_row_ptr<F16>(gal, gh, b_ok[u] ? brow : 0, Dp, h);
  }
  f64x4 acc[NB];
  ld_gram<F16, NB, false>(pa, pb, Dp, acc);
#pragma unroll
  for (int u = 0; u < NB; ++u) {
    const int tj = tj0 + u;
    const double s = ld_tile_cos(acc[u], lane, ti, tj, k, an, a_ok, bn[u], b_ok[u], sim);
    const double t = mmr::wave_sum(s);
    if (lane == 0) part[ti * nt - ti * (ti - 1) / 2 + (tj - ti)] = t;
  }
}

// workgroup = (list, ti), wave w = the tile pairs (ti, ti + 4 w + u), u = 0 .. 3, tj < nt
template <bool F16>
__global__ __launch_bounds__(256) void ld_tiles(const float* __restrict__ gal, const uint16_t* __restrict__ gh, int Dp,
                                                const double* __restrict__ gnorm, int64_t n, int64_t idx_base,
                                                const int64_t* __restrict__ idx, int k, int nt,
                                                double* __restrict__ part, double* __restrict__ out_sim) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t q = blockIdx.x / nt;
  const int ti = (int)(blockIdx.x % nt);
  const int tj0 = ti + 4 * wave;
  if (tj0 >= nt) return;
  const int64_t* list = idx + q * k;
  double* lp = part + q * (nt * (nt + 1) / 2);
  double* sim = out_sim ? out_sim + q * k * k : nullptr;
#define LD_ROW(NB) ld_tile_row<F16, NB>(gal, gh, Dp, gnorm, n, idx_base, list, k, nt, ti, tj0, lane, lp, sim)
  switch (nt - tj0) {
    case 1: LD_ROW(1); break;
    case 2: LD_ROW(2); break;
    case 3: LD_ROW(3); break;
    default: LD_ROW(4); break;
  }
#undef LD_ROW
}

__global__ __launch_bounds__(64) void ld_finish(const int64_t* __restrict__ idx, int k, int64_t n, int64_t idx_base,
                                                const uint64_t* __restrict__ glab, const double* __restrict__ part,
                                                int npairs, double* __restrict__ out_emb,
                                                double* __restrict__ out_lab, int32_t* __restrict__ out_valid) {
  const int lane = threadIdx.x;
  const int64_t q = blockIdx.x;
  double s = 0.0;
  for (int p = lane; p < npairs; p += 64) s += part[q * npairs + p];
  const double total = mmr::wave_sum(s);
  ld_outputs(idx + q * k, k, n, idx_base, glab, total, lane, out_emb + q, out_lab ? out_lab + q : nullptr,
             out_valid ? out_valid + q : nullptr);
}

template <bool F16>
mmr_status ld_run(const mmr_index* ix, const int64_t* idx, int64_t nq, int k, const uint64_t* glab, double* out_emb,
                  double* out_lab, int32_t* out_valid, double* out_sim, double* part, hipStream_t st) {
  const int nt = (k + 15) / 16, npairs = ld_pairs(k);
  for (int64_t q0 = 0; q0 < nq; q0 += LD_CHUNK) {
    const int64_t c = nq - q0 < LD_CHUNK ? nq - q0 : LD_CHUNK;
    const int64_t* li = idx + q0 * k;
    double* oe = out_emb + q0;
    double* ol = out_lab ? out_lab + q0 : nullptr;
    int32_t* ov = out_valid ? out_valid + q0 : nullptr;
    double* os = out_sim ? out_sim + q0 * k * k : nullptr;
    if (k <= 16) {
      ld_small<F16><<<dim3((unsigned)c), 64, 0, st>>>(ix->gal, ix->gh, ix->Dp, ix->norm64, ix->n, ix->idx_base, li, k,
                                                      glab, oe, ol, ov, os);
    } else {
      ld_tiles<F16><<<dim3((unsigned)(c * nt)), 256, 0, st>>>(ix->gal, ix->gh, ix->Dp, ix->norm64, ix->n, ix->idx_base,
                                                              li, k, nt, part, os);
      ld_finish<<<dim3((unsigned)c), 64, 0, st>>>(li, k, ix->n, ix->idx_base, glab, part, npairs, oe, ol, ov);
    }
    MMR_LAUNCH_CHECK();
  }
  return MMR_OK;
}

}  // namespace

extern "C" {

int64_t mmr_index_list_diversity_work_bytes(const mmr_index* ix, int64_t nq, int32_t k) {
  (void)ix;
  if (nq <= 0 || k <= 16 || k > LD_MAX_K) return 0;
  return mmr::round_up((nq < LD_CHUNK ? nq : LD_CHUNK) * ld_pairs(k) * 8, 256);
}

mmr_status mmr_index_list_diversity(const mmr_index* ix, const int64_t* idx, int64_t nq, int32_t k,
                                    const uint64_t* g_labels, double* out_emb, double* out_lab, int32_t* out_valid,
                                    double* out_sim, void* work, void* stream) {
  mmr::clear_error();
  MMR_REQUIRE(ix != nullptr, "mmr_index_list_diversity: index is NULL");
  MMR_REQUIRE(k >= 1 && k <= LD_MAX_K, "mmr_index_list_diversity: k=%d outside [1, %d]", k, LD_MAX_K);
  MMR_REQUIRE(nq >= 0, "mmr_index_list_diversity: nq < 0");
  MMR_REQUIRE((g_labels != nullptr) == (out_lab != nullptr),
              "mmr_index_list_diversity: g_labels and out_lab are both NULL or both set");
  if (nq == 0) return MMR_OK;
  MMR_REQUIRE(idx && out_emb, "mmr_index_list_diversity: NULL idx / out_emb");
  MMR_REQUIRE(k <= 16 || (work && aligned16(work)),
              "mmr_index_list_diversity: k > 16 needs work (mmr_index_list_diversity_work_bytes), 16-B aligned");
  DeviceGuard g(ix->device);
  hipStream_t st = mmr::as_stream(stream);
  if (ix->dtype == MMR_F16)
    return ld_run<true>(ix, idx, nq, k, g_labels, out_emb, out_lab, out_valid, out_sim, (double*)work, st);
  return ld_run<false>(ix, idx, nq, k, g_labels, out_emb, out_lab, out_valid, out_sim, (double*)work, st);
}

}  // extern "C"
